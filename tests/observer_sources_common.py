"""Shared by tests/test_observer_sources_host.py and tests/test_gpu_observer_sources.py: runs whose SOURCE count -- not their
point count -- walks the observer kernels (probes, tracers, survey; DESIGN.md sections 4.8-4.11) over many 256-source tiles,
many splits, ragged and empty last splits and the steps at which a launch plan changes form.  A cloud of initial free
vortices sets the source count directly, so a few steps of config 1 reach all of it.

With `cloud(n)` config 1 sheds no leading-edge vortex in the steps used here (checked with the Python oracle on the CPU for
n = 1180 and n = 4000 over 25 steps; every GPU test asserts it of its own run), so with npan = 80 bound vortices and
one trailing-edge vortex per step, in step i of a fresh run (anchor: step 0 for all i < 192)

    ns(i)    = nfree + i + 80        the sources the kernels walk (read on the device)
    ns_ub(i) = nfree + 2 i + 80      the bound the host plans the launch with

The launch rule itself (observer_plan of plan_rule.hpp) is NOT restated in code here (tests/test_observer_rule_host.py asks it
for the plans quoted below); the arithmetic of the three cases, for the reader:

case A  nfree = 1180, 24 steps.  ns_ub = 1280 at step 10: five full splits of 256; 1282 at step 11: a sixth split, empty
        through step 20; ns = 1280 exactly at step 20, 1281 at step 21: one source in the sixth split.  chunk = 256 in the
        plans of all three kernels (32 probes: want 1024; 37 tracers / 600 survey points: want 64; 1280 / 64 < 256).
case B  nfree = 16280, 25 steps.  ns_ub = 16384 at step 12: tracers and survey (few) run 64 splits of 256, the cap; at step 13
        (16386) 33 splits of 512.  Probes (P = 32, want 1024): 64 splits at step 12, 65 from step 13 -- the finisher's
        strided leg (sidx += 64) starts.  ns = 16384 at step 24; in step 25 the 65th probe split holds a source.  With 4096
        probes (want 16): 16 splits of 1024, then 13 of 1280.  (Config 1 sheds its first leading-edge vortex at step 26 by its
        own kinematics -- LESP reaches LESPcrit there with no cloud at all, plain oracle -- and at step 27 with this cloud
        on the device: no cloud postpones that, so the case ends at step 25, the last step with something of its own.)
case C  nfree = 20390, 14 steps.  ns_ub = 20480 at step 5, ns = 20480 at step 10.  Tracers and survey (few): 40 splits of 512
        (two tiles per split), then 41 with an empty last one, from step 11 one source in it.  Probes P = 32: 80 / 81 splits of
        256.  Probes P = 4096 (64 tiles, want 16): chunk 1280 (five tiles per one-wave workgroup) and 16 splits, then chunk
        1536 and 14 splits from step 6.

Two observer sets, each composing probes, tracers and a survey in one run:
few   probes32(); seeds37() released at steps 1, 7 and 50; a 600-point survey seeds_random(600)
many  4096 probes; 2561 tracers (5 tiles + 1) released by tile; a survey of 20481 points (41 tiles: want falls to 24, so its
      chunk is 256 / 768 / 1024 in A / B / C and case C's 21st split appears at step 6 and is first used in step 11) over a
      window around the case's boundary steps, checked at `survey_sample`'s points."""
import numpy as np

from conftest import CONFIG1
from oracle import c_oracle, ludvm_oracle as O
from probes_common import probes32
from tracers_common import releases_1_7_50, releases_by_tile, seeds37, seeds_random

NPAN = CONFIG1["Npoints"] - 1
TILE = 512                      # tracers and survey points per workgroup (kTracerTile, kSurveyTile)

# case -> (nfree, steps, boundary steps reported on their own, many-survey window (first, stop, every))
CASES = {"A": (1180, 24, (10, 11, 20, 21), (19, 22, 1)),
         "B": (16280, 25, (12, 13, 24, 25), (12, 15, 1)),
         "C": (20390, 14, (5, 6, 10, 11), (5, 12, 1))}
SETS = ("few", "many")

PROBE_VS_SOURCES = 1e-9         # of max|u|: the bound of test_overlapped_steps_probe_the_sources_of_their_own_roll_up
TRACER_VS_SOURCES = 1e-9        # of the largest displacement: the same construction's bound in tests/test_gpu_tracers.py
ROW0_VS_ORACLE = 1e-12          # of max|u|: row 0, the free-vortex field (test_marched_series_matches_the_oracle)
MEMBER_VS_SOLO = 1e-12          # sweep member against its solo 'f64' march, steps 1-10 (probes: of max|u|; particles: of the
                                # largest displacement): the bounds of the two sweep files' own solo tests


def cloud(n, seed=7):
    """n free vortices of +-(0.5 .. 1) 1e-3 in the box x in [-6, 2], z in [-1, 3] around the foil's path, as constructor keywords."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-6.0, 2.0, n)
    z = rng.uniform(-1.0, 3.0, n)
    g = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 1e-3
    return dict(circulation_freevort=g, xy_freevort=np.stack([x, z]))


def case_keywords(case):
    nfree, steps = CASES[case][:2]
    # (tf half a step short of the last level: t = arange(t0, tf + dt, dt) then has steps + 1 entries whatever the rounding)
    return dict(CONFIG1, tf=(steps - 0.5) * CONFIG1["dt"], **cloud(nfree))


def probes4096():
    rng = np.random.default_rng(4096)
    return np.stack([rng.uniform(-6.5, 2.5, 4096), rng.uniform(-1.5, 3.5, 4096)])


def survey_sample(K, count=1024, seed=29):
    """Sorted indices of at most `count` of K survey points: the first and the last point of every tile of 512, the rest drawn."""
    if K <= count:
        return np.arange(K)
    ends = np.array([k for t in range(0, K, TILE) for k in (t, min(t + TILE, K) - 1)])
    rest = np.random.default_rng(seed).choice(K, count - len(ends), replace=False)
    pick = np.unique(np.concatenate([ends, rest]))
    assert len(pick) <= count and np.isin(ends, pick).all()
    return pick


def observers(case, which):
    """-> dict(probes, tracers, release, survey, window, pick): the points of set `which` in `case` (lab frame).  `pick` is the
    sample of the survey that is checked (every point of the small one)."""
    nt = CASES[case][1] + 1
    if which == "few":
        K = 600
        return dict(probes=probes32(), tracers=seeds37(), release=releases_1_7_50(37), survey=seeds_random(K),
                    window=(1 if case == "A" else 2, nt, 1), pick=np.arange(K))
    M, K = 5 * TILE + 1, 40 * TILE + 1
    return dict(probes=probes4096(), tracers=seeds_random(M, seed=5), release=releases_by_tile(M, TILE, steps=(1, 5, 10 ** 6)),
                survey=seeds_random(K, seed=13), window=CASES[case][3], pick=survey_sample(K))


def run_keywords(obs):
    """The constructor keywords of a run that carries `obs`; every step's tracer row is recorded."""
    return dict(probes=obs["probes"], tracers=obs["tracers"], tracer_release=obs["release"], survey=obs["survey"],
                survey_steps=obs["window"])


def fast_iv():
    """The C oracle's pair sum on at most 16 threads (the NumPy one where the library is not built: the same numbers to
    1e-13, tests/test_c_oracle.py)."""
    if not c_oracle.available():
        return O.induced_velocity
    if c_oracle.threads() > 16:
        c_oracle.set_threads(16)
    return c_oracle.induced_velocity


def field(iv, sources, px, pz, v_core):
    """(u, w) of a step's sources (g_wake, x, z, g_foil, x, z) at the points: wake call + bound-vortex call, as the reference
    (LUDVM.py:1095-1106) and ProbedOracle add them.  `iv`: oracle.ludvm_oracle.induced_velocity or oracle.c_oracle's."""
    gw, xs, zs, gf, xf, zf = sources
    uw, ww = iv(gw, xs, zs, px, pz, v_core)
    uf, wf = iv(gf, xf, zf, px, pz, v_core)
    return uw + uf, ww + wf


def euler_step_by(iv, seeds_i, cur, rel, i, dt, v_core, sources):
    """tracers_common.euler_step with the pair sums of `iv` (the C oracle where NumPy's is too slow)."""
    new = seeds_i.copy()
    free = rel <= i
    if free.any():
        first = (rel == i)[free]
        px = np.where(first, seeds_i[0][free], seeds_i[0][free] if cur is None else cur[0][free])
        pz = np.where(first, seeds_i[1][free], seeds_i[1][free] if cur is None else cur[1][free])
        u, w = field(iv, sources, px, pz, v_core)
        new[0][free] = px + dt * u
        new[1][free] = pz + dt * w
    return new


def sorted_sources(g, x, z):
    """One step's sources in an order of their own (by x, then z, then circulation) -> [3, n]."""
    order = np.lexsort((g, z, x))
    return np.stack([x[order], z[order], g[order]])


def weakest_contribution(g, x, z, px, pz, v_core, rows=256):
    """min over the sources of (max over the points of the magnitude of that source's single contribution to (u, w))."""
    best = np.zeros(len(g))
    vc4 = v_core ** 4
    for a in range(0, len(px), rows):
        dx = px[a:a + rows, None] - x[None]
        dz = pz[a:a + rows, None] - z[None]
        r2 = dx * dx + dz * dz
        best = np.maximum(best, (np.abs(g)[None] / (2 * np.pi) * np.sqrt(r2 / np.sqrt(r2 * r2 + vc4))).max(axis=0))
    return best.min()


class CaseAOracle:
    """The full Python oracle of case A carrying both sets at once: one TracedOracle run with the tracers of both sets side by
    side (its `sources[i]` are the sources of every step's roll-up), and the field of those sources -- what ProbedOracle
    evaluates -- at the probes and survey points of both sets."""

    def __init__(self):
        from tracers_common import TracedOracle
        self.obs = {w: observers("A", w) for w in SETS}
        seeds = np.concatenate([self.obs[w]["tracers"] for w in SETS], axis=1)
        rel = np.concatenate([self.obs[w]["release"] for w in SETS])
        self.ref = TracedOracle(seeds, release=rel, **case_keywords("A"))
        self.nt, self.v_core, self.dt = self.ref.nt, self.ref.v_core, self.ref.dt
        assert self.nt == CASES["A"][1] + 1
        self._tcols = {"few": slice(0, 37), "many": slice(37, seeds.shape[1])}
        pts = [self.obs[w][k][:, self.obs[w]["pick"]] if k == "survey" else self.obs[w][k] for w in SETS for k in ("probes", "survey")]
        cuts = np.cumsum([0] + [p.shape[1] for p in pts])
        allp = np.concatenate(pts, axis=1)
        u, w = np.zeros([self.nt, allp.shape[1]]), np.zeros([self.nt, allp.shape[1]])
        kw = case_keywords("A")
        free = (kw["circulation_freevort"], kw["xy_freevort"][0], kw["xy_freevort"][1])
        # the small set by the NumPy oracle (ProbedOracle's bits), the large one by the C oracle (NumPy takes 8 s there)
        few = slice(0, cuts[2])
        for sl, iv in ((few, O.induced_velocity), (slice(cuts[2], cuts[4]), fast_iv())):
            u[0, sl], w[0, sl] = iv(*free, allp[0, sl], allp[1, sl], self.v_core)
            for i in range(1, self.nt):
                u[i, sl], w[i, sl] = field(iv, self.ref.sources[i], allp[0, sl], allp[1, sl], self.v_core)
        u.setflags(write=False); w.setflags(write=False)
        self._uw = {(wh, k): (u[:, cuts[j]:cuts[j + 1]], w[:, cuts[j]:cuts[j + 1]])
                    for j, (wh, k) in enumerate((wh, k) for wh in SETS for k in ("probes", "survey"))}

    def series(self, which, kind="probes"):
        """-> (u, w) [nt, P] at the probes (or the checked survey points) of set `which`."""
        return self._uw[which, kind]

    def tracer_rows(self, which):
        """-> [nt, 2, M]: the paths of set `which`."""
        return self.ref.path_rows()[:, :, self._tcols[which]]
