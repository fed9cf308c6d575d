"""Shared by tests/test_observers_off_unit_host.py and tests/test_gpu_observers_off_unit.py (G11): the observers -- probes, passive
tracers, the tracers' deformation gradient, the wake survey with its gradient sums and phase bins, and the three sweep observers
-- on G10's cases (oracle/g10_cases.py, taken by name), where chord, Uinf, dt and v_core differ from config 1's and sections are
cambered.  Every other observer test builds its run from CONFIG1.

Point sets are config 1's mapped by x -> chord x, z -> chord z: with x0 = 0 the foil starts at x in [-chord / 4, 3 chord / 4]
and, every case having h_max = chord (asserted), at z = chord, so the map about the foil's start is the plain product
test_gpu_g10 uses; dt Uinf / chord = 0.05 in every case, so the foil travels 2.5 chords in the 50 compared steps and the random
box [-3, 1.5] x [0, 2] chords spans that path as seeds_random's spans config 1's.

The reference is ONE oracle run per case (TracedOracle, which notes the sources of every step's roll-up): the observers are
passive, so probe rows, tracer rows and survey sums in either frame -- and what a subtly wrong implementation would give
instead (a foreign v_core, dt or shift row, bound vortices on the chord line) -- are sums over those sources, formed with the
operations ProbedOracle and TracedOracle use (tests/observer_sources_common.field, tests/tracers_common.euler_step)."""
import warnings
from fractions import Fraction

import numpy as np

from observer_sources_common import field
from oracle import g10_cases as G10
from oracle import ludvm_oracle as O
from probes_common import probes32
from survey_common import series_sums, series_umax, sums_errors, window
from tracers_common import TracedOracle, euler_step, releases_1_7_50, run_sources, seeds37, seeds_random

CASES = ("d23", "dhalf", "k45", "c4412d", "c2412", "c2412f")
SOLO_CASES = ("d23", "dhalf", "c4412d", "c2412")
SOURCES_CASES = ("d23", "c4412d", "c2412f")
FP32_CASES = ("d23", "dhalf")
BIN_CASES = ("d23", "k45")
FRAMES = ("lab", "tunnel")
STEPS = 50
MARGIN = 10.0                   # the host loop stays this far inside a bound the GPU tier asserts (tests/g10_common.MARGIN)
SENSITIVITY = 100.0             # a mutation moves a quantity at least this many bounds
# The compared steps 1 .. WINDOW[name] of the oracle comparisons.  Licensed by test_host_loop_matches_the_oracle: the host loop
# on the fake engine, which differs from the oracle by summation order only, measured over steps 1-50, worst of both frames
# (probes of max|u| | tracers of the largest displacement | survey means of max|u| / raw second moments of max|u|^2):
#   d23 3.6e-15 | 7.9e-16 | 1.3e-15 / 1.5e-15      dhalf 1.8e-15 | 1.6e-15 | 4.2e-16 / 4.1e-16
#   k45 1.3e-14 | 3.2e-14 | 4.1e-14 / 2.4e-14      c4412d 3.0e-15 | 7.0e-16 | 4.3e-16 / 2.5e-16
#   c2412 3.9e-15 | 1.6e-15 | 2.1e-16 / 8.7e-17    c2412f 4.1e-15 | 2.5e-15 | 5.7e-16 / 8.3e-16
#   d23r 4.3e-15 | 7.8e-16 | 5.6e-16 / 8.4e-16     c6409 2.5e-14 | 2.0e-15 | 1.4e-15 / 9.7e-16   (these two: the sweep's points)
# -- every one more than 10 x inside its bound (1e-9 | 1e-9 | 1e-9 / 3e-9): no window is shortened.
WINDOW = {name: STEPS for name in CASES + ("d23r", "c6409")}
PROBE_VS_ORACLE = 1e-9          # of max|u|: test_marched_series_matches_the_oracle
TRACER_VS_ORACLE = 1e-9         # of the largest displacement: test_marched_paths_match_the_oracle (tracers_common.path_error)
F_ROW_VS_INCREMENT = 1e-7       # of the largest single increment dt G F: tests/test_gpu_tracer_gradient.py's second bound (its
#                                 first, 1e-9 of max|F|, is survey_gradient_common.MEAN_BOUND's construction)
# ONE sweep of all seven 81-point cases, ordered so that every member differs from both its neighbours in dt, Uinf and v_core
# (the four members on D23's scales stand at 0, 2, 4, 6)
SWEEP = ("d23", "c2412", "d23r", "dhalf", "k45", "c6409", "c4412d")
SWEEP_PAIRS = [(m, m - 1) for m in range(1, len(SWEEP))] + [(m, m + 1) for m in range(len(SWEEP) - 1)]      # (member, the one taken for it)
SWEEP_F = ("c2412f", "c2412f")  # the 127-point case, 'Faure' beside 'Ramesh' (Npoints is common to a sweep)
PHASE0 = 0.35                   # survey_phase0 of the 5-bin tables: no step lies on a bin edge


def case_keywords(name, steps=None, **over):
    """The constructor keywords of G10's case `name` (oracle, host loop and device alike), cut to `steps` time steps."""
    c = G10.BY_NAME[name]
    kw = G10.kwargs(c if steps is None else dict(c, steps=steps), **over)
    assert kw.get("h_max", G10.KW_DEFAULTS["h_max"]) == kw["chord"]          # (what the map of the point sets rests on)
    return kw


def v_core_of(kw):
    return 1.3 * (kw["dt"] * kw["Uinf"] / kw["chord"]) * kw["chord"]


def observers(name):
    """-> dict(probes [2, 32], tracers [2, 37], release, survey [2, 600]): config 1's sets in the case's chords."""
    c = case_keywords(name)["chord"]
    return dict(probes=c * probes32(), tracers=c * seeds37(), release=releases_1_7_50(37), survey=c * seeds_random(600))


def sweep_observers():
    """One set for the mixed sweep: every third point of each set in chords of 2, 1 and 0.5 in turn, so that each member has
    points around its own foil (at z = its chord) and along its own path."""
    def mixed(pts):
        return np.concatenate([c * pts[:, k::3] for k, c in enumerate((2.0, 1.0, 0.5))], axis=1)
    return dict(probes=mixed(probes32()), tracers=mixed(seeds37()), release=releases_1_7_50(37), survey=mixed(seeds_random(600)))


def run_keywords(obs, frame, survey_steps):
    """The solo constructor keywords of a run that carries `obs` in `frame`."""
    return dict(probes=obs["probes"], probe_frame=frame, tracers=obs["tracers"], tracer_release=obs["release"], tracer_frame=frame,
                survey=obs["survey"], survey_frame=frame, survey_steps=survey_steps)


class OracleRun:
    """The oracle's run of a case over `steps` steps with the sources of every step's roll-up (`sources[i]`, i >= 1)."""

    def __init__(self, name, steps=STEPS, **over):
        self.name, self.kw = name, case_keywords(name, steps, **over)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = TracedOracle(np.zeros([2, 1]), **self.kw)
            flat = O.OracleLUDVM(**dict(self.kw, Naca="0012"), run=False)
        self.nt, self.dt, self.v_core, self.t, self.xpiv, self.Uinf = ref.nt, ref.dt, ref.v_core, ref.t, ref.xpiv, ref.Uinf
        self.sources = dict(ref.sources)
        assert sorted(self.sources) == list(range(1, self.nt)) and self.nt == steps + 1
        self.free0 = (np.asarray(ref.circulation_freevort, dtype=float), *np.array(ref.xy_freevort, dtype=float).reshape(2, -1))
        self.cambered = G10.is_cambered(G10.BY_NAME[name])
        # the same sources with the bound vortices on the chord line (eta = 0): what a sum that ignores the camber walks
        gp = flat.path["airfoil_gamma_points"]
        self.flat_sources = {i: s[:4] + (gp[i, 0].copy(), gp[i, 1].copy()) for i, s in self.sources.items()}

    def shift(self, frame):
        return self.xpiv if frame == "tunnel" else np.zeros(self.nt)


def probe_series(run, pts, shift, v_core=None, sources=None):
    """(u, w) [nt, P] at (pts[0] + shift[i], pts[1]) over the step's sources, as ProbedOracle.series forms them (row 0: the
    field of the initial free vortices).  v_core, sources: the run's, unless a mutation says otherwise."""
    vc = run.v_core if v_core is None else v_core
    src = run.sources if sources is None else sources
    u, w = np.zeros([run.nt, pts.shape[1]]), np.zeros([run.nt, pts.shape[1]])
    u[0], w[0] = O.induced_velocity(*run.free0, pts[0] + shift[0], pts[1], vc)
    for i in range(1, run.nt):
        u[i], w[i] = field(O.induced_velocity, src[i], pts[0] + shift[i], pts[1], vc)
    return u, w


def tracer_rows(run, seeds, rel, shift, dt=None, v_core=None, sources=None):
    """[nt, 2, M]: the paths by TracedOracle's definition (held at the seed of the step, then Euler steps over the step's
    sources); row 0: the seeds of step 0."""
    dt = run.dt if dt is None else dt
    vc = run.v_core if v_core is None else v_core
    src = run.sources if sources is None else sources
    rows, cur = np.zeros([run.nt, 2, seeds.shape[1]]), None
    rows[0] = np.stack([seeds[0] + shift[0], seeds[1]])
    for i in range(1, run.nt):
        rows[i] = cur = euler_step(np.stack([seeds[0] + shift[i], seeds[1]]), cur, rel, i, dt, vc, src[i])
    return rows


def seed_rows(run, seeds, shift):
    return np.stack([np.stack([seeds[0] + shift[i], seeds[1]]) for i in range(run.nt)])


def reference(run, obs, frame, survey_steps, **mutation):
    """-> dict(u, w [nt, 32]; rows [nt, 2, 37]; seeds [nt, 2, 37]; sums [5, 600], W, umax): what the observers of `obs` see in
    `frame`.  mutation: shift=, v_core=, dt=, sources= replace the run's own."""
    shift = mutation.pop("shift", None)
    shift = run.shift(frame) if shift is None else shift
    dt = mutation.pop("dt", None)
    u, w = probe_series(run, obs["probes"], shift, **mutation)
    rows = tracer_rows(run, obs["tracers"], obs["release"], shift, dt=dt, **mutation)
    su, sw = probe_series(run, obs["survey"], shift, **mutation)
    W = window(*survey_steps, run.nt)
    return dict(u=u, w=w, rows=rows, seeds=seed_rows(run, obs["tracers"], shift), sums=series_sums(su, sw, W), W=W,
                umax=series_umax(su, sw, W))


def errors(got, ref, first, last):
    """`got` (dict(u, w, rows, sums) of a run, an oracle reference or a mutation) against the reference `ref` over steps
    first .. last -> (probes of max|u|, tracers of the largest displacement -- tracers_common.path_error's measure --, survey
    means of max|u|, raw second moments of max|u|^2)."""
    sl = slice(first, last + 1)
    scale = max(np.abs(ref["u"][sl]).max(), np.abs(ref["w"][sl]).max())
    e_probe = max(np.abs(got["u"][sl] - ref["u"][sl]).max(), np.abs(got["w"][sl] - ref["w"][sl]).max()) / scale
    disp = np.abs(ref["rows"][sl] - ref["seeds"][sl]).max()
    assert scale > 0.0 and disp > 0.0
    e_tracer = np.abs(got["rows"][sl] - ref["rows"][sl]).max() / disp
    e_mean, e_mom = sums_errors(got["sums"], ref["sums"], len(ref["W"]), ref["umax"])
    return float(e_probe), float(e_tracer), float(e_mean), float(e_mom)


def of_run(sim):
    """A product run (solo with every tracer row recorded, or a sweep member with particle_steps = every compared step) as
    `errors` takes it."""
    steps = sim.tracer_path.steps()
    rows = np.zeros([sim.nt, 2, sim.tracer_xz.shape[1]])
    for s in steps:
        rows[s] = sim.tracer_path[s]
    return dict(u=sim.probe_u, w=sim.probe_w, rows=rows, sums=sim.survey_sums.reshape(5, -1))


# ---- the integer bin rule in exact arithmetic ------------------------------------------------------------------------------------

def exact_bin_table(t, kw, B, phase0=None, frequency=None):
    """-> (table int64 [nt], decided bool [nt]): floor(B frac(tau) + 1e-9) % B with tau = (t - phase0) f in exact rational
    arithmetic -- t: the float64 time levels as they stand, f = (k / pi) / 2 x Uinf / chord from the keywords (k / pi is 1/5 or
    3/10 exactly), phase0: t0 = 0 by default.  `decided`: B frac(tau) + 1e-9 is farther than 1e-10 from an integer, so a float64
    evaluation of the rule (errors of 1e-14) cannot differ; this holds wherever the phase is farther than 1e-6 from a bin edge
    AND at a step that sits on an edge exactly (a period of d23 is a whole 200 steps: 8 steps of 200 with B = 8), which the
    1e-9 of the rule sends up.  frequency: a Fraction replaces f (the mutation f = k / 2 pi)."""
    k_over_pi = Fraction(kw.get("k", G10.KW_DEFAULTS["k"]) / np.pi).limit_denominator(1000)
    f = k_over_pi / 2 * Fraction(kw["Uinf"]) / Fraction(kw["chord"]) if frequency is None else frequency
    p0 = Fraction(0) if phase0 is None else Fraction(phase0)
    table, decided = np.zeros(len(t), dtype=np.int64), np.zeros(len(t), dtype=bool)
    for i, ti in enumerate(t):
        tau = (Fraction(float(ti)) - p0) * f
        v = B * (tau - (tau.numerator // tau.denominator)) + Fraction(1, 10 ** 9)
        n = v.numerator // v.denominator
        table[i] = n % B
        decided[i] = min(v - n, n + 1 - v) > Fraction(1, 10 ** 10)
    return table, decided


def unit_frequency(kw):
    """f = k / 2 pi: the frequency of a rule that forgets chord and Uinf."""
    return Fraction(kw.get("k", G10.KW_DEFAULTS["k"]) / np.pi).limit_denominator(1000) / 2


def bin_settings():
    return [dict(survey_bins=8), dict(survey_bins=5, survey_phase0=PHASE0)]


# ---- the fp32 survey's guard at a core radius of the case's own ----------------------------------------------------------------------

GUARD_STEP = 3                  # the one sampled step: window (3, 4, 1) of a 4-step run
GUARD_EXTENT = {"dhalf": 14.08, "d23": 28.16}     # between 300 x 0.0325 and 300 x 0.065 | between 300 x 0.065 and 300 x 0.13


def guard_case(name):
    """A 4-step run of `name` whose every origin class at step 3 has an extent of GUARD_EXTENT[name]: a sheet of 256 free
    vortices (survey_f32_common.far_sheet: one whole source tile, slots 0-255) with the spacing extent / 128, beginning at
    x = -100, and two more free vortices -- slots 256 and 257, one on each parity of the tile that holds the shed and the bound
    vortices -- that extent ahead of the foil.  With the case's v_core the guard takes every class on `dhalf` and none on `d23`;
    with config 1's 0.065 it is the other way round.  -> (constructor keywords, survey points [2, 419]: on, within a core of
    and chords away from every other sheet vortex, and the probe set around the foil)."""
    from survey_f32_common import far_sheet, points_around
    E = GUARD_EXTENT[name]
    kw = case_keywords(name, GUARD_STEP + 1)
    g, x, z = far_sheet(n=256, x0=-100.0, spacing=E / 128)
    z = z + kw["chord"]
    g = np.concatenate([g, [1e-3, -1e-3]])
    x = np.concatenate([x, [E, E + 0.01]])
    z = np.concatenate([z, [kw["chord"], kw["chord"] + 0.01]])
    kw.update(circulation_freevort=g, xy_freevort=np.stack([x, z]))
    pts = np.concatenate([points_around(x[:256:2], z[:256:2], v_core_of(kw), chord=kw["chord"]), kw["chord"] * probes32()[:, :32]],
                         axis=1)
    return kw, pts


def stored_sources(sim, i):
    """(g, x, z) of step i's roll-up in the order the device holds them -- the free vortices, each step's TEV and, when shed, LEV
    in shedding order, the vortices shed in step i, the bound vortices -- from a run with the dense history (i >= 2, fewer than
    2048 free vortices: stored as given)."""
    g, x, z, gf, xf, zf = run_sources(sim, i)
    shed = sim.LEV_shed != -1
    itev, ilev, nf = i - 1, int(shed[:i].sum()), len(np.asarray(sim.circulation["FREE"]).reshape(-1))
    order, lev = list(range(itev + ilev, itev + ilev + nf)), 0
    for s in range(1, i):
        order.append(s - 1)
        if shed[s]:
            order.append(itev + lev)
            lev += 1
    order += list(range(itev + ilev + nf, len(g)))
    assert sorted(order) == list(range(len(g)))
    order = np.array(order)
    return np.concatenate([g[order], gf]), np.concatenate([x[order], xf]), np.concatenate([z[order], zf])
