"""Shared by tests/test_tracers_host.py and tests/test_gpu_tracers.py: the oracle carrying passive tracers through the
definition, seeds, release patterns and the error measure."""
import numpy as np

from conftest import load_golden
from oracle import ludvm_oracle as O


def gust_cloud():
    """G5's free vortices as constructor keywords."""
    g = load_golden("g5_freevort.npz")
    return dict(circulation_freevort=g["gamma_freevort"], xy_freevort=g["xy_freevort"])


def seeds37():
    """37 seeds around the foil and its young wake (lab frame of config 1: the foil starts at x in [-0.25, 0.75], heaves about
    z = 1 and moves towards -x): a rake above the chord, one below, a column behind the trailing edge."""
    above = np.stack([np.linspace(-0.6, 1.2, 13), np.full(13, 1.25)])
    below = np.stack([np.linspace(-0.6, 1.2, 13), np.full(13, 0.8)])
    behind = np.stack([np.full(11, 1.0), np.linspace(0.6, 1.4, 11)])
    return np.concatenate([above, below, behind], axis=1)


def seeds_random(M, seed=3):
    """M seeds in a box around the foil's path over the first 50 steps."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3.0, 1.5, M), rng.uniform(0.0, 2.0, M)])


def releases_1_7_50(M):
    """Release steps 1, 7 and 50 in turn (50 is one past the end of a 49-step run, or its last step of a 50-step one)."""
    return np.array([1, 7, 50], dtype=np.int64)[np.arange(M) % 3]


def releases_by_tile(M, tile, steps=(1, 5, 10 ** 6)):
    """Release steps that make whole tiles of `tile` tracers free from step 1 (tile 0, 3, ...), mixed (tile 1, 4, ...: released
    at steps[0], steps[1] or never, lane by lane) and wholly held for the run (tile 2, 5, ...)."""
    m = np.arange(M)
    kind = (m // tile) % 3
    rel = np.full(M, steps[0], dtype=np.int64)
    mixed = kind == 1
    rel[mixed] = np.array(steps, dtype=np.int64)[m[mixed] % 3]
    rel[kind == 2] = steps[2]
    return rel


class TracedOracle(O.OracleLUDVM):
    """The oracle, noting the sources of each step's roll-up calls (LUDVM.py:1095-1106) exactly as ProbedOracle of
    tests/probes_common.py does -- only `_wake` and `induced_velocity` are overridden -- and carrying tracers through the
    definition in NumPy: tracer m is held at (xs + shift[i], zs) while i < release[m]; in step i >= release[m] it goes from
    `start` (the seed of step i if i == release[m], else its position after step i - 1) to start + dt (u, w)_i(start), the
    oracle's float64 sums over the step's roll-up sources, written as the reference writes its own Euler update (:1120-1127).
    `rows[i]`: positions [2, M] after step i; `sources[i]`: (g_wake, x, z, g_foil, x, z) of step i."""

    def __init__(self, tracers, release=None, shift=None, **kw):
        self._txz = np.asarray(tracers, dtype=float)
        M = self._txz.shape[1]
        self._rel = np.ones(M, dtype=np.int64) if release is None else np.asarray(release, dtype=np.int64)
        self._shift = shift             # callable: oracle -> per-step x offsets (None: lab frame)
        self.rows, self.sources = {}, {}
        self._cur = None
        super().__init__(**kw)

    def seeds_at(self, i):
        sh = 0.0 if self._shift is None else self._shift(self)[i]
        return np.stack([self._txz[0] + sh, self._txz[1]])

    def _wake(self, i, n_tev, n_lev):
        got = super()._wake(i, n_tev, n_lev)
        self._last_wake = (i, n_tev - 1, got)
        return got

    def induced_velocity(self, circulation, xw, zw, xp, zp, viscous=True):
        last = getattr(self, "_last_wake", None)
        if last is not None and last[0] not in self.rows:
            i, itev, (gw, xs, zs) = last
            gp = self.path["airfoil_gamma_points"][i]
            if len(np.atleast_1d(xw)) == gp.shape[1] and np.array_equal(xw, gp[0]) and np.array_equal(zw, gp[1]) \
                    and np.array_equal(circulation, self.circulation["airfoil"][itev]):
                self.sources[i] = (gw.copy(), xs.copy(), zs.copy(), np.array(circulation, dtype=float), np.array(xw), np.array(zw))
                self.rows[i] = self._cur = euler_step(self.seeds_at(i), self._cur, self._rel, i, self.dt, self.v_core, self.sources[i])
        return super().induced_velocity(circulation, xw, zw, xp, zp, viscous)

    def path_rows(self):
        """-> [nt, 2, M]; row 0: the seeds (+ shift[0])."""
        out = np.zeros([self.nt, 2, self._txz.shape[1]])
        out[0] = self.seeds_at(0)
        for i, row in self.rows.items():
            out[i] = row
        return out


def euler_step(seeds_i, cur, rel, i, dt, v_core, sources):
    """One step of the definition: positions [2, M] after step i from the step's seeds, the positions after step i - 1 (None
    before the first step), the release steps and the step's sources."""
    gw, xs, zs, gf, xf, zf = sources
    new = seeds_i.copy()
    free = rel <= i
    if free.any():
        first = (rel == i)[free]
        px = np.where(first, seeds_i[0][free], seeds_i[0][free] if cur is None else cur[0][free])
        pz = np.where(first, seeds_i[1][free], seeds_i[1][free] if cur is None else cur[1][free])
        uw, ww = O.induced_velocity(gw, xs, zs, px, pz, v_core)
        uf, wf = O.induced_velocity(gf, xf, zf, px, pz, v_core)
        new[0][free] = px + dt * (uw + uf)
        new[1][free] = pz + dt * (ww + wf)
    return new


def path_error(path, ref, first, last):
    """max |path[s] - oracle row s| over the recorded steps first .. last of `path` (a mapping step -> [2, M] with .steps()),
    over the largest displacement the flow gave a tracer in those steps, |oracle row s - seeds of step s| (a held tracer of the
    tunnel frame rides with its seed: no displacement)."""
    rows = ref.path_rows()
    steps = [s for s in path.steps() if first <= s <= last]
    assert steps, "no recorded step in the range"
    worst = max(np.abs(path[s] - rows[s]).max() for s in steps)
    scale = max(np.abs(rows[s] - ref.seeds_at(s)).max() for s in steps)
    assert scale > 0.0
    return worst / scale


def run_sources(sim, i):
    """The sources of step i's roll-up as a run with the dense history says them itself (the construction of
    tests/test_gpu_probes.py::test_overlapped_steps_probe_the_sources_of_their_own_roll_up): the wake as row i - 1 holds it,
    the vortices shed in step i at their placement (LUDVM.py:672-681, :788-800), the bound vortices of step i.
    -> (g_wake, x, z, g_foil, x, z) as `euler_step` takes them; i >= 2."""
    P, C, foil, gp = sim.path, sim.circulation, sim.path["airfoil"], sim.path["airfoil_gamma_points"]
    shed = sim.LEV_shed != -1
    itev, ilev = i - 1, int(shed[:i].sum())                   # shed before step i
    te, le = foil[i, :, -1], foil[i, :, 0]
    new = [te + (P["TEV"][i - 1][:, itev - 1] - te) / 3]
    g_new = [C["TEV"][itev]]
    if shed[i]:
        new.append(le + (P["LEV"][i - 1][:, ilev - 1] - le) / 3 if (ilev > 0 and shed[i - 1]) else le)
        g_new.append(C["LEV"][ilev])
    new = np.array(new).T
    g = np.concatenate([C["TEV"][:itev], C["LEV"][:ilev], np.asarray(C["FREE"], float), g_new])
    x = np.concatenate([P["TEV"][i - 1, 0, :itev], P["LEV"][i - 1, 0, :ilev], P["FREE"][i - 1, 0], new[0]])
    z = np.concatenate([P["TEV"][i - 1, 1, :itev], P["LEV"][i - 1, 1, :ilev], P["FREE"][i - 1, 1], new[1]])
    return g, x, z, C["airfoil"][itev], gp[i, 0], gp[i, 1]
