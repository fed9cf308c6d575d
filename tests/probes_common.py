"""Shared by tests/test_probes_host.py and tests/test_gpu_probes.py: the reference's own roll-up field values (G3 fixture)
as probe points, and the oracle's probe series."""
import numpy as np

from conftest import grouped, load_golden
from oracle import ludvm_oracle as O

G3_STEPS = (1, 2, 3, 4, 5, 100)


def g3_probe_cases():
    """-> {step: (x, z, u, w)}: the targets of the reference's roll-up calls 3+4, 5+6, 7+8 of steps 1-5 and 100 of config 1
    (LUDVM.py:1105-1124: wake call + bound-vortex call on the TEV, LEV and FREE slices) and u_wake + u_foil there."""
    g3 = load_golden("g3_boundary_trace.npz")
    by = grouped(g3)
    per_step = {}
    for k in range(int(g3["ncalls"])):
        c = by[str(k)]
        per_step.setdefault(int(c["step"]), []).append(c)
    out = {}
    for s in G3_STEPS:
        cs = per_step[s]
        assert len(cs) == 9
        x, z, u, w = [], [], [], []
        for a in (3, 5, 7):
            wake, foil = cs[a], cs[a + 1]
            assert len(foil["g"]) == 80 and np.array_equal(wake["xp"], foil["xp"]) and np.array_equal(wake["zp"], foil["zp"])
            x.append(wake["xp"]); z.append(wake["zp"])
            u.append(wake["u"] + foil["u"]); w.append(wake["w"] + foil["w"])
        out[s] = tuple(np.concatenate(v) for v in (x, z, u, w))
    assert [len(out[s][0]) for s in G3_STEPS] == [3, 4, 5, 6, 7, 156]
    return out


def g3_probe_points(cases):
    """All 181 points, in step order -> ([2, 181], {step: slice})."""
    xs, zs, where, at = [], [], {}, 0
    for s in G3_STEPS:
        x, z = cases[s][0], cases[s][1]
        xs.append(x); zs.append(z)
        where[s] = slice(at, at + len(x))
        at += len(x)
    return np.stack([np.concatenate(xs), np.concatenate(zs)]), where


def g3_errors(sim, cases, where):
    """-> {step: max |probe - reference| / max|reference| over the step's points}"""
    err = {}
    for s in G3_STEPS:
        _, _, u, w = cases[s]
        scale = max(np.abs(u).max(), np.abs(w).max())
        err[s] = max(np.abs(sim.probe_u[s, where[s]] - u).max(), np.abs(sim.probe_w[s, where[s]] - w).max()) / scale
    return err


def probes32():
    """32 points: near wake, far field, ahead of the foil (lab frame of config 1: the foil starts at x in [-0.25, 0.75] and
    moves towards -x)."""
    rng = np.random.default_rng(11)
    near = np.stack([rng.uniform(-1.5, 1.0, 16), rng.uniform(0.4, 1.6, 16)])         # around the heaving foil and its young wake
    far = np.stack([rng.uniform(-20.0, 20.0, 8), rng.uniform(-15.0, 15.0, 8)])
    ahead = np.stack([rng.uniform(-6.0, -3.0, 8), rng.uniform(-1.0, 2.0, 8)])
    return np.concatenate([near, far, ahead], axis=1)


class ProbedOracle(O.OracleLUDVM):
    """The oracle, noting the sources of each step's roll-up calls (LUDVM.py:1095-1106) and evaluating them at the probes.
    Only `_wake` and `induced_velocity` are overridden: the wake of the roll-up is the last `_wake` gather of the step (the
    loads' one, :1049-1051, with the shed vortices in it), and the first call whose sources are the step's bound-vortex points
    with the step's panel circulations opens the roll-up."""

    def __init__(self, probes, shift=None, **kw):
        self._pxz = np.asarray(probes, dtype=float)
        self._shift = shift             # callable: oracle -> per-step x offsets (None: lab frame)
        self.rows = {}
        super().__init__(**kw)

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
                px = self._pxz[0] + (0.0 if self._shift is None else self._shift(self)[i])
                pz = self._pxz[1]
                uw, ww = O.induced_velocity(gw, xs, zs, px, pz, self.v_core)
                uf, wf = O.induced_velocity(circulation, xw, zw, px, pz, self.v_core)
                self.rows[i] = (uw + uf, ww + wf)
        return super().induced_velocity(circulation, xw, zw, xp, zp, viscous)

    def series(self):
        """-> (u, w) [nt, P]; row 0: the field of the initial free vortices."""
        P = self._pxz.shape[1]
        u, w = np.zeros([self.nt, P]), np.zeros([self.nt, P])
        px = self._pxz[0] + (0.0 if self._shift is None else self._shift(self)[0])
        free0 = np.array(self.xy_freevort, dtype=float).reshape(2, -1)
        u[0], w[0] = O.induced_velocity(np.asarray(self.circulation_freevort, dtype=float), free0[0], free0[1], px, self._pxz[1],
                                        self.v_core)
        for i, (ui, wi) in self.rows.items():
            u[i], w[i] = ui, wi
        return u, w


def series_error(sim, ou, ow, first, last):
    """max |class - oracle| / max|oracle| over steps first .. last"""
    sl = slice(first, last + 1)
    scale = max(np.abs(ou[sl]).max(), np.abs(ow[sl]).max())
    return max(np.abs(sim.probe_u[sl] - ou[sl]).max(), np.abs(sim.probe_w[sl] - ow[sl]).max()) / scale
