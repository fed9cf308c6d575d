"""Shared by tests/test_wake_integrals_host.py and tests/test_gpu_wake_integrals.py: the reference of the wake integrals
(DESIGN.md section 4.22), their bounds, the cases and a float64 model of the rows into which faults can be planted.

The SYSTEM of step i is the sources of step i's roll-up, `tracers_common.run_sources(sim, i)` (`first_step_sources` for i = 1) of
a dense-history run or of the CPU oracle: the wake before the step's Euler update, the vortices shed in the step at their
placement, the bound vortices of the step.  `reference(sim, i)` forms from them, in np.longdouble and never from the code under
test,

    sums[c, s, :]  for class c of FREE, TEV, LEV, BOUND and sign slot s (0: G >= 0, 1: G < 0): count, sum G, sum G x, sum G z,
                   sum G (x^2 + z^2), sum G^2
    W              1/2 sum_a sum_b G_a G_b / (4 pi) ln((r_ab^2 + s_ab) / 2), s = sqrt(r^4 + v_core^4), a = b included

The bounds are derived, not tuned; eps = 2^-52, ns the number of sources:

    |moment - ref| <= (ns + 16) eps sum |term|     fixed-order float64 adds (ns eps is the worst case of any order) of terms that
                                                   are themselves rounded products (16 ulp cover them); counts are exact
    |W - ref|      <= 1/2 sum_a |G_a| B_a + (ns + 16) eps sum_a |G_a psi_a| / 2
                                                   B_a: the per-target bound of psi that tests/scalar_field_common.py derives
                                                   (imported, not restated); the second term is the sum over a, as above
"""
import numpy as np

import scalar_field_common as SF
from ensemble_survey_grad_common import first_step_sources
from fake_engine import FakeEngine
from tracers_common import gust_cloud, run_sources

LD = np.longdouble
EPS = 2.0**-52
CLASSES = ("FREE", "TEV", "LEV", "BOUND")
FREE, TEV, LEV, BOUND = range(4)


def sources_and_classes(sim, i):
    """-> (g, x, z, cls) of every source of step i, the bound vortices included, in run_sources' order: the TEVs and the LEVs
    shed before step i, the free vortices, the vortices shed in step i (the TEV, then the LEV if one is shed), the bound ones."""
    gw, xw, zw, gf, xf, zf = first_step_sources(sim) if i == 1 else run_sources(sim, i)
    shed = np.asarray(sim.LEV_shed) != -1
    nf = len(np.atleast_1d(np.asarray(sim.circulation["FREE"], float)))
    itev, ilev = i - 1, int(shed[:i].sum())
    cls = np.concatenate([np.full(itev, TEV), np.full(ilev, LEV), np.full(nf, FREE), [TEV], [LEV] if shed[i] else [],
                          np.full(len(gf), BOUND)]).astype(np.int64)
    g, x, z = np.concatenate([gw, gf]), np.concatenate([xw, xf]), np.concatenate([zw, zf])
    assert len(cls) == len(g) == len(x) == len(z)
    return g, x, z, cls


def moment_terms(g, x, z):
    """long double [6, ns]: the terms of the six sums"""
    g, x, z = (np.asarray(a, LD) for a in (g, x, z))
    return np.stack([np.ones_like(g), g, g * x, g * z, g * (x * x + z * z), g * g])


_cache = {}


def reference(sim, i, energy=True):
    """-> dict: sums, mag (sum |term|) float64 [4, 2, 6] rounded from long double; ns; and -- energy -- W, W_bound, self (the
    a = b part of W).  Computed once per (run, step) and handed out read-only."""
    key = (id(sim), int(i))
    got = _cache.get(key)
    if got is None or (energy and "W" not in got):
        g, x, z, cls = sources_and_classes(sim, i)
        t = moment_terms(g, x, z)
        sums, mag = np.zeros([4, 2, 6], LD), np.zeros([4, 2, 6], LD)
        neg = np.asarray(g, float) < 0.0
        for c in range(4):
            for s in range(2):
                m = (cls == c) & (neg == bool(s))
                sums[c, s], mag[c, s] = t[:, m].sum(axis=1), np.abs(t[:, m]).sum(axis=1)
        got = dict(sums=sums.astype(float), mag=mag.astype(float), ns=len(g), sim=sim)
        if energy:
            vc = float(sim.v_core)
            psi = np.zeros(len(g), LD)                          # long double, a = b included; 512 targets at a time
            for lo in range(0, len(g), 512):
                gg, r2, s, _ = SF._pairs(g, x, z, x[lo:lo + 512], z[lo:lo + 512], vc)
                psi[lo:lo + 512] = (gg / (4 * SF.PI) * np.log((r2 + s) / 2)).sum(axis=1)
            ga = np.asarray(g, LD)
            _, bnd = SF.reference("psi", g, x, z, x, z, vc, rows=512)
            got["W"] = float(0.5 * (ga * psi).sum())
            got["W_bound"] = float(0.5 * (np.abs(ga) * bnd).sum() + (len(g) + 16) * EPS * 0.5 * np.abs(ga * psi).sum())
            got["self"] = float(np.log(LD(vc) ** 2 / 2) / (8 * SF.PI) * (ga * ga).sum())
        for v in got.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = got
    return got


def moment_bound(ref):
    return (ref["ns"] + 16) * EPS * ref["mag"]


def moment_ratio(row, ref):
    """worst |row - ref| / bound over the 40 sums that are not counts (0 / 0 -> 0: an empty class is exactly 0); the counts must
    be exact"""
    row = np.asarray(row, float)
    assert np.array_equal(row[:, :, 0], ref["sums"][:, :, 0]), (row[:, :, 0], ref["sums"][:, :, 0])
    err, bnd = np.abs(row[:, :, 1:] - ref["sums"][:, :, 1:]), moment_bound(ref)[:, :, 1:]
    assert not (err[bnd == 0.0] != 0.0).any()
    return float(np.max(np.where(bnd > 0.0, err / np.where(bnd > 0.0, bnd, 1.0), 0.0)))


def check_run(sim, ref_run, steps, energy_steps=(), what=""):
    """The rows of `sim` against the reference over `ref_run` (a dense-history run or the oracle of the same case) at `steps`:
    moments within their bounds, counts exact, the energy within its bound at `energy_steps` and NaN elsewhere.  Prints and
    returns the worst ratios (moments, energy)."""
    worst_m = worst_w = 0.0
    esteps = set(int(q) for q in energy_steps)
    for i in steps:
        ref = reference(ref_run, i, energy=i in esteps)
        worst_m = max(worst_m, moment_ratio(sim.integral_sums[i], ref))
        if i in esteps:
            worst_w = max(worst_w, abs(sim.wake_energy[i] - ref["W"]) / ref["W_bound"])
    print(f"{what}: worst |error| / bound over {len(list(steps))} steps: moments {worst_m:.2e}, energy {worst_w:.2e} "
          f"({len(esteps)} samples)")
    assert worst_m <= 1.0, worst_m
    assert worst_w <= 1.0, worst_w
    unsampled = np.ones(sim.nt, bool)
    unsampled[sorted(esteps)] = False
    assert np.isnan(sim.wake_energy[unsampled]).all() and np.isfinite(sim.wake_energy[~unsampled]).all()
    return worst_m, worst_w


def window_steps(win, nt):
    first, stop, every = win
    return list(range(first, min(stop, nt), every))


def class_census(run, steps):
    """int [4, 2]: the largest count every (class, sign) reaches over `steps` -- a case is asserted to fill what it claims to"""
    return np.max([reference(run, i, energy=False)["sums"][:, :, 0] for i in steps], axis=0).astype(int)


# ---- a float64 model of the rows, into which faults can be planted ---------------------------------------------------------------
FAULTS = ("tev_lev_swapped", "bound_dropped", "rows_shifted", "sign_flipped_at_zero", "self_terms_left_out")


def model_row(run, i, fault=None):
    """(sums [4, 2, 6], W) of step i as plain float64 NumPy forms them from the run's own sources, with one fault planted:
    tev_lev_swapped       the tags of the TEVs and the LEVs exchanged
    bound_dropped         the bound vortices left out of the sums and of W
    rows_shifted          (see model_rows: row i holds step i - 1)
    sign_flipped_at_zero  slot 0 is G > 0 and slot 1 is G <= 0
    self_terms_left_out   W without its a = b terms"""
    g, x, z, cls = sources_and_classes(run, i)
    if fault == "tev_lev_swapped":
        cls = np.where(cls == TEV, LEV, np.where(cls == LEV, TEV, cls))
    if fault == "bound_dropped":
        keep = cls != BOUND
        g, x, z, cls = g[keep], x[keep], z[keep], cls[keep]
    neg = (g <= 0.0) if fault == "sign_flipped_at_zero" else (g < 0.0)
    t = np.stack([np.ones_like(g), g, g * x, g * z, g * (x * x + z * z), g * g])
    row = np.zeros([4, 2, 6])
    for c in range(4):
        for s in range(2):
            row[c, s] = t[:, (cls == c) & (neg == bool(s))].sum(axis=1)
    dx, dz = x[:, None] - x[None, :], z[:, None] - z[None, :]
    r2 = dx * dx + dz * dz
    pair = g[:, None] * g[None, :] / (4 * np.pi) * np.log((r2 + np.sqrt(r2 * r2 + float(run.v_core) ** 4)) / 2)
    if fault == "self_terms_left_out":
        np.fill_diagonal(pair, 0.0)
    return row, 0.5 * pair.sum()


def model_rows(run, steps, fault=None):
    """{step: (sums, W)}; rows_shifted: row i is step i - 1's"""
    return {i: model_row(run, i - 1 if fault == "rows_shifted" else i, fault) for i in steps}


def model_misses(run, rows):
    """the steps at which a model row leaves its bounds (or miscounts), and those at which its W does"""
    bad_m, bad_w = [], []
    for i, (row, W) in rows.items():
        ref = reference(run, i)
        err, bnd = np.abs(row - ref["sums"]), moment_bound(ref)
        if not np.array_equal(row[:, :, 0], ref["sums"][:, :, 0]) or (err[:, :, 1:] > bnd[:, :, 1:]).any():
            bad_m.append(i)
        if abs(W - ref["W"]) > ref["W_bound"]:
            bad_w.append(i)
    return bad_m, bad_w


# ---- the per-step path without a GPU ---------------------------------------------------------------------------------------------
class FieldFakeEngine(FakeEngine):
    """tests/fake_engine.py plus Engine.scalar_field('psi') in float64 NumPy: what the per-step path takes the energy from"""

    def scalar_field(self, kind, circulation, xw, zw, xp, zp, v_core, precision="f64"):
        assert kind == "psi"
        g, xw, zw, xp, zp = (np.asarray(a, float) for a in (circulation, xw, zw, xp, zp))
        dx, dz = xp[:, None] - xw[None, :], zp[:, None] - zw[None, :]
        r2 = dx * dx + dz * dz
        return (g[None, :] / (4 * np.pi) * np.log((r2 + np.sqrt(r2 * r2 + float(v_core) ** 4)) / 2)).sum(axis=1)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def mixed_cloud(n=1100, seed=11):
    """about n free vortices of mixed sign in front of the foil (which starts at x in [-0.25, 0.75] and moves towards -x)"""
    rng = np.random.default_rng(seed)
    return dict(circulation_freevort=rng.normal(0.0, 0.01, n),
                xy_freevort=np.stack([rng.uniform(-4.0, -1.0, n), rng.uniform(-1.0, 1.0, n)]))
