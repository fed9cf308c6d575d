"""Shared by tests/test_survey_gradient_host.py and tests/test_gpu_survey_gradient.py: the five gradient terms of a sampled step
in np.longdouble (from tests/gradient_common.py's closed forms -- nothing from the product), their sums in step order, the error
measures with their bounds, and the checks of a gradient survey's derived attributes.

    ux = du/dx,   e = (du/dz + dw/dx) / 2,   om = dw/dx - du/dz,   Q = om^2 / 4 - ux^2 - e^2 = -ux^2 - du/dz dw/dx

Bounds, with gmax = max(|ux|, |uz|, |wx|) over the sampled steps and points:
    means of ux, e, om      1e-9 of gmax: the bound tests/test_gpu_tracer_gradient.py uses for the same construction (float64 sums over
                            the sources a run names itself, against the long-double closed form)
    means of om^2 and Q     3e-9 of gmax^2, by tests/survey_common.py's product rule for a product of two terms that are each
                            within 1e-9 of the scale: |ab - a'b'| <= |a||b - b'| + |b'||a - a'| <= 2e-9 gmax^2, and the
                            1e-18 term"""
import numpy as np

import gradient_common as GC
from gradient_common import LD

MEAN_BOUND = 1e-9               # of max|grad u|
SQUARE_BOUND = 3e-9             # of max|grad u|^2
NAMES = ("ux", "e", "omega", "omega2", "q")


def terms_from_gradient_ld(ux, uz, wx):
    """(ux, e, om, om^2, Q) in np.longdouble from the three components."""
    ux, uz, wx = (np.asarray(a, LD) for a in (ux, uz, wx))
    e, om = (uz + wx) / 2, wx - uz
    return ux, e, om, om * om, om * om / 4 - ux * ux - e * e


def all_sources(sources):
    """(g, x, z) of a step from tracers_common's (g_wake, x, z, g_foil, x, z)."""
    gw, xs, zs, gf, xf, zf = sources
    return np.concatenate([gw, gf]), np.concatenate([xs, xf]), np.concatenate([zs, zf])


def step_terms(sources, px, pz, v_core, rows=256):
    """-> (terms float64 [5, K] rounded from np.longdouble, max(|ux|, |uz|, |wx|) of the step): `rows` points at a time."""
    g, x, z = all_sources(sources)
    px, pz = np.asarray(px, float).reshape(-1), np.asarray(pz, float).reshape(-1)
    out, gmax = np.zeros([5, len(px)]), 0.0
    for lo in range(0, len(px), rows):
        sl = slice(lo, lo + rows)
        (ux, uz, wx), _ = GC.reference_ld(g, x, z, px[sl], pz[sl], v_core)
        for k, term in enumerate(terms_from_gradient_ld(ux, uz, wx)):
            out[k, sl] = term
        gmax = max(gmax, float(max(np.abs(ux).max(), np.abs(uz).max(), np.abs(wx).max())))
    return out, gmax


def reference_sums(steps, points_of, sources_of, v_core):
    """-> (gsums [5, K], gmax, per-step terms {i: [5, K]}): the five terms of every step of `steps` at points_of(i) over
    sources_of(i), added in step order."""
    total, gmax, per = None, 0.0, {}
    for i in steps:
        px, pz = points_of(i)
        t, m = step_terms(sources_of(i), px, pz, v_core)
        per[i] = t
        total = t.copy() if total is None else total + t
        gmax = max(gmax, m)
    return total, gmax, per


def sums_errors(gsums, ref, n, gmax):
    """-> (error of the means of ux, e, om over gmax, error of the means of om^2 and Q over gmax^2)."""
    gsums, ref = np.asarray(gsums).reshape(5, -1), np.asarray(ref).reshape(5, -1)
    d = np.abs(gsums - ref) / n
    return d[:3].max() / gmax, d[3:].max() / gmax ** 2


def check_derived(sim):
    """The attributes of a gradient survey against its own raw sums and the velocity survey's moments."""
    n, g = sim.survey_count, sim.survey_grad_sums
    assert g.shape == (5,) + sim.survey_x.shape
    ux, e, om = g[0] / n, g[1] / n, g[2] / n
    assert np.array_equal(sim.survey_mean_ux, ux) and np.array_equal(sim.survey_mean_strain, e)
    assert np.array_equal(sim.survey_mean_omega, om)
    assert np.array_equal(sim.survey_mean_uz, e - 0.5 * om) and np.array_equal(sim.survey_mean_wx, e + 0.5 * om)
    assert np.array_equal(sim.survey_omega2, g[3] / n) and np.array_equal(sim.survey_mean_q, g[4] / n)
    assert np.array_equal(sim.survey_omega_var, g[3] / n - om * om)
    assert np.array_equal(sim.survey_production, -(sim.survey_uu * ux + sim.survey_uw * (2.0 * e) - sim.survey_ww * ux))


def check_bin_derived(sim):
    """Likewise for the bins; coherent + random is the variance of omega over the binned samples at 1e-12 of max<omega^2>."""
    B, shape = sim.survey_nbins, sim.survey_x.shape
    g, n = sim.survey_bin_grad_sums, sim.survey_bin_count
    assert g.shape == (B, 5) + shape
    for b in range(B):
        if n[b] == 0:
            assert np.isnan(sim.survey_bin_mean_omega[b]).all() and np.isnan(sim.survey_bin_mean_q[b]).all()
            continue
        for name, c in (("mean_ux", 0), ("mean_strain", 1), ("mean_omega", 2), ("omega2", 3), ("mean_q", 4)):
            assert np.array_equal(getattr(sim, "survey_bin_" + name)[b], g[b, c] / n[b]), (name, b)
    N = int(n.sum())
    tot = g.sum(axis=0)
    ref = tot[3] / N - (tot[2] / N) ** 2
    got = sim.survey_coherent_omega2 + sim.survey_random_omega2
    assert got.shape == shape and np.abs(got - ref).max() <= 1e-12 * np.abs(tot[3] / N).max()
