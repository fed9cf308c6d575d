"""Shared by tests/test_survey_host.py and tests/test_gpu_survey.py: the sampled steps of a window, the five raw sums of a
velocity series (the oracle's, or a run's own probe rows), the error measures and the oracle cases."""
import numpy as np

from conftest import CONFIG1, load_golden
from probes_common import ProbedOracle

# (method, frame, with G5's free-vortex cloud)
ORACLE_CASES = [("Faure", "lab", False), ("Faure", "tunnel", False), ("Ramesh", "lab", False), ("Ramesh", "tunnel", False),
                ("Faure", "lab", True), ("Faure", "tunnel", True)]
CASE_IDS = [f"{m}-{f}{'-cloud' if c else ''}" for m, f, c in ORACLE_CASES]

MEAN_VS_ORACLE = 1e-9           # of max|u|: the project's bound for the oracle series
MOMENT_VS_ORACLE = 3e-9         # of max|u|^2: |ab - a'b'| <= |a||b - b'| + |b'||a - a'| <= 2e-9 max|u|^2, and the 1e-18 term
MEAN_VS_PROBES = 1e-12          # of max|u|: the project's bound for probe against tracer at one point
MOMENT_VS_PROBES = 3e-12        # of max|u|^2, by the same product rule


def gust_cloud():
    """G5's free vortices as constructor keywords."""
    g = load_golden("g5_freevort.npz")
    return dict(circulation_freevort=g["gamma_freevort"], xy_freevort=g["xy_freevort"])


def case_keywords(method, cloud, tf=2.5):
    kw = dict(CONFIG1, tf=tf, method=method)
    if cloud:
        kw.update(gust_cloud())
    return kw


def window(first, stop, every, nt):
    """The sampled steps: first <= i < min(stop, nt), (i - first) % every == 0."""
    return list(range(first, min(stop, nt), every))


def series_sums(u, w, steps):
    """[5, P]: sum u, sum w, sum u^2, sum w^2, sum u w over rows `steps` of the series u, w [nt, P], added in step order."""
    out = np.zeros([5, u.shape[1]])
    for i in steps:
        for acc, term in zip(out, (u[i], w[i], u[i] * u[i], w[i] * w[i], u[i] * w[i])):
            acc += term
    return out


def oracle_series(pts, method, frame, cloud, tf=2.5):
    """-> (u, w) [nt, P]: ProbedOracle's series at `pts` [2, P]."""
    shift = (lambda o: o.xpiv) if frame == "tunnel" else None
    return ProbedOracle(pts, shift=shift, **case_keywords(method, cloud, tf)).series()


def sums_errors(sums, ref, n, umax):
    """-> (means' error / max|u|, raw second moments' error / max|u|^2) of the sums [5, ...] over n samples against `ref`."""
    sums, ref = np.asarray(sums).reshape(5, -1), np.asarray(ref).reshape(5, -1)
    d = np.abs(sums - ref) / n
    return d[:2].max() / umax, d[2:].max() / umax ** 2


def series_umax(u, w, steps):
    return max(np.abs(u[steps]).max(), np.abs(w[steps]).max())


def check_derived(sim):
    """The attributes a run with a survey carries, against its own raw sums."""
    n, s = sim.survey_count, sim.survey_sums
    assert s.shape == (5,) + sim.survey_x.shape == (5,) + sim.survey_z.shape
    mu, mw = s[0] / n, s[1] / n
    assert np.array_equal(sim.survey_mean_u, mu) and np.array_equal(sim.survey_mean_w, mw)
    assert np.array_equal(sim.survey_uu, s[2] / n - mu * mu) and np.array_equal(sim.survey_ww, s[3] / n - mw * mw)
    assert np.array_equal(sim.survey_uw, s[4] / n - mu * mw)
