"""Shared by tests/test_survey_bins_host.py and tests/test_gpu_survey_bins.py: the integer phase rule, the reduction of a run's
own probe rows over the steps of each bin, and the checks of a binned survey's derived attributes."""
import numpy as np

from survey_common import MEAN_VS_PROBES, MOMENT_VS_PROBES, series_sums, series_umax, sums_errors


def integer_phase_rule(steps, steps_per_period, B):
    """The bin of time step i when a period is a whole number of steps."""
    i = np.asarray(steps, dtype=np.int64)
    return ((i % steps_per_period) * B // steps_per_period) % B


def steps_of_bin(sim, b):
    return [int(i) for i in np.flatnonzero(sim.survey_bin_of_step == b)]


def check_bins_against_probes(sim, label=""):
    """Every bin's sums against the reduction of probe_u / probe_w (probes at the survey's points) over that bin's steps, at
    the two probe bounds; the counts against the table."""
    sampled = [int(i) for i in np.flatnonzero(sim.survey_bin_of_step >= 0)]
    umax = series_umax(sim.probe_u, sim.probe_w, sampled)
    worst = [0.0, 0.0]
    for b in range(sim.survey_nbins):
        W = steps_of_bin(sim, b)
        assert sim.survey_bin_count[b] == len(W), b
        if not W:
            continue
        e_mean, e_mom = sums_errors(sim.survey_bin_sums[b], series_sums(sim.probe_u, sim.probe_w, W), len(W), umax)
        worst = [max(worst[0], e_mean), max(worst[1], e_mom)]
    print(f"{label}: bins vs the run's own probe rows: means {worst[0]:.2e} of max|u|, raw second moments {worst[1]:.2e} of max|u|^2")
    assert worst[0] <= MEAN_VS_PROBES, worst
    assert worst[1] <= MOMENT_VS_PROBES, worst


def check_bin_derived(sim):
    """The attributes of a binned survey against its own raw bin sums: shapes, the means and central moments within each bin
    (nan for an empty bin), and coherent + random = the total central moments of the binned samples at 1e-12 of max|u|^2."""
    B, shape = sim.survey_nbins, sim.survey_x.shape
    s, n = sim.survey_bin_sums, sim.survey_bin_count
    assert s.shape == (B, 5) + shape and n.shape == (B,) and n.dtype == np.int64
    for b in range(B):
        if n[b] == 0:
            assert np.isnan(sim.survey_bin_mean_u[b]).all() and np.isnan(sim.survey_bin_uw[b]).all()
            continue
        mu, mw = s[b, 0] / n[b], s[b, 1] / n[b]
        assert np.array_equal(sim.survey_bin_mean_u[b], mu) and np.array_equal(sim.survey_bin_mean_w[b], mw)
        assert np.array_equal(sim.survey_bin_uu[b], s[b, 2] / n[b] - mu * mu)
        assert np.array_equal(sim.survey_bin_ww[b], s[b, 3] / n[b] - mw * mw)
        assert np.array_equal(sim.survey_bin_uw[b], s[b, 4] / n[b] - mu * mw)
    N = int(n.sum())
    tot = s.sum(axis=0)
    mu, mw = tot[0] / N, tot[1] / N
    total = {"uu": tot[2] / N - mu * mu, "ww": tot[3] / N - mw * mw, "uw": tot[4] / N - mu * mw}
    umax2 = max(np.abs(tot[2]).max(), np.abs(tot[3]).max()) / N        # max of the mean squares: <= max|u|^2 over the samples
    for key, ref in total.items():
        got = getattr(sim, "survey_coherent_" + key) + getattr(sim, "survey_random_" + key)
        assert got.shape == shape
        assert np.abs(got - ref).max() <= 1e-12 * umax2, key
    return total, umax2
