"""Shared by tests/test_ensemble_integrals_host.py and tests/test_gpu_ensemble_integrals.py: the wake integrals of a sweep member
 against the reference and the bounds of the solo observer, which are imported from
tests/wake_integrals_common.py and not restated:

    moments   |sum - ref| <= (ns + 16) 2^-52 sum |term|, counts exact          (moment_bound, moment_ratio)
    W         |W - ref|   <= 1/2 sum_a |G_a| B_a + the summation term          (reference()["W_bound"])

The reference is over the member's OWN sources.  A member keeps its wake at snapshot_steps only, so the sweep under test is run
with snapshot_steps=range(1, nt): its `path` then holds every step, SparseHistory takes the indexing of the dense arrays, and
`wake_integrals_common.sources_and_classes` / `tracers_common.run_sources` build step i's sources from the member exactly as
they do from a dense-history run (`dense_snapshots`, `check_member`).  No twin is needed for the by-value tests.

Only the comparison of a member with its SOLO march (two runs, two wakes) needs more: both are within their own bounds of their
own references, and the two references differ by what the two wakes differ.  `twin_term` bounds that difference for sources
that agree to DELTA = 1e-12 in x, z and G -- the agreement tests/test_gpu_ensemble_survey_grad.py's
assert_twin_and_member_agree asserts of positions, and `assert_circulations_agree` below of G -- from the derivatives of the
terms:

    G          dG                                   G x            |G| dx + |x| dG          (G z likewise)
    G (x^2 + z^2)   2 |G| (|x| + |z|) d + (x^2 + z^2) d            G^2            2 |G| d
    W = 1/2 sum_a G_a psi_a:  dW/dG_a = psi_a,  |dW/dx_a| + |dW/dz_a| = |G_a| (|u_a| + |w_a|) <= |G_a| 2 sum_b |G_b| / (2 pi sqrt(2) v_core)
                              (the Vatistas kernel r / sqrt(r^4 + vc^4) is at most 1 / (sqrt(2) vc))
"""
import numpy as np

from wake_integrals_common import (BOUND, FREE, LEV, TEV, check_run, class_census, mixed_cloud, moment_bound, moment_ratio,  # noqa: F401
                                   reference, sources_and_classes, window_steps)

DELTA = 1e-12
ATTRS = ("integral_sums", "wake_energy")
PROPERTIES = ("wake_impulse", "wake_angular_impulse", "impulse_force", "impulse_Cl", "impulse_Cd", "wake_energy_interaction")


def W_bound(ref):
    """the energy bound of a reference (formed in wake_integrals_common.reference)"""
    return ref["W_bound"]


def dense_snapshots(nt):
    """snapshot_steps under which a member's path holds every step (at most 1024 of them)"""
    return range(1, nt)


def check_member(member, energy_steps=(), what="", steps=None):
    """Every row 1 .. nt - 1 of a member (or `steps`) against the reference over its own sources: moments within their bounds,
    counts exact, W within its bound at `energy_steps` and NaN elsewhere.  -> the worst ratios (moments, energy)."""
    steps = range(1, member.nt) if steps is None else steps
    return check_run(member, member, steps, energy_steps, what)


def lagged_misses(member, steps, energy_steps):
    """The planted fault: the reference over the sources of step i - 1 taken for step i's.  -> (worst moment miss, worst energy
    miss) in units of step i's bounds; a bound that can see a fault gives more than 10 for both."""
    worst_m = worst_w = 0.0
    esteps = set(int(q) for q in energy_steps)
    for i in steps:
        if i < 2:
            continue
        ref, late = reference(member, i, energy=i in esteps), reference(member, i - 1, energy=i in esteps)
        err, bnd = np.abs(late["sums"][:, :, 1:] - ref["sums"][:, :, 1:]), moment_bound(ref)[:, :, 1:]
        worst_m = max(worst_m, float(np.max(np.where(bnd > 0.0, err / np.where(bnd > 0.0, bnd, 1.0), 0.0))))
        if i in esteps:
            worst_w = max(worst_w, abs(late["W"] - ref["W"]) / W_bound(ref))
    return worst_m, worst_w


def assert_circulations_agree(a, b, label=""):
    """every shed and bound circulation of two runs of one case to DELTA (positions: assert_twin_and_member_agree)"""
    for key in ("TEV", "LEV", "airfoil"):
        x, y = np.asarray(a.circulation[key], float), np.asarray(b.circulation[key], float)
        assert x.shape == y.shape and (x.size == 0 or np.abs(x - y).max() <= DELTA), (label, key)


def twin_term(run, i, energy):
    """-> (float64 [4, 2, 6], float): how far the long-double sums and W of step i can move when every source moves by at most
    DELTA in x, z and G (the module's docstring); the counts' entry is 0."""
    g, x, z, cls = sources_and_classes(run, i)
    ag, ax, az = np.abs(g), np.abs(x), np.abs(z)
    r2 = x * x + z * z
    t = DELTA * np.stack([np.zeros_like(g), np.ones_like(g), ag + ax, ag + az, 2 * ag * (ax + az) + r2, 2 * ag])
    out, neg = np.zeros([4, 2, 6]), g < 0.0
    for c in range(4):
        for s in range(2):
            out[c, s] = t[:, (cls == c) & (neg == bool(s))].sum(axis=1)
    w = 0.0
    if energy:
        vc = float(run.v_core)
        # |psi_a| <= sum_b |G_b| |ln((r^2 + s) / 2)| / (4 pi) with the logarithm's size bounded over the cloud's extent
        span = 2.0 * (np.ptp(x) + np.ptp(z)) ** 2 + vc * vc + 2.0
        lnmax = max(abs(np.log(vc * vc / 2.0)), abs(np.log(span)))
        psi_max = ag.sum() * lnmax / (4 * np.pi)
        vel_max = 2.0 * ag.sum() / (2 * np.pi * np.sqrt(2.0) * vc)
        w = DELTA * float((psi_max + ag * vel_max).sum()) * 0.5 * 2.0       # (W is bilinear in G: both factors move)
    return out, w

