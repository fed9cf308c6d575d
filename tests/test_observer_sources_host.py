"""CPU tier of tests/test_gpu_observer_sources.py: what its references and its shapes rest on (observer_sources_common.py).
The full Python oracle of case A licenses `run_sources` + a float64 pair sum as the reference of cases B and C, where the
oracle itself is too slow (its cost is quadratic in the cloud); no source of any case is too weak for the bounds to see it
dropped or doubled; and the reference's own sensitivity to the order of summation lies far under the bounds."""
import numpy as np
import pytest

from observer_sources_common import (CASES, PROBE_VS_SOURCES, SETS, CaseAOracle, case_keywords, cloud, euler_step_by, field,
                                     observers, sorted_sources, survey_sample, weakest_contribution)
from oracle import c_oracle, ludvm_oracle as O
from probes_common import ProbedOracle, probes32
from tracers_common import euler_step, run_sources

SEEN_FACTOR = 1e3               # a single source's contribution over the tolerance
ORDER_BOUND = 1e-11             # of max|u|: a factor 100 under PROBE_VS_SOURCES


@pytest.fixture(scope="module")
def oracle_a():
    return CaseAOracle()


def test_no_lev_is_shed_in_case_a_and_the_wake_grows_by_one_per_step(oracle_a):
    ref = oracle_a.ref
    nfree, steps = CASES["A"][:2]
    assert ref.nt == steps + 1 and (np.asarray(ref.LEV_shed) == -1).all()
    for i in range(1, ref.nt):
        gw, _, _, gf, _, _ = ref.sources[i]
        # (the reference's wake gather carries one unshed LEV slot of zero circulation)
        assert np.count_nonzero(gw) == nfree + i and len(gf) == 80, i


def test_run_sources_on_the_oracle_gives_the_oracles_own_sources(oracle_a):
    """`run_sources` reads a dense history; TracedOracle notes what the roll-up was called with.  Steps 2-24 of case A, up to
    order and without the reference's unshed LEV slot (zero circulation): 1e-15 absolute (measured 1.4e-17: the placement of
    the shed vortex is recomputed)."""
    ref = oracle_a.ref
    worst = 0.0
    for i in range(2, ref.nt):
        gw, xs, zs, gf, xf, zf = ref.sources[i]
        keep = gw != 0.0
        assert np.count_nonzero(~keep) == 1, i
        g, x, z, g2, x2, z2 = run_sources(ref, i)
        assert len(g) == np.count_nonzero(keep) and np.array_equal(g2, gf) and np.array_equal(x2, xf) and np.array_equal(z2, zf), i
        worst = max(worst, np.abs(sorted_sources(g, x, z) - sorted_sources(gw[keep], xs[keep], zs[keep])).max())
    print(f"case A: run_sources on the oracle vs the oracle's roll-up sources, steps 2-24: {worst:.2e} absolute")
    assert worst <= 1e-15, worst


def test_the_helpers_are_the_projects_own_references(oracle_a):
    """`field` over TracedOracle's sources is ProbedOracle's series, and `euler_step_by` is `euler_step`: bit for bit."""
    ou, ow = ProbedOracle(probes32(), **case_keywords("A")).series()
    u, w = oracle_a.series("few")
    assert np.array_equal(u, ou) and np.array_equal(w, ow) and np.abs(ou[0]).max() > 0.0
    ref, obs = oracle_a.ref, oracle_a.obs["few"]
    rows = oracle_a.tracer_rows("few")
    for i in (1, 2, 7, 8, 24):
        cur = None if i == 1 else rows[i - 1]
        a = euler_step_by(O.induced_velocity, obs["tracers"], cur, obs["release"], i, ref.dt, ref.v_core, ref.sources[i])
        b = euler_step(obs["tracers"], cur, obs["release"], i, ref.dt, ref.v_core, ref.sources[i])
        assert np.array_equal(a, b) and np.array_equal(a, rows[i]), i


def test_the_survey_sample_holds_both_ends_of_every_tile():
    pick = survey_sample(20481)
    assert len(pick) <= 1024 and len(np.unique(pick)) == len(pick) and (np.diff(pick) > 0).all()
    for t in range(0, 20481, 512):
        assert t in pick and min(t + 512, 20481) - 1 in pick
    assert np.array_equal(survey_sample(600), np.arange(600))


def _sources(case, oracle_a):
    """The sources the check is made with: case A's last step from the oracle (cloud, wake and bound vortices), the cloud
    alone -- all but about a hundred of the sources -- in B and C."""
    if case == "A":
        gw, xs, zs, gf, xf, zf = oracle_a.ref.sources[CASES["A"][1]]
        keep = gw != 0.0
        return np.concatenate([gw[keep], gf]), np.concatenate([xs[keep], xf]), np.concatenate([zs[keep], zf]), oracle_a.v_core
    c = cloud(CASES[case][0])
    return c["circulation_freevort"], c["xy_freevort"][0], c["xy_freevort"][1], oracle_a.v_core


@pytest.mark.parametrize("case", list(CASES))
def test_no_source_may_go_unseen(oracle_a, case):
    """For every observer kind of both sets: the weakest source's largest single contribution at a checked point is at least
    SEEN_FACTOR x the tolerance x max|u| (measured: 5e-3 of max|u| for the cloud alone at probes32() with n = 1180, 1.3e-3 with
    n = 20390; about 1e-5 with case A's bound vortices in), so a dropped or doubled source cannot pass.  (A tracer's bound
    is taken of its largest displacement, at most steps x dt x max|u|, and one source moves it by dt x its contribution per
    step: the margin there is SEEN_FACTOR / steps >= 35.)  The large sets are sampled (their first 512 points): more points
    can only raise a source's largest contribution."""
    g, x, z, vc = _sources(case, oracle_a)
    steps = CASES[case][1]
    for which in SETS:
        obs = observers(case, which)
        for kind, pts in (("probes", obs["probes"]), ("tracers", obs["tracers"][:, obs["release"] <= steps]),
                          ("survey", obs["survey"][:, obs["pick"]])):
            pts = pts[:, :512]
            u, w = O.induced_velocity(g, x, z, pts[0], pts[1], vc)
            umax = max(np.abs(u).max(), np.abs(w).max())
            weakest = weakest_contribution(g, x, z, pts[0], pts[1], vc)
            need = SEEN_FACTOR * PROBE_VS_SOURCES * umax
            print(f"case {case} {which} {kind}: weakest source's largest contribution {weakest / umax:.2e} of max|u| = {umax:.3e} "
                  f"(needed {need / umax:.1e})")
            assert weakest >= need, (which, kind, weakest, need)


@pytest.mark.parametrize("case", list(CASES))
def test_the_references_own_order_sensitivity_is_far_under_the_bounds(oracle_a, case):
    """The sources summed forwards and backwards at probes32() by the pair sum the GPU tests use for this case: at most
    ORDER_BOUND of max|u| (measured 2.8e-16 for case A's 1284 sources with NumPy's pairwise sum, 8.5e-15 and 7.7e-15 for the
    clouds of B and C with the C oracle's sequential sum)."""
    g, x, z, vc = _sources(case, oracle_a)
    iv = O.induced_velocity if case == "A" or not c_oracle.available() else c_oracle.induced_velocity
    px, pz = probes32()
    fu, fw = iv(g, x, z, px, pz, vc)
    bu, bw = iv(g[::-1].copy(), x[::-1].copy(), z[::-1].copy(), px, pz, vc)
    umax = max(np.abs(fu).max(), np.abs(fw).max())
    err = max(np.abs(fu - bu).max(), np.abs(fw - bw).max()) / umax
    print(f"case {case}: forwards vs backwards sum over {len(g)} sources: {err:.2e} of max|u|")
    assert err <= ORDER_BOUND, err
    assert ORDER_BOUND * 100 <= PROBE_VS_SOURCES


def test_field_adds_the_wake_and_the_bound_vortices(oracle_a):
    """`field` with the C oracle against the NumPy one on case A's last step: 1e-13 of max|u| (the C oracle's own bound)."""
    if not c_oracle.available():
        pytest.skip("oracle/libpair_oracle.so not built")
    src = oracle_a.ref.sources[CASES["A"][1]]
    px, pz = probes32()
    a = field(O.induced_velocity, src, px, pz, oracle_a.v_core)
    b = field(c_oracle.induced_velocity, src, px, pz, oracle_a.v_core)
    umax = max(np.abs(a[0]).max(), np.abs(a[1]).max())
    assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) <= 1e-13 * umax
