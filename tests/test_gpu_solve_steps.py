"""GPU tier: every time-step SOLVE of a time loop, checked by value (tests/solve_steps_common.py).

A run that holds the wake before every step is taken apart step by step: from row i - 1 and the run's own circulations the
host rebuilds the placements, the downwash terms (float64 pair sums), the exact solution of the step's linear conditions, the
Fourier rows, the bound vorticity and the loads (their chord velocity from a direct pair sum), and step i's stored results must
be those to the bounds of the common module -- 64 x the host floor, not below the 1e-12 float64 contract -- at EVERY step,
whatever the flow has amplified by then; the shedding decision must be the host's.  The solve reads the float64 masters, so the
bounds are the same in every precision.  The runs go through march_solve (serial and overlapped steps), the sweep's own solve,
the host solve of the per-step path, the chord launch under its stale anchor bound, and the real serial -> overlapped threshold.

Each test prints one line: the worst residual over its bound, where it occurred (step, quantity, wake size before the step), the
smallest decision margin, and the worst residual over its scale per quantity.
"""
import os
import sys

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from observer_sources_common import fast_iv
from oracle import g10_cases, g9_cases
from rollup_common import CLOUDS, case_keywords
import solve_steps_common as S

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sym_rule  # noqa: E402

pytestmark = pytest.mark.gpu

EXEMPT_MARGIN = 1e-8        # real thresholds only: below it a step is exempt from the decision check alone
EXEMPT_SHARE = 0.01         # ... and at most this share of a run's steps


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


def solo(kw, precision, march=True, threshold=None, cls=None, **extra):
    """One run on an engine of its own, dense history."""
    from ludvm_amd import Engine, LUDVM
    e = Engine(0)
    try:
        if threshold is not None:
            e.set_symmetric(threshold)
        return (cls or LUDVM)(**kw, verbose=False, engine=e, precision=precision, history="full", march=march, **extra)
    finally:
        try:
            e.set_symmetric(1)
        finally:
            e.close()


def check_run(label, sim, iv, steps=None, exempt=False):
    """Every checked step of `sim`: residuals within their bounds, the decision the host's, Ramesh's conditions within
    `maxerror`.  exempt: a step whose margin is below 1e-8 may decide either way (at most 1 % of the steps)."""
    steps = range(1, sim.nt) if steps is None else steps
    fails, worst, margin, exempted = [], (-1.0, None, None, None), np.inf, 0
    per_q = {}
    for i in steps:
        s = S.step_solve_residuals(sim, i, iv)
        margin = min(margin, s.margin)
        if s.shed != s.shed_run:
            if exempt and s.margin < EXEMPT_MARGIN:
                exempted += 1
            else:
                fails.append((i, "decision", s.margin, s.n_wake))
        r, q = S.worst(s)
        if r > worst[0]:
            worst = (r, i, q, s.n_wake)
        for k, v in s.res.items():
            per_q[k] = max(per_q.get(k, 0.0), max(v - s.allow.get(k, 0.0), 0.0) / s.scale[k])
        over = S.over_bound(s)
        if over:
            fails.append((i, over, s.n_wake))
        if s.newton and not (s.newton["kelvin"] <= sim.maxerror and s.newton["lesp_cond"] <= sim.maxerror):
            fails.append((i, "newton", s.newton))
    print(f"{label}: worst residual / bound {worst[0]:.2e} at step {worst[1]} ({worst[2]}, wake {worst[3]}), {len(steps)} steps, "
          f"smallest margin {margin:.2e}, exempt {exempted}; residual / scale: "
          + ", ".join(f"{k} {v:.1e}" for k, v in per_q.items()))
    assert not fails, fails[:6]
    assert exempted <= EXEMPT_SHARE * len(steps)


# ---- solo, dense history, config 1 over all 400 steps ----------------------------------------------------------------------
@pytest.mark.parametrize("path", ["serial", "overlapped", "per-step"])
@pytest.mark.parametrize("precision", ["f64", "f32", "f32x2"])
@pytest.mark.parametrize("method", ["Faure", "Ramesh"])
def test_config1_every_step(method, precision, path, iv):
    """The README case (wake 1 -> 603).  serial: the march with the direct kernels; overlapped: set_symmetric(64), the chain beside
    the symmetric kernel once the wake's lower bound passes 64 (fp32 precisions; 'f64' stays serial); per-step: march=False, the
    solve in its host matrix form."""
    sim = solo(dict(CONFIG1, method=method), precision, march=path != "per-step", threshold=64 if path == "overlapped" else None)
    assert sim.nt == 401
    check_run(f"config1 {method} {precision} {path}", sim, iv)


@pytest.mark.parametrize("name", CLOUDS)
def test_cloud_cases_every_step(name, iv):
    """100 marched 'f32' steps behind 150 .. 397 free vortices: the chord launch with two and with four source splits."""
    sim = solo(case_keywords(name), "f32")
    assert sim.nt == 101
    check_run(f"{name} Faure f32 march", sim, iv)


@pytest.mark.parametrize("method", ["Faure", "Ramesh"])
def test_cambered_off_unit_case_every_step(method, iv):
    """G10's c4412d (NACA 4412, chord 2, Uinf 3, rho 0.9), marched: the camber row of the downwash, every power of chord and
    Uinf in the solve and the loads, Faure's A0 without 1 / Uinf on a shedding step against Ramesh's with it."""
    kw = g10_cases.kwargs(g10_cases.BY_NAME["c4412d"], method=method)
    sim = solo(kw, "f64")
    assert sim.nt == 201 and sim.chord == 2 and sim.Uinf == 3
    check_run(f"c4412d {method} f64 march", sim, iv)


# ---- the sweep's own solve ------------------------------------------------------------------------------------------------
def check_members(label, sims, iv):
    for m, sim in enumerate(sims):
        rows = set(sim.path["TEV"].steps())
        assert rows >= set(range(sim.nt - 1)), (label, m)
        check_run(f"{label} member {m} ({sim.method}, {sim.nt - 1} steps)", sim, iv)


def test_sweep_of_mixed_members_every_step(iv):
    """One sweep of 'Faure' and 'Ramesh' members of config 1 and of the off-unit c4412d, a snapshot at every step: step s + 1 is
    checked from row s for every s."""
    from ludvm_amd import Engine, LUDVM, _ffi
    c = g10_cases.BY_NAME["c4412d"]
    cases = [dict(CONFIG1, method="Faure"), dict(CONFIG1, method="Ramesh"), g10_cases.kwargs(c, method="Ramesh"),
             g10_cases.kwargs(c, method="Faure")]
    assert 400 <= _ffi.ENSEMBLE_MAX_SNAPSHOTS
    e = Engine(0)
    try:
        sims = LUDVM.sweep(cases, engine=e, snapshot_steps=range(1, 401))
    finally:
        e.close()
    assert [s.nt for s in sims] == [401, 401, 201, 201]
    check_members("sweep", sims, iv)


@pytest.mark.parametrize("name", ["a2-4", "a256-64"])
def test_sweep_at_the_ends_of_the_panel_range(name, iv):
    """Npoints - 1 = 2 and 256, the ends of G9's panel range: 100 steps behind 120 free vortices, both methods in one sweep."""
    from ludvm_amd import Engine, LUDVM
    c = g9_cases.BY_NAME[name]
    e = Engine(0)
    try:
        sims = LUDVM.sweep([g9_cases.kwargs(c, m) for m in ("Faure", "Ramesh")], engine=e, snapshot_steps=range(1, 101))
    finally:
        e.close()
    assert [s.nt for s in sims] == [101, 101] and sims[0].Npoints - 1 == c["npan"]
    check_members(f"sweep {name}", sims, iv)


# ---- the real thresholds --------------------------------------------------------------------------------------------------
BIG_STEPS = 450
BIG_SEED = 9911
A_NFREE = g9_cases.A_NFREE       # the cloud's strengths are scaled to the total of G9's 120 vortices


def big_case(method="Faure"):
    """Config 1 behind a free cloud that puts the wake's lower bound across kSymMinNMarch (asked of the library's rule, not
    copied) inside a 450-step run; strengths scaled by 120 / nfree, so the cloud's field stays of the order of G9's."""
    thr = sym_rule.constants()["kSymMinNMarch"]
    nfree = thr - 264
    g, xy = g9_cases.free_cloud(BIG_SEED, nfree)
    return thr, dict(CONFIG1, tf=(BIG_STEPS - 0.5) * CONFIG1["dt"], method=method,
                     circulation_freevort=g * (A_NFREE / nfree), xy_freevort=xy)



def march_geometry(sim, thr):
    """(forked[], anchors[]) per step from the wake sizes the run reports: step s is sized from the anchor step
    A(s) = max(64 (s // 64 - 2) - 1, 0) (Engine.march_anchor_steps) and is overlapped once n_lo = n(A) + (s - 1 - A) >= thr."""
    shed = np.asarray(sim.LEV_shed) != -1
    n_after = sim.path["FREE"].shape[2] + np.arange(sim.nt) + np.cumsum(shed)
    anchors = np.array([max(64 * (s // 64 - 2) - 1, 0) for s in range(sim.nt)])
    n_lo = n_after[anchors] + (np.arange(sim.nt) - 1 - anchors)
    forked = n_lo >= thr
    forked[0] = False
    return forked, anchors, n_after


RESULTS = ("Fn", "Fs", "L", "D", "M", "LESP", "LESP_prev", "LEV_shed", "fourier")


def same_bits(a, b):
    for k in RESULTS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("TEV", "LEV", "bound", "airfoil", "gamma_airfoil"):
        assert np.array_equal(a.circulation[k], b.circulation[k]), k
    for k in ("TEV", "LEV", "FREE"):
        assert np.array_equal(a.path[k], b.path[k]), k


@pytest.fixture(scope="module")
def big_whole(iv):
    """The 'f32' run in one call of ludvm_march_run per 512 steps (the default of a dense history)."""
    thr, kw = big_case()
    return thr, solo(kw, "f32")


def test_real_threshold_in_one_call(big_whole, iv):
    """A marched 'f32' run with default thresholds whose wake crosses kSymMinNMarch: serial steps, the first forked step and
    more than 100 overlapped ones, past four anchor renewals -- every chord launch planned from an anchor up to 192 steps old."""
    thr, sim = big_whole
    assert sim.nt == BIG_STEPS + 1 and sim.precision == "f32"
    forked, anchors, n_after = march_geometry(sim, thr)
    first = int(np.argmax(forked))
    assert forked.any() and first > 64 and not forked[1:first].any() and forked[first:].all(), first
    assert forked.sum() >= 100 and len(set(anchors[1:])) >= 5 and sim.nt - 1 > 320
    assert n_after[0] < thr < n_after[-1]
    # the launch rule takes the symmetric kernel at the first forked step's size
    assert sym_rule.rule([int(n_after[anchors[first]] + 2 * (first - anchors[first]))], march=True)[0].symmetric
    check_run(f"big f32 whole (first forked step {first}, {int(forked.sum())} overlapped)", sim, iv, exempt=True)


@pytest.mark.parametrize("every,begins", [(127, (128, 192)), (255, (256, 320, 384, 448))])
def test_real_threshold_cut_into_calls(every, begins, big_whole, iv, tmp_path):
    """The same run cut into calls of at most 64 steps that also end at every checkpoint: they begin on multiples of 64
    (`begins`) and off them.  Identical bits, asserted here at this size -- and the checker passes on the cut run itself."""
    from ludvm_amd import LUDVM
    thr, whole = big_whole
    _, kw = big_case()

    class Cut(LUDVM):
        _march_chunk = 64
        calls = []

        def _march_call(self, S, i, j, rec_i, print_dt):
            Cut.calls.append(i)
            return super()._march_call(S, i, j, rec_i, print_dt)

    Cut.calls = []
    sim = solo(kw, "f32", cls=Cut, checkpoint_every=every, checkpoint_path=str(tmp_path / "ck.npz"))
    assert set(begins) <= set(Cut.calls) and sum(c % 64 != 0 for c in Cut.calls) >= 3, Cut.calls
    same_bits(sim, whole)
    check_run(f"big f32 cut (checkpoint_every {every}, calls begin at {Cut.calls})", sim, iv, exempt=True)


def test_real_threshold_f64_all_serial(iv):
    """The same case in 'f64': every step serial, the direct float64 kernel."""
    thr, kw = big_case()
    sim = solo(kw, "f64")
    assert sim.nt == BIG_STEPS + 1
    check_run("big f64", sim, iv, exempt=True)


def test_real_threshold_ramesh(iv):
    """The same case with Ramesh's Newton in march_solve, 'f32'."""
    thr, kw = big_case("Ramesh")
    sim = solo(kw, "f32")
    forked, _, _ = march_geometry(sim, thr)
    assert forked.sum() >= 100 and not forked[1:65].any()
    check_run("big f32 Ramesh", sim, iv, exempt=True)
