"""GPU tier: every fp32 wake roll-up step of a time loop, checked by value (tests/rollup_common.py).

A run with the dense history is taken apart step by step: the sources of step i's roll-up are what the run itself holds in
row i - 1 plus what it shed and solved in step i, and row i must be their float64 pair sums' explicit Euler step to the fp32
contract -- 1e-5 of the step's largest velocity in 'f32' (include/ludvm_hip.h), 3e-6 in 'f32x2' -- at
EVERY step of the run, whatever the flow has amplified by then.  The runs go through the origin-block edge (256 vortices),
the 512 tile edge, a shed pair straddling or opening a block, the last bound vortex opening one, the serial and the
overlapped march, the per-step path, the direct and the symmetric kernel and both of its tiles.

Each test prints one line: the worst residual over its scale, where it occurred (step, family, wake size before the step).
"""
import numpy as np
import pytest

from observer_sources_common import fast_iv
from rollup_common import CLOUDS, case_keywords, check_alignments, euler_slack, step_residuals

pytestmark = pytest.mark.gpu

BOUND = {"f32": 1e-5, "f32x2": 3e-6}      # of the step's scale, every family of every step
PHANTOM_MARCHED = 1e-9                    # the zero-strength LEV slot of a marched step comes from the float64 chord launch


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


def run(name, precision, march, threshold=None, tile=0):
    """One run of case `name` on an engine of its own, dense history."""
    from ludvm_amd import Engine, LUDVM
    e = Engine(0)
    try:
        if threshold is not None:
            e.set_symmetric(threshold)
        if tile:
            e.set_sym_tuning(tile, 0)
        return LUDVM(**case_keywords(name), verbose=False, engine=e, precision=precision, history="full", march=march)
    finally:
        try:
            e.set_symmetric(1)
            e.set_sym_tuning(0, 0)
        finally:
            e.close()


@pytest.fixture(scope="module")
def f64_last_rows():
    """case -> the last TEV row of its 'f64' run (made once per case)."""
    made = {}

    def get(name):
        if name not in made:
            sim = run(name, "f64", True)
            made[name] = sim.path["TEV"][sim.nt - 1].copy()
        return made[name]
    return get


def check_run(label, name, sim, precision, march, iv, f64_row):
    worst = (-1.0, None, None, None)
    fails = []
    for i in range(2, sim.nt):
        s = step_residuals(sim, i, iv)
        slack = euler_slack(s, sim.dt)
        for fam, r in s.res.items():
            tol = PHANTOM_MARCHED if (fam == "PHANTOM" and march) else BOUND[precision]
            if fam != "PHANTOM" or not march:
                if r / s.scale > worst[0]:
                    worst = (r / s.scale, i, fam, s.align[0])
            if not r <= tol * s.scale + slack:
                fails.append((i, fam, s.align, r / s.scale))
    print(f"{label}: worst residual / scale {worst[0]:.2e} at step {worst[1]} ({worst[2]}, n0 = {worst[3]}), "
          f"steps 2-{sim.nt - 1}, bound {BOUND[precision]:.0e}")
    assert not fails, fails[:8]
    last = sim.path["TEV"][sim.nt - 1]
    assert last.shape == f64_row.shape and not np.array_equal(last, f64_row), "the fp32 route did not run"
    check_alignments(name, sim)


@pytest.mark.parametrize("threshold", [None, 8, 300])
@pytest.mark.parametrize("march", [True, False])
@pytest.mark.parametrize("precision", ["f32", "f32x2"])
def test_config1_every_step(precision, march, threshold, iv, f64_last_rows):
    """The README case, all 400 steps (wake 3 -> 603).  Threshold None: the direct kernels throughout; 8: the symmetric
    kernel and, in the march, overlapped steps from the start; 300: the switch falls between the two block edges."""
    sim = run("config1", precision, march, threshold)
    assert sim.nt == 401
    check_run(f"config1 {precision} march={march} threshold={threshold}", "config1", sim, precision, march, iv, f64_last_rows("config1"))


@pytest.mark.parametrize("tile", [4, 8])
def test_config1_every_step_with_a_forced_tile(tile, iv, f64_last_rows):
    """Overlapped steps from the start with the symmetric kernel's tile forced to 256 and to 512 vortices."""
    sim = run("config1", "f32", True, 8, tile)
    check_run(f"config1 f32 march=True threshold=8 tile={tile}", "config1", sim, "f32", True, iv, f64_last_rows("config1"))


@pytest.mark.parametrize("threshold", [None, 8])
@pytest.mark.parametrize("march", [True, False])
@pytest.mark.parametrize("name", CLOUDS)
def test_cloud_cases_every_step(name, march, threshold, iv, f64_last_rows):
    """100 steps behind a cloud of free vortices that puts a shed pair on a block or tile edge."""
    sim = run(name, "f32", march, threshold)
    assert sim.nt == 101
    check_run(f"{name} f32 march={march} threshold={threshold}", name, sim, "f32", march, iv, f64_last_rows(name))
