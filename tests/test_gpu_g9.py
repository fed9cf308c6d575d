"""GPU tier of G9 (oracle/g9_cases.py, tests/golden/g9_edge_runs.npz): sweep members (ensemble_march, csrc/ensemble_kernels.hpp)
and solo marched / per-step runs at the panel, coefficient and wake counts where their lane arithmetic changes -- against the
unmodified reference's runs.  Every other GPU test of the sweep runs 80 panels and 30 coefficients.

Bounds are the reference's windows, not new numbers: loads 1e-9 over steps 0-99 (tier T3, as
test_members_against_solo_runs_on_the_same_engine), circulations, Kelvin's sum and the stored wake rows (step 50: the position
bound of DESIGN section 2) 1e-9.  The reference's own sensitivity to the order of its pair sums over these steps is 1.2e-11 at
worst (two oracle runs per group-A case, sources visited forwards and backwards), a factor of 80 under the bound."""
import signal
import warnings

import numpy as np
import pytest

from conftest import CONFIG1
from g9_common import product_errors, reference_run, show
from oracle import g9_cases as G9
from oracle import ludvm_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(autouse=True)
def _time_limit():
    """A limit on every test's host-side time.  (The handler runs between Python instructions: a test stuck INSIDE a HIP call
    is ended by the time limit that wraps the pytest command, not by this.)"""
    def expired(signum, frame):
        raise TimeoutError("GPU test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _assert_within(label, err, tol=TOL):
    show(label, err)
    for k, v in err.items():
        assert v <= tol, (label, k, v)


def _id(c):
    return f"{c['npan']}-{c['ncoef']}" if c["group"] == "A" else c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in G9.GROUP_A + G9.GROUP_B], ids=[_id(c) for c in G9.GROUP_A + G9.GROUP_B])
def test_sweep_members_at_edge_shapes(eng, name):
    """One sweep per case.  Group A: the 'Faure' and the 'Ramesh' member (member 1 starts at non-zero offsets in every packed
    array); group B: the case behind a 20-step member with the default free vortex, so its free vortices, kinematics, rows and
    wake records all start at non-zero offsets, and the snapshot step (30) is its last step and lies past the first member's."""
    from ludvm_amd import sweep
    c = G9.BY_NAME[name]
    if c["group"] == "A":
        methods = ("Faure", "Ramesh")
        sims = sweep([G9.kwargs(c, m) for m in methods], engine=eng, snapshot_steps=(c["snap"],))
    else:
        methods = ("Faure",)
        front, sim = sweep([dict(CONFIG1, tf=1, Npoints=c["npan"] + 1, Ncoeffs=c["ncoef"]), G9.kwargs(c)], engine=eng,
                           snapshot_steps=(c["snap"],))
        assert front.nt == 21 and front.path["TEV"].steps() == [0, 20]
        sims = [sim]
    for m, sim in zip(methods, sims):
        _assert_within(f"sweep {name} {m}", product_errors(sim, reference_run(c, m), c))


@pytest.mark.parametrize("name", [c["name"] for c in G9.GROUP_A], ids=[_id(c) for c in G9.GROUP_A])
def test_marched_and_per_step_runs_at_edge_shapes(eng, name):
    """The solo float64 run, marched on the device (npan + 3 chord targets per step: pair_f64_few from the step at which the
    wake passes one 128-source tile, pair_f64<128> before that and at 126 panels and more) and one round trip per step."""
    from ludvm_amd import LUDVM
    c = G9.BY_NAME[name]
    ref = reference_run(c, "Faure")
    for march in (True, False):
        sim = LUDVM(**G9.kwargs(c), verbose=False, engine=eng, precision="f64", history="sparse", march=march,
                    snapshot_steps=(c["snap"],))
        _assert_within(f"{'march' if march else 'per-step'} {name}", product_errors(sim, ref, c))


def _small_bits(eng):
    from ludvm_amd import sweep
    s = sweep([dict(CONFIG1, tf=1)], engine=eng)[0]
    return [s.Cl, s.Cd, s.Cm, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1]]


def test_a_member_at_the_wake_capacity(eng):
    """nfree + 2 (nt - 1) = ENSEMBLE_MAX_WAKE exactly: the member, the reference and the solo run.  The wake rows after the
    one step to 1e-12 of the largest coordinate (the per-call float64 contract of include/ludvm_hip.h, 1e-12 max|u|, times
    dt; one step carries no amplification), Cl to 1e-9.  One free vortex more is refused by `sweep` (ValueError) and by
    Engine.ensemble_run (E_ARG) before anything is launched, and the sweep after it gives the bits of the sweep before it."""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    c, = G9.GROUP_C
    assert c["nfree"] + 2 == _ffi.ENSEMBLE_MAX_WAKE
    ref = reference_run(c, "Faure")
    before = _small_bits(eng)
    member, = sweep([G9.kwargs(c)], engine=eng)
    solo = LUDVM(**G9.kwargs(c), verbose=False, engine=eng, precision="f64", history="sparse")
    top = max(np.abs(ref[k]).max() for k in ("TEV", "LEV", "FREE"))
    for label, sim in (("member", member), ("solo", solo)):
        err = product_errors(sim, ref, c)
        show(f"capacity {label} (rows / {top:.3g})", err)
        for k in ("row_TEV", "row_LEV", "row_FREE"):
            assert err[k] <= 1e-12 * top, (label, k, err[k])
        assert err["Cl"] <= 1e-9 and err["Cd"] <= 1e-9 and err["Cm"] <= 1e-9 and err["kelvin"] <= 1e-9, (label, err)
    for k in ("TEV", "LEV", "FREE"):
        d = np.abs(np.asarray(member.path[k][1]) - np.asarray(solo.path[k][1])).max()
        print(f"capacity member vs solo {k}: {d:.2e}")
        assert d <= 1e-12 * top, (k, d)

    # one vortex too many
    over = G9.over_capacity_kwargs()
    assert len(over["circulation_freevort"]) == c["nfree"] + 1
    reached = []
    inner = eng.ensemble_run
    eng.ensemble_run = lambda *a, **k: reached.append(1) or inner(*a, **k)
    try:
        with pytest.raises(ValueError, match="on its own"):
            sweep([dict(CONFIG1, tf=1), over], engine=eng)
    finally:
        del eng.ensemble_run
    assert not reached
    npan, ncoef, nf = 80, 30, c["nfree"] + 1
    desc = np.array([[2, 0, nf, 0, 0, 0]], dtype=np.int64)
    scalars = np.ones([1, 12])
    scalars[:, 8:] = 0.0
    with pytest.raises(LudvmHipError) as e:
        eng.ensemble_run(npan, ncoef, scalars, np.zeros([1, 8 * npan + ncoef * npan + (ncoef - 1) * npan]),
                         np.zeros([2, 7 + 2 * npan]), np.zeros([1, 8 + ncoef]), np.zeros(3 * nf), desc)
    assert e.value.code == _ffi.E_ARG and "member 0" in str(e.value) and str(_ffi.ENSEMBLE_MAX_WAKE) in str(e.value), str(e.value)
    after = _small_bits(eng)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_more_snapshot_records_than_lanes(eng):
    """300 snapshot steps -- more records than the workgroup has lanes (the strided part of the loop that clears rec_n runs)
    and more than any member has steps: members of 30, 60 and 100 steps keep a row for each of their own steps and for no
    other, the rows of steps <= 50 equal the oracle's to 1e-9, and everything else a member returns has the bits of the same
    sweep without snapshots."""
    from ludvm_amd import sweep
    cases = [dict(CONFIG1, tf=tf) for tf in (1.5, 3, 5)]
    sims = sweep(cases, engine=eng, snapshot_steps=range(1, 301))
    plain = sweep(cases, engine=eng, snapshot_steps=())
    worst = 0.0
    for kw, sim, bare in zip(cases, sims, plain):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = O.OracleLUDVM(**kw)
        nt = sim.nt
        assert nt == ref.nt == int(round(kw["tf"] / kw["dt"])) + 1
        for key in ("TEV", "LEV", "FREE"):
            assert sim.path[key].steps() == list(range(nt)), key             # (row 0: the state before the first step)
            assert bare.path[key].steps() == [0, nt - 1], key
        assert np.array_equal(sim.LEV_shed, ref.LEV_shed)
        for s in range(1, min(nt - 1, 50) + 1):
            for key in ("TEV", "LEV", "FREE"):
                row = np.asarray(sim.path[key][s])
                assert row.shape[1] >= 1 and np.isfinite(row).all(), (key, s)
                if key == "TEV":
                    assert row.shape[1] == s
                d = np.abs(row - ref.path[key][s][:, :row.shape[1]]).max()
                worst = max(worst, d)
                assert d <= 1e-9, (kw["tf"], key, s, d)
        for name in ("Cl", "Cd", "Cm", "Cn", "Cs", "Ct", "Fn", "Fs", "L", "D", "T", "M", "LESP", "LESP_prev", "LEV_shed", "fourier"):
            assert np.array_equal(getattr(sim, name), getattr(bare, name)), name
        for key in ("TEV", "LEV", "bound", "airfoil"):
            assert np.array_equal(sim.circulation[key], bare.circulation[key]), key
        assert (sim.itev, sim.ilev) == (bare.itev, bare.ilev)
        for key in ("TEV", "LEV", "FREE"):
            assert np.array_equal(np.asarray(sim.path[key][nt - 1]), np.asarray(bare.path[key][nt - 1])), key
    print(f"G9 300 snapshot records: rows of steps <= 50 against the oracle, max |d| {worst:.2e}")
