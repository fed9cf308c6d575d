"""GPU tier of G10 (oracle/g10_cases.py, tests/golden/g10_off_unit_runs.npz): the device time loops -- march_solve of the solo
march (csrc/march_kernels.hpp), its copy in a sweep member (csrc/ensemble_kernels.hpp), the per-step path -- with chord, Uinf
and rho pairwise different and off 1 and with cambered sections, against the unmodified reference's runs.  Every other GPU test
of a time loop runs chord = Uinf = 1 and (one sweep member aside, compared with the march only) a symmetric section: there the
camber product of the downwash row, every power of chord and Uinf in the solve and the loads, and the mean line in the
bound-vortex positions are multiplied by 1 or by 0.

Bounds are the reference's windows (tests/g10_common.py), licensed by the CPU tier (tests/test_g10_fixture.py: the host loop,
which differs from the reference by summation order only, stays 10 x inside): every load, LESP, A0 .. A3 and circulation
series within 1e-9 of its maximum over the first 100 steps and 1e-7 over the first 200, the wake rows after step 100 within
1e-9 of the largest coordinate, identical shedding.  float64 has no overlapped steps (march.hip runs the symmetric kernel and
march_finish_sym in 'f32' / 'f32x2' only), so those run in the fp32 test, with the symmetric threshold lowered to 64."""
import signal
import warnings

import numpy as np
import pytest

from g10_common import assert_within, fixture, oracle_sim, product_arrays, raw, safe_shedding_steps, window_errors
from observer_sources_common import PROBE_VS_SOURCES, field
from oracle import g10_cases as G10
from oracle import ludvm_oracle as O
from probes_common import probes32
from tracers_common import run_sources

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in G10.CASES]
T2_LOADS = 1e-2                 # Cl, Cd, Cm over the first 100 steps in fp32


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


@pytest.fixture(scope="module")
def g10():
    return fixture()


def _solo(eng, c, **extra):
    from ludvm_amd import LUDVM
    kw = dict(precision="f64", history="sparse", snapshot_steps=(G10.SNAP,))
    kw.update(extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered section's "mean line unpinned" warning
        return LUDVM(**G10.kwargs(c), verbose=False, engine=eng, **kw)


def _scaled(a, b, n=None):
    return float(np.abs(a[:n] - b[:n]).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("name", NAMES)
def test_solo_float64_runs_off_the_unit_point(eng, g10, name):
    """precision='f64' on its own: one round trip per step, and marched on the device -- each against the reference in the T3
    windows, and against each other to test_march_fills_every_result_like_the_per_step_path's tolerances (1e-10 on every load,
    100 x that on the Fourier rows, 10 x on the circulations, over the first 100 steps; of max(1, the series' maximum): the
    forces here are up to 1e3 in size).
    Measured [MI355X], worst series over the first 100 | 200 steps, per-step path / march (march against per-step path):
      d23 1.2e-12 | 1.8e-11 / 2.6e-12 | 1.6e-11 (2.0e-12), d23r 1.3e-11 | 8.7e-11 / 1.4e-11 | 5.9e-11 (1.3e-11),
      dhalf 1.2e-11 / 6.8e-12 (8.0e-12), k45 2.1e-11 | 9.7e-10 / 1.7e-11 | 5.8e-10 (5.9e-13),
      c2412 5.5e-12 | 7.3e-12 / 7.5e-12 | 1.0e-11 (1.3e-12), c6409 6.0e-14 | 3.6e-13 / 5.0e-14 | 3.3e-13 (3.3e-15),
      c4412d 4.1e-12 | 4.9e-11 / 1.9e-11 | 4.4e-10 (7.1e-12), c2412f 2.6e-12 / 2.5e-12 (9.7e-14)."""
    c = G10.BY_NAME[name]
    step = _solo(eng, c, march=False)
    assert_within(f"{name} per-step path", window_errors(product_arrays(step), g10[name], name))
    march = _solo(eng, c, march=True)
    assert_within(f"{name} march", window_errors(product_arrays(march), g10[name], name))
    a, b, n, tol = march, step, 100, 1e-10
    assert np.array_equal(a.LEV_shed, b.LEV_shed) and (a.itev, a.ilev) == (b.itev, b.ilev)
    worst = 0.0
    for k in ("Cl", "Cd", "Cm", "Cn", "Cs", "Ct", "L", "D", "T", "M", "Fn", "Fs", "LESP", "LESP_prev"):
        d = _scaled(getattr(a, k), getattr(b, k), n)
        worst = max(worst, d)
        assert d <= tol, (k, d)
    assert _scaled(a.fourier, b.fourier, n) <= 100 * tol
    for k in ("TEV", "LEV", "bound", "airfoil", "gamma_airfoil", "Gamma_airfoil"):
        assert _scaled(a.circulation[k], b.circulation[k], n) <= 10 * tol, k
        assert np.any(a.circulation[k] != 0), k
    assert a.circulation["IC"] == b.circulation["IC"]
    print(f"G10 {name}: march vs per-step path, loads over the first 100 steps {worst:.2e}")


def test_float64_march_has_no_overlapped_steps(eng, g10):
    """The marched float64 run of c4412d with the symmetric threshold lowered to 64, as the overlapped fp32 tests lower it:
    the same bits as with the default -- float64 steps are serial whatever the threshold, so the windows above are all there
    is to hold in 'f64'; march_finish_sym off the unit point runs in the fp32 test below."""
    c = G10.BY_NAME["c4412d"]
    plain = _solo(eng, c, march=True)
    eng.set_symmetric(64)
    try:
        low = _solo(eng, c, march=True)
    finally:
        eng.set_symmetric(1)
    assert all(np.array_equal(x, y) for x, y in zip(_bits(plain), _bits(low)))
    assert_within("c4412d march, symmetric threshold 64", window_errors(product_arrays(low), g10["c4412d"], "c4412d"))


def _bits(sim):
    last = sim.nt - 1
    return [sim.Cl, sim.fourier, sim.circulation["TEV"], sim.circulation["LEV"], sim.circulation["bound"], sim.circulation["airfoil"],
            sim.path["TEV"][last], sim.path["LEV"][last], sim.path["FREE"][last], sim.path["TEV"][G10.SNAP]]


@pytest.mark.parametrize("npoints", sorted({G10.kwargs(c)["Npoints"] for c in G10.CASES}))
def test_sweep_members_off_the_unit_point(eng, g10, npoints):
    """Every G10 case as a member of ONE sweep -- chords, speeds, densities, time steps, sections, kinematics, methods and step
    counts differing from member to member (Npoints is common to a sweep, so the 127-point case with its free vortices runs
    in a second one, 'Faure' beside 'Ramesh') -- and the same batch reversed: each member in the T3 windows, and with the same
    bits wherever it stands.
    Measured [MI355X], worst series over the first 100 | 200 steps: d23 1.1e-12 | 2.4e-11, d23r 5.1e-12 | 6.5e-11,
    dhalf 5.7e-12, k45 3.0e-11 | 1.4e-9, c2412 3.8e-12 | 7.8e-12, c6409 7.4e-14 | 1.6e-13, c4412d 2.3e-12 | 6.6e-11,
    c2412f 2.8e-13 ('Ramesh' beside it, against the oracle: 3.8e-12)."""
    from ludvm_amd import sweep
    cases = [c for c in G10.CASES if G10.kwargs(c)["Npoints"] == npoints]
    batch = [G10.kwargs(c) for c in cases]
    if len(batch) == 1:
        batch.append(G10.kwargs(cases[0], method="Ramesh"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sims = sweep(batch, engine=eng, snapshot_steps=(G10.SNAP,))
        back = sweep(batch[::-1], engine=eng, snapshot_steps=(G10.SNAP,))[::-1]
    for c, sim in zip(cases, sims):
        assert_within(f"{c['name']} sweep member", window_errors(product_arrays(sim), g10[c["name"]], c["name"]))
    if len(cases) == 1:         # (the oracle reproduces every stored run bit for bit: tests/test_g10_fixture.py)
        c = cases[0]
        ref = G10.unpack(G10.pack(oracle_sim(c, method="Ramesh"), c))
        assert_within(f"{c['name']} 'Ramesh' sweep member vs the oracle", window_errors(product_arrays(sims[1]), ref, c["name"]))
    for m, (a, b) in enumerate(zip(sims, back)):
        assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), m
    assert len({s.chord for s in sims}) == min(3, len(cases)) and len({s.nt for s in sims}) == min(2, len(cases))


@pytest.mark.parametrize("threshold", [1, 64], ids=["serial", "overlapped"])
@pytest.mark.parametrize("precision", ["f32", "f32x2"])
@pytest.mark.parametrize("name", ["d23", "c4412d"])
def test_fp32_marches_off_the_unit_point(eng, g10, name, precision, threshold):
    """The fp32 marches -- serial steps, and overlapped ones from 64 vortices on (symmetric kernel, march_finish_sym; reached
    near step 50) -- inside SURVEY T2's contract: Cl, Cd, Cm within 1e-2 (of max(1, the series' maximum)) over the first 100
    steps, shedding identical over the steps the CPU tier found safe from an fp32 rounding (all 200 in both cases).
    Measured [MI355X], largest deviation of Cl, Cd, Cm at 50 / 75 / 100 steps:
      d23    f32 serial 7.9e-7 / 1.4e-5 / 1.8e-4, overlapped 3.8e-7 / 2.7e-6 / 2.2e-5; f32x2 serial 3.8e-7 / 5.1e-6 / 1.1e-4,
             overlapped 4.0e-7 / 3.2e-6 / 1.2e-5
      c4412d f32 serial 3.5e-8 / 2.1e-5 / 8.8e-4, overlapped 4.1e-8 / 8.9e-6 / 5.9e-4; f32x2 serial 1.9e-8 / 3.2e-5 / 1.6e-3,
             overlapped 2.2e-8 / 5.1e-6 / 2.4e-4"""
    c, ref = G10.BY_NAME[name], g10[name]
    eng.set_symmetric(threshold)
    try:
        sim = _solo(eng, c, precision=precision, march=True)
    finally:
        eng.set_symmetric(1)
    n = safe_shedding_steps(ref)
    dev = {hi: max(_scaled(getattr(sim, k), ref[k], hi) for k in ("Cl", "Cd", "Cm")) for hi in (50, 75, 100)}
    print(f"G10 {name} {precision} {'overlapped' if threshold > 1 else 'serial'}: loads at 50 / 75 / 100 steps "
          + " / ".join(f"{dev[hi]:.2e}" for hi in (50, 75, 100)) + f"; shedding compared over {n} steps")
    assert np.array_equal(sim.LEV_shed[:n + 1], ref["LEV_shed"][:n + 1])
    assert sim.nt == ref["nt"] and np.isfinite(sim.Cl).all()
    assert dev[100] <= T2_LOADS, dev


def test_flowfield_of_a_cambered_dimensional_run(eng):
    """LUDVM.flowfield of c4412d in float64 (the bound vortices sit on the cambered line; chord 2, Uinf 3) against the
    reference's fields of steps 1 and 100: G4's 1e-10 of each field's maximum.
    Measured [MI355X]: step 1 u 8.5e-16 w 5.5e-16 vorticity 4.1e-16; step 100 u 2.9e-11 w 2.7e-11 vorticity 4.3e-11 (the host
    loop on the fake engine: 1.7e-11, 3.0e-11, 4.7e-11)."""
    from ludvm_amd import LUDVM
    c = G10.BY_NAME[G10.FIELD_CASE]
    sim = _solo(eng, c, snapshot_steps=LUDVM.flowfield_rows_needed(list(G10.FIELD_BOXES)))
    for s, (xmin, xmax, zmin, zmax, dr) in G10.FIELD_BOXES.items():
        f = raw()["field"][str(s)]
        sim.flowfield(xmin=xmin, xmax=xmax, zmin=zmin, zmax=zmax, dr=dr, tsteps=[s])
        assert np.array_equal(sim.x_ff, f[0]) and np.array_equal(sim.z_ff, f[1])
        e = [float(np.abs(a[0] - b).max() / np.abs(b).max()) for a, b in ((sim.u_ff, f[2]), (sim.w_ff, f[3]), (sim.ome_ff, f[4]))]
        print(f"G10 c4412d flow field of step {s} / each field's maximum: u {e[0]:.2e} w {e[1]:.2e} vorticity {e[2]:.2e}")
        assert max(e) <= 1e-10, (s, e)


def test_probes_in_the_tunnel_frame_off_the_unit_point(eng):
    """Probe rows of d23 with probe_frame='tunnel' -- the frame moves with -Uinf t, Uinf = 3, and the points are the probe
    set scaled by the chord -- against the float64 pair sum over the sources the run's own dense history states for each
    step's roll-up, at the points probe_positions gives: 1e-9 of max|u| (the bound of
    test_overlapped_steps_probe_the_sources_of_their_own_roll_up).  Measured [MI355X]: 1.8e-15."""
    c = G10.BY_NAME["d23"]
    kw = G10.kwargs(c)
    pts = kw["chord"] * probes32()
    sim = _solo(eng, c, history="full", snapshot_steps=(), probes=pts, probe_frame="tunnel")
    assert sim.probe_u.shape == (sim.nt, 32) and np.array_equal(sim.xpiv, -kw["Uinf"] * sim.t)
    worst = 0.0
    for i in range(2, sim.nt):
        pos = sim.probe_positions(i)
        assert np.array_equal(pos[0], pts[0] + sim.xpiv[i]) and np.array_equal(pos[1], pts[1])
        u, w = field(O.induced_velocity, run_sources(sim, i), pos[0], pos[1], sim.v_core)
        scale = max(np.abs(u).max(), np.abs(w).max())
        worst = max(worst, max(np.abs(sim.probe_u[i] - u).max(), np.abs(sim.probe_w[i] - w).max()) / scale)
    print(f"G10 d23 probes in the tunnel frame vs the run's own sources: {worst:.2e} of max|u|")
    assert worst <= PROBE_VS_SOURCES, worst
