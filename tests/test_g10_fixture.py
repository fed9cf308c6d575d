"""CPU tier of G10 (tests/golden/g10_off_unit_runs.npz, oracle/g10_cases.py): time loops with chord, Uinf and rho off 1 and with
cambered sections.  The fixture is the table; the oracle reproduces every case; the section's tables of the product and of the
oracle are the reference's bit for bit; the product's host loop reproduces every case 10 x inside the windows the GPU tier
asserts (tests/test_gpu_g10.py), which licenses them; LUDVM.airfoil_downwash reproduces the recorded calls; the shedding
decision of every case is safe from an fp32 rounding for at least 50 steps; and no case can be met by a run that ignores
chord, Uinf, rho or the camber.

Measured here (host loop on the fake engine against the reference, worst series relative to its maximum, first 100 | first 200
steps): d23 1.0e-12 | 1.3e-11, d23r 2.6e-11 | 3.0e-10, dhalf 1.6e-11, k45 2.0e-11 | 8.7e-10, c2412 2.7e-12 | 4.5e-12,
c6409 6.4e-14 | 3.4e-13, c4412d 5.7e-12 | 2.4e-10, c2412f 2.5e-12; the flow field of c4412d at step 100: 4.7e-11 of the
vorticity's maximum (step 1: 5.7e-16); the 22 recorded downwash calls: 0; the oracle: 0 everywhere.  Every case keeps
| |A0| - |LESPcrit| | above 1e-4 over all of its steps; putting one quantity back moves Cl, Cd or Cm by 0.23 .. 13 within
20 steps."""
import os
import warnings

import numpy as np
import pytest

from g10_common import (MARGIN, SHED_MIN_STEPS, T3_100, T3_200, WINDOW, assert_within, downwash_calls, fixture, oracle_sim,
                        product_arrays, raw, safe_shedding_steps, window_errors, worst)
from oracle import g10_cases as G10
from oracle.g9_cases import SERIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in G10.CASES]


@pytest.fixture(scope="module")
def g10():
    return fixture()


def _product(c, **extra):
    from fake_engine import FakeEngine
    from ludvm_amd import LUDVM
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered section's "mean line unpinned" warning
        return LUDVM(**G10.kwargs(c), verbose=False, engine=FakeEngine(), **extra)


def test_g10_fixture_is_the_table(g10):
    assert sorted(raw()) == sorted(NAMES + ["downwash", "field"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g10_off_unit_runs.npz")) < 1 << 19
    for c in G10.CASES:
        ref = g10[c["name"]]
        assert np.array_equal(ref["params"], G10.params(c)), c["name"]
        n = c["steps"]
        assert ref["nt"] == n + 1 and ref["itev"] == n - 1 and len(ref["Cl"]) == n + 1 and len(ref["circ_TEV"]) == n
        assert ref["TEV"].shape == (2, G10.SNAP) and ref["FREE"].shape == (2, max(c["nfree"], 1)), c["name"]
        assert ref["fourier4"].shape == (n + 1, 2, 4) and ref["LESP_prev"].shape == (n + 1,), c["name"]
        assert all(np.isfinite(v).all() for v in ref.values() if isinstance(v, np.ndarray)), c["name"]
        assert ref["ilev"] > 0, c["name"]                                   # every case sheds leading-edge vortices
        kw = G10.kwargs(c)
        assert ref["v_core"] == 1.3 * (kw["dt"] * kw["Uinf"] / kw["chord"]) * kw["chord"]
        assert ("eta" in ref) == G10.is_cambered(c)
    # the rules of the dimensional cases, and the sections
    for c in G10.CASES:
        kw = G10.kwargs(c)
        if kw["chord"] != 1:
            assert len({kw["chord"], kw["Uinf"], kw["rho"], 1}) == 4, c["name"]
            assert abs(kw["dt"] * kw["Uinf"] / kw["chord"] - 0.05) < 1e-15, c["name"]
    d23 = G10.kwargs(G10.BY_NAME["d23"])
    assert (d23["chord"], d23["Uinf"]) == (2, 3)        # c^a U^b = 2^a 3^b: distinct for distinct (a, b)
    assert [G10.kwargs(c)["Naca"] for c in G10.CAMBERED] == ["2412", "6409", "4412", "2412"]
    assert {c["method"] for c in G10.CAMBERED} == {"Faure", "Ramesh"} == {c["method"] for c in G10.CASES if not G10.is_cambered(c)}
    # the recorded downwash calls and the flow fields
    calls = downwash_calls()
    assert sorted({int(c["step"]) for c in calls}) == list(G10.SPY_STEPS)
    for s, (xmin, xmax, zmin, zmax, dr) in G10.FIELD_BOXES.items():
        f = raw()["field"][str(s)]
        assert f.shape[0] == 5 and f.shape[1] <= 40 and f.shape[2] <= 24 and np.abs(f[2:]).max() > 0, s


@pytest.mark.parametrize("name", NAMES)
def test_g10_python_oracle_reproduces_the_reference(g10, name):
    """OracleLUDVM on every case: every series and wake row to 1e-10 of its maximum (tests/test_g9_fixture.py's oracle bound;
    measured 0: the same float64 operations in the same order), identical LEV_shed, the section's tables bit for bit."""
    c = G10.BY_NAME[name]
    sim = oracle_sim(c)
    got, ref = G10.unpack(G10.pack(sim, c)), g10[name]
    assert np.array_equal(got["LEV_shed"], ref["LEV_shed"]) and (got["nt"], got["itev"], got["ilev"]) == (ref["nt"], ref["itev"], ref["ilev"])
    top = 0.0
    for k in SERIES[:-1] + ("TEV", "LEV", "FREE", "fourier4", "LESP_prev"):
        assert got[k].shape == ref[k].shape, k
        d = np.abs(got[k] - ref[k]).max() / (np.abs(ref[k]).max() or 1.0)
        assert d <= 1e-10, (k, d)
        top = max(top, d)
    print(f"G10 {name}: oracle vs reference, worst relative difference {top:.2e}")
    for k in G10.FOIL_KEYS if G10.is_cambered(c) else ():
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("name", [c["name"] for c in G10.CAMBERED])
def test_g10_section_tables_of_the_product_are_the_references(g10, name):
    c = G10.BY_NAME[name]
    sim = _product(c, run=False)
    for k in G10.FOIL_KEYS:
        assert np.array_equal(sim.airfoil[k], g10[name][k]), k
    assert np.abs(g10[name]["eta"]).max() > 0.015 * G10.kwargs(c)["chord"] and np.abs(g10[name]["detadx_panel"]).max() > 0.05


@pytest.mark.parametrize("name", NAMES)
def test_g10_host_loop_reproduces_the_fixture_on_the_fake_engine(g10, name):
    """The product's per-step host loop (pair sums by the CPU oracle) differs from the reference by summation order only: it
    stays MARGIN = 10 x inside the T3 windows over the steps WINDOW gives the case -- the condition under which the GPU tier
    asserts those windows.  c4412d also evaluates the flow field of steps 1 and 100 (G4's 1e-10 of each field's maximum)."""
    c = G10.BY_NAME[name]
    sim = _product(c)
    err = window_errors(product_arrays(sim), g10[name], name)
    assert_within(f"{name} host loop vs reference (asserted {MARGIN:.0f} x inside)", err, factor=MARGIN)
    w100, w200 = worst(err)
    assert w100 <= T3_100 / MARGIN and (w200 is None) == (WINDOW[name] <= 100) and (w200 is None or w200 <= T3_200 / MARGIN)
    if name == G10.FIELD_CASE:
        for s, e in field_errors(sim).items():
            print(f"G10 {name} host loop: flow field of step {s} / each field's maximum: u {e[0]:.2e} w {e[1]:.2e} vorticity {e[2]:.2e}")
            assert max(e) <= 1e-10, (s, e)


def field_errors(sim):
    """{step: (u, w, vorticity) of LUDVM.flowfield against the fixture, each relative to the field's maximum}."""
    out = {}
    for s, (xmin, xmax, zmin, zmax, dr) in G10.FIELD_BOXES.items():
        f = raw()["field"][str(s)]
        sim.flowfield(xmin=xmin, xmax=xmax, zmin=zmin, zmax=zmax, dr=dr, tsteps=[s])
        assert np.array_equal(sim.x_ff, f[0]) and np.array_equal(sim.z_ff, f[1])
        out[s] = tuple(float(np.abs(a[0] - b).max() / np.abs(b).max()) for a, b in ((sim.u_ff, f[2]), (sim.w_ff, f[3]), (sim.ome_ff, f[4])))
    return out


def test_g10_airfoil_downwash_against_the_recorded_calls():
    """LUDVM.airfoil_downwash of c4412d (cambered, chord 2, Uinf 3) on the arguments of every call the reference made in steps
    1, 2 and 50 (the Newton iterations of 'Ramesh'): 1e-12 of max|W| -- the oracle's pair sum is the reference's."""
    sim = _product(G10.BY_NAME[G10.SPY_CASE], run=False)
    calls = downwash_calls()
    assert len(calls) >= 9
    top = 0.0
    for c in calls:
        W = sim.airfoil_downwash(c["g"], c["xw"], c["zw"], int(c["step"]))
        assert W.shape == c["W"].shape
        top = max(top, np.abs(W - c["W"]).max() / np.abs(c["W"]).max())
    print(f"G10 airfoil_downwash: {len(calls)} recorded calls, worst difference {top:.2e} of max|W|")
    assert top <= 1e-12


def test_g10_shedding_is_safe_from_an_fp32_rounding_for_50_steps(g10):
    """N of every case: the leading steps over which the reference's |A0| stays 1e-4 away from |LESPcrit| at the decision.
    The fp32 GPU tests assert identical shedding over those steps only."""
    for name in NAMES:
        n = safe_shedding_steps(g10[name])
        print(f"G10 {name}: shedding decision safe from an fp32 rounding over the first {n} steps")
        assert n >= SHED_MIN_STEPS, (name, n)


RHO_FREE = "rho"


@pytest.mark.parametrize("name,what,back", [
    ("d23", "chord", dict(chord=1)), ("d23", "Uinf", dict(Uinf=1)), ("d23", RHO_FREE, dict(rho=1.225)),
    ("dhalf", "chord", dict(chord=1)), ("dhalf", "Uinf", dict(Uinf=1)), ("dhalf", RHO_FREE, dict(rho=1.225)),
    ("k45", "chord", dict(chord=1)), ("k45", "Uinf", dict(Uinf=1)),
    ("c2412", "camber", dict(Naca="0012")), ("c6409", "camber", dict(Naca="0012")), ("c4412d", "camber", dict(Naca="0012")),
    ("c4412d", "chord", dict(chord=1)), ("c4412d", "Uinf", dict(Uinf=1)), ("c4412d", RHO_FREE, dict(rho=1.225)),
    ("c2412f", "camber", dict(Naca="0012")), ("c2412f", "chord", dict(chord=1)),
])
def test_g10_no_case_can_be_met_by_a_run_that_ignores_a_quantity(g10, name, what, back):
    """The oracle's run with ONE quantity put back to config 1's value is more than 1e-3 away from the fixture in Cl, Cd or Cm
    within the first 20 steps: before the flow amplifies anything, the fixture cannot be met by a run that ignores it.
    rho: the coefficients are free of rho by construction (forces / (rho U^2 c / 2)), so the run that ignores rho is the one
    whose FORCES are those of rho = 1.225 while the coefficients are formed with the case's rho -- what a device solve with
    a wrong rho would hand the host."""
    c = G10.BY_NAME[name]
    sim, ref = oracle_sim(c, **back), g10[name]
    if what == RHO_FREE:
        kw = G10.kwargs(c)
        qc = 0.5 * kw["rho"] * kw["Uinf"] ** 2 * kw["chord"]
        got = dict(Cl=sim.L / qc, Cd=sim.D / qc, Cm=sim.M / (qc * kw["chord"]))
    else:
        got = dict(Cl=sim.Cl, Cd=sim.Cd, Cm=sim.Cm)
    d = max(np.abs(got[k][:21] - ref[k][:21]).max() for k in ("Cl", "Cd", "Cm"))
    print(f"G10 {name} with {what} put back: {d:.2e} away within 20 steps")
    assert d > 1e-3, (name, what, d)
