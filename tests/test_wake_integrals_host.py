"""CPU tier of the wake integrals (tests/wake_integrals_common.py): the product's host loop (per-step path on
tests/fake_engine.py) and its NumPy formulas against the long-double reference over the run's own sources; Kelvin's total from the
oracle; the sign of the impulse convention and its Kutta-Joukowski limit; planted faults; refusals; checkpoints; the C ABI.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import wake_integrals_common as WI
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from observers_off_unit_common import case_keywords
from oracle import ludvm_oracle as O

ENERGY_WIN = (1, 380, 57)           # begins at step 1, skips steps, ends before the run does


@pytest.fixture(scope="module")
def host1():
    """config 1's 400 steps through the per-step path, dense history: the wake grows from 3 to 603"""
    return LUDVM(**CONFIG1, verbose=False, engine=WI.FieldFakeEngine(), wake_integrals=True, wake_energy_steps=ENERGY_WIN)


@pytest.fixture(scope="module")
def oracle1():
    return O.OracleLUDVM(**CONFIG1)


def formulas_on(run, kw):
    """the class's host formulas over rows formed by the REFERENCE from `run` (an oracle): a LUDVM that never runs, carrying them"""
    s = LUDVM(**kw, verbose=False, engine=FakeEngine(), wake_integrals=True, run=False)
    s.integral_sums = np.zeros([run.nt, 4, 2, 6])
    for i in range(1, run.nt):
        s.integral_sums[i] = WI.reference(run, i, energy=False)["sums"]
    return s


def test_host_rows_and_formulas_against_the_reference(host1):
    sim = host1
    assert sim.integral_sums.shape == (sim.nt, 4, 2, 6) and sim.wake_energy.shape == (sim.nt,)
    assert sim.integral_classes == WI.CLASSES
    steps = range(1, sim.nt)
    WI.check_run(sim, sim, steps, WI.window_steps(ENERGY_WIN, sim.nt), "host loop, config 1")
    # the case fills what it claims to: both signs of TEV, LEV and BOUND, and a free vortex (config 1's zero-strength one)
    census = WI.class_census(sim, steps)
    print("largest counts [class, sign]:", census.tolist())
    assert (census[[WI.TEV, WI.LEV, WI.BOUND]] > 0).all() and census[WI.FREE, 0] == 1
    # row 0: the initial free vortices alone
    assert sim.integral_sums[0, WI.FREE, 0, 0] == 1.0 and not sim.integral_sums[0, 1:].any() and np.isnan(sim.wake_energy[0])
    # the formulas
    i = 333
    ref = WI.reference(sim, i, energy=False)["sums"]
    tot = ref.sum(axis=(0, 1))
    assert np.allclose(sim.wake_circulation()[i], tot[1], rtol=0, atol=1e-13)
    assert np.allclose(sim.wake_circulation("LEV")[i], ref[WI.LEV, :, 1].sum(), rtol=0, atol=1e-13)
    assert np.allclose(sim.wake_circulation("TEV", "-")[i], ref[WI.TEV, 1, 1], rtol=0, atol=1e-13)
    assert np.allclose(sim.wake_circulation(sign="+")[i], ref[:, 0, 1].sum(), rtol=0, atol=1e-13)
    assert np.allclose(sim.wake_centroid("LEV", "+")[i], ref[WI.LEV, 0, 2:4] / ref[WI.LEV, 0, 1], rtol=1e-12)
    assert np.isnan(sim.wake_centroid("FREE", "-")).all() and np.isnan(sim.wake_centroid("LEV", "+")[1]).all()
    assert np.allclose(sim.wake_impulse[i], sim.rho * np.array([-tot[3], tot[2]]), rtol=1e-12)
    assert np.allclose(sim.wake_angular_impulse[i], 0.5 * sim.rho * tot[4], rtol=1e-12)
    F = sim.impulse_force
    assert np.isnan(F[:2]).all() and np.isfinite(F[2:]).all()
    assert np.allclose(F[i], -(sim.wake_impulse[i] - sim.wake_impulse[i - 1]) / sim.dt, rtol=1e-12)
    q = 0.5 * sim.rho * sim.Uinf**2 * sim.chord
    assert np.allclose(sim.impulse_Cl[2:], F[2:, 1] / q) and np.allclose(sim.impulse_Cd[2:], F[2:, 0] / q)
    w = WI.window_steps(ENERGY_WIN, sim.nt)
    self_part = np.array([WI.reference(sim, k)["self"] for k in w])
    assert np.allclose(sim.wake_energy_interaction[w], sim.wake_energy[w] - self_part, rtol=0, atol=1e-12 * np.abs(self_part).max())
    for bad in ("WAKE", 4, -1):
        with pytest.raises(ValueError, match="class"):
            sim.wake_circulation(bad)
    with pytest.raises(ValueError, match="sign"):
        sim.wake_centroid("TEV", 0)
    with pytest.raises(ValueError, match="wake_integrals=True"):
        LUDVM(**dict(CONFIG1, tf=0.5), verbose=False, engine=FakeEngine()).wake_impulse


def test_free_cloud_and_off_unit_case():
    """FREE in both signs (a mixed cloud in front of the foil); chord, Uinf, rho != 1 and camber (G10's c4412d): rho and the frame"""
    kw = dict(CONFIG1, tf=1.5, **WI.mixed_cloud(60))
    sim = LUDVM(**kw, verbose=False, engine=WI.FieldFakeEngine(), wake_integrals=True, wake_energy_steps=(2, 30, 9))
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps((2, 30, 9), sim.nt), "host loop, mixed cloud")
    assert (WI.class_census(sim, range(1, sim.nt))[WI.FREE] > 10).all()
    assert sim.integral_sums[0, WI.FREE, :, 0].sum() == 60
    kw = case_keywords("c4412d", steps=40)
    sim = LUDVM(**kw, verbose=False, engine=WI.FieldFakeEngine(), wake_integrals=True, wake_energy_steps=(1, 41, 13))
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps((1, 41, 13), sim.nt), "host loop, c4412d")
    tot = WI.reference(sim, 30, energy=False)["sums"].sum(axis=(0, 1))
    assert kw["rho"] == 0.9 and np.allclose(sim.wake_impulse[30], 0.9 * np.array([-tot[3], tot[2]]), rtol=1e-12)


def test_kelvin_total_from_the_oracle(oracle1):
    """What the oracle's own arrays say: at every step the circulation of the wake classes plus circulation['bound'] of the step
    is +circulation['IC'] to rounding (k45: IC = -5.27, so the sign is seen; config 1: IC = 0).  The BOUND class is the STAGED
    bound vortices, the panel circulations the roll-up uses: their sum is a quadrature of the bound vorticity (config 1: within
    4e-3 of circulation['bound'], measured on the oracle), and off unit chord the reference stages chord x bound (d23: twice) --
    so the eight sums of a row add up to IC only where chord = 1, and there to that quadrature."""
    for run in (O.OracleLUDVM(**case_keywords("k45", steps=60)), oracle1):
        C = run.circulation
        scale = worst = 0.0
        for i in range(1, run.nt, 7 if run is oracle1 else 1):
            g = WI.reference(run, i, energy=False)["sums"][:, :, 1]
            scale = max(scale, np.abs(g).sum())
            worst = max(worst, abs(g[:WI.BOUND].sum() + C["bound"][i - 1] - C["IC"]))
            if run is oracle1:
                assert abs(g.sum() - C["IC"]) <= 1e-2, (i, g.sum())
        print(f"IC = {C['IC']:.6f}: worst |wake + bound - IC| = {worst:.2e} (sum |G| up to {scale:.2f})")
        assert worst <= 64 * WI.EPS * scale * run.nt
    assert abs(C["IC"]) == 0.0


def test_impulse_lift_has_the_sign_of_the_loads_and_the_kutta_joukowski_limit(oracle1):
    """impulse_Cl over the oracle's config 1 correlates positively with the oracle's Cl (the convention I = rho (-sum G z, sum G x),
    F = -dI/dt stands); and for a foil held at 2 degrees, 20 chords after its start, it is the Kutta-Joukowski lift of the bound
    circulation, 2 Gamma_b / (U c), to 5 % -- what is left of the starting transient there (Wagner: about 1 - phi(40) = 2 % of the
    lift, and as much again in the shed sheet's share of dI/dt); positive, like the oracle's Cl."""
    s = formulas_on(oracle1, CONFIG1)
    corr = np.corrcoef(s.impulse_Cl[2:], oracle1.Cl[2:])[0, 1]
    d = (s.impulse_Cl - oracle1.Cl)[200:]
    print(f"config 1 (oracle): corr(impulse_Cl, Cl) = {corr:.4f}; after the first period max |diff| = {np.abs(d).max():.3f}, "
          f"rms = {np.sqrt((d * d).mean()):.3f}, max |Cl| = {np.abs(oracle1.Cl[200:]).max():.3f}")
    assert corr > 0.9
    kw = dict(CONFIG1, alpha_m=2, alpha_max=0, h_max=0)
    held = O.OracleLUDVM(**kw)
    s = formulas_on(held, kw)
    kj = 2.0 * s.wake_circulation("BOUND")[-1] / (held.Uinf * held.chord)
    print(f"held at 2 degrees, step {held.nt - 1}: impulse_Cl = {s.impulse_Cl[-1]:.4f}, 2 Gamma_b / (U c) = {kj:.4f}, Cl = {held.Cl[-1]:.4f}")
    assert kj > 0.0 and held.Cl[-1] > 0.0 and s.impulse_Cl[-1] > 0.0
    assert abs(s.impulse_Cl[-1] - kj) <= 0.05 * kj


@pytest.fixture(scope="module")
def short_oracle():
    return O.OracleLUDVM(**dict(CONFIG1, tf=5.0))


def test_the_model_without_a_fault_is_inside_the_bounds(short_oracle):
    bad_m, bad_w = WI.model_misses(short_oracle, WI.model_rows(short_oracle, range(2, 100, 3)))
    assert not bad_m and not bad_w


@pytest.mark.parametrize("fault", WI.FAULTS)
def test_the_check_sees_a_planted_fault(fault, short_oracle):
    """Each fault, planted into a float64 model of the rows over an oracle run's sources, leaves the bounds: the swapped tags from
    the first LEV on, the dropped bound vortices and the shifted rows at every step, the sign rule at Gamma = 0 in the count of
    config 1's zero-strength free vortex, the missing a = b terms in W alone."""
    steps = range(2, 100, 3)
    shed = np.flatnonzero(np.asarray(short_oracle.LEV_shed) != -1)
    assert len(shed) and shed[0] < 90
    bad_m, bad_w = WI.model_misses(short_oracle, WI.model_rows(short_oracle, steps, fault))
    if fault == "self_terms_left_out":
        assert not bad_m and bad_w == list(steps)
    elif fault == "tev_lev_swapped":
        assert bad_m == list(steps) and not bad_w            # (the TEVs are mislabelled from the start; W has no classes)
    elif fault == "sign_flipped_at_zero":
        assert bad_m == list(steps) and not bad_w
    else:
        assert bad_m == list(steps) and bad_w == list(steps)


def test_refusals_come_before_any_engine(monkeypatch):
    import ludvm_amd.ludvm as M
    import ludvm_amd.multi as MM

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the keywords were checked")

    def no_front(*a, **k):
        raise AssertionError("replica threads were created before the keywords were checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    monkeypatch.setattr(MM, "MultiDeviceLUDVM", no_front)
    for bad in (1, "yes", None, [True]):
        with pytest.raises(ValueError, match="wake_integrals must be a bool"):
            LUDVM(**CONFIG1, verbose=False, wake_integrals=bad)
    with pytest.raises(ValueError, match="wake_energy_steps needs wake_integrals=True"):
        LUDVM(**CONFIG1, verbose=False, wake_energy_steps=(1, 10, 1))
    for win in ((0, 10, 1), (1, 10, 0), (5, 5, 1), (1, 10), (1.5, 10, 1), "abc", (500, 600, 1)):
        with pytest.raises(ValueError, match="wake_energy_steps"):
            LUDVM(**CONFIG1, verbose=False, wake_integrals=True, wake_energy_steps=win)
    for dist in (True, "rccl", object()):
        with pytest.raises(ValueError, match="one GPU: not with `distributed`"):
            LUDVM(**CONFIG1, verbose=False, wake_integrals=True, distributed=dist)
    for devs in ([0, 1], 2):
        with pytest.raises(ValueError, match="one GPU: not with more than one device"):
            LUDVM(**CONFIG1, verbose=False, wake_integrals=True, devices=devs)
    short = dict(CONFIG1, tf=1.0)
    for cases, kw in (([short, dict(short, wake_integrals=True)], {}), ([short, short], dict(wake_integrals=True)),
                      ([short, dict(short, wake_energy_steps=(1, 5, 1))], {}), ([short, short], dict(wake_energy_steps=(1, 5, 1)))):
        with pytest.raises(ValueError, match="solo keyword"):
            LUDVM.sweep(cases, **kw)


def test_an_engine_that_marches_without_the_entry_is_refused():
    class Marching(FakeEngine):
        def march_run(self, *a, **k):
            raise AssertionError("marched")
    with pytest.raises(RuntimeError, match="march_set_integrals"):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Marching(), wake_integrals=True)
    with pytest.raises(RuntimeError, match="scalar_field"):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=FakeEngine(), wake_integrals=True, wake_energy_steps=(1, 5, 1))


def test_without_the_keyword_nothing_changes():
    kw = dict(CONFIG1, tf=1.0)
    sim = LUDVM(**kw, verbose=False, engine=FakeEngine())
    for name in ("integral_sums", "wake_energy", "wake_energy_steps"):
        assert not hasattr(sim, name), name
    assert "wake_integrals" not in sim._ctor and "wake_energy_steps" not in sim._ctor
    obs = LUDVM(**kw, verbose=False, engine=WI.FieldFakeEngine(), wake_integrals=True, wake_energy_steps=(1, 20, 3))
    assert obs._ctor["wake_integrals"] is True and obs._ctor["wake_energy_steps"] == [1, 20, 3]
    assert np.array_equal(obs.Cl, sim.Cl) and np.array_equal(obs.path["TEV"], sim.path["TEV"])


@pytest.mark.parametrize("history", ["full", "sparse"])
def test_checkpoint_resume_continues_the_rows(tmp_path, history):
    kw = dict(CONFIG1, tf=3.0)
    obs = dict(wake_integrals=True, wake_energy_steps=(2, 55, 5))
    ck = str(tmp_path / "ck.npz")
    a = LUDVM(**kw, verbose=False, engine=WI.FieldFakeEngine(), history=history, **obs)
    LUDVM(**kw, verbose=False, engine=WI.FieldFakeEngine(), history=history, checkpoint_every=23, checkpoint_path=ck, **obs)
    R = np.load(ck)
    assert int(R["next_step"]) == 47 and R["integral_sums"].shape == (47, 4, 2, 6) and R["wake_energy"].shape == (47,)
    c = LUDVM.resume(ck, engine=WI.FieldFakeEngine(), verbose=False)
    assert c.wake_energy_steps == (2, 55, 5)
    assert np.array_equal(c.integral_sums, a.integral_sums) and np.array_equal(c.wake_energy, a.wake_energy, equal_nan=True)
    assert np.array_equal(c.Cl, a.Cl)
    assert a.integral_sums[47:, WI.LEV, :, 0].max() > 0          # (the resumed part has LEVs whose tags come from the slot maps)
    with pytest.raises(ValueError, match="one GPU"):
        LUDVM.resume(ck, devices=[0, 1], verbose=False)


def test_abi_7_declares_and_exports_the_entry_points():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    for name, nargs in (("ludvm_march_set_integrals", 7), ("ludvm_march_read_integrals", 4)):
        assert name in _ffi.SIGNATURES and name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name)
        assert hasattr(_ffi.load(_ffi.EXP_LIB_PATH), name)
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header).group(1)
        assert len(decl.split(",")) == len(_ffi.SIGNATURES[name]) == nargs
    assert re.search(r"#define\s+LUDVM_INTEGRAL_SUMS\s+48", header)
    assert lib.ludvm_march_set_integrals(None, 1, None, 0, 0, 0, 0) == _ffi.E_ARG
    assert lib.ludvm_march_read_integrals(None, None, None, 0) == _ffi.E_ARG


def test_the_launch_rule_is_a_constant_of_its_own():
    """kObserverKinds and kObserverRules stay as they were; the energy's rule stands next to them"""
    text = open(os.path.join(ROOT, "ludvm_amd", "csrc", "plan_rule.hpp")).read()
    assert "kObsSurveyF32, kObserverKinds }" in text
    assert re.search(r"constexpr ObserverRule kEnergyRule = \{512, 256, 1024, 64\};", text)


def test_integral_kernels_use_no_scratch():
    """Register budget of the five kernels as hipcc compiles them for gfx950 (no GPU needed): no scratch, no spills."""
    src = os.path.join(ROOT, "ludvm_amd", "csrc", "march.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull],
                         check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            kernels[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            kernels[cur][k.strip()] = v.strip()
    mine = {k: v for k, v in kernels.items() if "march_integral_" in k or "march_energy_" in k}
    assert len(mine) == 5, sorted(mine)
    for name, r in mine.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (name, r)
