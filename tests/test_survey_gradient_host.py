"""CPU tier: gradient sums of the wake survey (LUDVM(..., survey=, survey_gradient=True)) -- the identity
behind Q in np.longdouble, the keyword's refusals (from the keywords alone), the sweep's refusals, what the object and its
constructor keywords carry, the C ABI of the two entry points, the compiler's report of the three kernels, and the per-step path
with its checkpoint over a FakeEngine whose gradient_field is tests/gradient_common.py's reference.  The kernels themselves run in
tests/test_gpu_survey_gradient.py."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import gradient_common as GC
import survey_gradient_common as SG
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM

NAMES = ("ludvm_march_set_survey_gradient", "ludvm_march_read_survey_gradient")
PTS = np.stack([np.linspace(-1.5, 1.0, 7), np.array([0.7, 0.9, 1.05, 1.2, 0.95, 1.1, 0.8])])


def test_q_is_the_same_in_both_forms_in_long_double():
    """Q = om^2 / 4 - ux^2 - e^2 = -ux^2 - uz wx, for any three components: a few ulp of long double of the largest product."""
    rng = np.random.default_rng(11)
    ux, uz, wx = (rng.normal(0.0, 10.0 ** rng.uniform(-3, 3, 5000)).astype(GC.LD) for _ in range(3))
    _, e, om, om2, q = SG.terms_from_gradient_ld(ux, uz, wx)
    other = -ux * ux - uz * wx
    scale = np.maximum.reduce([ux * ux, uz * uz, wx * wx])
    assert (np.abs(q - other) <= 8 * np.finfo(GC.LD).eps * scale).all()
    assert np.array_equal(om2, om * om) and np.array_equal(e, (uz + wx) / 2)
    # ... and on the closed forms themselves: a wake-like source set, points inside and outside the cores
    g, xs, zs = GC.wake_strip(300)
    xt, zt = GC.targets(64)
    xt[:8], zt[:8] = xs[:8] + 0.3 * GC.V_CORE, zs[:8]            # (inside a core: om and a positive Q)
    (cux, cuz, cwx), _ = GC.reference_ld(g, xs, zs, xt, zt, GC.V_CORE)
    t = SG.terms_from_gradient_ld(cux, cuz, cwx)
    scale = np.maximum.reduce([cux * cux, cuz * cuz, cwx * cwx])
    assert (np.abs(t[4] - (-cux * cux - cuz * cwx)) <= 8 * np.finfo(GC.LD).eps * scale).all()
    assert np.abs(t[2]).max() > 0.0 and (t[4] > 0).any() and (t[4] < 0).any()


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before survey_gradient was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    import ludvm_amd.multi as multi
    monkeypatch.setattr(multi, "MultiDeviceLUDVM", NoEngine)
    with pytest.raises(ValueError, match="survey_gradient needs `survey`"):
        LUDVM(**CONFIG1, verbose=False, survey_gradient=True)
    for bad in ("yes", 1, None, 1.0):
        with pytest.raises(ValueError, match="survey_gradient must be True or False"):
            LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=bad)
    with pytest.raises(ValueError, match="survey_gradient needs a float64 survey.*f32"):
        LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=True, survey_precision="f32")
    for dist in ("rccl", True):
        with pytest.raises(ValueError, match="one GPU"):
            LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=True, distributed=dist)
    with pytest.raises(ValueError, match="survey_gradient runs on one GPU.*devices"):
        LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=True, devices=[0, 1])
    with pytest.raises(ValueError, match="survey_gradient needs `survey`"):
        LUDVM(**CONFIG1, verbose=False, survey_gradient=True, devices=2)
    with pytest.raises(ValueError, match="survey_gradient must be True or False"):
        LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient="on", devices=2)


def test_a_sweep_refuses_the_keyword():
    member = dict(CONFIG1, tf=1.0)
    for value in (True, False):
        with pytest.raises(ValueError, match=r"sweep: survey_gradient.*LUDVM\(\.\.\., survey="):
            LUDVM.sweep([member, member], survey=PTS, survey_gradient=value)
        with pytest.raises(ValueError, match=r"sweep: member 1: survey_gradient.*LUDVM\(\.\.\., survey="):
            LUDVM.sweep([member, dict(member, survey_gradient=value)], survey=PTS)


class GradEngine(FakeEngine):
    """FakeEngine with `gradient_field` answered by tests/gradient_common.py's long-double reference."""

    def gradient_field(self, circulation, xw, zw, xp, zp, v_core):
        (ux, uz, wx), _ = GC.reference(circulation, xw, zw, xp, zp, v_core)
        return ux, uz, wx


def test_false_is_the_default_and_the_constructor_keywords_carry_only_true():
    kw = dict(CONFIG1, tf=1.0)
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS)
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS, survey_gradient=False)
    assert a.survey_gradient is False and b.survey_gradient is False
    assert a._ctor == b._ctor and "survey_gradient" not in a._ctor
    assert not any(k.startswith("survey_grad_") or k in ("survey_mean_omega", "survey_mean_q") for k in vars(a))
    assert np.array_equal(a.survey_sums, b.survey_sums)
    plain = LUDVM(**kw, verbose=False, engine=FakeEngine())
    assert not any(k.startswith("survey") for k in vars(plain)) and not any(k.startswith("survey") for k in plain._ctor)
    c = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS, survey_gradient=True, run=False)
    assert c.survey_gradient is True and c._ctor["survey_gradient"] is True


class Marcher(FakeEngine):
    def march_run(self, *a, **k):
        raise AssertionError("the march was entered")

    def march_setup(self, *a, **k):
        raise AssertionError("the march was set up")

    def march_set_survey(self, *a, **k):
        raise AssertionError("the survey was set")


def test_an_engine_that_cannot_serve_it_raises():
    """An engine that marches without the new entry point, and a per-step run over an engine without gradient_field:
    RuntimeError, no step run."""
    kw = dict(CONFIG1, tf=1.0)
    with pytest.raises(RuntimeError, match="march_set_survey_gradient"):
        LUDVM(**kw, verbose=False, engine=Marcher(), survey=PTS, survey_gradient=True)
    with pytest.raises(RuntimeError, match="survey_gradient.*gradient_field"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS, survey_gradient=True)
    with pytest.raises(RuntimeError, match="survey_gradient.*gradient_field"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS, survey_gradient=True, march=False)


def test_the_class_sets_the_gradient_behind_the_survey_and_its_bins():
    seen = []

    class Stop(Exception):
        pass

    class Recorder(FakeEngine):
        def march_setup(self, *a, **k):
            seen.append("setup")

        def march_set_survey(self, *a, **k):
            seen.append("survey")

        def march_set_survey_bins(self, *a, **k):
            seen.append("bins")

        def march_set_survey_gradient(self, on, gsums=None, bin_gsums=None):
            seen.append(("gradient", on, gsums, bin_gsums))

        def march_anchor_steps(self, *a, **k):
            raise Stop

        def march_run(self, *a, **k):
            raise Stop
    kw = dict(CONFIG1, tf=1.0)
    with pytest.raises(Stop):
        LUDVM(**kw, verbose=False, engine=Recorder(), history="sparse", survey=PTS, survey_bins=4, survey_period=0.5,
              survey_gradient=True)
    assert seen == ["setup", "survey", "bins", ("gradient", True, None, None)]
    del seen[:]
    with pytest.raises(Stop):
        LUDVM(**kw, verbose=False, engine=Recorder(), history="sparse", survey=PTS)
    assert seen == ["setup", "survey"]


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1)


def test_header_exports_and_binding_agree_on_the_new_entries():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # additions to ABI 7: detected by symbol
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        params = [p.strip() for p in _prototype(name).split(",")]
        assert len(params) == len(_ffi.SIGNATURES[name]) and params[0].startswith("ludvm_ctx*"), (name, params)
        assert name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name) and hasattr(_ffi.load(_ffi.EXP_LIB_PATH), name)
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M)
    assert lib.ludvm_march_set_survey_gradient(None, 1, None, None) == _ffi.E_ARG
    assert lib.ludvm_march_read_survey_gradient(None, None, None) == _ffi.E_ARG
    from ludvm_amd.engine import Engine
    assert hasattr(Engine, "march_set_survey_gradient") and hasattr(Engine, "march_survey_gradient")


def test_the_gradient_survey_kernels_use_no_scratch_and_the_plain_ones_are_compiled_as_before():
    """march_grad_survey_partial / march_grad_survey_finish / march_binned_grad_survey_finish for gfx950 through
    tools/kernel_resources.py (no GPU needed): no scratch, no spills, the three float64 planes of one 256-source tile in LDS.
    march_survey_partial / march_survey_finish / march_binned_survey_finish beside them keep the registers and LDS the commit
    before this feature compiled them with (52 VGPRs, 6144 bytes; 14 VGPRs, none; 14 VGPRs, none)."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.resources(unit="march.hip")
    for kernel, lds in (("march_grad_survey_partial", 3 * 256 * 8), ("march_grad_survey_finish", 0),
                        ("march_binned_grad_survey_finish", 0)):
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) == lds, (name, r)
    for kernel, want in {"march_survey_partial": (52, 6144, 0), "march_survey_finish": (14, 0, 0),
                         "march_binned_survey_finish": (14, 0, 0)}.items():
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        assert (int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"])) == want, (name, r)


class NotingEngine(GradEngine):
    """... that also notes the sources and points of every gradient_field call, in call order."""

    def __init__(self):
        super().__init__()
        self.noted = []

    def gradient_field(self, circulation, xw, zw, xp, zp, v_core):
        self.noted.append(tuple(np.array(a, dtype=float) for a in (circulation, xw, zw, xp, zp)))
        return super().gradient_field(circulation, xw, zw, xp, zp, v_core)


@pytest.fixture(scope="module")
def per_step_run():
    eng = NotingEngine()
    kw = dict(CONFIG1, tf=1.5)
    table = np.full(31, -1)
    table[4:26] = np.arange(22) % 3
    sim = LUDVM(**kw, verbose=False, engine=eng, march=False, survey=PTS, survey_frame="tunnel", survey_steps=(3, 28, 2),
                survey_bins=table, survey_gradient=True)
    return sim, eng, table


def test_the_per_step_path_adds_the_five_terms_of_every_sampled_step(per_step_run):
    """march=False over the fake engine: one gradient_field call per sampled step, over the step's sources (old wake, shed
    vortices, bound vortices: as many as the step's velocity calls see) at the step's points; the sums are the NumPy recursion
    over the long-double terms of exactly those calls -- to 1e-12 of the scales (the host forms e, om and Q from rounded float64
    components) -- and every bin's block is the recursion over its own steps.  The derived attributes follow from the sums."""
    sim, eng, table = per_step_run
    W = list(range(3, 28, 2))
    assert sim.survey_count == len(W) == len(eng.noted)
    ref, bref, gmax = np.zeros([5, 7]), np.zeros([3, 5, 7]), 0.0
    for i, (g, x, z, px, pz) in zip(W, eng.noted):
        assert np.array_equal(px, PTS[0] + sim.xpiv[i]) and np.array_equal(pz, PTS[1])
        # (the resident wake of step i: i trailing-edge slots -- slot 0 is the start-up vortex -- and the leading-edge ones)
        assert len(g) == i + int((sim.LEV_shed[:i] != -1).sum()) + 1 + int(sim.LEV_shed[i] != -1) + sim.Npoints - 1
        t, m = SG.step_terms((g, x, z, np.zeros(0), np.zeros(0), np.zeros(0)), px, pz, sim.v_core)
        ref += t
        gmax = max(gmax, m)
        if table[i] >= 0:
            bref[table[i]] += t
    e_mean, e_sq = SG.sums_errors(sim.survey_grad_sums, ref, len(W), gmax)
    print(f"per-step sums vs the long-double recursion: means {e_mean:.2e} of max|grad u| ({gmax:.3f}), squares {e_sq:.2e}")
    assert gmax > 0.1 and e_mean <= 1e-12 and e_sq <= 1e-12
    assert sim.survey_bin_grad_sums.shape == (3, 5, 7)
    for b in range(3):
        nb = int(sim.survey_bin_count[b])
        assert nb == sum(1 for i in W if table[i] == b) > 0
        eb = SG.sums_errors(sim.survey_bin_grad_sums[b], bref[b], nb, gmax)
        assert max(eb) <= 1e-12, (b, eb)
    SG.check_derived(sim)
    SG.check_bin_derived(sim)


def test_a_checkpoint_inside_the_window_and_a_resume_reproduce_the_sums(per_step_run, tmp_path):
    sim, _, table = per_step_run
    ck = str(tmp_path / "ck.npz")
    kw = dict(CONFIG1, tf=1.5)
    LUDVM(**kw, verbose=False, engine=GradEngine(), march=False, survey=PTS, survey_frame="tunnel", survey_steps=(3, 28, 2),
          survey_bins=table, survey_gradient=True, checkpoint_every=12, checkpoint_path=ck)
    R = np.load(ck, allow_pickle=False)
    assert 3 < int(R["next_step"]) < 28 and 0 < int(R["survey_samples"]) < sim.survey_count
    assert R["survey_grad_sums"].shape == (5, 7) and R["survey_bin_grad_sums"].shape == (3, 5, 7)
    assert np.abs(R["survey_grad_sums"]).max() > 0.0 and "survey_gradient" in str(R["ctor"])
    again = LUDVM.resume(ck, engine=GradEngine(), verbose=False, march=False)
    assert again.survey_gradient is True and again.survey_count == sim.survey_count
    assert np.array_equal(again.survey_grad_sums, sim.survey_grad_sums)
    assert np.array_equal(again.survey_bin_grad_sums, sim.survey_bin_grad_sums)
    assert np.array_equal(again.survey_sums, sim.survey_sums) and np.array_equal(again.survey_bin_sums, sim.survey_bin_sums)
    assert np.array_equal(again.survey_production, sim.survey_production)
