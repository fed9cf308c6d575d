"""CPU tier: the survey's gradient sums in hi+lo fp32 (LUDVM(..., survey=, survey_gradient='f32x2')) -- the
keyword's refusals (from the keywords alone), the sweep's refusals, the defaults as they were, the errors of an engine that cannot
serve it, the call order, what the object and a checkpoint carry and what a resume hands back, the C ABI of the new entry, the
compiler's report of the new kernel and of its neighbours, and the derived tolerance held against the NumPy restatement of the
fused walk.  The kernel itself runs in tests/test_gpu_survey_gradient_f32x2.py."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gradient_common as GC
import gradient_f32x2_common as GF
import survey_gradient_common as SG
import survey_gradient_f32x2_common as C
import tracer_gradient_f32x2_common as TF
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from survey_f32_common import far_sheet, points_around
from tracers_common import seeds_random

NAME = "ludvm_march_set_survey_gradient_f32x2"
PTS = np.stack([np.linspace(-1.5, 1.0, 7), np.array([0.7, 0.9, 1.05, 1.2, 0.95, 1.1, 0.8])])
F32 = dict(survey=PTS, survey_gradient="f32x2")


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before survey_gradient was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    import ludvm_amd.multi as multi
    monkeypatch.setattr(multi, "MultiDeviceLUDVM", NoEngine)
    with pytest.raises(ValueError, match="survey_gradient needs `survey`"):
        LUDVM(**CONFIG1, verbose=False, survey_gradient="f32x2")
    # the route is not a survey precision, and takes none beside it
    for prec in ("f32", "f32x2"):
        with pytest.raises(ValueError, match="survey_gradient='f32x2' brings its own arithmetic.*survey_precision='%s'" % prec):
            LUDVM(**CONFIG1, verbose=False, **F32, survey_precision=prec)
    with pytest.raises(ValueError, match="survey_precision must be"):
        LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_precision="f32x2")
    # other values keep their message, extended; True keeps every message it has
    for bad in ("f32", "F32X2", "f64", "yes", 1, 2, None, 1.0):
        with pytest.raises(ValueError, match="^survey_gradient must be True or False, or 'f32x2' \\(got "):
            LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=bad)
    with pytest.raises(ValueError, match="survey_gradient needs a float64 survey.*f32"):
        LUDVM(**CONFIG1, verbose=False, survey=PTS, survey_gradient=True, survey_precision="f32")
    for kw in (dict(march=False), dict(march=False, run=False)):
        with pytest.raises(ValueError, match="survey_gradient='f32x2' is evaluated inside the device-resident march: not with march=False"):
            LUDVM(**CONFIG1, verbose=False, **F32, **kw)
    with pytest.raises(ValueError, match="march=False"):
        M.LUDVM._check_survey_gradient("f32x2", True, "f64", False)
    M.LUDVM._check_survey_gradient(True, True, "f64", False)             # (the float64 sums have a per-step path)
    for dist in ("rccl", True):
        with pytest.raises(ValueError, match="one GPU"):
            LUDVM(**CONFIG1, verbose=False, **F32, distributed=dist)
    with pytest.raises(ValueError, match="survey_gradient runs on one GPU.*devices"):
        LUDVM(**CONFIG1, verbose=False, **F32, devices=[0, 1])
    with pytest.raises(ValueError, match="survey_gradient needs `survey`"):
        LUDVM(**CONFIG1, verbose=False, survey_gradient="f32x2", devices=2)
    with pytest.raises(ValueError, match="march=False"):
        LUDVM(**CONFIG1, verbose=False, **F32, march=False, devices=2)


def test_a_sweep_refuses_the_value():
    member = dict(CONFIG1, tf=1.0)
    with pytest.raises(ValueError, match=r"sweep: survey_gradient='f32x2'.*LUDVM\(\.\.\., survey="):
        LUDVM.sweep([member, member], survey=PTS, survey_gradient="f32x2")
    with pytest.raises(ValueError, match=r"sweep: member 1: survey_gradient='f32x2'.*LUDVM\(\.\.\., survey="):
        LUDVM.sweep([member, dict(member, survey_gradient="f32x2")], survey=PTS)


class GradEngine(FakeEngine):
    def gradient_field(self, circulation, xw, zw, xp, zp, v_core):
        (ux, uz, wx), _ = GC.reference(circulation, xw, zw, xp, zp, v_core)
        return ux, uz, wx


def test_false_and_true_behave_store_and_checkpoint_as_before(tmp_path):
    kw = dict(CONFIG1, tf=1.0)
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS)
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=PTS, survey_gradient=False)
    assert a.survey_gradient is False and b.survey_gradient is False
    assert a._ctor == b._ctor and "survey_gradient" not in a._ctor and not hasattr(a, "survey_grad_sums")
    ck = str(tmp_path / "ck.npz")
    c = LUDVM(**kw, verbose=False, engine=GradEngine(), march=False, survey=PTS, survey_gradient=True, checkpoint_every=12,
              checkpoint_path=ck)
    assert c.survey_gradient is True and c._ctor["survey_gradient"] is True
    SG.check_derived(c)
    R = np.load(ck, allow_pickle=False)
    assert json.loads(str(R["ctor"]))["survey_gradient"] is True and R["survey_grad_sums"].shape == (5, 7)
    again = LUDVM.resume(ck, engine=GradEngine(), verbose=False, march=False)
    assert again.survey_gradient is True and np.array_equal(again.survey_grad_sums, c.survey_grad_sums)
    assert np.array_equal(again.survey_sums, c.survey_sums)
    d = LUDVM(**kw, verbose=False, engine=FakeEngine(), **F32, run=False)
    assert d.survey_gradient == "f32x2" and d.survey_gradient and d._ctor["survey_gradient"] == "f32x2"
    assert d.survey_precision == "f64" and "survey_precision" not in d._ctor


class Marcher(FakeEngine):
    def march_run(self, *a, **k):
        raise AssertionError("the march was entered")

    def march_setup(self, *a, **k):
        raise AssertionError("the march was set up")

    def march_set_survey(self, *a, **k):
        raise AssertionError("the survey was set")

    def march_set_survey_gradient(self, *a, **k):
        raise AssertionError("the float64 gradient was set")


def test_a_run_that_cannot_take_the_march_raises():
    """survey_gradient='f32x2' over an engine that does not march (with or without gradient_field: no per-step float64 in its
    place), over one that marches with the float64 setter but without the new entry, and in a run the march does not take:
    RuntimeError, no step run."""
    kw = dict(CONFIG1, tf=1.0)
    for eng in (FakeEngine(), GradEngine()):
        with pytest.raises(RuntimeError, match="survey_gradient='f32x2'.*cannot take"):
            LUDVM(**kw, verbose=False, engine=eng, **F32)
        assert eng.calls["advect"] == 0 and eng.calls.get("step", 0) == 0
    with pytest.raises(RuntimeError, match="survey_gradient='f32x2'.*march_set_survey_gradient_f32x2"):
        LUDVM(**kw, verbose=False, engine=Marcher(), **F32)

    class Full(Marcher):
        def march_set_survey_gradient_f32x2(self, *a, **k):
            raise AssertionError("the gradient was set")
    with pytest.raises(RuntimeError, match="survey_gradient='f32x2'.*cannot take"):
        LUDVM(**dict(kw, Ncoeffs=70), verbose=False, engine=Full(), **F32)


class Stop(Exception):
    pass


class Recorder(FakeEngine):
    """notes the march's set calls and stops the run at the first thing a march call asks the engine"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def march_setup(self, *a, **k):
        self.seen.append("setup")

    def march_set_survey(self, *a, **k):
        self.seen.append("survey")

    def march_set_survey_precision(self, precision):
        self.seen.append(("precision", precision))

    def march_set_survey_bins(self, *a, **k):
        self.seen.append("bins")

    def march_set_survey_gradient(self, on, gsums=None, bin_gsums=None):
        self.seen.append(("gradient", on, gsums, bin_gsums))

    def march_set_survey_gradient_f32x2(self, gsums=None, bin_gsums=None):
        self.seen.append(("gradient_f32x2", gsums, bin_gsums))

    def march_anchor_steps(self, *a, **k):
        raise Stop

    def march_run(self, *a, **k):
        raise Stop


def test_the_class_calls_the_one_setter_behind_the_survey_and_its_bins():
    kw = dict(CONFIG1, tf=1.0)
    rec = Recorder()
    with pytest.raises(Stop):
        LUDVM(**kw, verbose=False, engine=rec, history="sparse", **F32, survey_bins=4, survey_period=0.5)
    assert rec.seen == ["setup", "survey", "bins", ("gradient_f32x2", None, None)]
    rec = Recorder()
    with pytest.raises(Stop):
        LUDVM(**kw, verbose=False, engine=rec, history="sparse", **F32)
    assert rec.seen == ["setup", "survey", ("gradient_f32x2", None, None)]
    rec = Recorder()
    with pytest.raises(Stop):
        LUDVM(**kw, verbose=False, engine=rec, history="sparse", survey=PTS, survey_bins=4, survey_period=0.5, survey_gradient=True)
    assert rec.seen == ["setup", "survey", "bins", ("gradient", True, None, None)]


class StateEngine(FakeEngine):
    """what `_write_checkpoint_file` asks of a marching engine that carries a binned gradient survey"""

    def __init__(self, sums, samples, bsums, bcounts, gsums, bgsums):
        super().__init__()
        self._state = (sums, samples, bsums, bcounts, gsums, bgsums)

    def march_survey(self):
        return self._state[0].copy(), self._state[1]

    def march_survey_bins(self):
        return self._state[2].copy(), self._state[3].copy()

    def march_survey_gradient(self):
        return self._state[4].copy(), self._state[5].copy()


def test_a_checkpoint_carries_the_route_and_a_resume_hands_both_sum_arrays_back(tmp_path):
    """`survey_gradient` holds 'f32x2', the stored constructor keywords name it, the checkpoint carries the gradient sums and their
    bin blocks as the float64 route's does, and LUDVM.resume sets survey, bins and then the route through the new method with
    exactly the stored arrays."""
    rng = np.random.default_rng(5)
    sums, bsums = rng.normal(0, 1, (5, 7)), rng.normal(0, 1, (3, 5, 7))
    gsums, bgsums = rng.normal(0, 1, (5, 7)), rng.normal(0, 1, (3, 5, 7))
    bcounts = np.array([2, 1, 1], dtype=np.int64)
    ck = str(tmp_path / "ck.npz")
    kw = dict(CONFIG1, tf=1.0)
    sim = LUDVM(**kw, verbose=False, engine=StateEngine(sums, 4, bsums, bcounts, gsums, bgsums), history="sparse", **F32,
                survey_steps=(2, 20, 1), survey_bins=3, survey_period=0.3, run=False, checkpoint_path=ck)
    assert sim.survey_gradient == "f32x2"
    S = sim._loop_begin()
    sim._free_slot, sim.itev, sim.ilev = S.fslot, 0, 0     # (what time_loop has set by the time it writes a checkpoint)
    S.can_march = True
    assert S.sgsums.shape == (5, 7) and S.sbgsums.shape == (3, 5, 7)
    sim._write_checkpoint_file(S, 6)
    R = np.load(ck, allow_pickle=False)
    assert np.array_equal(R["survey_grad_sums"], gsums) and np.array_equal(R["survey_bin_grad_sums"], bgsums)
    assert int(R["survey_samples"]) == 4 and json.loads(str(R["ctor"]))["survey_gradient"] == "f32x2"
    rec = Recorder()
    with pytest.raises(Stop):
        LUDVM.resume(ck, engine=rec, verbose=False)
    assert rec.seen[:3] == ["setup", "survey", "bins"] and len(rec.seen) == 4
    name, g, bg = rec.seen[3]
    assert name == "gradient_f32x2" and np.array_equal(g, gsums) and np.array_equal(bg, bgsums)
    again = LUDVM(**json.loads(str(R["ctor"])), verbose=False, engine=FakeEngine(), run=False)
    assert again.survey_gradient == "f32x2" and again.survey_nbins == 3


def test_header_exports_and_binding_agree_on_the_new_entry():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert NAME in _ffi.SIGNATURES and len(_ffi.SIGNATURES[NAME]) == 3 and NAME in _ffi.ADDED_IN_ABI_7
    assert _ffi.SURVEY_PRECISIONS == {"f64": 0, "f32": 1}                 # (the route is not a survey precision)
    assert hasattr(lib, NAME) and hasattr(_ffi.load(_ffi.EXP_LIB_PATH), NAME)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*ludvm_ctx\s*\*\s*ctx\s*,\s*const\s+double\s*\*\s*gsums\s*,\s*const\s+double\s*\*\s*"
                     r"bin_gsums\s*\)\s*;", code)
    assert re.search(r"\bT " + NAME + r"$", exported, flags=re.M)
    assert getattr(lib, NAME)(None, None, None) == _ffi.E_ARG
    from ludvm_amd.engine import Engine
    assert callable(getattr(Engine, "march_set_survey_gradient_f32x2"))


def test_the_fused_survey_kernel_uses_no_scratch_and_its_neighbours_are_compiled_as_before():
    """march_f32x2_grad_survey_partial for gfx950 through tools/kernel_resources.py (no GPU needed): no scratch, no spills, the five
    float planes of one 256-source tile in LDS, at most 128 VGPRs (four waves per SIMD); the figures DESIGN.md section 4.20 quotes
    are printed.  The kernels beside it keep the registers, LDS and scratch the commit before this feature compiled them with."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.resources(unit="march.hip")
    (name, r), = {k: v for k, v in report.items() if "march_f32x2_grad_survey_partial" in k}.items()
    print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == 5 * TF.TILE * 4 == 5120 and int(r["VGPRs"]) <= 128, r
    assert int(r["Occupancy [waves/SIMD]"]) >= 4, r
    before = {"march_grad_survey_partial": (68, 6144, 0), "march_f32x2_grad_tracer_partial": (122, 5120, 0),
              "march_f32_survey_partial": (119, 9248, 0), "march_survey_partial": (52, 6144, 0),
              "march_survey_finish": (14, 0, 0), "march_binned_survey_finish": (14, 0, 0)}
    for kernel, want in before.items():
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        assert (int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"])) == want, (name, r)
    kernels = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    per_lane = {k: int(re.search(r"constexpr int %s = (\d+);" % k, kernels).group(1)) for k in ("kSurveyGradF32PerLane", "kSurveyF32PerLane")}
    assert per_lane["kSurveyF32PerLane"] % per_lane["kSurveyGradF32PerLane"] == 0      # whole workgroups per tile of the plan


def _tolerance_cases():
    """the GPU tier's point sets over gradient_common.wake_strip sources (moved to the points' box), and its sheet far away"""
    g, xs, zs = GC.wake_strip(1300)
    strip = (g, xs / 60.0 * 4.5 + 1.5, 1.0 + zs)                         # x in [-3, 1.5], z about 1: seeds_random's box
    cases = {"strip_600": (strip, seeds_random(600), GC.V_CORE),
             "strip_2049": (strip, seeds_random(2049, seed=17), GC.V_CORE)}
    for x0 in (-55.0, -5000.0):
        g, x, z = far_sheet(x0=x0)
        cases[f"sheet_at_{x0:g}"] = ((g, x, z), points_around(x, z, GF.V_CORE_SMALL), GF.V_CORE_SMALL)
    return cases


@pytest.mark.parametrize("name", ["strip_600", "strip_2049", "sheet_at_-55", "sheet_at_-5000"])
def test_the_restated_walk_stays_within_the_per_term_tolerance(name):
    """tracer_gradient_f32x2_common.fused_hilo_f32 -- the walk's NumPy restatement -- over one step's sources at the GPU tier's
    points; ux, e, om, om^2 and Q formed in float64 as the finisher forms them, against survey_gradient_common's long-double terms:
    each within survey_gradient_f32x2_common.step_tolerance, near the origin, at x = -55 and at x = -5000 with the small core; and
    the tolerance is below the cap of a point set."""
    (g, xs, zs), pts, v_core = _tolerance_cases()[name]
    src = (g, xs, zs, np.zeros(0), np.zeros(0), np.zeros(0))
    want, gmax = SG.step_terms(src, pts[0], pts[1], v_core)
    tol = C.step_tolerance(src, pts[0], pts[1], v_core, want)
    _, _, A, B, Cc = TF.fused_hilo_f32(g, xs, zs, pts[0], pts[1], v_core)
    ux, e, om = -A / np.pi, B / (2 * np.pi), -(v_core ** 4 * Cc) / np.pi
    got = np.stack([ux, e, om, om * om, 0.25 * (om * om) - ux * ux - e * e])
    scale = np.array([gmax] * 3 + [gmax ** 2] * 2)[:, None]
    allow = np.array([SG.MEAN_BOUND] * 3 + [SG.SQUARE_BOUND] * 2)[:, None] * scale
    ratio = np.abs(got - want) / (tol + allow)
    print(f"{name}: {len(g)} sources, {pts.shape[1]} points: worst error {ratio.max():.3f} of the tolerance "
          f"({', '.join(f'{n} {r:.3f}' for n, r in zip(SG.NAMES, ratio.max(axis=1)))}); {(np.abs(got - want) / scale).max():.2e} of "
          f"max|grad u| ({gmax:.3f}); largest tolerance {((tol + allow) / scale).max():.2e} of it")
    assert gmax > 0.0 and (ratio <= 1.0).all()
    assert ((tol + allow) / scale).max() < C.CAP
    assert not np.array_equal(got, want)
