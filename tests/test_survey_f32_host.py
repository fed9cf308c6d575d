"""CPU tier: the fp32 wake survey (LUDVM(..., survey=..., survey_precision='f32')) -- the keyword's
refusals and what the object carries, the sweep's refusals, the C ABI of ludvm_march_set_survey_precision, the compiler's
report of march_f32_survey_partial, and a NumPy restatement of the scheme (tests/survey_f32_common.py) against the float64
field far from the coordinate origin.  The kernel itself runs in tests/test_gpu_survey_f32.py."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from probes_common import probes32
from survey_f32_common import (FAR_X, MAX_EXTENT, MEAN_VS_F64, far_cloud, far_sheet, f64_field, field_error, local_f32_field,
                               points_around)


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before survey_precision was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    ok = np.zeros([2, 3])
    with pytest.raises(ValueError, match="survey_precision needs `survey`"):
        LUDVM(**CONFIG1, verbose=False, survey_precision="f32")
    for bad in ("f16", "F32", "f32x2", 1, None, 32.0):
        with pytest.raises(ValueError, match="survey_precision must be"):
            LUDVM(**CONFIG1, verbose=False, survey=ok, survey_precision=bad)
        with pytest.raises(ValueError, match="survey_precision must be"):
            LUDVM(**CONFIG1, verbose=False, survey_precision=bad)
    with pytest.raises(ValueError, match="march=False"):
        LUDVM(**CONFIG1, verbose=False, survey=ok, survey_precision="f32", march=False)
    with pytest.raises(ValueError, match="survey_precision"):
        LUDVM(**CONFIG1, verbose=False, survey=ok, survey_precision="f32", march=False, run=False)


def _public(sim):
    return {k: v for k, v in vars(sim).items() if k not in ("engine", "path", "start_time", "etime", "elapsed")}


def test_f64_is_the_default_and_changes_nothing():
    """survey_precision='f64' and no keyword over the fake engine: the same attributes, the same stored constructor keywords
    (so the same checkpoints); without a survey the object carries no survey attribute at all."""
    kw = dict(CONFIG1, tf=1.0)
    pts = probes32()
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_steps=(2, 20, 3))
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_steps=(2, 20, 3), survey_precision="f64")
    assert a.survey_precision == b.survey_precision == "f64"
    assert a._ctor == b._ctor and "survey_precision" not in a._ctor
    va, vb = _public(a), _public(b)
    assert set(va) == set(vb)
    for key in va:
        if isinstance(va[key], np.ndarray):
            assert np.array_equal(va[key], vb[key], equal_nan=True), key
        elif isinstance(va[key], (int, float, str, tuple, bool, type(None))):
            assert va[key] == vb[key], key
    assert np.array_equal(a.survey_sums, b.survey_sums) and a.survey_count == b.survey_count == 6
    plain = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey_precision="f64")
    assert not any(k.startswith("survey") for k in vars(plain)) and not any(k.startswith("survey") for k in plain._ctor)
    # 'f32' travels with the constructor keywords a checkpoint stores
    c = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_precision="f32", run=False)
    assert c.survey_precision == "f32" and c._ctor["survey_precision"] == "f32"


def test_no_silent_fallback_to_float64():
    """'f32' over an engine that does not march, and over one that marches without the new entry: RuntimeError, no run."""
    kw = dict(CONFIG1, tf=1.0)
    with pytest.raises(RuntimeError, match="survey_precision='f32'"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=[[1.0], [0.5]], survey_precision="f32")

    class Marcher(FakeEngine):
        def march_run(self, *a, **k):
            raise AssertionError("the march was entered")

        def march_setup(self, *a, **k):
            raise AssertionError("the march was set up")

        def march_set_survey(self, *a, **k):
            raise AssertionError("the survey was set")
    with pytest.raises(RuntimeError, match="march_set_survey_precision"):
        LUDVM(**kw, verbose=False, engine=Marcher(), survey=[[1.0], [0.5]], survey_precision="f32")
    # a method the march does not take, with an engine that has everything: raised before a step is run
    class Full(Marcher):
        def march_set_survey_precision(self, *a, **k):
            raise AssertionError("the precision was set")
    with pytest.raises(RuntimeError, match="survey_precision='f32'"):
        LUDVM(**dict(kw, Ncoeffs=70), verbose=False, engine=Full(), survey=[[1.0], [0.5]], survey_precision="f32")


def test_a_sweep_refuses_the_keyword():
    member = dict(CONFIG1, tf=1.0)
    ok = np.zeros([2, 3])
    for value in ("f32", "f64"):
        with pytest.raises(ValueError, match="sweep: survey_precision"):
            LUDVM.sweep([member, member], survey=ok, survey_precision=value)
        with pytest.raises(ValueError, match="sweep: survey_precision"):
            LUDVM.sweep([member], survey_precision=value)
        with pytest.raises(ValueError, match=r"sweep: member 1: survey_precision"):
            LUDVM.sweep([member, dict(member, survey_precision=value)], survey=ok)


def test_header_exports_and_binding_agree_on_the_new_entry():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    name = "ludvm_march_set_survey_precision"
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert name in _ffi.SIGNATURES and name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*ludvm_ctx\s*\*\s*ctx\s*,\s*int\s+precision\s*\)", code)
    assert re.search(r"\bT " + name + r"$", exported, flags=re.M)
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    assert _ffi.SURVEY_PRECISIONS == {"f64": 0, "f32": 1}
    assert lib.ludvm_march_set_survey_precision(None, 1) == _ffi.E_ARG
    # the constants the tests and the binding restate
    kernels = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    assert int(re.search(r"constexpr int kSurveyF32PerLane = (\d+);", kernels).group(1)) == _ffi.SURVEY_F32_PER_LANE
    assert float(re.search(r"constexpr double kSurveyF32MaxExtent = ([\d.]+);", kernels).group(1)) == MAX_EXTENT


def test_the_fp32_survey_kernel_uses_no_scratch():
    """The compiler's report of march_f32_survey_partial for gfx950 (no GPU needed), through tools/kernel_resources.py: no
    scratch, no spills; the figures DESIGN.md section 4.11 quotes are printed."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    found = {k: v for k, v in mod.resources(unit="march.hip").items() if "march_f32_survey_partial" in k}
    assert len(found) == 1
    (name, r), = found.items()
    print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) <= 16384 and int(r["Occupancy [waves/SIMD]"]) >= 4, r


@pytest.mark.parametrize("which", ["cloud", "sheet"])
def test_the_scheme_keeps_the_bound_far_from_the_origin_and_plain_fp32_does_not(which):
    """G5's free-vortex cloud (v_core of its run) and a 600-vortex sheet 1e-3 apart (v_core 1.3e-3), both at x = -55, at
    points on the vortices, within one core of them and several chords away: the restated scheme within 1e-5 of max|u| of
    the float64 field, no class guarded.  The same sums on coordinates rounded to float32 as they stand are not, on the sheet
    (1e-3 and more).  On the cloud they come to 9.7e-6 -- its core, 0.065, is 17 000 roundings of x = -55 wide, so plain
    float32 sits AT the bound there, not past it -- against 1.6e-7 with local origins: there the test tells the two apart by
    their ratio, the 2^7 between the rounding of a coordinate near 55 and that of an offset below 0.5, less a margin of 4."""
    if which == "cloud":
        g, x, z = far_cloud()
        v_core = float(np.load(os.path.join(ROOT, "tests", "golden", "g5_freevort.npz"))["v_core"])
    else:
        g, x, z = far_sheet()
        v_core = 1.3e-3
    assert abs(x.mean() - FAR_X) < 1.0
    pts = points_around(x, z, v_core)
    ref = f64_field(g, x, z, pts[0], pts[1], v_core)
    u, w, guarded, classes = local_f32_field(g, x, z, pts[0], pts[1], v_core)
    e_local = field_error((u, w), ref)
    up, wp, _, _ = local_f32_field(g, x, z, pts[0], pts[1], v_core, plain=True)
    e_plain = field_error((up, wp), ref)
    print(f"{which}: {len(g)} vortices at x = {FAR_X}, {pts.shape[1]} points: local origins {e_local:.2e} of max|u| "
          f"({guarded} of {classes} classes guarded), plain float32 coordinates {e_plain:.2e}")
    assert guarded == 0 and classes == 2 * ((len(g) + 255) // 256)
    assert e_local <= MEAN_VS_F64, e_local
    if which == "sheet":
        assert e_plain > MEAN_VS_F64, e_plain
    else:
        assert e_plain > 32 * e_local, (e_plain, e_local)


def test_the_guard_takes_a_sparse_class_and_leaves_float64_arithmetic():
    """A sheet stretched to 10 v_core between neighbours: every class is wider than 300 v_core, is guarded, and the result is
    the float64 field to rounding."""
    g, x, z = far_sheet(spacing=10 * 1.3e-3)
    pts = points_around(x, z, 1.3e-3)
    u, w, guarded, classes = local_f32_field(g, x, z, pts[0], pts[1], 1.3e-3)
    assert guarded == classes == 6
    assert field_error((u, w), f64_field(g, x, z, pts[0], pts[1], 1.3e-3)) <= 1e-12
