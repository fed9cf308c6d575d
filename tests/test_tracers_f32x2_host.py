"""CPU tier: passive tracers in hi+lo fp32 (LUDVM(..., tracers=..., tracer_precision='f32x2')) -- a NumPy
restatement of the scheme (tests/tracers_f32x2_common.py) against the float64 field on the five cases of section 4.9's table,
the keyword's refusals and what the object carries, the sweep's refusals, the errors of an engine that cannot serve it, the
C ABI of ludvm_march_set_tracer_precision, and the compiler's report of march_f32x2_tracer_partial beside the two float64 tracer
kernels.  The kernel itself runs in tests/test_gpu_tracers_f32x2.py."""
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
from survey_f32_common import f64_field, field_error, points_around
from tracers_f32x2_common import TILE, VELOCITY_VS_F64, hilo_f32_field, table_cases

CASES = ("cloud256_at_-55", "cloud256_at_-5000", "sheet600_1e-3_at_-55", "sheet2000_5e-3", "sparse_cloud")


@pytest.mark.parametrize("which", CASES)
def test_the_scheme_keeps_the_hilo_tier_wherever_the_wake_is(which):
    """The restated scheme at points on the sources, within one core of them and 3 - 8 chords away: within 2e-6 of max|u| of
    the float64 field -- at x = -55 and at x = -5000 alike, on a sheet whose neighbours are 1e-3 apart, and on the two source
    sets every origin class of which is wider than 300 v_core (where the local-origin scheme of the survey falls to float64).
    Measured: 5.5e-7, 5.5e-7, 2.8e-7, 3.7e-7, 4.9e-7."""
    cases = table_cases()
    assert tuple(cases) == CASES
    g, x, z, v_core = cases[which]
    pts = points_around(x, z, v_core)
    ref = f64_field(g, x, z, pts[0], pts[1], v_core)
    err = field_error(hilo_f32_field(g, x, z, pts[0], pts[1], v_core), ref)
    print(f"{which}: {len(g)} vortices ({(len(g) + TILE - 1) // TILE} tiles), {pts.shape[1]} points: hi+lo fp32 {err:.2e} of max|u|")
    assert err <= VELOCITY_VS_F64, err


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before tracer_precision was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    ok = np.zeros([2, 3])
    with pytest.raises(ValueError, match="tracer_precision needs `tracers`"):
        LUDVM(**CONFIG1, verbose=False, tracer_precision="f32x2")
    for bad in ("f16", "F32X2", "f32", 2, None, 32.0):
        with pytest.raises(ValueError, match="tracer_precision must be"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_precision=bad)
        with pytest.raises(ValueError, match="tracer_precision must be"):
            LUDVM(**CONFIG1, verbose=False, tracer_precision=bad)
    with pytest.raises(ValueError, match="march=False"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_precision="f32x2", march=False)
    with pytest.raises(ValueError, match="tracer_precision"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_precision="f32x2", march=False, run=False)


def test_a_sweep_refuses_the_keyword():
    member = dict(CONFIG1, tf=1.0)
    ok = np.zeros([2, 3])
    for value in ("f32x2", "f64"):
        with pytest.raises(ValueError, match=r"sweep: tracer_precision.*LUDVM\(\.\.\., tracers="):
            LUDVM.sweep([member, member], particles=ok, tracer_precision=value)
        with pytest.raises(ValueError, match="sweep: tracer_precision"):
            LUDVM.sweep([member], tracer_precision=value)
        with pytest.raises(ValueError, match=r"sweep: member 1: tracer_precision.*LUDVM\(\.\.\., tracers="):
            LUDVM.sweep([member, dict(member, tracer_precision=value)], particles=ok)


def _public(sim):
    return {k: v for k, v in vars(sim).items() if k not in ("engine", "path", "start_time", "etime", "elapsed", "tracer_path")}


def test_f64_is_the_default_and_the_checkpoint_constructor_carries_only_f32x2():
    """tracer_precision='f64' and no keyword over the fake engine: the same attributes, the same stored constructor keywords
    (so the same checkpoints); without tracers the object carries no tracer attribute at all; 'f32x2' travels with the
    constructor keywords a checkpoint stores."""
    kw = dict(CONFIG1, tf=1.0)
    seeds = [[1.0, 0.4], [0.5, 1.2]]
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_release=[1, 7])
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_release=[1, 7], tracer_precision="f64")
    assert a.tracer_precision == b.tracer_precision == "f64"
    assert a._ctor == b._ctor and "tracer_precision" not in a._ctor
    va, vb = _public(a), _public(b)
    assert set(va) == set(vb)
    for key in va:
        if isinstance(va[key], np.ndarray):
            assert np.array_equal(va[key], vb[key], equal_nan=True), key
        elif isinstance(va[key], (int, float, str, tuple, bool, type(None))):
            assert va[key] == vb[key], key
    assert a.tracer_path.steps() == b.tracer_path.steps()
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s])
    plain = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracer_precision="f64")
    assert not any(k.startswith("tracer") for k in vars(plain)) and not any(k.startswith("tracer") for k in plain._ctor)
    c = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_precision="f32x2", run=False)
    assert c.tracer_precision == "f32x2" and c._ctor["tracer_precision"] == "f32x2"


def test_no_silent_fallback_to_float64():
    """'f32x2' over an engine that does not march, over one that marches without the new entry, and in a run the march does
    not take: RuntimeError, no step run."""
    kw = dict(CONFIG1, tf=1.0)
    with pytest.raises(RuntimeError, match="tracer_precision='f32x2'"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=[[1.0], [0.5]], tracer_precision="f32x2")

    class Marcher(FakeEngine):
        def march_run(self, *a, **k):
            raise AssertionError("the march was entered")

        def march_setup(self, *a, **k):
            raise AssertionError("the march was set up")

        def march_set_tracers(self, *a, **k):
            raise AssertionError("the tracers were set")
    with pytest.raises(RuntimeError, match="march_set_tracer_precision"):
        LUDVM(**kw, verbose=False, engine=Marcher(), tracers=[[1.0], [0.5]], tracer_precision="f32x2")

    class Full(Marcher):
        def march_set_tracer_precision(self, *a, **k):
            raise AssertionError("the precision was set")
    with pytest.raises(RuntimeError, match="tracer_precision='f32x2'.*cannot take"):
        LUDVM(**dict(kw, Ncoeffs=70), verbose=False, engine=Full(), tracers=[[1.0], [0.5]], tracer_precision="f32x2")


def test_the_engine_wrapper_sets_the_precision_behind_the_tracers():
    """An engine that marches and has the entry: the class sets the tracers, then 'f32x2', before the first march call."""
    seen = []

    class Stop(Exception):
        pass

    class Recorder(FakeEngine):
        def march_setup(self, *a, **k):
            seen.append("setup")

        def march_set_tracers(self, *a, **k):
            seen.append("tracers")

        def march_set_tracer_precision(self, precision):
            seen.append(("precision", precision))

        def march_anchor_steps(self, *a, **k):      # (the first thing a march call asks the engine)
            raise Stop

        def march_run(self, *a, **k):
            raise Stop
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Recorder(), history="sparse", tracers=[[1.0], [0.5]],
              tracer_precision="f32x2")
    assert seen == ["setup", "tracers", ("precision", "f32x2")]
    del seen[:]
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Recorder(), history="sparse", tracers=[[1.0], [0.5]])
    assert seen == ["setup", "tracers"]


def test_header_exports_and_binding_agree_on_the_new_entry():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    name = "ludvm_march_set_tracer_precision"
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert name in _ffi.SIGNATURES and name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*ludvm_ctx\s*\*\s*ctx\s*,\s*int\s+precision\s*\)", code)
    assert re.search(r"\bT " + name + r"$", exported, flags=re.M)
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    assert _ffi.TRACER_PRECISIONS == {"f64": 0, "f32x2": 2}
    for code_ in (0, 1, 2, 3):
        assert lib.ludvm_march_set_tracer_precision(None, code_) == _ffi.E_ARG
    # the constants the tests and the binding restate
    kernels = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    assert int(re.search(r"constexpr int kTracerF32PerLane = (\d+);", kernels).group(1)) == _ffi.TRACER_F32X2_PER_LANE
    assert int(re.search(r"constexpr int kHiloTile = (\d+);", kernels).group(1)) == TILE


@pytest.fixture(scope="module")
def march_report():
    """The compiler's report of every kernel of march.hip for gfx950 (no GPU needed), through tools/kernel_resources.py."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources(unit="march.hip")


def test_the_f32x2_tracer_kernel_uses_no_scratch(march_report):
    """march_f32x2_tracer_partial: no scratch, no spills, at least 4 waves per SIMD, the five float planes of one 256-source
    tile in LDS; the figures DESIGN.md section 4.9 quotes are printed (122 VGPRs, 5120 bytes, 4 waves / SIMD)."""
    found = {k: v for k, v in march_report.items() if "march_f32x2_tracer_partial" in k}
    assert len(found) == 1, sorted(march_report)
    (name, r), = found.items()
    print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == 5 * TILE * 4 and int(r["Occupancy [waves/SIMD]"]) >= 4, r


def test_the_float64_tracer_kernels_are_compiled_as_before(march_report):
    """march_tracer_partial and march_tracer_finish beside the new kernel: the registers, LDS and scratch they had before it
    existed (52 VGPRs, 6144 bytes of LDS; 18 VGPRs, no LDS; no scratch)."""
    assert any("march_f32x2_tracer_partial" in k for k in march_report), sorted(march_report)
    before = {"march_tracer_partial": (52, 6144, 0), "march_tracer_finish": (18, 0, 0)}
    for kernel, want in before.items():
        (name, r), = {k: v for k, v in march_report.items() if kernel in k}.items()
        got = (int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"]))
        print(name, "VGPRs, LDS, scratch", got)
        assert got == want, (name, got, want)
