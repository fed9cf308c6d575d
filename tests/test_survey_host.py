"""CPU tier: wake-survey statistics (LUDVM(..., survey=...)) -- the host logic of the drop-in class over the fake engine
(per-step path: ludvm_amd/ludvm.py, `_roll_up`) against the oracle's series and against the probes of the same run, the
window arithmetic, the refusals, checkpoint / resume, the C ABI of the two new entry points and the compiler's report of the
two survey kernels.  The marched path runs in tests/test_gpu_survey.py."""
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
from survey_common import (CASE_IDS, MEAN_VS_ORACLE, MOMENT_VS_ORACLE, ORACLE_CASES, case_keywords, check_derived, oracle_series,
                           series_sums, series_umax, sums_errors, window)


@pytest.mark.parametrize("method,frame,cloud", ORACLE_CASES, ids=CASE_IDS)
def test_survey_sums_match_the_oracle(method, frame, cloud):
    """The five sums over steps 1-50 at probes32()'s points against the same statistics of ProbedOracle's series: means at 1e-9
    of max|u|, raw second moments at 3e-9 of max|u|^2."""
    pts = probes32()
    ou, ow = oracle_series(pts, method, frame, cloud)
    steps = window(1, 51, 1, 51)
    ref, umax = series_sums(ou, ow, steps), series_umax(ou, ow, steps)
    sim = LUDVM(**case_keywords(method, cloud), verbose=False, engine=FakeEngine(), survey=pts, survey_frame=frame,
                survey_steps=(1, 51, 1))
    assert sim.nt == 51 and sim.survey_count == 50 and sim.survey_steps == (1, 51, 1) and sim.survey_frame == frame
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, 50, umax)
    print(f"{method} {frame} cloud={cloud}: survey vs oracle, steps 1-50: means {e_mean:.2e} of max|u|, raw second moments "
          f"{e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE, e_mean
    assert e_mom <= MOMENT_VS_ORACLE, e_mom
    assert np.array_equal(sim.survey_x, pts[0]) and np.array_equal(sim.survey_z, pts[1])
    check_derived(sim)
    assert (sim.survey_uu >= -1e-12 * umax ** 2).all() and sim.survey_uu.max() > 0.0      # a variance; the wake does fluctuate


@pytest.mark.parametrize("steps", [None, (1, 51, 1), (7, 40, 3), (5, 10 ** 6, 2), (20, 51, 100), (50, 51, 1)])
def test_window_arithmetic(steps):
    """survey_count and the sums against the matching reduction of probe_u / probe_w of the same run at the same points, at
    1e-12 of max|u| (of max|u|^2 for the second moments): every step, a strided window, stop past the end, `every` larger
    than the window (one sample), the last step alone."""
    pts = probes32()
    kw = dict(CONFIG1, tf=2.5)
    extra = {} if steps is None else dict(survey_steps=steps)
    sim = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, probes=pts, survey_frame="tunnel", probe_frame="tunnel", **extra)
    first, stop, every = steps or (1, 51, 1)
    W = window(first, stop, every, sim.nt)
    assert W and sim.survey_count == len(W) and sim.survey_steps == (first, min(stop, 51), every)
    assert len(W) == {None: 50, (1, 51, 1): 50, (7, 40, 3): 11, (5, 10 ** 6, 2): 23, (20, 51, 100): 1, (50, 51, 1): 1}[steps]
    ref, umax = series_sums(sim.probe_u, sim.probe_w, W), series_umax(sim.probe_u, sim.probe_w, W)
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, len(W), umax)
    print(f"window {steps}: {len(W)} samples; vs the run's probe rows: means {e_mean:.2e}, second moments {e_mom:.2e}")
    assert e_mean <= 1e-12 and e_mom <= 1e-12, (e_mean, e_mom)
    check_derived(sim)


def test_dict_and_array_forms_of_a_mesh_give_identical_bits():
    mesh = dict(xmin=-1.0, xmax=1.1, zmin=0.4, zmax=1.5, dr=0.3)
    x1, z1 = np.arange(-1.0, 1.1, 0.3), np.arange(0.4, 1.5, 0.3)
    X, Z = np.meshgrid(x1, z1, indexing="ij")
    kw = dict(CONFIG1, tf=1.0)
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=mesh, survey_steps=(2, 18, 2))
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=np.stack([X.ravel(), Z.ravel()]), survey_steps=(2, 18, 2))
    assert a.survey_x.shape == (len(x1), len(z1)) == (8, 4) and b.survey_x.shape == (32,)
    assert np.array_equal(a.survey_x, X) and np.array_equal(a.survey_z, Z)
    assert a.survey_count == b.survey_count == 8
    for name in ("survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw"):
        va, vb = getattr(a, name), getattr(b, name)
        assert va.shape[-2:] == (8, 4) and np.array_equal(va.reshape(vb.shape), vb), name
    check_derived(a)
    assert a._ctor["survey"] == mesh and a._ctor["survey_steps"] == [2, 18, 2]


def _result_arrays(sim):
    out = {k: getattr(sim, k) for k in ("Cl", "Cd", "Cm", "Fn", "Fs", "L", "D", "T", "M", "fourier", "LESP", "LESP_prev", "LEV_shed")}
    out.update({"circ_" + k: np.asarray(v) for k, v in sim.circulation.items()})
    for key in ("TEV", "LEV", "FREE"):
        P = sim.path[key]
        if isinstance(P, np.ndarray):
            out["path_" + key] = P
        else:
            for s in P.steps():
                out[f"path_{key}_{s}"] = P[s]
    return out


@pytest.mark.parametrize("history", ["full", "sparse"])
def test_a_survey_is_passive_on_the_per_step_path(history):
    """Every other result array with and without a survey, with probes and tracers set in both runs: bit-identical."""
    kw = dict(CONFIG1, tf=2.0, history=history, snapshot_steps=[5, 17])
    pts = probes32()
    both = dict(probes=pts[:, :5], tracers=pts[:, 5:9], tracer_release=[1, 3, 7, 100])
    e0, e1 = FakeEngine(), FakeEngine()
    plain = LUDVM(**kw, verbose=False, engine=e0, **both)
    surveyed = LUDVM(**kw, verbose=False, engine=e1, survey=pts, survey_frame="tunnel", survey_steps=(3, 30, 2), **both)
    a, b = _result_arrays(plain), _result_arrays(surveyed)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(e0.wake_read(0, e0.wake_size(), gamma=True), e1.wake_read(0, e1.wake_size(), gamma=True)):
        assert np.array_equal(x, y)
    assert np.array_equal(plain.probe_u, surveyed.probe_u) and np.array_equal(plain.probe_w, surveyed.probe_w)
    assert plain.tracer_path.steps() == surveyed.tracer_path.steps()
    for s in plain.tracer_path.steps():
        assert np.array_equal(plain.tracer_path[s], surveyed.tracer_path[s]), s
    assert surveyed.survey_count == 14


def test_without_a_survey_nothing_changes():
    eng = FakeEngine()
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng)
    assert not any(k.startswith("survey") for k in vars(sim)) and not any(k.startswith("survey") for k in sim._ctor)
    assert eng.calls["induce"] == 0 and eng.calls["points"] == 0
    # steps outside the window make no engine call
    eng2 = FakeEngine()
    s = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng2, survey=[[1.0], [0.5]], survey_steps=(4, 13, 4))
    assert s.survey_count == 3 and eng2.calls["induce"] == 3 and eng2.calls["points"] == 3
    assert np.array_equal(s.Cl, sim.Cl)


@pytest.mark.parametrize("history,frame", [("full", "lab"), ("sparse", "tunnel")])
def test_checkpoint_inside_the_window_and_resume(tmp_path, history, frame):
    """Window 10 .. 55 every 3; checkpoints after steps 23 and 46 (both inside it); resumed from the last: the sums and the
    count are those of the uninterrupted run, bit for bit."""
    kw = dict(CONFIG1, tf=3.0)
    pts = probes32()
    ck = str(tmp_path / "ck.npz")
    common = dict(verbose=False, history=history, snapshot_steps=[10, 40], survey=pts, survey_frame=frame, survey_steps=(10, 56, 3))
    a = LUDVM(**kw, engine=FakeEngine(), **common)
    LUDVM(**kw, engine=FakeEngine(), **common, checkpoint_every=23, checkpoint_path=ck)
    R = np.load(ck)
    assert int(R["next_step"]) == 47 and R["survey_sums"].shape == (5, 32) and int(R["survey_samples"]) == len(window(10, 47, 3, 61)) == 13
    c = LUDVM.resume(ck, engine=FakeEngine(), verbose=False)
    assert c.survey_frame == frame and c.survey_steps == (10, 56, 3) and np.array_equal(c.survey_x, pts[0])
    assert c.survey_count == a.survey_count == 16
    assert np.array_equal(c.survey_sums, a.survey_sums) and np.array_equal(c.survey_uw, a.survey_uw) and np.array_equal(c.Cl, a.Cl)
    assert not np.array_equal(R["survey_sums"], a.survey_sums)          # (the window went on after the checkpoint)
    with pytest.raises(ValueError, match="one GPU"):
        LUDVM.resume(ck, devices=[0, 1], verbose=False)


def test_refusals_come_before_any_engine(monkeypatch):
    import ludvm_amd.ludvm as M
    import ludvm_amd.multi as MM

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the survey was checked")

    def no_front(*a, **k):
        raise AssertionError("replica threads were created before the survey was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    monkeypatch.setattr(MM, "MultiDeviceLUDVM", no_front)
    ok = np.zeros([2, 3])
    mesh = dict(xmin=0.0, xmax=1.0, zmin=0.0, zmax=1.0, dr=0.25)
    # the window: empty, first < 1, every < 1 (config 1: nt = 401)
    for steps in ((5, 5, 1), (9, 4, 1), (401, 500, 1), (0, 10, 1), (-3, 10, 1), (1, 10, 0), (1, 10, -2), (1, 10), (1.5, 10, 1), 7, "abc"):
        with pytest.raises(ValueError, match="survey_steps"):
            LUDVM(**CONFIG1, verbose=False, survey=ok, survey_steps=steps)
    with pytest.raises(ValueError, match="survey_steps"):
        LUDVM(**CONFIG1, verbose=False, survey_steps=(1, 10, 1))            # (without a survey)
    # the points: not finite, K = 0, one too many, malformed
    bad = [[[0.0, np.nan], [1.0, 2.0]], [[0.0, np.inf], [1.0, 2.0]], np.zeros([2, 0]), np.zeros([2, 1048577]), np.zeros(3),
           np.zeros([3, 4]), np.zeros([2, 2, 2]), [[0.0, "a"], [1.0, 2.0]]]
    for pts in bad:
        with pytest.raises(ValueError, match="survey"):
            LUDVM(**CONFIG1, verbose=False, survey=pts)
        with pytest.raises(ValueError, match="survey"):
            LUDVM(**CONFIG1, verbose=False, survey=pts, devices=[0, 1])
    for d in (dict(mesh, dr=0.0), dict(mesh, dr=-0.1), dict(mesh, dr=np.nan), dict(mesh, xmax=np.inf), dict(mesh, xmax=-1.0),
              dict(mesh, dr=1e-4), {k: v for k, v in mesh.items() if k != "dr"}, dict(mesh, extra=1.0), dict(mesh, zmin="low")):
        with pytest.raises(ValueError, match="survey"):
            LUDVM(**CONFIG1, verbose=False, survey=d)
    for frame in ("body", None):
        with pytest.raises(ValueError, match="survey_frame"):
            LUDVM(**CONFIG1, verbose=False, survey=ok, survey_frame=frame)
    with pytest.raises(ValueError, match="survey_frame"):
        LUDVM(**CONFIG1, verbose=False, survey_frame="body")
    for dist in (True, "rccl", object()):
        with pytest.raises(ValueError, match="distributed"):
            LUDVM(**CONFIG1, verbose=False, survey=ok, distributed=dist)
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, survey=ok, devices=[0, 1])
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, survey=mesh, devices=2)
    with pytest.raises(ValueError, match="survey"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0), dict(CONFIG1, tf=1.0, survey=ok)])
    with pytest.raises(ValueError, match="survey"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0, survey_steps=(1, 5, 1))])
    with pytest.raises(ValueError, match="survey"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0, survey_frame="tunnel")])
    # the limit itself is fine
    s = LUDVM(**CONFIG1, verbose=False, engine=FakeEngine(), survey=np.zeros([2, 1048576]), survey_steps=(400, 10 ** 9, 5), run=False)
    assert s.survey_x.shape == (1048576,) and s.survey_steps == (400, 401, 5)


def test_an_engine_that_marches_without_the_entry_is_refused():
    class Marcher(FakeEngine):
        def march_run(self, *a, **k):
            raise AssertionError("the march was entered")
    with pytest.raises(RuntimeError, match="march_set_survey"):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Marcher(), survey=[[1.0], [0.5]])
    s = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Marcher(), survey=[[1.0], [0.5]], march=False)
    assert s.survey_count == 20


def test_header_exports_and_binding_agree_on_the_survey_entry_points():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ("ludvm_march_set_survey", "ludvm_march_read_survey"):
        assert name in _ffi.SIGNATURES and name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M), name
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    assert re.search(r"#define\s+LUDVM_MARCH_MAX_SURVEY\s+1048576", header) and _ffi.MARCH_MAX_SURVEY == 1048576
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header)
    comment = re.search(r"/\*(?:(?!\*/).)*?wake survey.*?\*/\s*#define\s+LUDVM_MARCH_MAX_SURVEY", header, flags=re.S)
    assert comment and "LUDVM.py:1095-1106" in comment.group(0)
    assert lib.ludvm_march_set_survey(None, None, None, 0, None, 0, 1, 2, 1, None, 0) == _ffi.E_ARG
    assert lib.ludvm_march_read_survey(None, None, None) == _ffi.E_ARG


def test_survey_kernels_use_no_scratch_and_six_kib_of_lds():
    """The compiler's report of the two survey kernels for gfx950 (no GPU needed), through tools/kernel_resources.py: no
    scratch, no spills, LDS <= 6 KiB."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    survey = {k: v for k, v in mod.resources(unit="march.hip").items() if "march_survey_" in k}
    assert len(survey) == 2 and any("march_survey_partial" in k for k in survey) and any("march_survey_finish" in k for k in survey)
    for name, r in survey.items():
        print(name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 6144, (name, r)
