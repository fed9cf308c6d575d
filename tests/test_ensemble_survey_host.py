"""CPU tier of the wake survey in a sweep (`sweep(cases, survey=..., survey_frame=..., survey_steps=...)`): the host side over
a test-side engine that answers `ensemble_run_surveyed` with solo per-step runs in the device layout (include/ludvm_hip.h,
ludvm_ensemble_run_surveyed), every refusal, the C ABI of the new entry point and the resources of the four instantiations of
the surveyed kernel as hipcc compiles them for gfx950.  The kernel itself runs in tests/test_gpu_ensemble_survey.py."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from probes_common import probes32
from survey_common import check_derived, window
from test_ensemble_host import Counting, EnsembleFake, SetupRecorder, mixed_cases
from tracers_common import seeds37

SNAPS = (1, 2, 10, 70)
WINDOW = (5, 90, 4)             # (90 lies beyond the last step of the shorter members: clipped for them)


class SurveyedEnsembleFake(EnsembleFake):
    """EnsembleFake whose solo runs carry the sweep's survey (and probes and tracers, when given): `ensemble_run_surveyed`
    checks and answers the packed inputs as `ensemble_run` does and adds the solo runs' raw sums as [members, 5, K]."""

    def __init__(self, cases, snapshot_steps, survey, frame, steps, probes=None, probe_frame="lab", seeds=None):
        FakeEngine.__init__(self)
        from ludvm_amd import LUDVM
        self.snaps = sorted(int(s) for s in snapshot_steps if s >= 1)
        self.solos, self.setups = [], []
        self.ensemble_calls = self.plain_calls = self.probed_calls = self.traced_calls = self.surveyed_calls = 0
        self.handed = None
        extra = {} if probes is None else dict(probes=probes, probe_frame=probe_frame)
        if seeds is not None:
            extra.update(tracers=seeds)
        for kw in cases:
            self.solos.append(LUDVM(**kw, verbose=False, engine=FakeEngine(), precision="f64", history="full", march=False,
                                    survey=survey, survey_frame=frame, survey_steps=steps, **extra))
            rec = SetupRecorder()
            obj = LUDVM(**kw, verbose=False, engine=rec, precision="f64", history="sparse", run=False)
            S = obj._loop_begin()
            obj._free_slot, S.fsl = None, slice(0, S.nf)
            obj._loop_prepare_engine(S)
            self.setups.append(rec.setup)

    def ensemble_run(self, *packed):
        self.plain_calls += 1
        return EnsembleFake.ensemble_run(self, *packed)

    def ensemble_run_probed(self, *packed, **k):
        self.probed_calls += 1
        raise AssertionError("ensemble_run_probed reached")

    def ensemble_run_traced(self, *packed, **k):
        self.traced_calls += 1
        raise AssertionError("ensemble_run_traced reached")

    def ensemble_run_surveyed(self, *packed, survey_x, survey_z, survey_steps, survey_shift_x=None, seed_x=(), seed_z=(), release=(),
                              shift_x=None, record_steps=(), probe_x=None, probe_z=None, probe_shift_x=None):
        self.surveyed_calls += 1
        rows, wakes, wake_n = EnsembleFake.ensemble_run(self, *packed)
        opt = lambda a: None if a is None else np.array(a)
        self.handed = dict(survey_x=np.array(survey_x), survey_z=np.array(survey_z), survey_steps=tuple(survey_steps),
                           survey_shift_x=opt(survey_shift_x), seed_x=np.array(seed_x), seed_z=np.array(seed_z),
                           release=np.array(release), shift_x=opt(shift_x), record_steps=list(record_steps), probe_x=opt(probe_x),
                           probe_z=opt(probe_z), probe_shift_x=opt(probe_shift_x))
        kin_rows = sum(s.nt for s in self.solos)
        assert np.asarray(packed[4]).shape[0] == kin_rows and (survey_shift_x is None or len(survey_shift_x) == kin_rows)
        first, stop, every = survey_steps
        assert first >= 1 and every >= 1
        K, M = len(survey_x), len(seed_x)
        sums = np.zeros([len(self.solos), 5, K])
        rec = list(record_steps)
        trows = np.zeros([len(self.solos), len(rec) + 1, 2, M])
        for m, solo in enumerate(self.solos):
            assert solo.survey_count == len(window(first, stop, every, solo.nt))
            sums[m] = solo.survey_sums.reshape(5, K)
            if M:
                for r, step in enumerate(rec):
                    if step <= solo.nt - 1:
                        trows[m, r] = solo.tracer_path[step]
                trows[m, len(rec)] = solo.tracer_path[solo.nt - 1]
        if probe_x is None:
            return rows, wakes, wake_n, trows, sums
        pu = np.concatenate([s.probe_u for s in self.solos])
        pw = np.concatenate([s.probe_w for s in self.solos])
        return rows, wakes, wake_n, trows, pu, pw, sums


def _fake(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SurveyedEnsembleFake(*a, **k)


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_sweep_hands_the_survey_over_and_stores_every_members_statistics(frame):
    from ludvm_amd import LUDVM
    pts = probes32()[:, :11]
    fake = _fake(mixed_cases(), SNAPS, pts, frame, WINDOW)
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS, survey=pts, survey_frame=frame, survey_steps=WINDOW)
    assert (fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 0, 0, 1)
    h = fake.handed
    assert np.array_equal(h["survey_x"], pts[0]) and np.array_equal(h["survey_z"], pts[1]) and h["survey_steps"] == WINDOW
    assert len(h["seed_x"]) == 0 and len(h["release"]) == 0 and h["record_steps"] == [] and h["shift_x"] is None
    assert h["probe_x"] is None and h["probe_z"] is None and h["probe_shift_x"] is None
    if frame == "lab":
        assert h["survey_shift_x"] is None
    else:
        assert np.array_equal(h["survey_shift_x"], np.concatenate([s.xpiv for s in fake.solos]))
    assert [s.nt - 1 for s in fake.solos] == [60, 40, 100, 100, 80]
    counts = []
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        nt = solo.nt
        assert sim.survey_count == solo.survey_count == len(window(*WINDOW, nt)), m
        assert sim.survey_steps == solo.survey_steps == (5, min(90, nt), 4), m
        assert sim.survey_frame == frame and sim.survey_sums.shape == (5, 11) and sim.survey_sums.dtype == np.float64
        assert np.array_equal(sim.survey_x, pts[0]) and np.array_equal(sim.survey_z, pts[1])
        assert np.array_equal(sim.survey_sums, solo.survey_sums), m
        for name in ("survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw"):
            assert np.array_equal(getattr(sim, name), getattr(solo, name)), (m, name)
        check_derived(sim)
        assert np.abs(sim.survey_mean_u).max() > 0.0 and sim.survey_uu.min() >= -1e-18
        assert np.abs(sim.Cl - solo.Cl).max() <= 1e-13 and np.array_equal(sim.LEV_shed, solo.LEV_shed), m
        assert not hasattr(sim, "probe_u") and not hasattr(sim, "tracer_path")
        counts.append(sim.survey_count)
    assert counts == [14, 9, 22, 22, 19]
    # without a survey: the calls a sweep made before there was one, and no survey attribute
    plain = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS)
    assert (fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 0, 1, 2)
    for sim in plain:
        for name in ("survey_x", "survey_sums", "survey_count", "survey_mean_u", "survey_steps", "survey_frame"):
            assert not hasattr(sim, name), name


def test_the_default_window_is_every_step_of_each_member():
    from ludvm_amd import LUDVM
    pts = probes32()[:, :3]
    cases = mixed_cases()[:2]
    fake = _fake(cases, (), pts, "lab", None)
    sims = LUDVM.sweep(cases, engine=fake, survey=pts)
    assert fake.handed["survey_steps"][0] == 1 and fake.handed["survey_steps"][2] == 1 and fake.handed["survey_steps"][1] >= 61
    for sim, solo in zip(sims, fake.solos):
        assert sim.survey_count == solo.nt - 1 and sim.survey_steps == (1, solo.nt, 1)
        assert np.array_equal(sim.survey_sums, solo.survey_sums)
        check_derived(sim)


def test_the_mesh_dict_and_the_equivalent_array_give_identical_arrays():
    from ludvm_amd import LUDVM
    mesh = dict(xmin=-1.0, xmax=1.1, zmin=0.4, zmax=1.5, dr=0.3)
    x1, z1 = np.arange(-1.0, 1.1, 0.3), np.arange(0.4, 1.5, 0.3)
    X, Z = np.meshgrid(x1, z1, indexing="ij")
    flat = np.stack([X.ravel(), Z.ravel()])
    cases = mixed_cases()[:2]
    fa, fb = _fake(cases, (), mesh, "tunnel", (2, 30, 2)), _fake(cases, (), flat, "tunnel", (2, 30, 2))
    a = LUDVM.sweep(cases, engine=fa, survey=mesh, survey_frame="tunnel", survey_steps=(2, 30, 2))
    b = LUDVM.sweep(cases, engine=fb, survey=flat, survey_frame="tunnel", survey_steps=[2, 30, 2])
    assert np.array_equal(fa.handed["survey_x"], flat[0]) and np.array_equal(fa.handed["survey_z"], flat[1])
    for sa, sb in zip(a, b):
        assert sa.survey_x.shape == (len(x1), len(z1)) == (8, 4) and sb.survey_x.shape == (32,)
        assert np.array_equal(sa.survey_x, X) and np.array_equal(sa.survey_z, Z)
        assert sa.survey_sums.shape == (5, 8, 4) and sa.survey_count == sb.survey_count == 14
        for name in ("survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw"):
            assert np.array_equal(getattr(sa, name).reshape(-1), getattr(sb, name).reshape(-1)), name
        check_derived(sa)
        check_derived(sb)


def test_survey_probes_and_particles_compose_in_one_call():
    from ludvm_amd import LUDVM
    pts, rake, seeds = probes32()[:, 8:15], probes32()[:, :8], seeds37()[:, :9]
    fake = _fake(mixed_cases(), SNAPS, pts, "lab", WINDOW, probes=rake, probe_frame="tunnel", seeds=seeds)
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS, survey=pts, survey_steps=WINDOW, probes=rake,
                       probe_frame="tunnel", particles=seeds)
    assert (fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 0, 0, 1)
    h = fake.handed
    assert h["survey_shift_x"] is None and h["shift_x"] is None
    assert np.array_equal(h["probe_shift_x"], np.concatenate([s.xpiv for s in fake.solos]))
    assert np.array_equal(h["probe_x"], rake[0]) and np.array_equal(h["seed_x"], seeds[0]) and np.array_equal(h["seed_z"], seeds[1])
    assert np.array_equal(h["release"], np.ones(9, dtype=np.int64)) and h["record_steps"] == [1, 2, 10, 70]
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert np.array_equal(sim.survey_sums, solo.survey_sums) and sim.survey_count == solo.survey_count, m
        assert np.array_equal(sim.probe_u, solo.probe_u) and np.array_equal(sim.probe_w, solo.probe_w), m
        for s in sim.tracer_path.steps():
            assert np.array_equal(sim.tracer_path[s], solo.tracer_path[s]), (m, s)
        assert np.array_equal(sim.tracer_last, solo.tracer_last), m
        check_derived(sim)


class CountingSurveyed(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


class CountingTracedOnly(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


OK = np.zeros([2, 3])


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([dict(tf=1)], dict(survey=np.zeros([2, 4097])), CountingSurveyed, "at most 4096"),
    ([dict(tf=1)], dict(survey=dict(xmin=0.0, xmax=65.0, zmin=0.0, zmax=64.0, dr=1.0)), CountingSurveyed, "at most 4096"),
    # 6554 members x 4096 points x 40 bytes = 1.00 GiB and a little
    ([dict(tf=0.1, dt=5e-2)] * 6554, dict(survey=np.zeros([2, 4096])), CountingSurveyed, "split the case list"),
    ([dict(tf=1)], dict(survey=OK, survey_frame="body"), CountingSurveyed, "survey_frame"),
    ([dict(tf=1)], dict(survey_frame="body"), CountingSurveyed, "survey_frame"),
    ([dict(tf=1)], dict(survey=OK, survey_steps=(0, 5, 1)), CountingSurveyed, "first >= 1"),
    ([dict(tf=1)], dict(survey=OK, survey_steps=(1, 5, 0)), CountingSurveyed, "every >= 1"),
    ([dict(tf=1)], dict(survey=OK, survey_steps=(1, 5)), CountingSurveyed, "three integers"),
    ([dict(tf=1)], dict(survey=OK, survey_steps=(1, 5.5, 1)), CountingSurveyed, "three integers"),
    ([dict(tf=1)], dict(survey=OK, survey_steps=(5, 5, 1)), CountingSurveyed, "holds no time step"),
    ([dict(tf=1)], dict(survey=[[0.0, np.nan], [1.0, 2.0]]), CountingSurveyed, "finite"),
    ([dict(tf=1)], dict(survey=np.zeros([3, 4])), CountingSurveyed, "survey"),
    ([dict(tf=1)], dict(survey=np.zeros([2, 0])), CountingSurveyed, "survey"),
    # tf = 1, dt = 5e-2: 20 steps; the window begins at the longer member's step 30
    ([dict(tf=2, dt=5e-2), dict(tf=1, dt=5e-2), dict(tf=2, dt=5e-2)], dict(survey=OK, survey_steps=(30, 40, 1)), CountingSurveyed,
     "member 1: survey_steps"),
    ([dict(tf=1)], dict(survey_steps=(1, 5, 1)), CountingSurveyed, "survey_steps needs `survey`"),
    ([dict(tf=1), dict(tf=1, survey=OK)], {}, CountingSurveyed, "(?s)member 1: survey=.*common to it: sweep\\(cases, survey="),
    ([dict(tf=1), dict(tf=1, survey=OK)], dict(survey=OK), CountingSurveyed, "member 1: survey="),
    ([dict(tf=1, survey_steps=(1, 5, 1))], dict(survey=OK), CountingSurveyed, "(?s)survey_steps=.*common to it"),
    ([dict(tf=1, survey_frame="tunnel")], dict(survey=OK), CountingSurveyed, "(?s)survey_frame=.*common to it"),
    ([dict(tf=1)], dict(survey=OK), CountingTracedOnly, "ensemble_run_surveyed"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word) as e:
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []
    if word == "split the case list":
        assert str(6554 * 40 * 4096) in str(e.value) and "1.00 GiB" in str(e.value)


def test_the_limits_themselves_are_fine():
    """4096 points, a member's last step alone, a lab frame named in a member, and a case list exactly at the byte cap
    (6553 members x 4096 points x 40 bytes < 1 GiB < 6554 members') pass the checks."""
    from ludvm_amd import ensemble, sweep

    class Reached(Exception):
        pass

    class Stop(FakeEngine):
        def ensemble_run(self, *a, **k):
            raise AssertionError("not called")

        def ensemble_run_surveyed(self, *a, survey_x, survey_steps, **k):
            raise Reached(f"{np.asarray(a[4]).shape[0]} rows, {len(survey_x)} points, steps {tuple(survey_steps)}")
    with pytest.raises(Reached, match=r"21 rows, 4096 points, steps \(20, 1000, 7\)"):
        sweep([dict(CONFIG1, tf=1, survey_frame="lab")], engine=Stop(), survey=np.zeros([2, 4096]), survey_steps=(20, 1000, 7))
    merged = [dict(t0=0, tf=0.1, dt=5e-2)] * 6553
    xz, shape, win = ensemble._check_sweep_survey(np.zeros([2, 4096]), "lab", None, merged)
    assert xz.shape == (2, 4096) and shape == (4096,) and win[0] == 1 and win[2] == 1
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_survey(np.zeros([2, 4096]), "lab", None, merged + merged[:1])
    assert ensemble._check_sweep_survey(dict(xmin=0.0, xmax=64.0, zmin=0.0, zmax=64.0, dr=1.0), "tunnel", (2, 3, 1), merged[:2])[1] == (64, 64)


def test_abi_7_declares_and_exports_the_surveyed_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header) and re.search(r"#define\s+LUDVM_ENSEMBLE_DESC\s+6\b", header)
    limit = re.search(r"#define\s+LUDVM_ENSEMBLE_MAX_SURVEY\s+(\d+)", header)
    assert limit and int(limit.group(1)) == _ffi.ENSEMBLE_MAX_SURVEY == 4096 and _ffi.ENSEMBLE_SURVEY_BYTES == 1 << 30
    name = "ludvm_ensemble_run_surveyed"
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert decl and name in _ffi.SIGNATURES and hasattr(lib, name) and name in _ffi.ADDED_IN_ABI_7
    # ludvm_ensemble_run_traced's arguments, then the ten of the survey
    ll = _ffi.c_longlong
    extra = [_ffi._pd, _ffi._pd, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t, ll, ll, ll, _ffi._pd, _ffi.c_size_t]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run_traced"] + extra
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    traced = re.search(r"\bint\s+ludvm_ensemble_run_traced\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert params[:-10] == [" ".join(p.split()) for p in traced.group(1).split(",")]
    assert params[-10:] == ["const double* survey_x", "const double* survey_z", "size_t nsurvey", "const double* sshift_x",
                            "size_t sshift_rows", "long long first", "long long stop", "long long every", "double* survey_sums",
                            "size_t survey_doubles"]
    assert len(params) == len(_ffi.SIGNATURES[name])
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    assert getattr(lib, name)(*([None] + [0 if t in (_ffi.c_int, _ffi.c_size_t, ll) else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG


def test_the_four_instantiations_of_the_surveyed_kernel_fit():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_surveyed<PROBES, TRACERS> exists four times beside the
    two ensemble_march and the two ensemble_traced kernels; they use no scratch, spill no vector register, have no dynamic
    stack, keep at least two waves per SIMD and no more static LDS than ensemble_march's 16272 bytes.  (SGPRs, VGPRs, scratch,
    occupancy, SGPR spill, VGPR spill, LDS) as DESIGN.md section 4.12 records them: <false, false> (106, 218, 0, 2, 106, 0,
    16272), <true, false> (106, 218, 0, 2, 162, 0, 16272), <false, true> (106, 219, 0, 2, 181, 0, 16272), <true, true> (106,
    219, 0, 2, 170, 0, 16272)."""
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

    def tup(r):
        return tuple(int(r[k]) for k in ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
                                         "VGPRs Spill", "LDS Size [bytes/block]"))
    surveyed = {k: v for k, v in kernels.items() if "ensemble_surveyed" in k}
    assert len(surveyed) == 4, sorted(kernels)
    assert all("ensemble_traced" not in k and "ensemble_march" not in k for k in surveyed), sorted(surveyed)
    for flags in ("ILb0ELb0E", "ILb1ELb0E", "ILb0ELb1E", "ILb1ELb1E"):
        found = [v for k, v in surveyed.items() if "ensemble_surveyed" + flags in k]
        assert len(found) == 1, (flags, sorted(surveyed))
        r = found[0]
        print("ensemble_surveyed" + flags + ":", tup(r))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= 16272, r
