"""CPU tier of the phase-locked wake survey in a sweep (`sweep(cases, survey=..., survey_phases=...)`): the host side over a
test-side engine that answers `ensemble_run_surveyed_binned` with solo per-step runs in the device layout (include/ludvm_hip.h,
ludvm_ensemble_run_surveyed_binned), every member's table against the solo run's, every refusal, the C ABI of the new entry
point and the resources of the four instantiations of the binned kernel as hipcc compiles them for gfx950.  The kernel itself
runs in tests/test_gpu_ensemble_survey_bins.py."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from probes_common import probes32
from survey_bins_common import check_bin_derived, integer_phase_rule
from survey_common import check_derived, window
from test_ensemble_host import Counting
from test_ensemble_survey_host import SurveyedEnsembleFake
from tracers_common import seeds37

PI = np.pi
BIN_ATTRS = ("survey_bin_sums", "survey_bin_count", "survey_bin_mean_u", "survey_bin_mean_w", "survey_bin_uu", "survey_bin_ww",
             "survey_bin_uw", "survey_coherent_uu", "survey_coherent_ww", "survey_coherent_uw", "survey_random_uu",
             "survey_random_ww", "survey_random_uw")


def period_cases():
    """Members that differ in k, dt and tf: periods of 20, 40 and 25 steps, 40 / 30 / 40 steps long."""
    return [dict(CONFIG1, tf=2.0, k=2 * PI), dict(CONFIG1, tf=1.5, k=PI, method="Ramesh"), dict(CONFIG1, tf=1.6, dt=4e-2, k=2 * PI)]


PERIOD_STEPS = (20, 40, 25)


class BinnedEnsembleFake(SurveyedEnsembleFake):
    """SurveyedEnsembleFake with `ensemble_run_surveyed_binned`: a second solo per-step run per case carries the survey with
    survey_bins= (the int B, or that member's table); the call checks the table handed over against those runs' and answers
    `ensemble_run_surveyed`'s tuple with their bin sums as [members, B, 5, K]."""

    def __init__(self, cases, snapshot_steps, survey, frame, steps, bins, **observers):
        SurveyedEnsembleFake.__init__(self, cases, snapshot_steps, survey, frame, steps, **observers)
        from ludvm_amd import LUDVM
        self.binned_calls = 0
        self.binned = [LUDVM(**kw, verbose=False, engine=FakeEngine(), precision="f64", history="sparse", march=False, survey=survey,
                             survey_frame=frame, survey_steps=steps, survey_bins=bins if isinstance(bins, int) else bins[m])
                       for m, kw in enumerate(cases)]

    def ensemble_run_surveyed_binned(self, *packed, bin_of_step, nbins, **surveyed):
        self.binned_calls += 1
        out = SurveyedEnsembleFake.ensemble_run_surveyed(self, *packed, **surveyed)
        self.surveyed_calls -= 1
        table = np.asarray(bin_of_step)
        assert table.shape == (sum(s.nt for s in self.binned),) and table.dtype.kind == "i"
        assert np.array_equal(table, np.concatenate([s.survey_bin_of_step for s in self.binned]))
        self.handed.update(bin_of_step=table.copy(), nbins=nbins)
        K = len(surveyed["survey_x"])
        bsums = np.zeros([len(self.binned), nbins, 5, K])
        for m, solo in enumerate(self.binned):
            assert solo.survey_nbins <= nbins
            bsums[m, :solo.survey_nbins] = solo.survey_bin_sums.reshape(solo.survey_nbins, 5, K)
        return out + (bsums,)


def _fake(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return BinnedEnsembleFake(*a, **k)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("frame,steps", [("lab", None), ("tunnel", (3, 38, 2))])
def test_an_int_bins_every_member_by_its_own_motion_and_stores_the_solo_attributes(frame, steps):
    from ludvm_amd import LUDVM
    pts = probes32()[:, :7]
    cases = period_cases()
    fake = _fake(cases, (2,), pts, frame, steps, 5)
    sims = LUDVM.sweep(cases, engine=fake, snapshot_steps=(2,), survey=pts, survey_frame=frame, survey_steps=steps, survey_phases=5)
    assert (fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (1, 0, 0, 0, 0)
    assert fake.handed["nbins"] == 5 and fake.handed["probe_x"] is None and len(fake.handed["seed_x"]) == 0
    assert [s.nt - 1 for s in sims] == [40, 30, 40]
    first, stop, every = steps or (1, 10 ** 9, 1)
    for m, (sim, solo, n) in enumerate(zip(sims, fake.binned, PERIOD_STEPS)):
        W = window(first, stop, every, sim.nt)
        assert sim.survey_nbins == solo.survey_nbins == 5 and sim.survey_count == len(W) == solo.survey_count
        assert sim.survey_bin_of_step.dtype == np.int64 and np.array_equal(sim.survey_bin_of_step, solo.survey_bin_of_step), m
        # a period of n steps: the exact integer rule on the sampled steps, -1 elsewhere (row 0 included)
        expect = np.full(sim.nt, -1)
        expect[W] = integer_phase_rule(W, n, 5)
        assert np.array_equal(sim.survey_bin_of_step, expect), m
        assert np.array_equal(sim.survey_phase, (np.arange(5) + 0.5) / 5) and np.array_equal(sim.survey_phase, solo.survey_phase)
        assert np.array_equal(sim.survey_bin_count, np.bincount(expect[W], minlength=5))
        for name in BIN_ATTRS:
            assert _same(getattr(sim, name), getattr(solo, name)), (m, name)
        for name in ("survey_sums", "survey_mean_u", "survey_uw"):      # (the plain sums: the fake's plain solo runs)
            assert np.array_equal(getattr(sim, name), getattr(fake.solos[m], name)), (m, name)
        assert sim.survey_bin_sums.shape == (5, 5, 7) and sim.survey_bin_count.dtype == np.int64
        check_derived(sim)
        check_bin_derived(sim)
    # members of different k and dt got different tables under the one B
    assert not np.array_equal(sims[0].survey_bin_of_step[:31], sims[1].survey_bin_of_step)
    assert not np.array_equal(sims[0].survey_bin_of_step, sims[2].survey_bin_of_step)


def test_tables_per_member_with_gaps_an_empty_bin_probes_and_particles():
    """One table per member: -1 entries inside the window, bin 1 empty for member 0 (nan, as solo), B = 1 + the largest entry over
    all members.  Probes and particles ride in the same call."""
    from ludvm_amd import LUDVM
    pts, rake, seeds = probes32()[:, 8:13], probes32()[:, :4], seeds37()[:, :6]
    cases = period_cases()[:2]
    t0 = np.where(np.arange(41) % 3 == 1, -1, np.where(np.arange(41) % 2 == 0, 0, 2))
    t1 = np.arange(31) % 3
    fake = _fake(cases, (), pts, "lab", (2, 35, 1), [t0, t1], probes=rake, probe_frame="tunnel", seeds=seeds)
    sims = LUDVM.sweep(cases, engine=fake, survey=pts, survey_steps=(2, 35, 1), survey_phases=[t0, list(t1)], probes=rake,
                       probe_frame="tunnel", particles=seeds)
    assert (fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (1, 0, 0, 0, 0)
    assert fake.handed["nbins"] == 3 and np.array_equal(fake.handed["probe_x"], rake[0]) and np.array_equal(fake.handed["seed_x"], seeds[0])
    for m, (sim, solo, plain) in enumerate(zip(sims, fake.binned, fake.solos)):
        assert sim.survey_nbins == 3 and sim.survey_phase is None and solo.survey_phase is None
        assert np.array_equal(sim.survey_bin_of_step, solo.survey_bin_of_step) and (sim.survey_bin_of_step[:2] == -1).all()
        for name in BIN_ATTRS:
            assert _same(getattr(sim, name), getattr(solo, name)), (m, name)
        assert np.array_equal(sim.probe_u, plain.probe_u) and np.array_equal(sim.tracer_last, plain.tracer_last)
        check_bin_derived(sim)
    assert sims[0].survey_bin_count[1] == 0 and np.isnan(sims[0].survey_bin_mean_u[1]).all() and np.isnan(sims[0].survey_bin_uw[1]).all()
    assert sims[0].survey_bin_count.sum() < sims[0].survey_count          # (the -1 entries are sampled but have no bin)
    assert sims[1].survey_bin_count.sum() == sims[1].survey_count == 29


def test_without_survey_phases_the_calls_are_the_ones_made_before():
    from ludvm_amd import LUDVM
    pts = probes32()[:, :3]
    cases = period_cases()[:2]
    fake = _fake(cases, (), pts, "lab", None, 4)
    sims = LUDVM.sweep(cases, engine=fake, survey=pts)
    assert (fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (0, 1, 0, 0, 0)
    assert "bin_of_step" not in fake.handed
    for sim in sims:
        for name in BIN_ATTRS + ("survey_nbins", "survey_bin_of_step", "survey_phase"):
            assert not hasattr(sim, name), name
    LUDVM.sweep(cases, engine=fake)
    assert (fake.binned_calls, fake.surveyed_calls, fake.plain_calls) == (0, 1, 1)


class CountingBinned(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


class CountingSurveyedOnly(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


OK = np.zeros([2, 3])
S1 = dict(tf=1, dt=5e-2)            # 21 time levels
T21 = np.arange(21) % 4


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([S1], dict(survey_phases=4), CountingBinned, "survey_phases needs `survey`"),
    ([S1], dict(survey=OK, survey_phases=True), CountingBinned, "survey_phases must be an int B or a sequence"),
    ([S1], dict(survey=OK, survey_phases=2.5), CountingBinned, "survey_phases must be an int B or a sequence"),
    ([S1], dict(survey=OK, survey_phases=0), CountingBinned, r"1 <= B <= 64 \(got 0\)"),
    ([S1], dict(survey=OK, survey_phases=65), CountingBinned, r"1 <= B <= 64 \(got 65\)"),
    ([S1], dict(survey=OK, survey_phases=-3), CountingBinned, "1 <= B <= 64"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21]), CountingBinned, r"one table per member \(1 tables for 2 members\)"),
    ([S1], dict(survey=OK, survey_phases=[T21, T21]), CountingBinned, "one table per member"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21, T21[:-1]]), CountingBinned, r"member 1: survey_phases: a table holds one integer per time step, \[nt\] with nt = 21"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21, T21.reshape(1, -1)]), CountingBinned, "member 1: survey_phases: a table holds"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21.astype(float), T21]), CountingBinned, "member 0: survey_phases: a table holds"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21, np.where(T21 == 2, -2, T21)]), CountingBinned, "member 1: survey_phases: a table's entries are -1"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21, np.arange(21) + 44]), CountingBinned, r"member 1: survey_phases: at most 64 bins \(the table's largest entry is 64\)"),
    ([S1, S1], dict(survey=OK, survey_phases=[T21, np.full(21, -1)]), CountingBinned, "member 1: survey_phases: no sampled step"),
    # member 1's only binned step lies outside the window
    ([S1, S1], dict(survey=OK, survey_steps=(5, 21, 1), survey_phases=[T21, np.where(np.arange(21) == 3, 0, -1)]), CountingBinned,
     "member 1: survey_phases: no sampled step"),
    ([S1, dict(S1, k=0.0)], dict(survey=OK, survey_phases=4), CountingBinned, r"member 1: survey_phases=4: the motion has no period \(k = 0\)"),
    ([S1, dict(S1, survey_phases=4)], dict(survey=OK), CountingBinned, "member 1: `survey_phases` belongs to the sweep"),
    ([S1, dict(S1, survey_bins=4)], dict(survey=OK), CountingBinned, "(?s)member 1: survey_bins=4.*survey_phases.*solo"),
    ([S1], dict(survey=OK, survey_bins=4), CountingBinned, "(?s)survey_bins=4.*survey_phases.*solo"),
    ([S1], dict(survey=OK, survey_period=1.0), CountingBinned, "(?s)survey_period=1.0.*survey_phases.*solo"),
    ([S1], dict(survey=OK, survey_phase0=0.5), CountingBinned, "(?s)survey_phase0=0.5.*survey_phases.*solo"),
    ([S1], dict(survey=OK, survey_phases=4), CountingSurveyedOnly, "survey_phases: this engine has no ensemble_run_surveyed_binned"),
    # 1311 members x (4 bins + 1) x 4096 points x 40 bytes = 1.00 GiB and a little (1310: just under)
    ([dict(tf=0.1, dt=5e-2)] * 1311, dict(survey=np.zeros([2, 4096]), survey_phases=4), CountingBinned, "split the case list"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word) as e:
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []
    if word == "split the case list":
        assert str(1311 * 5 * 40 * 4096) in str(e.value) and "1.00 GiB" in str(e.value) and "survey_phases" in str(e.value)


def test_the_limits_themselves_are_fine():
    """64 bins, a table whose largest entry is 63, a case list exactly at the byte cap (1310 members x 5 x 4096 points x 40
    bytes < 1 GiB < 1311 members'), and a k = 0 member under explicit tables pass the checks."""
    from ludvm_amd import _ffi, ensemble
    merged = [dict(t0=0, tf=0.1, dt=5e-2)] * 1310
    surveyed = ensemble._check_sweep_survey(np.zeros([2, 4096]), "lab", None, merged)
    tables, B, phase = ensemble._check_sweep_phases(4, surveyed, merged)
    assert B == 4 and len(tables) == 1310 and tables[0].shape == (4,) and tables[0][0] == -1 and len(phase) == 4
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_phases(4, surveyed, merged + merged[:1])
    two = [dict(S1), dict(S1, k=0.0)]
    surveyed = ensemble._check_sweep_survey(OK, "lab", None, two)
    assert ensemble._check_sweep_phases(64, surveyed, two[:1])[1] == 64
    tables, B, phase = ensemble._check_sweep_phases([np.arange(21) % 2, np.arange(21) + 43], surveyed, two)
    assert B == 64 == _ffi.ENSEMBLE_MAX_SURVEY_BINS and phase is None and tables[1][0] == -1 and tables[1][20] == 63
    assert ensemble._check_sweep_phases(None, surveyed, two) is None and ensemble._check_sweep_phases(None, None, two) is None


def test_abi_7_declares_and_exports_the_binned_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header) and re.search(r"#define\s+LUDVM_ENSEMBLE_DESC\s+6\b", header)
    limit = re.search(r"#define\s+LUDVM_ENSEMBLE_MAX_SURVEY_BINS\s+(\d+)", header)
    assert limit and int(limit.group(1)) == _ffi.ENSEMBLE_MAX_SURVEY_BINS == 64
    name = "ludvm_ensemble_run_surveyed_binned"
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert decl and name in _ffi.SIGNATURES and hasattr(lib, name) and name in _ffi.ADDED_IN_ABI_7
    # ludvm_ensemble_run_surveyed's arguments, then the five of the bins
    extra = [_ffi.POINTER(_ffi.c_int), _ffi.c_size_t, _ffi.c_int, _ffi._pd, _ffi.c_size_t]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run_surveyed"] + extra
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    surveyed = re.search(r"\bint\s+ludvm_ensemble_run_surveyed\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert params[:-5] == [" ".join(p.split()) for p in surveyed.group(1).split(",")]
    assert params[-5:] == ["const int* bin_of_step", "size_t bin_rows", "int nbins", "double* bin_sums", "size_t bin_doubles"]
    assert len(params) == len(_ffi.SIGNATURES[name])
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    ints = (_ffi.c_int, _ffi.c_size_t, _ffi.c_longlong)
    assert getattr(lib, name)(*([None] + [0 if t in ints else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG
    from ludvm_amd import Engine
    assert hasattr(Engine, "ensemble_run_surveyed_binned")


def test_the_four_instantiations_of_the_binned_kernel_fit():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_binned<PROBES, TRACERS> exists four times beside the four
    ensemble_surveyed kernels; they use no scratch, spill no vector register, have no dynamic stack, keep two waves per SIMD and
    no more static LDS than ensemble_march's 16272 bytes.  (SGPRs, VGPRs, scratch, occupancy, SGPR spill, VGPR spill, LDS) as
    DESIGN.md section 4.19 records them: <false, false> (106, 218, 0, 2, 129, 0, 16272), <true, false> (106, 218, 0, 2, 158, 0,
    16272), <false, true> (106, 219, 0, 2, 173, 0, 16272), <true, true> (106, 219, 0, 2, 172, 0, 16272); the spilled SGPRs live
    in lanes of vector registers, not in scratch memory."""
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
    binned = {k: v for k, v in kernels.items() if "ensemble_binned" in k}
    assert len(binned) == 4, sorted(kernels)
    assert len([k for k in kernels if "ensemble_surveyed" in k]) == 4
    for flags in ("ILb0ELb0E", "ILb1ELb0E", "ILb0ELb1E", "ILb1ELb1E"):
        found = [v for k, v in binned.items() if "ensemble_binned" + flags in k]
        assert len(found) == 1, (flags, sorted(binned))
        r = found[0]
        print("ensemble_binned" + flags + ":", tup(r))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= 16272, r
