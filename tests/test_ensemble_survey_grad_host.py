"""CPU tier of the wake survey's gradient sums in a sweep (`sweep(cases, survey=..., survey_grad=True)`): the host side over a
test-side engine that answers `ensemble_run_surveyed_graded` with the long-double closed forms over the sources of solo per-step
runs (tests/survey_gradient_common.py's reference_sums) in the device layout (include/ludvm_hip.h,
ludvm_ensemble_run_surveyed_graded), every refusal, the C ABI of the new entry point and the resources of the four
instantiations of the graded kernel as hipcc compiles them for gfx950.  The kernel itself runs in
tests/test_gpu_ensemble_survey_grad.py."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import survey_gradient_common as SG
from conftest import ROOT
from ensemble_survey_grad_common import BIN_GRAD_ATTRS, GRAD_ATTRS, member_window, reference_of
from probes_common import probes32
from survey_bins_common import check_bin_derived
from survey_common import check_derived
from test_ensemble_host import Counting
from test_ensemble_survey_bins_host import BIN_ATTRS, BinnedEnsembleFake, CountingBinned, period_cases
from test_ensemble_survey_host import SurveyedEnsembleFake
from tracers_common import seeds37


class GradedEnsembleFake(BinnedEnsembleFake):
    """BinnedEnsembleFake with `ensemble_run_surveyed_graded`: answers the binned call's tuple (the surveyed call's and None
    without bins) and appends the long-double gradient sums over the sources of its plain solo runs (dense history), [members,
    5, K], and -- with bins -- the same terms added per bin, [members, B, 5, K]."""

    def __init__(self, cases, snapshot_steps, survey, frame, steps, bins, **observers):
        if bins is None:                # (no bins: the surveyed fake's runs alone)
            SurveyedEnsembleFake.__init__(self, cases, snapshot_steps, survey, frame, steps, **observers)
            self.binned_calls, self.binned = 0, []
        else:
            BinnedEnsembleFake.__init__(self, cases, snapshot_steps, survey, frame, steps, bins, **observers)
        self.graded_calls = 0
        self.frame, self.steps = frame, steps

    def ensemble_run_surveyed_graded(self, *packed, bin_of_step=None, nbins=0, **surveyed):
        self.graded_calls += 1
        if nbins:
            out = BinnedEnsembleFake.ensemble_run_surveyed_binned(self, *packed, bin_of_step=bin_of_step, nbins=nbins, **surveyed)
            self.binned_calls -= 1
        else:
            assert bin_of_step is None
            out = SurveyedEnsembleFake.ensemble_run_surveyed(self, *packed, **surveyed) + (None,)
            self.surveyed_calls -= 1
        xz = np.stack([np.asarray(surveyed["survey_x"]), np.asarray(surveyed["survey_z"])])
        K = xz.shape[1]
        gsums = np.zeros([len(self.solos), 5, K])
        bgsums = np.zeros([len(self.solos), nbins, 5, K]) if nbins else None
        off = 0
        for m, solo in enumerate(self.solos):
            W = member_window(surveyed["survey_steps"], solo.nt)
            table = None if not nbins else np.asarray(bin_of_step)[off:off + solo.nt]
            gsums[m], _, b = reference_of(solo, xz, self.frame, W, table, nbins)
            if nbins:
                bgsums[m] = b
            off += solo.nt
        self.gsums, self.bgsums = gsums, bgsums
        return out + (gsums, bgsums)


def _fake(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return GradedEnsembleFake(*a, **k)


@pytest.mark.parametrize("frame,steps", [("lab", None), ("tunnel", (3, 38, 2))])
def test_every_member_gets_the_solo_attributes_from_the_graded_call(frame, steps):
    from ludvm_amd import LUDVM
    pts = probes32()[:, :7]
    cases = period_cases()
    fake = _fake(cases, (2,), pts, frame, steps, None)
    sims = LUDVM.sweep(cases, engine=fake, snapshot_steps=(2,), survey=pts, survey_frame=frame, survey_steps=steps, survey_grad=True)
    assert (fake.graded_calls, fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (1, 0, 0, 0, 0, 0)
    assert fake.bgsums is None and "bin_of_step" not in fake.handed
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert sim.survey_gradient is True and sim.survey_grad_sums.shape == (5, 7) and sim.survey_grad_sums.dtype == np.float64
        assert np.array_equal(sim.survey_grad_sums, fake.gsums[m]) and np.abs(sim.survey_grad_sums[3]).min() > 0.0
        assert np.array_equal(sim.survey_sums, solo.survey_sums) and sim.survey_count == solo.survey_count
        for name in GRAD_ATTRS:
            assert getattr(sim, name).shape[-1] == 7 and np.isfinite(getattr(sim, name)).all(), (m, name)
        for name in BIN_GRAD_ATTRS + BIN_ATTRS:
            assert not hasattr(sim, name), name
        check_derived(sim)
        SG.check_derived(sim)


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_with_survey_phases_the_bins_get_their_gradient_blocks(frame):
    from ludvm_amd import LUDVM
    pts = probes32()[:, :7]
    cases = period_cases()
    fake = _fake(cases, (), pts, frame, (2, 40, 1), 5)
    sims = LUDVM.sweep(cases, engine=fake, survey=pts, survey_frame=frame, survey_steps=(2, 40, 1), survey_phases=5, survey_grad=True)
    assert (fake.graded_calls, fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (1, 0, 0, 0, 0, 0)
    assert fake.handed["nbins"] == 5
    for m, (sim, solo) in enumerate(zip(sims, fake.binned)):
        assert sim.survey_gradient is True and sim.survey_bin_grad_sums.shape == (5, 5, 7)
        assert np.array_equal(sim.survey_grad_sums, fake.gsums[m]) and np.array_equal(sim.survey_bin_grad_sums, fake.bgsums[m])
        for name in BIN_ATTRS:
            assert np.array_equal(getattr(sim, name), getattr(solo, name), equal_nan=True), (m, name)
        for name in GRAD_ATTRS + BIN_GRAD_ATTRS:
            assert hasattr(sim, name), name
        # every sampled step has a bin: the blocks add up to the plain gradient sums
        assert np.abs(sim.survey_bin_grad_sums.sum(axis=0) - sim.survey_grad_sums).max() <= 1e-12 * np.abs(sim.survey_grad_sums).max()
        check_derived(sim)
        check_bin_derived(sim)
        SG.check_derived(sim)
        SG.check_bin_derived(sim)


def test_tables_with_gaps_an_empty_bin_probes_and_particles():
    from ludvm_amd import LUDVM
    pts, rake, seeds = probes32()[:, 8:13], probes32()[:, :4], seeds37()[:, :6]
    cases = period_cases()[:2]
    t0 = np.where(np.arange(41) % 3 == 1, -1, np.where(np.arange(41) % 2 == 0, 0, 2))
    t1 = np.arange(31) % 3
    fake = _fake(cases, (), pts, "tunnel", (2, 35, 1), [t0, t1], probes=rake, probe_frame="tunnel", seeds=seeds)
    sims = LUDVM.sweep(cases, engine=fake, survey=pts, survey_frame="tunnel", survey_steps=(2, 35, 1), survey_phases=[t0, list(t1)],
                       probes=rake, probe_frame="tunnel", particles=seeds, survey_grad=True)
    assert (fake.graded_calls, fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls) == (1, 0, 0, 0, 0, 0)
    assert fake.handed["nbins"] == 3 and np.array_equal(fake.handed["probe_x"], rake[0]) and np.array_equal(fake.handed["seed_x"], seeds[0])
    for m, (sim, plain) in enumerate(zip(sims, fake.solos)):
        assert np.array_equal(sim.probe_u, plain.probe_u) and np.array_equal(sim.tracer_last, plain.tracer_last)
        assert np.array_equal(sim.survey_bin_grad_sums, fake.bgsums[m])
        SG.check_derived(sim)
        SG.check_bin_derived(sim)
    assert sims[0].survey_bin_count[1] == 0 and not sims[0].survey_bin_grad_sums[1].any()
    assert np.isnan(sims[0].survey_bin_mean_omega[1]).all() and np.isnan(sims[0].survey_bin_omega2[1]).all()
    assert np.isfinite(sims[0].survey_coherent_omega2).all() and np.isfinite(sims[0].survey_random_omega2).all()


def test_without_survey_grad_the_calls_are_the_ones_made_before():
    from ludvm_amd import LUDVM
    pts = probes32()[:, :3]
    cases = period_cases()[:2]
    fake = _fake(cases, (), pts, "lab", None, 4)
    counts = lambda: (fake.graded_calls, fake.binned_calls, fake.surveyed_calls, fake.traced_calls, fake.probed_calls, fake.plain_calls)  # noqa: E731
    for kw, expect in ((dict(survey=pts), (0, 0, 1, 0, 0, 0)), (dict(survey=pts, survey_grad=False), (0, 0, 2, 0, 0, 0)),
                       (dict(survey=pts, survey_phases=4), (0, 1, 2, 0, 0, 0)),
                       (dict(survey=pts, survey_phases=4, survey_grad=False), (0, 2, 2, 0, 0, 0)), (dict(), (0, 2, 2, 0, 0, 1)),
                       (dict(survey_grad=False), (0, 2, 2, 0, 0, 2))):
        sims = LUDVM.sweep(cases, engine=fake, **kw)
        assert counts() == expect, kw
        for sim in sims:
            for name in GRAD_ATTRS + BIN_GRAD_ATTRS + ("survey_gradient",):
                assert not hasattr(sim, name), name
    # an engine from before the entry point serves every sweep it served
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        old = BinnedEnsembleFake(cases, (), pts, "lab", None, 4)
    assert not hasattr(old, "ensemble_run_surveyed_graded")
    LUDVM.sweep(cases, engine=old, survey=pts, survey_phases=4)
    LUDVM.sweep(cases, engine=old, survey=pts)
    assert (old.binned_calls, old.surveyed_calls) == (1, 1)
    with pytest.raises(ValueError, match="survey_grad: this engine has no ensemble_run_surveyed_graded"):
        LUDVM.sweep(cases, engine=old, survey=pts, survey_grad=True)
    assert (old.binned_calls, old.surveyed_calls, old.plain_calls) == (1, 1, 0)


class CountingGraded(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
                     "ensemble_run_surveyed_graded"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


OK = np.zeros([2, 3])
S1 = dict(tf=1, dt=5e-2)            # 21 time levels
TINY = dict(tf=0.1, dt=5e-2)


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([S1], dict(survey_grad=True), CountingGraded, "survey_grad needs `survey`"),
    ([S1], dict(survey=OK, survey_grad=1), CountingGraded, "survey_grad=1: survey_grad must be True or False"),
    ([S1], dict(survey=OK, survey_grad=None), CountingGraded, "survey_grad must be True or False"),
    ([S1], dict(survey=OK, survey_grad="yes"), CountingGraded, "survey_grad must be True or False"),
    ([S1], dict(survey=OK, survey_grad="f32x2"), CountingGraded, "(?s)survey_grad='f32x2'.*float64"),
    ([S1], dict(survey_grad="f32x2"), CountingGraded, "(?s)survey_grad='f32x2'.*float64"),
    ([S1, dict(S1, survey_grad=True)], dict(survey=OK), CountingGraded, "member 1: `survey_grad` belongs to the sweep"),
    ([S1, dict(S1, survey_grad=False)], dict(survey=OK, survey_grad=True), CountingGraded, "member 1: `survey_grad` belongs to the sweep"),
    # `survey_gradient` stays a solo keyword, with the messages it had
    ([S1], dict(survey=OK, survey_grad=True, survey_gradient=True), CountingGraded, r"sweep: survey_gradient.*LUDVM\(\.\.\., survey="),
    ([S1, dict(S1, survey_gradient="f32x2")], dict(survey=OK, survey_grad=True), CountingGraded,
     r"sweep: member 1: survey_gradient.*LUDVM\(\.\.\., survey="),
    ([S1], dict(survey=OK, survey_grad=True), CountingBinned, "survey_grad: this engine has no ensemble_run_surveyed_graded"),
    ([S1], dict(survey=OK, survey_phases=4, survey_grad=True), CountingBinned, "survey_grad: this engine has no ensemble_run_surveyed_graded"),
    # 3277 members x 4096 points x 80 bytes = 1.00 GiB and a little (3276: just under)
    ([TINY] * 3277, dict(survey=np.zeros([2, 4096]), survey_grad=True), CountingGraded, "split the case list"),
    # 656 members x (4 bins + 1) x 4096 points x 80 bytes likewise (655: just under)
    ([TINY] * 656, dict(survey=np.zeros([2, 4096]), survey_phases=4, survey_grad=True), CountingGraded, "split the case list"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word) as e:
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []
    if word == "split the case list":
        B = kwargs.get("survey_phases", 0)
        assert str(len(cases) * (B + 1) * 80 * 4096) in str(e.value) and "1.00 GiB" in str(e.value) and "survey_grad" in str(e.value)


def test_the_limit_itself_is_fine_and_one_byte_over_is_not(monkeypatch):
    from ludvm_amd import _ffi, ensemble
    assert _ffi.ENSEMBLE_SURVEY_BYTES == 1 << 30
    # the largest case lists under the cap, without and with four bins
    merged = [dict(t0=0, **TINY)] * 3276
    surveyed = ensemble._check_sweep_survey(np.zeros([2, 4096]), "lab", None, merged)
    assert ensemble._check_sweep_grad(True, surveyed, None, merged) is True
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_grad(True, surveyed, None, merged + merged[:1])
    binned = ensemble._check_sweep_phases(4, surveyed, merged[:655])
    assert ensemble._check_sweep_grad(True, surveyed, binned, merged[:655]) is True
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_grad(True, surveyed, binned, merged[:656])
    assert ensemble._check_sweep_grad(False, surveyed, binned, merged) is False and ensemble._check_sweep_grad(False, None, None, merged) is False
    # exactly the cap, and one byte less room: 7 members x (4 bins + 1) x 4096 points x 80 bytes
    size = 7 * 5 * 80 * 4096
    monkeypatch.setattr(_ffi, "ENSEMBLE_SURVEY_BYTES", size)
    assert ensemble._check_sweep_grad(True, surveyed, binned, merged[:7]) is True
    monkeypatch.setattr(_ffi, "ENSEMBLE_SURVEY_BYTES", size - 1)
    with pytest.raises(ValueError, match=f"{size} bytes"):
        ensemble._check_sweep_grad(True, surveyed, binned, merged[:7])


def test_abi_7_declares_and_exports_the_graded_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    name = "ludvm_ensemble_run_surveyed_graded"
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert decl and name in _ffi.SIGNATURES and hasattr(lib, name) and name in _ffi.ADDED_IN_ABI_7
    # ludvm_ensemble_run_surveyed_binned's arguments, then the four of the gradient sums
    extra = [_ffi._pd, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run_surveyed_binned"] + extra
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    binned = re.search(r"\bint\s+ludvm_ensemble_run_surveyed_binned\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert params[:-4] == [" ".join(p.split()) for p in binned.group(1).split(",")]
    assert params[-4:] == ["double* grad_sums", "size_t grad_doubles", "double* bin_grad_sums", "size_t bin_grad_doubles"]
    assert len(params) == len(_ffi.SIGNATURES[name])
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    ints = (_ffi.c_int, _ffi.c_size_t, _ffi.c_longlong)
    assert getattr(lib, name)(*([None] + [0 if t in ints else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG
    from ludvm_amd import Engine
    assert hasattr(Engine, "ensemble_run_surveyed_graded")


BINNED_TUPLES = {"ILb0ELb0E": (106, 218, 0, 2, 129, 0, 16272), "ILb1ELb0E": (106, 218, 0, 2, 158, 0, 16272),
                 "ILb0ELb1E": (106, 219, 0, 2, 173, 0, 16272), "ILb1ELb1E": (106, 219, 0, 2, 172, 0, 16272)}


def test_the_four_instantiations_of_the_graded_kernel_fit_and_the_binned_ones_are_compiled_as_before():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_graded<PROBES, TRACERS> exists four times; they use no
    scratch, spill no vector register, have no dynamic stack, use no AGPRs, keep two waves per SIMD and no more static LDS than
    the family's 16272 bytes.  (SGPRs, VGPRs, scratch, occupancy, SGPR spill, VGPR spill, LDS) as DESIGN.md section 4.21 records
    them: <false, false> (106, 218, 0, 2, 120, 0, 16272), <true, false> (106, 218, 0, 2, 144, 0, 16272), <false, true> (106, 219,
    0, 2, 163, 0, 16272), <true, true> (106, 219, 0, 2, 182, 0, 16272).  The four ensemble_binned kernels report the tuples
    they reported before there were gradient sums."""
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
    graded = {k: v for k, v in kernels.items() if "ensemble_graded" in k}
    assert len(graded) == 4, sorted(kernels)
    assert not [k for k in graded if "ensemble_binned" in k or "ensemble_surveyed" in k]
    for flags in BINNED_TUPLES:
        found = [v for k, v in graded.items() if "ensemble_graded" + flags in k]
        assert len(found) == 1, (flags, sorted(graded))
        r = found[0]
        print("ensemble_graded" + flags + ":", tup(r))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= 16272, r
    binned = {k: v for k, v in kernels.items() if "ensemble_binned" in k}
    assert len(binned) == 4 and len([k for k in kernels if "ensemble_surveyed" in k]) == 4
    for flags, expect in BINNED_TUPLES.items():
        found = [v for k, v in binned.items() if "ensemble_binned" + flags in k]
        assert len(found) == 1 and tup(found[0]) == expect, (flags, [tup(v) for v in found])
