"""CPU tier: the binned (phase-locked) wake survey, LUDVM(..., survey=..., survey_bins=...) -- the host logic of the class over
the fake engine (per-step path: ludvm_amd/ludvm.py, `_roll_up`): the phase table, the bins against the probes of the same run
and against plain surveys of each bin's steps, passivity, the triple decomposition, checkpoint / resume, the refusals, the C
ABI of the two new entry points and the compiler's report of the binned finisher.  The marched path runs in
tests/test_gpu_survey_bins.py."""
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
from survey_bins_common import check_bin_derived, check_bins_against_probes, integer_phase_rule
from survey_common import check_derived


def test_phase_table():
    """Config 1 to tf = 10: 201 time levels, 200 steps per period (k = 0.2 pi, dt = 0.05).  The table of survey_bins=8 is the
    exact integer rule, 25 steps per bin; with a strided window the unsampled steps read -1 and the counts add up."""
    kw = dict(CONFIG1, tf=10.0)
    pts = probes32()[:, :3]
    sim = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=8)
    assert sim.nt == 201 and sim.survey_nbins == 8 and abs(1.0 / sim.f / sim.dt - 200.0) < 1e-9
    table = sim.survey_bin_of_step
    assert table.dtype == np.int64 and table.shape == (201,) and table[0] == -1
    assert np.array_equal(table[1:], integer_phase_rule(np.arange(1, 201), 200, 8))
    assert np.array_equal(sim.survey_bin_count, np.full(8, 25)) and sim.survey_count == 200
    assert np.array_equal(sim.survey_phase, (np.arange(8) + 0.5) / 8)
    check_derived(sim)
    check_bin_derived(sim)
    win = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=8, survey_steps=(7, 190, 3))
    sampled = np.zeros(201, dtype=bool)
    sampled[7:190:3] = True
    assert (win.survey_bin_of_step[~sampled] == -1).all()
    assert np.array_equal(win.survey_bin_of_step[sampled], integer_phase_rule(np.flatnonzero(sampled), 200, 8))
    assert win.survey_bin_count.sum() == win.survey_count == 61
    assert np.array_equal(win.survey_bin_count, np.bincount(win.survey_bin_of_step[sampled], minlength=8))
    # the formula is the exact rule for the other bin counts too, and follows survey_period / survey_phase0
    for B in (4, 7, 16, 64):
        s = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=B, run=False)
        assert np.array_equal(s.survey_bin_of_step[1:], integer_phase_rule(np.arange(1, 201), 200, B)), B
    s = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=4, survey_period=2.0, survey_phase0=0.5, run=False)
    assert np.array_equal(s.survey_bin_of_step[1:], integer_phase_rule(np.arange(1, 201) - 10, 40, 4))
    assert s._ctor["survey_bins"] == 4 and s._ctor["survey_period"] == 2.0 and s._ctor["survey_phase0"] == 0.5


@pytest.mark.parametrize("steps", [None, (7, 190, 3)])
def test_bins_are_the_reduction_of_the_probe_rows_of_the_same_run(steps):
    pts = probes32()
    extra = {} if steps is None else dict(survey_steps=steps)
    sim = LUDVM(**dict(CONFIG1, tf=10.0), verbose=False, engine=FakeEngine(), survey=pts, probes=pts, survey_frame="tunnel",
                probe_frame="tunnel", survey_bins=8, **extra)
    check_bins_against_probes(sim, f"per-step path, window {steps}")
    check_bin_derived(sim)


def test_a_bin_is_bit_identical_to_the_plain_survey_of_its_steps():
    """Window (5, 50, 1) with the explicit table bin = (i - 5) % 3: bin b's sums are the sums of a plain survey with
    survey_steps = (5 + b, 50, 3), bit for bit, and one bin covering every sampled step is the plain sums."""
    kw = dict(CONFIG1, tf=2.5)
    pts = probes32()
    table = (np.arange(51) - 5) % 3
    binned = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_frame="tunnel", survey_steps=(5, 50, 1), survey_bins=table)
    assert binned.survey_nbins == 3 and binned.survey_phase is None and binned.survey_count == 45
    assert (binned.survey_bin_of_step[:5] == -1).all() and binned.survey_bin_of_step[50] == -1
    for b in range(3):
        plain = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_frame="tunnel", survey_steps=(5 + b, 50, 3))
        assert binned.survey_bin_count[b] == plain.survey_count == 15
        assert np.array_equal(binned.survey_bin_sums[b], plain.survey_sums), b
        assert np.array_equal(binned.survey_bin_mean_u[b], plain.survey_mean_u) and np.array_equal(binned.survey_bin_uw[b], plain.survey_uw)
    one = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_frame="tunnel", survey_steps=(5, 50, 1),
                survey_bins=np.zeros(51, dtype=np.int64))
    assert one.survey_nbins == 1 and one.survey_bin_count[0] == one.survey_count == 45
    assert np.array_equal(one.survey_bin_sums[0], one.survey_sums) and np.array_equal(one.survey_sums, binned.survey_sums)


def _result_arrays(sim):
    out = {k: getattr(sim, k) for k in ("Cl", "Cd", "Cm", "Fn", "Fs", "L", "D", "T", "M", "fourier", "LESP", "LESP_prev", "LEV_shed",
                                        "survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw",
                                        "probe_u", "probe_w", "tracer_last")}
    out["survey_count"] = np.array(sim.survey_count)
    out.update({"circ_" + k: np.asarray(v) for k, v in sim.circulation.items()})
    for key in ("TEV", "LEV", "FREE"):
        P = sim.path[key]
        if isinstance(P, np.ndarray):
            out["path_" + key] = P
        else:
            for s in P.steps():
                out[f"path_{key}_{s}"] = P[s]
    for s in sim.tracer_path.steps():
        out[f"tracer_{s}"] = sim.tracer_path[s]
    return out


@pytest.mark.parametrize("history", ["full", "sparse"])
def test_bins_are_passive_on_the_per_step_path(history):
    """With and without bins, probes and tracers set in both runs: the plain survey sums, the count and every other result
    array are bit-identical."""
    kw = dict(CONFIG1, tf=2.0, history=history, snapshot_steps=[5, 17])
    pts = probes32()
    both = dict(probes=pts[:, :5], tracers=pts[:, 5:9], tracer_release=[1, 3, 7, 100], survey=pts, survey_frame="tunnel",
                survey_steps=(3, 30, 2))
    e0, e1 = FakeEngine(), FakeEngine()
    plain = LUDVM(**kw, verbose=False, engine=e0, **both)
    binned = LUDVM(**kw, verbose=False, engine=e1, survey_bins=5, survey_period=1.0, **both)
    a, b = _result_arrays(plain), _result_arrays(binned)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(e0.wake_read(0, e0.wake_size(), gamma=True), e1.wake_read(0, e1.wake_size(), gamma=True)):
        assert np.array_equal(x, y)
    assert e0.calls == e1.calls                                    # (the bins cost no engine call)
    assert binned.survey_bin_count.sum() == binned.survey_count == 14 and (binned.survey_bin_count > 0).all()
    assert not any(k.startswith("survey_bin") or k in ("survey_nbins", "survey_phase") for k in vars(plain))


def test_coherent_plus_random_is_the_total():
    """coherent + random = the total central moments of the binned samples (inside check_bin_derived, at 1e-12 of max|u|^2) --
    and = survey_uu / ww / uw when every sampled step has a bin; with unbinned samples it is the moments of the binned ones."""
    pts = probes32()
    kw = dict(CONFIG1, tf=10.0)
    sim = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_frame="tunnel", survey_bins=8)
    total, umax2 = check_bin_derived(sim)
    for key in ("uu", "ww", "uw"):
        got = getattr(sim, "survey_coherent_" + key) + getattr(sim, "survey_random_" + key)
        assert np.abs(got - getattr(sim, "survey_" + key)).max() <= 1e-12 * umax2, key
    assert (sim.survey_coherent_uu >= 0.0).all() and sim.survey_coherent_uu.max() > 0.0 and sim.survey_random_uu.max() > 0.0
    table = np.full(201, -1)
    table[40:160] = np.arange(120) % 7
    table[100:110] = -1
    part = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=table, survey_steps=(30, 170, 1))
    assert part.survey_nbins == 7 and part.survey_count == 140 and part.survey_bin_count.sum() == 110
    check_bin_derived(part)
    # an empty bin: nan moments, and it takes no part in the decomposition
    gap = np.where(table == 3, -1, table)
    holed = LUDVM(**kw, verbose=False, engine=FakeEngine(), survey=pts, survey_bins=gap, survey_steps=(30, 170, 1))
    assert holed.survey_nbins == 7 and holed.survey_bin_count[3] == 0
    check_bin_derived(holed)
    assert np.isfinite(holed.survey_coherent_uw).all() and np.isfinite(holed.survey_random_ww).all()


@pytest.mark.parametrize("history,form", [("full", "int"), ("sparse", "table")])
def test_checkpoint_inside_the_window_and_resume(tmp_path, history, form):
    """Window 10 .. 55 every 3, checkpoints after steps 23 and 46 (inside it), resumed from the last: bin sums and counts of the
    uninterrupted run, bit for bit.  A run without bins writes the checkpoint keys it wrote before."""
    kw = dict(CONFIG1, tf=3.0)
    pts = probes32()
    ck, ck0 = str(tmp_path / "ck.npz"), str(tmp_path / "ck0.npz")
    bins = dict(survey_bins=4, survey_period=1.3, survey_phase0=0.2) if form == "int" else dict(survey_bins=np.arange(61) % 5 - 1)
    common = dict(verbose=False, history=history, snapshot_steps=[10, 40], survey=pts, survey_frame="tunnel", survey_steps=(10, 56, 3))
    a = LUDVM(**kw, engine=FakeEngine(), **common, **bins)
    LUDVM(**kw, engine=FakeEngine(), **common, **bins, checkpoint_every=23, checkpoint_path=ck)
    LUDVM(**kw, engine=FakeEngine(), **common, checkpoint_every=23, checkpoint_path=ck0)
    R, R0 = np.load(ck), np.load(ck0)
    B = a.survey_nbins
    assert int(R["next_step"]) == 47 and R["survey_bin_sums"].shape == (B, 5, 32) and R["survey_bin_counts"].shape == (B,)
    assert set(R.files) - set(R0.files) == {"survey_bin_sums", "survey_bin_counts"} and set(R0.files) <= set(R.files)
    import json
    c0, c1 = json.loads(str(R0["ctor"])), json.loads(str(R["ctor"]))
    assert set(c1) - set(c0) == {"survey_bins", "survey_period", "survey_phase0"} and not any("bin" in k for k in c0)
    assert np.array_equal(R["survey_sums"], R0["survey_sums"])
    c = LUDVM.resume(ck, engine=FakeEngine(), verbose=False)
    assert c.survey_nbins == B and np.array_equal(c.survey_bin_of_step, a.survey_bin_of_step)
    assert np.array_equal(c.survey_bin_count, a.survey_bin_count) and np.array_equal(c.survey_bin_sums, a.survey_bin_sums)
    assert np.array_equal(c.survey_sums, a.survey_sums) and c.survey_count == a.survey_count == 16
    assert np.array_equal(c.survey_coherent_uw, a.survey_coherent_uw) and np.array_equal(c.Cl, a.Cl)
    assert 0 < R["survey_bin_counts"].sum() < a.survey_bin_count.sum()          # (the window went on after the checkpoint)


def test_refusals_come_before_any_engine(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the bins were checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    ok = np.zeros([2, 3])
    nt = 401
    good = np.arange(nt) % 4

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            LUDVM(**CONFIG1, verbose=False, **kw)
    # any of the three keywords without a survey
    refused("survey", survey_bins=4)
    refused("survey", survey_period=1.0)
    refused("survey", survey_phase0=0.0)
    refused("survey_bins", survey=ok, survey_period=1.0)                   # (a period without bins)
    # B outside 1 .. 64
    for B in (0, -1, 65, True):
        refused("survey_bins", survey=ok, survey_bins=B)
    refused("survey_bins", survey=ok, survey_bins=np.arange(nt) % 66)
    # bins x points over the cap
    refused("survey_bins", survey=np.zeros([2, 65537]), survey_bins=64)
    refused("survey_bins", survey=np.zeros([2, 1048576]), survey_bins=np.arange(nt) % 5)
    # a table of the wrong length, with non-integers, with values below -1
    for table in (good[:-1], np.append(good, 0), good.astype(float), good.reshape(1, -1), np.where(good == 2, -2, good), 2.5, "abc",
                  [0.5] * nt):
        refused("survey_bins", survey=ok, survey_bins=table)
    # a period that is not finite and positive
    for period in (0.0, -1.0, np.nan, np.inf, "long"):
        refused("survey_period", survey=ok, survey_bins=4, survey_period=period)
    refused("survey_phase0", survey=ok, survey_bins=4, survey_phase0=np.nan)
    # the int form needs a period
    with pytest.raises(ValueError, match="survey_period"):
        LUDVM(**dict(CONFIG1, k=0.0), verbose=False, survey=ok, survey_bins=4)
    # no sampled step has a bin
    refused("no sampled step", survey=ok, survey_bins=np.full(nt, -1))
    only = np.full(nt, -1)
    only[10] = 0
    refused("no sampled step", survey=ok, survey_bins=only, survey_steps=(11, 400, 1))
    refused("no sampled step", survey=ok, survey_bins=only, survey_steps=(9, 400, 2))
    # several GPUs refuse any survey, as before
    refused("distributed", survey=ok, survey_bins=4, distributed=True)
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, survey=ok, survey_bins=4, devices=[0, 1])
    # a sweep: in a member and at sweep level
    short = dict(CONFIG1, tf=1.0)
    for key, value in (("survey_bins", 4), ("survey_period", 1.0), ("survey_phase0", 0.0)):
        with pytest.raises(ValueError, match="solo"):
            LUDVM.sweep([short, dict(short, **{key: value})], survey=ok)
        with pytest.raises(ValueError, match="solo"):
            LUDVM.sweep([short], survey=ok, **{key: value})
    # the limits themselves are fine
    s = LUDVM(**dict(CONFIG1, k=0.0), verbose=False, engine=FakeEngine(), survey=np.zeros([2, 65536]), survey_bins=64, survey_period=4.0,
              run=False)
    assert s.survey_nbins == 64 and s.survey_bin_of_step[0] == -1 and s.survey_bin_of_step.max() == 63
    s = LUDVM(**CONFIG1, verbose=False, engine=FakeEngine(), survey=ok, survey_bins=only, survey_steps=(10, 400, 5), run=False)
    assert s.survey_nbins == 1


def test_an_engine_that_marches_without_the_entry_is_refused():
    class Marcher(FakeEngine):
        def march_run(self, *a, **k):
            raise AssertionError("the march was entered")

        def march_set_survey(self, *a, **k):
            raise AssertionError("the survey was set")
    with pytest.raises(RuntimeError, match="march_set_survey_bins"):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Marcher(), survey=[[1.0], [0.5]], survey_bins=2, survey_period=0.5)
    s = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Marcher(), survey=[[1.0], [0.5]], survey_bins=2, survey_period=0.5, march=False)
    assert s.survey_bin_count.sum() == s.survey_count == 20


def test_header_exports_and_binding_agree_on_the_bin_entry_points():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ("ludvm_march_set_survey_bins", "ludvm_march_read_survey_bins"):
        assert name in _ffi.SIGNATURES and name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M), name
    decl = re.search(r"int\s+ludvm_march_set_survey_bins\s*\(([^)]*)\)", code).group(1)
    assert len(decl.split(",")) == len(_ffi.SIGNATURES["ludvm_march_set_survey_bins"]) == 6
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    assert re.search(r"#define\s+LUDVM_MARCH_MAX_SURVEY_BINS\s+64\b", header) and _ffi.MARCH_MAX_SURVEY_BINS == 64
    assert re.search(r"#define\s+LUDVM_MARCH_MAX_SURVEY_BIN_POINTS\s+4194304\b", header) and _ffi.MARCH_MAX_SURVEY_BIN_POINTS == 4194304
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header)
    assert lib.ludvm_march_set_survey_bins(None, None, 0, 0, None, None) == _ffi.E_ARG
    assert lib.ludvm_march_read_survey_bins(None, None, None) == _ffi.E_ARG


def test_the_binned_finisher_uses_no_scratch_and_no_lds():
    """The compiler's report of march_binned_survey_finish for gfx950 (no GPU needed), through tools/kernel_resources.py: no
    scratch, no spills, no LDS."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    found = {k: v for k, v in mod.resources(unit="march.hip").items() if "march_binned_survey_finish" in k}
    assert len(found) == 1
    for name, r in found.items():
        print(name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) == 0, (name, r)
