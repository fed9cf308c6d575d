"""GPU tier: the binned (phase-locked) wake survey inside the device-resident march (march_binned_survey_finish,
ludvm_march_set_survey_bins / ludvm_march_read_survey_bins) -- against the probes of the same run, bit for bit against plain
surveys of each bin's steps on both sides of the finisher's block, passive on every other result, independent of how a run is
cut into calls, against the per-step path, and the codes of the two entry points."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from probes_common import probes32
from survey_bins_common import check_bin_derived, check_bins_against_probes
from survey_common import series_umax, sums_errors, window
from tracers_common import seeds37, seeds_random

pytestmark = pytest.mark.gpu

MAX_BINS = 64            # LUDVM_MARCH_MAX_SURVEY_BINS
MAX_BIN_POINTS = 4194304  # LUDVM_MARCH_MAX_SURVEY_BIN_POINTS


@pytest.fixture(autouse=True)
def _time_limit():
    """A limit on every test's host-side time.  (The handler runs between Python instructions: a test stuck INSIDE a HIP call
    is ended by the time limit that wraps the pytest command, not by this.)"""
    def expired(signum, frame):
        raise TimeoutError("GPU test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(240)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _ludvm():
    from ludvm_amd import LUDVM
    return LUDVM


def _chunked(chunk, **attrs):
    return type("Chunked", (_ludvm(),), dict(_march_chunk=chunk, **attrs))


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


@pytest.mark.parametrize("case", ["f64_serial", "f32_overlapped"])
def test_bins_are_the_reduction_of_the_probe_rows_of_the_same_run(eng, case):
    """Eight phase bins at the probes' own points against the reduction of probe_u / probe_w over each bin's steps: means at
    1e-12 of max|u|, raw second moments at 3e-12 of max|u|^2.  Serial 'f64' steps (window 7 .. 190 every 3) and overlapped
    fp32 steps 70-200 (symmetric threshold lowered to 64)."""
    pts = probes32()
    kw = dict(CONFIG1, tf=10.0)
    prec, steps, sym = ("f64", (7, 190, 3), 1) if case == "f64_serial" else ("f32", (70, 201, 1), 64)
    eng.set_symmetric(sym)
    try:
        sim = _ludvm()(**kw, verbose=False, engine=eng, precision=prec, history="sparse", probes=pts, probe_frame="tunnel", survey=pts,
                       survey_frame="tunnel", survey_steps=steps, survey_bins=8)
    finally:
        eng.set_symmetric(1)
    W = window(*steps, sim.nt)
    assert sim.nt == 201 and sim.survey_count == len(W) == sim.survey_bin_count.sum()
    check_bins_against_probes(sim, case)
    check_bin_derived(sim)


@pytest.mark.parametrize("K", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("sym", [1, 64], ids=["serial", "overlapped"])
@pytest.mark.parametrize("survey_precision", ["f64", "f32"])
def test_a_bin_is_bit_identical_to_the_plain_survey_of_its_steps(eng, survey_precision, sym, K):
    """Config 1 (401 steps) in fp32, window (20, 390, 1), table (i - 20) % 3: bin b's block is array_equal to the sums of a
    plain survey with survey_steps = (20 + b, 390, 3) and the counts match; the plain sums of the binned run are those of the
    run without bins.  Both survey precisions, serial and overlapped steps, K on both sides of the finisher's block of 256
    lanes and two tiles of the partial kernel."""
    pts = seeds_random(K)
    table = (np.arange(401) - 20) % 3
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=pts, survey_frame="tunnel",
                  survey_precision=survey_precision)
    eng.set_symmetric(sym)
    try:
        binned = _ludvm()(**CONFIG1, **common, survey_steps=(20, 390, 1), survey_bins=table)
        whole = _ludvm()(**CONFIG1, **common, survey_steps=(20, 390, 1))
        plain = [_ludvm()(**CONFIG1, **common, survey_steps=(20 + b, 390, 3)) for b in range(3)]
    finally:
        eng.set_symmetric(1)
    assert binned.nt == 401 and binned.survey_nbins == 3 and binned.survey_bin_sums.shape == (3, 5, K)
    assert binned.survey_count == whole.survey_count == 370 and np.array_equal(binned.survey_sums, whole.survey_sums)
    for b in range(3):
        assert binned.survey_bin_count[b] == plain[b].survey_count and plain[b].survey_count in (123, 124)
        assert np.array_equal(binned.survey_bin_sums[b], plain[b].survey_sums), b
    assert np.isfinite(binned.survey_bin_sums).all() and np.abs(binned.survey_bin_sums[:, 2]).min() > 0.0      # every point was written
    one = _ludvm()(**dict(CONFIG1, tf=2.5), **common, survey_steps=(5, 50, 1), survey_bins=np.zeros(51, dtype=np.int64))
    assert one.survey_bin_count[0] == one.survey_count == 45 and np.array_equal(one.survey_bin_sums[0], one.survey_sums)


def _same_run(a, b):
    assert np.array_equal(a.Cl, b.Cl) and np.array_equal(a.Cd, b.Cd) and np.array_equal(a.Cm, b.Cm)
    assert np.array_equal(a.LEV_shed, b.LEV_shed) and np.array_equal(a.fourier, b.fourier)
    assert set(a.circulation) == set(b.circulation)
    for key in a.circulation:
        assert np.array_equal(a.circulation[key], b.circulation[key]), key
    for key in ("TEV", "LEV", "FREE"):
        if a.history == "full":
            assert np.array_equal(a.path[key], b.path[key]), key
        else:
            assert a.path[key].steps() == b.path[key].steps()
            for s in a.path[key].steps():
                assert np.array_equal(a.path[key][s], b.path[key][s]), (key, s)


@pytest.mark.parametrize("case", ["f64_dense", "f32_dense_overlapped", "f32_sparse_overlapped", "f32_sparse_serial"])
def test_bins_are_passive(eng, case):
    """With and without bins on a survey of 600 points, probes and tracers set in both runs: the plain survey sums and count,
    Cl / Cd / Cm, every circulation[...], LEV_shed, the history rows, the final resident wake, probe_u / probe_w and the tracer
    paths are the same arrays, bit for bit -- serial and overlapped steps, dense and sparse history."""
    LUDVM = _ludvm()
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_dense_overlapped": dict(precision="f32", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101]),
             "f32_sparse_serial": dict(precision="f32", history="sparse", snapshot_steps=[64])}[case]
    pts = seeds_random(600)
    others = dict(probes=probes32(), probe_frame="tunnel", tracers=seeds37(), tracer_release=np.array([1, 40, 130], dtype=np.int64)[np.arange(37) % 3],
                  tracer_steps=[1, 64, 128, 129, 400], survey=pts, survey_frame="tunnel", survey_steps=(5, 395, 3))
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**CONFIG1, verbose=False, engine=eng, **others, **extra)
        wake_plain = _final_wake(eng)
        binned = LUDVM(**CONFIG1, verbose=False, engine=eng, survey_bins=7, survey_period=3.1, **others, **extra)
        wake_binned = _final_wake(eng)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "survey_bin_sums")
    _same_run(plain, binned)
    for a, b in zip(wake_plain, wake_binned):
        assert np.array_equal(a, b)
    assert plain.survey_count == binned.survey_count == 130 and np.array_equal(plain.survey_sums, binned.survey_sums)
    assert np.array_equal(plain.survey_uw, binned.survey_uw)
    assert np.array_equal(plain.probe_u, binned.probe_u) and np.array_equal(plain.probe_w, binned.probe_w)
    assert plain.tracer_path.steps() == binned.tracer_path.steps()
    for s in plain.tracer_path.steps():
        assert np.array_equal(plain.tracer_path[s], binned.tracer_path[s]), s
    assert np.array_equal(plain.tracer_last, binned.tracer_last)
    assert binned.survey_bin_count.sum() == 130 and (binned.survey_bin_count > 0).all()
    assert np.isfinite(binned.survey_bin_sums).all() and np.abs(binned.survey_bin_sums[:, 2]).min() > 0.0
    check_bin_derived(binned)


@pytest.mark.parametrize("sym", [1, 64])
def test_bin_sums_do_not_depend_on_the_chunking(eng, tmp_path, sym):
    """The same bin sums and counts, bit for bit, across _march_chunk = 32768 / 100 / 7, snapshot_steps inside the window, dense
    or sparse history, and a checkpoint after step 300 (a window step) with a resume -- serial steps and overlapped ones.  400
    steps of config 1 in fp32, 600 points, window 20 .. 390 every 7, five phase bins."""
    kw = dict(CONFIG1)
    pts = seeds_random(600)
    steps = (20, 390, 7)
    assert 300 in window(*steps, 401)
    common = dict(verbose=False, engine=eng, precision="f32", survey=pts, survey_frame="tunnel", survey_steps=steps, survey_bins=5,
                  survey_period=4.3, survey_phase0=0.35)
    eng.set_symmetric(sym)
    try:
        base = _chunked(32768)(**kw, **common, history="sparse")
        assert base.nt == 401 and base.survey_count == 53 == base.survey_bin_count.sum()
        runs = {
            "again": _chunked(32768)(**kw, **common, history="sparse"),
            "chunk 100 + snapshots": _chunked(100)(**kw, **common, history="sparse", snapshot_steps=[27, 28, 64, 192, 193, 300]),
            "chunk 7": _chunked(7)(**kw, **common, history="sparse"),
            "dense": _ludvm()(**kw, **common, history="full"),
            "dense, chunk 7": _chunked(7)(**kw, **common, history="full"),
        }
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, history="sparse", checkpoint_every=300, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 301 and R["survey_bin_sums"].shape == (5, 5, 600)
        assert int(R["survey_bin_counts"].sum()) == int(R["survey_samples"]) == len(window(20, 301, 7, 401))
        runs["resumed from 300"] = _ludvm().resume(ck, engine=eng, verbose=False)
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert np.array_equal(r.survey_bin_count, base.survey_bin_count), name
        assert np.array_equal(r.survey_bin_sums, base.survey_bin_sums), name
        assert np.array_equal(r.survey_sums, base.survey_sums) and np.array_equal(r.Cl, base.Cl), name
    assert not np.array_equal(R["survey_bin_sums"], base.survey_bin_sums) and (base.survey_bin_count > 0).all()


def test_marched_and_per_step_bins_agree(eng):
    """march=True and march=False in 'f64', window steps 1-10, four bins: 1e-12 of max|u| (of max|u|^2 for the second
    moments), the bound the plain sums of the two paths hold."""
    kw = dict(CONFIG1, tf=1.0)
    pts = probes32()
    common = dict(verbose=False, engine=eng, precision="f64", survey=pts, survey_frame="tunnel", survey_steps=(1, 11, 1), probes=pts,
                  probe_frame="tunnel", survey_bins=4, survey_period=0.3)
    a = _ludvm()(**kw, **common, march=True)
    b = _ludvm()(**kw, **common, march=False)
    assert np.array_equal(a.survey_bin_count, b.survey_bin_count) and a.survey_bin_count.sum() == 10 and (a.survey_bin_count > 0).all()
    umax = series_umax(b.probe_u, b.probe_w, window(1, 11, 1, 21))
    for k in range(4):
        e_mean, e_mom = sums_errors(a.survey_bin_sums[k], b.survey_bin_sums[k], int(a.survey_bin_count[k]), umax)
        print(f"march vs per-step: bin {k} ({a.survey_bin_count[k]} samples): means {e_mean:.2e} of max|u|, second moments {e_mom:.2e} "
              "of max|u|^2")
        assert e_mean <= 1e-12 and e_mom <= 1e-12, (k, e_mean, e_mom)


def _prepared(eng, **extra):
    """A 20-step 'f64' run set up for the march (ludvm_march_setup and the survey's set calls done, no step run)."""
    sim = _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", run=False, **extra)
    S = sim._loop_begin()
    sim._free_slot = S.fslot
    S.fsl = slice(0, S.nf)
    sim._loop_prepare_engine(S)
    assert S.can_march
    return sim, S


def _code_of(call):
    from ludvm_amd import LudvmHipError
    with pytest.raises(LudvmHipError) as e:
        call()
    return e.value.code


def test_entry_points_answer_the_documented_codes(eng):
    from ludvm_amd import _ffi
    pts = probes32()[:, :5]
    table = np.arange(21) % 3 - 1                                       # (-1, 0, 1 in turn)
    # LUDVM_E_STATE before a survey is set, and on read without bins
    _prepared(eng)
    assert _code_of(lambda: eng.march_set_survey_bins(table, 2)) == _ffi.E_STATE
    assert _code_of(eng.march_survey_bins) == _ffi.E_STATE
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    assert _code_of(eng.march_survey_bins) == _ffi.E_STATE
    eng.march_set_survey_bins(table, 2)
    sums0, n0 = eng.march_survey_bins()                                 # valid before any step: zeros, no samples
    assert sums0.shape == (2, 5, 5) and not sums0.any() and n0.shape == (2,) and not n0.any()
    sim._march_call(S, 1, 7, False, 50)                                 # steps 1 .. 6: samples at 2 (bin 1), 4 (bin 0), 6 (none)
    sums6, n6 = eng.march_survey_bins()
    plain6, m6 = eng.march_survey()
    assert m6 == 3 and np.array_equal(n6, [1, 1]) and np.abs(sums6[:, 2]).min() > 0.0
    # refused arguments change nothing
    nan_sums = sums6.copy()
    nan_sums[1, 3, 2] = np.nan
    for bad in (lambda: eng.march_set_survey_bins(table[:-1], 2),
                lambda: eng.march_set_survey_bins(np.append(table, 0), 2),
                lambda: eng.march_set_survey_bins(np.where(table == 1, 2, table), 2),
                lambda: eng.march_set_survey_bins(np.where(table == 1, -2, table), 2),
                lambda: eng.march_set_survey_bins(table, MAX_BINS + 1),
                lambda: eng.march_set_survey_bins(table, -1),
                lambda: eng.march_set_survey_bins(table, 2, sums=sums6),
                lambda: eng.march_set_survey_bins(table, 2, counts=n6),
                lambda: eng.march_set_survey_bins(table, 2, sums=nan_sums, counts=n6),
                lambda: eng.march_set_survey_bins(table, 2, sums=sums6, counts=[1, -1])):
        assert _code_of(bad) == _ffi.E_ARG
        again, n_again = eng.march_survey_bins()
        assert np.array_equal(n_again, n6) and np.array_equal(again, sums6)
    # the survey's precision does not forget the bins; continuing from (sums, counts) gives the uninterrupted run's bits
    eng.march_set_survey_precision("f64")
    assert np.array_equal(eng.march_survey_bins()[0], sums6)
    eng.march_set_survey_bins([], 0)                                    # nbins = 0 removes the bins
    assert _code_of(eng.march_survey_bins) == _ffi.E_STATE
    assert np.array_equal(eng.march_survey()[0], plain6)
    eng.march_set_survey_bins(table, 2, sums=sums6, counts=n6)
    sim._march_call(S, 7, 13, False, 50)                                # steps 7 .. 12: samples at 8 (bin 1), 10 (bin 0), 12 (none)
    sums12, n12 = eng.march_survey_bins()
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table)
    whole._march_call(Sw, 1, 13, False, 50)
    sums_whole, n_whole = eng.march_survey_bins()
    assert np.array_equal(n12, n_whole) and np.array_equal(n_whole, [2, 2]) and np.array_equal(sums12, sums_whole)
    assert eng.march_survey()[1] == 6
    # ludvm_march_set_survey forgets the bins, and so does ludvm_march_setup
    eng.march_set_survey(pts[0], pts[1])
    assert _code_of(eng.march_survey_bins) == _ffi.E_STATE and eng.march_survey()[1] == 0
    eng.march_set_survey_bins(table, 2)
    eng.march_setup(whole.Npoints - 1, whole.Ncoeffs, *whole._march_inputs(Sw))
    assert _code_of(eng.march_survey_bins) == _ffi.E_STATE


def test_the_storage_cap(eng):
    """nbins * count one point over LUDVM_MARCH_MAX_SURVEY_BIN_POINTS is refused (and leaves the bins that were set); the cap
    itself -- 64 bins x 65 536 points -- run for 10 steps gives finite sums whose counts add up to the samples."""
    from ludvm_amd import _ffi
    K = MAX_BIN_POINTS // MAX_BINS
    assert K == 65536
    rng = np.random.default_rng(29)
    over = np.stack([rng.uniform(-3.0, 1.5, K + 1), rng.uniform(0.0, 2.0, K + 1)])
    table = np.arange(21) % MAX_BINS
    sim, S = _prepared(eng, survey=over, survey_steps=(1, 11, 1))
    eng.march_set_survey_bins(table, MAX_BINS - 1)                      # (63 x 65 537 is under the cap)
    assert _code_of(lambda: eng.march_set_survey_bins(table, MAX_BINS)) == _ffi.E_ARG
    assert eng.march_survey_bins()[1].shape == (MAX_BINS - 1,)
    with pytest.raises(ValueError, match="survey_bins"):
        _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, survey=over, survey_bins=MAX_BINS, survey_period=4.0)
    full = table.copy()
    full[0] = MAX_BINS - 1                                              # (step 0 is never sampled: the table only names 64 bins)
    sim = _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", history="sparse", survey=over[:, :K],
                   survey_frame="tunnel", survey_steps=(1, 11, 1), survey_bins=full)
    assert sim.survey_nbins == MAX_BINS and sim.survey_bin_sums.shape == (MAX_BINS, 5, K)
    assert sim.survey_count == 10 == sim.survey_bin_count.sum() and np.array_equal(sim.survey_bin_count[1:11], np.ones(10))
    assert np.isfinite(sim.survey_bin_sums).all() and np.abs(sim.survey_bin_sums[1:11, 2]).min() > 0.0
    assert not sim.survey_bin_sums[11:].any() and not sim.survey_bin_sums[0].any()
