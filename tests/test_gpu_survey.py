"""GPU tier: wake-survey statistics accumulated inside the device-resident march (march_survey_partial / march_survey_finish,
ludvm_march_set_survey / ludvm_march_read_survey) -- against the oracle, against the probes of the same run, passive on every
other result, independent of how a run is cut into calls, on both sides of every tile boundary up to the limit, against the
per-step path, and the codes of the two entry points."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from probes_common import ProbedOracle, probes32
from survey_common import (CASE_IDS, MEAN_VS_ORACLE, MEAN_VS_PROBES, MOMENT_VS_ORACLE, MOMENT_VS_PROBES, ORACLE_CASES, case_keywords,
                           check_derived, oracle_series, series_sums, series_umax, sums_errors, window)
from tracers_common import seeds37, seeds_random

pytestmark = pytest.mark.gpu

TILE = 512          # kSurveyTile of march_kernels.hpp: 256 lanes x 2 points
LIMIT = 1048576     # LUDVM_MARCH_MAX_SURVEY


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


@pytest.mark.parametrize("method,frame,cloud", ORACLE_CASES, ids=CASE_IDS)
def test_marched_sums_match_the_oracle(eng, method, frame, cloud):
    """Check 1 of the CPU tier through the real march in 'f64', dense and sparse history: the sums over steps 1-50 at
    probes32()'s points against ProbedOracle's series -- means at 1e-9 of max|u|, raw second moments at 3e-9 of max|u|^2."""
    pts = probes32()
    ou, ow = oracle_series(pts, method, frame, cloud)
    steps = window(1, 51, 1, 51)
    ref, umax = series_sums(ou, ow, steps), series_umax(ou, ow, steps)
    for hist in ("full", "sparse"):
        sim = _ludvm()(**case_keywords(method, cloud), verbose=False, engine=eng, precision="f64", history=hist, survey=pts,
                       survey_frame=frame, survey_steps=(1, 51, 1))
        assert sim.survey_count == 50
        e_mean, e_mom = sums_errors(sim.survey_sums, ref, 50, umax)
        print(f"{method} {frame} cloud={cloud} ({hist}): marched survey vs oracle, steps 1-50: means {e_mean:.2e} of max|u|, raw "
              f"second moments {e_mom:.2e} of max|u|^2")
        assert e_mean <= MEAN_VS_ORACLE, (hist, e_mean)
        assert e_mom <= MOMENT_VS_ORACLE, (hist, e_mom)
        check_derived(sim)


@pytest.mark.parametrize("case", ["f64_serial", "f32_overlapped"])
def test_survey_is_the_reduction_of_the_probe_rows_of_the_same_run(eng, case):
    """The survey at the probes' own points against the reduction of probe_u / probe_w over the window's steps: means at 1e-12
    of max|u|, raw second moments at 3e-12 of max|u|^2.  Serial 'f64' steps (window 7 .. 190 every 3), and overlapped fp32
    steps 70-200 (symmetric threshold lowered to 64: the survey launch rides the second stream behind the solve and the
    probes, beside the symmetric kernel; a launch placed behind the Euler finisher would see the wake a step later)."""
    pts = probes32()
    kw = dict(CONFIG1, tf=10.0)
    prec, steps, sym = ("f64", (7, 190, 3), 1) if case == "f64_serial" else ("f32", (70, 201, 1), 64)
    eng.set_symmetric(sym)
    try:
        sim = _ludvm()(**kw, verbose=False, engine=eng, precision=prec, history="sparse", probes=pts, probe_frame="tunnel", survey=pts,
                       survey_frame="tunnel", survey_steps=steps)
    finally:
        eng.set_symmetric(1)
    W = window(*steps, sim.nt)
    assert sim.nt == 201 and sim.survey_count == len(W)
    ref, umax = series_sums(sim.probe_u, sim.probe_w, W), series_umax(sim.probe_u, sim.probe_w, W)
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, len(W), umax)
    print(f"{case}: survey vs the run's own probe rows over {len(W)} steps: means {e_mean:.2e} of max|u|, raw second moments "
          f"{e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_PROBES, e_mean
    assert e_mom <= MOMENT_VS_PROBES, e_mom


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
def test_a_survey_is_passive(eng, case):
    """With and without a survey of 600 points (two tiles), with probes and tracers set in both runs: Cl / Cd / Cm, every
    circulation[...], LEV_shed, the history rows, the final wake, probe_u / probe_w and the tracer paths are the same arrays,
    bit for bit -- serial and overlapped steps (symmetric threshold lowered), dense and sparse history."""
    LUDVM = _ludvm()
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_dense_overlapped": dict(precision="f32", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101]),
             "f32_sparse_serial": dict(precision="f32", history="sparse", snapshot_steps=[64])}[case]
    pts = seeds_random(600)
    others = dict(probes=probes32(), probe_frame="tunnel", tracers=seeds37(), tracer_release=np.array([1, 40, 130], dtype=np.int64)[np.arange(37) % 3],
                  tracer_steps=[1, 64, 128, 129, 400])
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**CONFIG1, verbose=False, engine=eng, **others, **extra)
        wake_plain = _final_wake(eng)
        surveyed = LUDVM(**CONFIG1, verbose=False, engine=eng, survey=pts, survey_frame="tunnel", survey_steps=(5, 395, 3), **others, **extra)
        wake_surveyed = _final_wake(eng)
        bare = LUDVM(**CONFIG1, verbose=False, engine=eng, survey=pts, **extra)          # (and without probes and tracers)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "survey_sums")
    _same_run(plain, surveyed)
    _same_run(plain, bare)
    for a, b in zip(wake_plain, wake_surveyed):
        assert np.array_equal(a, b)
    assert np.array_equal(plain.probe_u, surveyed.probe_u) and np.array_equal(plain.probe_w, surveyed.probe_w)
    assert plain.tracer_path.steps() == surveyed.tracer_path.steps()
    for s in plain.tracer_path.steps():
        assert np.array_equal(plain.tracer_path[s], surveyed.tracer_path[s]), s
    assert np.array_equal(plain.tracer_last, surveyed.tracer_last)
    assert surveyed.survey_count == 130 and bare.survey_count == 400
    assert np.isfinite(surveyed.survey_sums).all() and surveyed.survey_uu.max() > 0.0


@pytest.mark.parametrize("sym", [1, 64])
def test_survey_sums_do_not_depend_on_the_chunking(eng, tmp_path, sym):
    """The same bits across _march_chunk = 32768 / 100 / 7, snapshot_steps inside the window, dense or sparse history, the
    caps on one call's probe and tracer rows, run to run, and across a checkpoint after step 300 (a window step) with a resume --
    serial steps (sym = 1) and overlapped ones (threshold 64).  400 steps of config 1 in fp32, 600 points, window 20 .. 390
    every 7."""
    kw = dict(CONFIG1)
    pts = seeds_random(600)
    steps = (20, 390, 7)
    W = window(*steps, 401)
    assert 300 in W
    common = dict(verbose=False, engine=eng, precision="f32", survey=pts, survey_frame="tunnel", survey_steps=steps)
    capped = dict(probes=probes32(), tracers=seeds37(), tracer_steps=[1, 27, 28, 29, 300, 400])
    eng.set_symmetric(sym)
    try:
        base = _chunked(32768)(**kw, **common, history="sparse")
        assert base.nt == 401 and base.survey_count == len(W) == 53
        runs = {
            "again": _chunked(32768)(**kw, **common, history="sparse"),
            "chunk 100 + snapshots": _chunked(100)(**kw, **common, history="sparse", snapshot_steps=[27, 28, 64, 192, 193, 300]),
            "chunk 7": _chunked(7)(**kw, **common, history="sparse"),
            "dense": _ludvm()(**kw, **common, history="full"),
            "dense, chunk 7": _chunked(7)(**kw, **common, history="full"),
            "probe and tracer row caps": _chunked(32768, _probe_call_bytes=16 * 32 * 9, _tracer_call_bytes=16 * 37 * 2)(
                **kw, **common, **capped, history="sparse"),
        }
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, history="sparse", checkpoint_every=300, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 301 and R["survey_sums"].shape == (5, 600) and int(R["survey_samples"]) == len(window(20, 301, 7, 401))
        runs["resumed from 300"] = _ludvm().resume(ck, engine=eng, verbose=False)
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert r.survey_count == base.survey_count, name
        assert np.array_equal(r.survey_sums, base.survey_sums), name
        assert np.array_equal(r.Cl, base.Cl), name
    assert not np.array_equal(R["survey_sums"], base.survey_sums) and np.abs(base.survey_sums[2]).min() > 0.0


def test_resume_inside_the_window_in_f64(eng, tmp_path):
    """60 steps in 'f64', window 10 .. 55 every 3, checkpoints every 23 and every 30 steps (steps 46 and 30: 46 is a window
    step), resumed: the same sums and count, bit for bit."""
    kw = dict(CONFIG1, tf=3.0)
    common = dict(verbose=False, engine=eng, precision="f64", survey=probes32(), survey_frame="tunnel", survey_steps=(10, 56, 3))
    base = _ludvm()(**kw, **common)
    assert base.survey_count == 16
    for every, nxt in ((23, 47), (30, 31)):
        ck = str(tmp_path / f"ck{every}.npz")
        _ludvm()(**kw, **common, checkpoint_every=every, checkpoint_path=ck)
        assert int(np.load(ck)["next_step"]) == nxt
        c = _ludvm().resume(ck, engine=eng, verbose=False)
        assert c.survey_count == 16 and np.array_equal(c.survey_sums, base.survey_sums), every


@pytest.fixture(scope="module")
def oracle30():
    """ProbedOracle over 30 steps (tunnel frame) at 1537 points: its series serves every small count."""
    pts = seeds_random(1537, seed=17)
    ref = ProbedOracle(pts, shift=lambda o: o.xpiv, **dict(CONFIG1, tf=1.5))
    return pts, ref.series()


@pytest.mark.parametrize("K", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1])
def test_point_counts_on_both_sides_of_every_tile_boundary(eng, oracle30, K):
    """K points over 30 steps in 'f64' against the oracle at every point, at 1e-9 (3e-9 of max|u|^2 for the raw second
    moments): one lane, one tile and the next (511 / 512 / 513), two and three tiles and one point."""
    pts, (ou, ow) = oracle30
    W = window(1, 31, 1, 31)
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="sparse", survey=pts[:, :K],
                   survey_frame="tunnel")
    assert sim.survey_count == 30 and sim.survey_sums.shape == (5, K)
    ref, umax = series_sums(ou[:, :K], ow[:, :K], W), series_umax(ou, ow, W)
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, 30, umax)
    print(f"K = {K}: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE and e_mom <= MOMENT_VS_ORACLE, (e_mean, e_mom)


def test_the_largest_survey(eng):
    """K = 1 048 576 points over 30 steps in 'f64': a random sample of 512 points against the oracle at 1e-9, and every point
    bit for bit against a second run of the same K."""
    rng = np.random.default_rng(23)
    pts = np.stack([rng.uniform(-3.0, 1.5, LIMIT), rng.uniform(0.0, 2.0, LIMIT)])
    pick = np.sort(rng.choice(LIMIT, 512, replace=False))
    W = window(1, 31, 1, 31)
    ou, ow = ProbedOracle(pts[:, pick], shift=lambda o: o.xpiv, **dict(CONFIG1, tf=1.5)).series()
    kw = dict(CONFIG1, tf=1.5)
    a = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel")
    b = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel")
    assert a.survey_count == 30 and a.survey_sums.shape == (5, LIMIT)
    ref, umax = series_sums(ou, ow, W), series_umax(ou, ow, W)
    e_mean, e_mom = sums_errors(a.survey_sums[:, pick], ref, 30, umax)
    print(f"K = {LIMIT}: 512 sampled points: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE and e_mom <= MOMENT_VS_ORACLE, (e_mean, e_mom)
    assert np.array_equal(a.survey_sums, b.survey_sums)
    assert np.isfinite(a.survey_sums).all() and np.abs(a.survey_sums[2]).min() > 0.0         # every point was written


def test_marched_and_per_step_sums_agree(eng):
    """march=True and march=False in 'f64', window steps 1-10: 1e-12 of max|u| (of max|u|^2 for the second moments)."""
    kw = dict(CONFIG1, tf=1.0)
    pts = probes32()
    common = dict(verbose=False, engine=eng, precision="f64", survey=pts, survey_frame="tunnel", survey_steps=(1, 11, 1), probes=pts,
                  probe_frame="tunnel")
    a = _ludvm()(**kw, **common, march=True)
    b = _ludvm()(**kw, **common, march=False)
    assert a.survey_count == b.survey_count == 10
    umax = series_umax(b.probe_u, b.probe_w, window(1, 11, 1, 21))
    e_mean, e_mom = sums_errors(a.survey_sums, b.survey_sums, 10, umax)
    print(f"march vs per-step: survey sums, steps 1-10: means {e_mean:.2e} of max|u|, second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= 1e-12 and e_mom <= 1e-12, (e_mean, e_mom)


def test_one_point_too_many_is_refused(eng):
    from ludvm_amd import LudvmHipError, _ffi
    with pytest.raises(ValueError, match="1048576"):
        _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, survey=np.zeros([2, LIMIT + 1]))
    sim = _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64")      # (leaves the march set up)
    with pytest.raises(LudvmHipError) as e:
        eng.march_set_survey(np.zeros(LIMIT + 1), np.zeros(LIMIT + 1))
    assert e.value.code == _ffi.E_ARG and sim.nt == 21


def _prepared(eng, **extra):
    """A 20-step 'f64' run set up for the march (ludvm_march_setup and ludvm_march_set_survey done, no step run)."""
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


def test_before_setup_and_on_a_sharded_context_the_answer_is_e_state():
    """ludvm_march_set_survey / ludvm_march_read_survey before ludvm_march_setup, and on a context sharded through
    ludvm_set_shard (whatever the arguments; nothing is launched): LUDVM_E_STATE."""
    import torch
    from ludvm_amd import Engine, _ffi
    pts = probes32()[:, :5]
    fresh = Engine(0)
    try:
        assert _code_of(lambda: fresh.march_set_survey([0.0], [0.0])) == _ffi.E_STATE
        assert _code_of(fresh.march_survey) == _ffi.E_STATE
        _prepared(fresh)
        acc = torch.zeros([64], dtype=torch.int64, device=torch.device("cuda", fresh.device))
        fresh.set_shard(0, 2, lambda count, stream: None, acc.data_ptr(), 64 * 8)
        assert _code_of(lambda: fresh.march_set_survey(pts[0], pts[1])) == _ffi.E_STATE
        assert _code_of(fresh.march_survey) == _ffi.E_STATE
        fresh.set_shard(0, 1)
        fresh.march_set_survey(pts[0], pts[1])                      # (unsharded again: accepted)
        assert fresh.march_survey()[1] == 0
    finally:
        fresh.close()


def test_entry_points_answer_the_documented_codes(eng):
    from ludvm_amd import _ffi
    code_of = _code_of
    pts = probes32()[:, :5]
    # the uninterrupted run: steps 1 .. 12 in one call
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    whole._march_call(Sw, 1, 13, False, 50)
    sums_whole, n_whole = eng.march_survey()
    assert n_whole == 6
    # the same in two calls, the survey taken out and set again from (sums, samples) in between
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    sums0, n0 = eng.march_survey()                                  # valid before any step: zeros, no samples
    assert n0 == 0 and sums0.shape == (5, 5) and not sums0.any()
    sim._march_call(S, 1, 7, False, 50)                             # steps 1 .. 6: samples at 2, 4, 6
    sums6, n6 = eng.march_survey()
    assert n6 == 3 and np.abs(sums6[2]).min() > 0.0
    # refused arguments change nothing
    nan_sums = sums6.copy()
    nan_sums[3, 2] = np.nan
    for bad in (lambda: eng.march_set_survey(np.zeros(LIMIT + 1), np.zeros(LIMIT + 1)),
                lambda: eng.march_set_survey([0.0, np.nan], [0.0, 0.0]),
                lambda: eng.march_set_survey([0.0, 1.0], [0.0, np.inf]),
                lambda: eng.march_set_survey([0.0], [0.0], shift_x=np.zeros(3)),
                lambda: eng.march_set_survey([0.0], [0.0], shift_x=np.full(21, np.nan)),
                lambda: eng.march_set_survey([0.0], [0.0], steps=(0, 10, 1)),
                lambda: eng.march_set_survey([0.0], [0.0], steps=(1, 10, 0)),
                lambda: eng.march_set_survey([0.0], [0.0], steps=(1, 10, -1)),
                lambda: eng.march_set_survey(pts[0], pts[1], sums=sums6, samples=-1),
                lambda: eng.march_set_survey(pts[0], pts[1], sums=nan_sums, samples=3)):
        assert code_of(bad) == _ffi.E_ARG
        again, n_again = eng.march_survey()
        assert n_again == 3 and np.array_equal(again, sums6)
    # count = 0 removes the survey
    eng.march_set_survey([], [])
    assert code_of(eng.march_survey) == _ffi.E_STATE
    # continuing from (sums, samples): the bits of the uninterrupted run
    eng.march_set_survey(pts[0], pts[1], steps=(2, 20, 2), sums=sums6, samples=n6)
    sim._march_call(S, 7, 13, False, 50)                            # steps 7 .. 12: samples at 8, 10, 12
    sums12, n12 = eng.march_survey()
    assert n12 == n_whole == 6 and np.array_equal(sums12, sums_whole)
    # ludvm_march_setup forgets the survey ...
    eng.march_setup(sim.Npoints - 1, sim.Ncoeffs, *sim._march_inputs(S))
    assert code_of(eng.march_survey) == _ffi.E_STATE
    # ... and a run after it is the run it was
    S.survey = None
    sim._march_call(S, 13, 17, False, 50)
    assert code_of(eng.march_survey) == _ffi.E_STATE
    plain = _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64")
    assert np.array_equal(plain.Fn[1:17], sim.Fn[1:17])
