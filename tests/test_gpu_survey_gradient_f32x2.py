"""GPU tier: the survey's gradient sums in hi+lo fp32 (march_f32x2_grad_survey_partial under the kObsSurveyF32 plan, the float64
finishers behind it, ludvm_march_set_survey_gradient_f32x2; LUDVM(..., survey=, survey_gradient='f32x2'))
-- the gradient sums by value against the long-double closed forms over the sources a run names itself within the derived
tolerance (many source tiles and splits, point counts on both sides of every tile boundary, the largest survey, an overlapped
fp32 run, far from the origin with a small core), the velocity sums of the same runs by value, passive on every other result, a
bin bit for bit the plain survey of its steps, independent of how a run is cut, and the entry point's codes.

The tolerance (tests/survey_gradient_f32x2_common.py) is derived, not tuned: per step and point gradient_f32x2_common's bounds of
ux, e and omega, carried through the squares, summed over the steps, plus survey_gradient_common's float64 allowance.  Every
by-value test first asserts, from the reference alone, that the tolerance is below 1e-2 of the scale at every point and that the
sums over a wake taken one step late are off by more than ten tolerances somewhere."""
import json
import signal

import numpy as np
import pytest

import observer_sources_common as OS
import survey_gradient_common as SG
import survey_gradient_f32x2_common as C
from conftest import CONFIG1
from probes_common import probes32
from survey_f32_common import far_sheet, points_around
from test_gpu_survey_gradient import first_step_sources
from tracers_common import run_sources, seeds37, seeds_random

pytestmark = pytest.mark.gpu

PLAN_TILE = 1024    # kSurveyF32Tile of march_kernels.hpp: the tile of the launch plan (kObsSurveyF32)
GROUP = 512         # kSurveyGradF32Tile: the points of one workgroup of the fused kernel
LIMIT = 1048576     # LUDVM_MARCH_MAX_SURVEY
F32X2 = dict(survey_gradient="f32x2")


@pytest.fixture(autouse=True)
def _time_limit():
    """A limit on every test's host-side time (the handler runs between Python instructions)."""
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


def _chunked(chunk):
    return type("Chunked", (_ludvm(),), dict(_march_chunk=chunk))


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


def _sources_of(sim):
    return lambda i: first_step_sources(sim) if i == 1 else run_sources(sim, i)


def _check_by_value(sim, steps, what, pick=None):
    """The run's ten sums (at the points `pick`) against the references over the run's own sources, added in step order;
    -> (worst gradient error / tolerance, / scale)."""
    pick = np.arange(sim._survey_xz.shape[1]) if pick is None else pick
    pts = lambda i: tuple(c[pick] for c in sim._survey_points(i))       # noqa: E731
    assert sim.survey_count == len(steps) and sim.survey_gradient == "f32x2"
    R = C.reference(steps, pts, _sources_of(sim), sim.v_core)
    out = C.check_sums(sim.survey_grad_sums.reshape(5, -1)[:, pick], R, what)
    C.check_velocity(sim.survey_sums.reshape(5, -1)[:, pick], steps, pts, _sources_of(sim), sim.v_core, OS.fast_iv(), OS.field, what)
    return out


def test_the_tiles_are_what_the_tests_assume():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    per_lane = {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kSurveyF32PerLane", "kSurveyGradF32PerLane")}
    assert 256 * per_lane["kSurveyF32PerLane"] == PLAN_TILE and 256 * per_lane["kSurveyGradF32PerLane"] == GROUP


@pytest.mark.parametrize("case", ["A", "B"])
def test_by_value_over_the_runs_own_sources_at_many_source_tiles(eng, case):
    """Cases A and B of tests/observer_sources_common.py with the 600-point survey, 'f64', dense history.  Case A, all 24 steps:
    five full splits of 256 sources, a sixth that stays empty through step 20 and holds one source from step 21.  Case B, window
    (12, 14, 1): 64 splits of 256 at step 12, 33 of 512 at step 13."""
    obs = OS.observers(case, "few")
    win = (1, OS.CASES[case][1] + 1, 1) if case == "A" else (12, 14, 1)
    sim = _ludvm()(**OS.case_keywords(case), verbose=False, engine=eng, precision="f64", history="full", survey=obs["survey"],
                   survey_steps=win, **F32X2)
    assert sim.nt == OS.CASES[case][1] + 1 and (sim.LEV_shed[1:] == -1).all()
    steps = list(range(win[0], min(win[1], sim.nt), win[2]))
    assert len(steps) == (24 if case == "A" else 2)
    _check_by_value(sim, steps, f"case {case}")
    SG.check_derived(sim)


@pytest.mark.parametrize("K", [1, GROUP - 1, GROUP, GROUP + 1, PLAN_TILE - 1, PLAN_TILE, PLAN_TILE + 1, 2 * PLAN_TILE + 1])
def test_point_counts_on_both_sides_of_every_tile_boundary(eng, K):
    """K survey points over 30 steps of config 1 in 'f64', dense history, tunnel frame, every step sampled: one lane, one workgroup of
    the fused kernel and the next (511 / 512 / 513), one tile of the plan and the next (1023 / 1024 / 1025), two tiles and one
    point -- by value, every point written."""
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="full", survey=seeds_random(K, seed=17),
                   survey_frame="tunnel", **F32X2)
    assert sim.nt == 31 and sim.survey_grad_sums.shape == (5, K)
    _check_by_value(sim, list(range(1, 31)), f"K = {K}")
    assert np.isfinite(sim.survey_grad_sums).all() and (sim.survey_grad_sums[3] > 0.0).all()


def test_the_largest_survey(eng):
    """K = 1 048 576 points on the last two steps of the README case (LUDVM() with its default arguments), dense history: 1024
    sampled points by value, every point written.  (observer_sources_common.survey_sample takes both ends of EVERY 512-point tile:
    4096 points here, over its 1024.  The same idea within 1024: both ends of the first and the last workgroup of 512 and of 254
    drawn ones, the other 512 points drawn.)"""
    rng = np.random.default_rng(23)
    pts = np.stack([rng.uniform(-1.0, 13.0, LIMIT), rng.uniform(-1.0, 3.0, LIMIT)])
    groups = np.concatenate([[0, LIMIT // GROUP - 1], rng.choice(np.arange(1, LIMIT // GROUP - 1), 254, replace=False)])
    pick = np.unique(np.concatenate([groups * GROUP, groups * GROUP + GROUP - 1, rng.choice(LIMIT, 512, replace=False)]))
    assert 1000 <= len(pick) <= 1024 and pick[0] == 0 and pick[-1] == LIMIT - 1
    nt = _ludvm()(verbose=False, engine=eng, run=False).nt
    assert nt > 800
    sim = _ludvm()(verbose=False, engine=eng, history="full", survey=pts, survey_frame="tunnel", survey_steps=(nt - 2, nt, 1), **F32X2)
    assert sim.nt == nt and sim.survey_count == 2 and sim.survey_grad_sums.shape == (5, LIMIT)
    _check_by_value(sim, [nt - 2, nt - 1], f"K = {LIMIT}", pick=pick)
    assert np.isfinite(sim.survey_grad_sums).all() and (sim.survey_grad_sums[3] > 0.0).all()


def test_by_value_in_an_overlapped_fp32_run(eng):
    """200 steps of config 1 in fp32 with the symmetric threshold at 64 (overlapped steps), dense history, probes set, 128 points
    in the tunnel frame sampled at every step 70 .. 200: the sources (196 at step 70, 384 at step 200) pass one 256-source tile, so
    the plan goes from one split to several.  (They do not reach 512 within 200 steps of config 1.)"""
    eng.set_symmetric(64)
    try:
        sim = _ludvm()(**dict(CONFIG1, tf=10.0), verbose=False, engine=eng, precision="f32", history="full", probes=probes32(),
                       survey=seeds_random(128), survey_frame="tunnel", survey_steps=(70, 201, 1), **F32X2)
    finally:
        eng.set_symmetric(1)
    ns = [len(run_sources(sim, s)[0]) + 80 for s in (70, 200)]
    print(f"sources of step 70: {ns[0]}, of step 200: {ns[1]}")
    assert sim.nt == 201 and ns[0] < 256 < ns[1]
    _check_by_value(sim, list(range(70, 201)), "overlapped fp32, steps 70-200")
    SG.check_derived(sim)


_sheet = {}


def _sheet_run(eng, x0, window):
    """the sheet at x0 as free vortices, surveyed over `window` at survey_f32_common.points_around's 1800 points"""
    g, x, z = far_sheet(x0=x0)
    pts = points_around(x, z, 1.3e-3)
    sim = _ludvm()(**dict(CONFIG1, dt=1e-3, tf=8e-3, circulation_freevort=g, xy_freevort=np.stack([x, z])), verbose=False,
                   engine=eng, precision="f64", history="full", survey=pts, survey_steps=window, **F32X2)
    assert abs(sim.v_core - 1.3e-3) < 1e-15 and sim.nt >= 9 and pts.shape == (2, 1800)
    return sim


@pytest.mark.parametrize("x0", [-55.0, -5000.0])
def test_far_from_the_origin_with_a_small_core(eng, x0):
    """A 600-vortex sheet 1e-3 apart at x = x0 as free vortices, v_core = 1.3e-3 (dt = 1e-3): 1800 survey points on the vortices,
    within one core of them and chords away (survey_f32_common.points_around), steps 1 .. 8 by value -- under the same tolerance
    at x0 = -55 and at x0 = -5000: the bound knows nothing of the offset."""
    _sheet[x0] = _check_by_value(_sheet_run(eng, x0, (1, 9, 1)), list(range(1, 9)), f"sheet at {x0:g}")
    assert 0.0 < _sheet[x0][0] <= 1.0


def test_error_over_tolerance_is_the_same_at_both_places(eng):
    """The same sheet at x = -55 and at x = -5000, sampled in step 1 -- the step in which the two places hold the same problem, one
    a translation of the other: the worst error over the tolerance, as printed (three decimals), is the same at both.

    Only step 1 can be compared digit for digit.  The foil sits at the origin in both runs, 55 chords from one sheet and 5000 from
    the other, so from the first roll-up on the two sheets are different flows: after 8 steps their vortices, measured from x0,
    differ by 3.5e-10, more than the rounding of a near difference in fp32 (5.8e-11 at 1e-3), and the long-double references of
    the two places differ by 0.41 tolerances.  Their fp32 roundings are then independent draws: over steps 1 .. 8 the runs above
    print 0.015 and 0.012 of the (same) tolerance, in step 8 alone 0.026 and 0.023, in step 1 alone 0.0177 and 0.0177 [MI355X]."""
    printed = []
    for x0 in (-55.0, -5000.0):
        sim = _sheet_run(eng, x0, (1, 2, 1))
        assert sim.survey_count == 1
        R = C.reference([1], lambda i: sim._survey_points(i), _sources_of(sim), sim.v_core, late=False)
        ratio, _ = C.check_sums(sim.survey_grad_sums.reshape(5, -1), R, f"sheet at {x0:g}, step 1")
        printed.append(f"{ratio:.3f}")
    assert printed[0] == printed[1] and float(printed[0]) > 0.0, printed


def _same_run(a, b, surveys=True):
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
    assert np.array_equal(a.probe_u, b.probe_u) and np.array_equal(a.probe_w, b.probe_w)
    assert a.tracer_path.steps() == b.tracer_path.steps()
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s]), ("tracer_path", s)
    assert np.array_equal(a.tracer_last, b.tracer_last)
    assert a.survey_count == b.survey_count
    assert hasattr(a, "survey_bin_sums") == hasattr(b, "survey_bin_sums")
    if hasattr(a, "survey_bin_sums"):
        assert np.array_equal(a.survey_bin_count, b.survey_bin_count)
    if surveys:
        assert np.array_equal(a.survey_sums, b.survey_sums)
        if hasattr(a, "survey_bin_sums"):
            assert np.array_equal(a.survey_bin_sums, b.survey_bin_sums)
        assert hasattr(a, "survey_grad_sums") == hasattr(b, "survey_grad_sums")
        if hasattr(a, "survey_grad_sums"):
            assert np.array_equal(a.survey_grad_sums, b.survey_grad_sums)
        if hasattr(a, "survey_bin_grad_sums"):
            assert np.array_equal(a.survey_bin_grad_sums, b.survey_bin_grad_sums)


def _velocity_sums_close(sums, ref, n):
    """velocity sums of the fused walk against a float64 survey's [5, ...]: means within VELOCITY_VS_F64 of max|u|, raw second
    moments within 3 times that of max|u|^2 -- with the largest root mean square in max|u|'s place, which is no larger"""
    from survey_common import sums_errors
    umax = float(np.sqrt(np.asarray(ref)[2:4].max() / n))
    e_mean, e_sq = sums_errors(sums, ref, n, umax)
    assert umax > 0.0 and e_mean <= C.VELOCITY_VS_F64 and e_sq <= C.MOMENT_VS_F64, (e_mean, e_sq)
    return e_mean, e_sq


@pytest.mark.parametrize("bins", [False, True], ids=["plain", "binned"])
@pytest.mark.parametrize("case", ["f64_dense", "f32_sparse_overlapped"])
def test_the_route_is_passive(eng, case, bins):
    """A plain survey, survey_gradient=True, survey_gradient='f32x2', then True and plain again, on one context, 600 points with
    probes and tracers set: Cl / Cd / Cm, every circulation[...], LEV_shed, the history rows, the final resident wake, the probe
    rows and the tracer paths of the 'f32x2' run are the plain run's arrays, bit for bit; its velocity sums differ from them,
    within the hi+lo tier; the later runs reproduce the bits of the earlier ones of their kind."""
    LUDVM = _ludvm()
    kw = dict(CONFIG1, tf=10.0)
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101])}[case]
    others = dict(probes=probes32(), probe_frame="tunnel", tracers=seeds37(),
                  tracer_release=np.array([1, 40, 130], dtype=np.int64)[np.arange(37) % 3], tracer_steps=[1, 64, 128, 129, 200],
                  survey=seeds_random(600), survey_frame="tunnel", survey_steps=(5, 195, 3))
    if bins:
        others.update(survey_bins=7, survey_period=3.1)
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**kw, verbose=False, engine=eng, **others, **extra)
        wake_plain = _final_wake(eng)
        f64 = LUDVM(**kw, verbose=False, engine=eng, survey_gradient=True, **others, **extra)
        grad = LUDVM(**kw, verbose=False, engine=eng, **F32X2, **others, **extra)
        wake_grad = _final_wake(eng)
        f64_again = LUDVM(**kw, verbose=False, engine=eng, survey_gradient=True, **others, **extra)
        plain_again = LUDVM(**kw, verbose=False, engine=eng, **others, **extra)
    finally:
        eng.set_symmetric(1)
    assert grad.survey_gradient == "f32x2" and f64.survey_gradient is True and plain.survey_gradient is False
    _same_run(plain, grad, surveys=False)
    for a, b in zip(wake_plain, wake_grad):
        assert np.array_equal(a, b)
    _same_run(f64, f64_again)
    _same_run(plain, plain_again)
    assert not hasattr(plain_again, "survey_grad_sums")
    n = grad.survey_count
    assert not np.array_equal(grad.survey_sums, plain.survey_sums)
    e = _velocity_sums_close(grad.survey_sums, plain.survey_sums, n)
    print(f"{case}, {'binned' if bins else 'plain'}: velocity sums vs the float64 survey's: means {e[0]:.2e} of the largest rms "
          f"velocity, second moments {e[1]:.2e} of its square")
    assert grad.survey_grad_sums.shape == (5, 600) and np.isfinite(grad.survey_grad_sums).all()
    assert (grad.survey_grad_sums[3] > 0.0).all()                       # every point was written
    assert not np.array_equal(grad.survey_grad_sums, f64.survey_grad_sums)
    g_mean, g_sq = SG.sums_errors(grad.survey_grad_sums, f64.survey_grad_sums, n, float(np.sqrt(f64.survey_grad_sums[3].max() / n)))
    print(f"    gradient sums vs the float64 route's: means {g_mean:.2e} of the largest rms vorticity, squares {g_sq:.2e}")
    SG.check_derived(grad)
    if bins:
        assert grad.survey_bin_grad_sums.shape == (7, 5, 600) and (grad.survey_bin_grad_sums[:, 3] > 0.0).all()
        SG.check_bin_derived(grad)
        for b in range(7):
            _velocity_sums_close(grad.survey_bin_sums[b], plain.survey_bin_sums[b], int(grad.survey_bin_count[b]))
        tot = grad.survey_bin_grad_sums.sum(axis=0)
        assert np.abs(tot - grad.survey_grad_sums).max() <= 1e-12 * np.abs(grad.survey_grad_sums).max()
    else:
        assert not hasattr(grad, "survey_bin_grad_sums")


@pytest.mark.parametrize("K", [1, GROUP + 1])
@pytest.mark.parametrize("sym", [1, 64], ids=["serial", "overlapped"])
def test_a_bin_is_bit_identical_to_the_plain_survey_of_its_steps(eng, sym, K):
    """200 steps of config 1 in fp32, window (20, 190, 1), table (i - 20) % 3: both blocks of bin b, velocity and gradient, are
    array_equal to the sums of a plain 'f32x2' survey with survey_steps = (20 + b, 190, 3); the plain sums of the binned run are
    those of the run without bins."""
    kw = dict(CONFIG1, tf=10.0)
    pts = seeds_random(K)
    table = (np.arange(201) - 20) % 3
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=pts, survey_frame="tunnel", **F32X2)
    eng.set_symmetric(sym)
    try:
        binned = _ludvm()(**kw, **common, survey_steps=(20, 190, 1), survey_bins=table)
        whole = _ludvm()(**kw, **common, survey_steps=(20, 190, 1))
        plain = [_ludvm()(**kw, **common, survey_steps=(20 + b, 190, 3)) for b in range(3)]
    finally:
        eng.set_symmetric(1)
    assert binned.nt == 201 and binned.survey_bin_grad_sums.shape == (3, 5, K)
    assert binned.survey_count == whole.survey_count == 170 and np.array_equal(binned.survey_grad_sums, whole.survey_grad_sums)
    assert np.array_equal(binned.survey_sums, whole.survey_sums)
    for b in range(3):
        assert binned.survey_bin_count[b] == plain[b].survey_count and plain[b].survey_count in (56, 57)
        assert np.array_equal(binned.survey_bin_grad_sums[b], plain[b].survey_grad_sums), b
        assert np.array_equal(binned.survey_bin_sums[b], plain[b].survey_sums), b
    assert np.isfinite(binned.survey_bin_grad_sums).all() and (binned.survey_bin_grad_sums[:, 3] > 0.0).all()


def test_the_sums_do_not_depend_on_the_chunking_a_resume_or_the_run(eng, tmp_path):
    """All ten sums, plain and binned, bit for bit across _march_chunk = 32768 / 7, a repeated run, and a checkpoint after step
    100 (inside the window) with LUDVM.resume, which continues on the route the file names.  200 steps of config 1 in fp32
    (overlapped: symmetric threshold 64), 600 points, window 20 .. 190 every 3, five phase bins."""
    kw = dict(CONFIG1, tf=10.0)
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=seeds_random(600), survey_frame="tunnel",
                  survey_steps=(20, 190, 3), survey_bins=5, survey_period=4.3, survey_phase0=0.35, **F32X2)
    eng.set_symmetric(64)
    try:
        base = _chunked(32768)(**kw, **common)
        assert base.nt == 201 and base.survey_count == 57 == base.survey_bin_count.sum()
        runs = {"again": _chunked(32768)(**kw, **common), "chunk 7": _chunked(7)(**kw, **common)}
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, checkpoint_every=100, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 101 and R["survey_grad_sums"].shape == (5, 600)
        assert R["survey_bin_grad_sums"].shape == (5, 5, 600) and int(R["survey_samples"]) == 27
        assert (R["survey_grad_sums"][3] > 0.0).all() and not np.array_equal(R["survey_grad_sums"], base.survey_grad_sums)
        assert json.loads(str(R["ctor"]))["survey_gradient"] == "f32x2"
        runs["resumed from 100"] = _ludvm().resume(ck, engine=eng, verbose=False)
        assert runs["resumed from 100"].survey_gradient == "f32x2"
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert r.survey_count == base.survey_count and np.array_equal(r.survey_bin_count, base.survey_bin_count), name
        assert np.array_equal(r.survey_sums, base.survey_sums) and np.array_equal(r.survey_bin_sums, base.survey_bin_sums), name
        assert np.array_equal(r.survey_grad_sums, base.survey_grad_sums), name
        assert np.array_equal(r.survey_bin_grad_sums, base.survey_bin_grad_sums), name
        assert np.array_equal(r.Cl, base.Cl), name
    assert (base.survey_bin_count > 0).all() and (base.survey_grad_sums[3] > 0.0).all()


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


def test_the_entry_point_answers_the_documented_codes(eng):
    from ludvm_amd import _ffi
    pts = probes32()[:, :5]
    table = np.arange(21) % 3 - 1                                       # (-1, 0, 1 in turn)
    setter = eng.march_set_survey_gradient_f32x2
    # no survey set: LUDVM_E_STATE
    _prepared(eng)
    assert _code_of(setter) == _ffi.E_STATE
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    # bin sums without bins, or without the plain sums: LUDVM_E_ARG, and the route stays off
    assert _code_of(lambda: setter(gsums=np.zeros([5, 5]), bin_gsums=np.zeros([2, 5, 5]))) == _ffi.E_ARG
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_bins(table, 2)
    assert _code_of(lambda: setter(bin_gsums=np.zeros([2, 5, 5]))) == _ffi.E_ARG
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    # the fp32 (local-origin) survey is set: LUDVM_E_STATE; and the route refuses that precision while it is on
    eng.march_set_survey_precision("f32")
    assert _code_of(setter) == _ffi.E_STATE
    eng.march_set_survey_precision("f64")
    setter()
    g0, bg0 = eng.march_survey_gradient()                               # valid before any step: zeros
    assert g0.shape == (5, 5) and bg0.shape == (2, 5, 5) and not g0.any() and not bg0.any()
    assert _code_of(lambda: eng.march_set_survey_precision("f32")) == _ffi.E_STATE
    sim._march_call(S, 1, 7, False, 50)                                 # steps 1 .. 6: samples at 2 (bin 1), 4 (bin 0), 6 (none)
    g6, bg6 = eng.march_survey_gradient()
    sums6, m6 = eng.march_survey()
    assert m6 == 3 and (g6[3] > 0.0).all() and (bg6[:, 3] > 0.0).all()
    # the same steps through the class: the same bits; by the float64 pair: other bits, in the gradient and the velocity sums
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table, **F32X2)
    whole._march_call(Sw, 1, 7, False, 50)
    assert np.array_equal(eng.march_survey_gradient()[0], g6) and np.array_equal(eng.march_survey()[0], sums6)
    f64, Sf = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table, survey_gradient=True)
    f64._march_call(Sf, 1, 7, False, 50)
    g6_f64, sums6_f64 = eng.march_survey_gradient()[0], eng.march_survey()[0]
    assert not np.array_equal(g6_f64, g6) and not np.array_equal(sums6_f64, sums6)
    # ludvm_march_set_survey_gradient(ctx, 1, ..) while the route is on switches to the float64 pair
    sw, Ss = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table, **F32X2)
    eng.march_set_survey_gradient(True)
    sw._march_call(Ss, 1, 7, False, 50)
    assert np.array_equal(eng.march_survey_gradient()[0], g6_f64) and np.array_equal(eng.march_survey()[0], sums6_f64)
    eng.march_set_survey_precision("f64")
    # samples without sums: LUDVM_E_STATE; values that are not finite: LUDVM_E_ARG; a refused call leaves the sums as they were
    plain, Sp = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table)
    plain._march_call(Sp, 1, 7, False, 50)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE          # (ludvm_march_setup reset it)
    assert _code_of(setter) == _ffi.E_STATE
    setter(gsums=g6, bin_gsums=bg6)
    bad_g, bad_bg = g6.copy(), bg6.copy()
    bad_g[2, 1], bad_bg[1, 4, 0] = np.nan, np.inf
    for bad, code in ((lambda: setter(gsums=bad_g, bin_gsums=bg6), _ffi.E_ARG), (lambda: setter(gsums=g6, bin_gsums=bad_bg), _ffi.E_ARG),
                      (lambda: setter(bin_gsums=bg6), _ffi.E_ARG), (setter, _ffi.E_STATE),
                      (lambda: eng.march_set_survey_precision("f32"), _ffi.E_STATE)):
        assert _code_of(bad) == code
        g, bg = eng.march_survey_gradient()
        assert np.array_equal(g, g6) and np.array_equal(bg, bg6)
    with pytest.raises(ValueError):
        setter(gsums=g6[:, :3])
    # carried over (the velocity sums are the float64 survey's of steps 1 .. 6 here), the route continues: steps 7 .. 12 add what
    # they add in the uninterrupted 'f32x2' run
    plain._march_call(Sp, 7, 13, False, 50)                             # samples at 8 (bin 1), 10 (bin 0), 12 (none)
    g12, bg12 = eng.march_survey_gradient()
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table, **F32X2)
    whole._march_call(Sw, 1, 13, False, 50)
    gw, bgw = eng.march_survey_gradient()
    assert eng.march_survey()[1] == 6 and np.array_equal(g12, gw) and np.array_equal(bg12, bgw)
    # on = 0 removes the sums and the route; ludvm_march_set_survey_bins and ludvm_march_set_survey reset it
    setter(gsums=gw, bin_gsums=bgw)
    eng.march_set_survey_gradient(False)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_precision("f32")                               # (no longer refused)
    eng.march_set_survey_precision("f64")
    setter(gsums=gw, bin_gsums=bgw)
    sbins, nbins = eng.march_survey_bins()
    eng.march_set_survey_bins(table, 2, sums=sbins, counts=nbins)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    setter(gsums=gw, bin_gsums=bgw)
    eng.march_set_survey(pts[0], pts[1])
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    setter()                                                            # a fresh survey: no samples, sums from zero
    g, bg = eng.march_survey_gradient()
    assert not g.any() and bg is None
