"""GPU tier: gradient sums of the wake survey inside the device-resident march (march_grad_survey_partial /
march_grad_survey_finish / march_binned_grad_survey_finish, ludvm_march_set_survey_gradient / ludvm_march_read_survey_gradient;
LUDVM(..., survey=, survey_gradient=True)) -- passive on every other result, by value against the
long-double closed forms over the sources a run names itself (many source tiles and splits, point counts on both sides of the
512-point tile, the largest survey), a bin bit for bit against the plain gradient survey of its steps, independent of how a run
is cut, against the per-step path, against centred differences of the survey's own mean velocity, and the entry points' codes.

Bounds (tests/survey_gradient_common.py): means of ux, e, omega within 1e-9 of max|grad u| over the sampled steps and points,
means of omega^2 and Q within 3e-9 of max|grad u|^2."""
import signal

import numpy as np
import pytest

import gradient_common as GC
import observer_sources_common as OS
import survey_gradient_common as SG
from conftest import CONFIG1
from oracle import ludvm_oracle as O
from probes_common import probes32
from tracers_common import run_sources, seeds37, seeds_random

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


def _chunked(chunk):
    return type("Chunked", (_ludvm(),), dict(_march_chunk=chunk))


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


def first_step_sources(sim):
    """run_sources for step 1 (it starts at 2): the free vortices as row 0 holds them, the first TEV half a step behind the
    initial trailing edge (LUDVM.py:672-681), an LEV shed in step 1 at the leading edge, the bound vortices of step 1."""
    P, C, foil, gp = sim.path, sim.circulation, sim.path["airfoil"], sim.path["airfoil_gamma_points"]
    new = [foil[0, :, -1] + np.array([0.5 * sim.Uinf * sim.dt, 0.0])]
    g_new = [C["TEV"][0]]
    if sim.LEV_shed[1] != -1:
        new.append(foil[1, :, 0])
        g_new.append(C["LEV"][0])
    new = np.array(new).T
    g = np.concatenate([np.asarray(C["FREE"], float), g_new])
    return (g, np.concatenate([P["FREE"][0, 0], new[0]]), np.concatenate([P["FREE"][0, 1], new[1]]), C["airfoil"][0], gp[1, 0],
            gp[1, 1])


def _sources_of(sim):
    return lambda i: first_step_sources(sim) if i == 1 else run_sources(sim, i)


def _check_by_value(sim, steps, what, pick=None):
    """The run's gradient sums (at the points `pick`) against the long-double terms over the run's own sources, added in step
    order; -> (reference sums, gmax, per-step terms)."""
    pick = np.arange(sim._survey_xz.shape[1]) if pick is None else pick
    pts = lambda i: tuple(c[pick] for c in sim._survey_points(i))       # noqa: E731
    ref, gmax, per = SG.reference_sums(steps, pts, _sources_of(sim), sim.v_core)
    assert sim.survey_count == len(steps)
    e_mean, e_sq = SG.sums_errors(sim.survey_grad_sums.reshape(5, -1)[:, pick], ref, len(steps), gmax)
    print(f"{what}: {len(steps)} steps, {len(pick)} points: means of ux, e, omega {e_mean:.2e} of max|grad u| ({gmax:.3f}); "
          f"means of omega^2, Q {e_sq:.2e} of max|grad u|^2")
    assert gmax > 0.0
    assert e_mean <= SG.MEAN_BOUND, e_mean
    assert e_sq <= SG.SQUARE_BOUND, e_sq
    return ref, gmax, per


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
    assert a.survey_count == b.survey_count and np.array_equal(a.survey_sums, b.survey_sums)
    assert np.array_equal(a.survey_uw, b.survey_uw)
    assert hasattr(a, "survey_bin_sums") == hasattr(b, "survey_bin_sums")
    if hasattr(a, "survey_bin_sums"):
        assert np.array_equal(a.survey_bin_count, b.survey_bin_count) and np.array_equal(a.survey_bin_sums, b.survey_bin_sums)
    assert np.array_equal(a.probe_u, b.probe_u) and np.array_equal(a.probe_w, b.probe_w)
    assert a.tracer_path.steps() == b.tracer_path.steps()
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s]), ("tracer_path", s)
    assert np.array_equal(a.tracer_last, b.tracer_last)


@pytest.mark.parametrize("bins", [False, True], ids=["plain", "binned"])
@pytest.mark.parametrize("case", ["f64_dense", "f32_sparse_overlapped"])
def test_the_gradient_sums_are_passive(eng, case, bins):
    """With and without survey_gradient on a survey of 600 points, probes and tracers set in both runs: the velocity sums, plain
    and binned, their counts, Cl / Cd / Cm, every circulation[...], LEV_shed, the history rows, the final resident wake, the probe
    rows and the tracer paths are the same arrays, bit for bit; and a later run without the flag on the same context enqueues
    the plain pair again."""
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
        grad = LUDVM(**kw, verbose=False, engine=eng, survey_gradient=True, **others, **extra)
        wake_grad = _final_wake(eng)
        again = LUDVM(**kw, verbose=False, engine=eng, **others, **extra)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "survey_grad_sums") and plain.survey_gradient is False
    _same_run(plain, grad)
    _same_run(plain, again)
    for a, b in zip(wake_plain, wake_grad):
        assert np.array_equal(a, b)
    assert grad.survey_grad_sums.shape == (5, 600) and np.isfinite(grad.survey_grad_sums).all()
    assert (grad.survey_grad_sums[3] > 0.0).all()                       # every point was written
    SG.check_derived(grad)
    if bins:
        assert grad.survey_bin_grad_sums.shape == (7, 5, 600) and (grad.survey_bin_grad_sums[:, 3] > 0.0).all()
        SG.check_bin_derived(grad)
        # every sampled step has a bin here: the bins' blocks add up to the plain sums to rounding
        tot = grad.survey_bin_grad_sums.sum(axis=0)
        assert np.abs(tot - grad.survey_grad_sums).max() <= 1e-12 * np.abs(grad.survey_grad_sums).max()
    else:
        assert not hasattr(grad, "survey_bin_grad_sums")


@pytest.mark.parametrize("case", ["A", "B"])
def test_by_value_over_the_runs_own_sources_at_many_source_tiles(eng, case):
    """Cases A and B of tests/observer_sources_common.py with the 600-point survey, 'f64', dense history: every sampled step's
    five terms from the long-double closed forms over tracers_common.run_sources(sim, i), added in step order.  Case A, all
    steps: five full splits of 256 sources, a sixth that stays empty through step 20 and holds one source from step 21.  Case
    B, window (12, 14, 1): 64 splits of 256 at step 12, 33 of 512 at step 13."""
    obs = OS.observers(case, "few")
    win = (1, OS.CASES[case][1] + 1, 1) if case == "A" else (12, 14, 1)
    sim = _ludvm()(**OS.case_keywords(case), verbose=False, engine=eng, precision="f64", history="full", survey=obs["survey"],
                   survey_steps=win, survey_gradient=True)
    assert sim.nt == OS.CASES[case][1] + 1 and (sim.LEV_shed[1:] == -1).all()
    steps = list(range(win[0], min(win[1], sim.nt), win[2]))
    assert len(steps) == (24 if case == "A" else 2)
    _check_by_value(sim, steps, f"case {case}")
    SG.check_derived(sim)


@pytest.mark.parametrize("K", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_point_counts_on_both_sides_of_the_tile(eng, K):
    """K survey points over 30 steps in 'f64', dense history, tunnel frame, every step sampled: one lane, one point short of a
    tile, a whole tile, a tile and one point, two tiles and one point -- by value."""
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="full", survey=seeds_random(K, seed=17),
                   survey_frame="tunnel", survey_gradient=True)
    assert sim.nt == 31 and sim.survey_grad_sums.shape == (5, K)
    _check_by_value(sim, list(range(1, 31)), f"K = {K}")
    assert (sim.survey_grad_sums[3] > 0.0).all()


@pytest.mark.parametrize("K", [1, TILE + 1])
@pytest.mark.parametrize("sym", [1, 64], ids=["serial", "overlapped"])
def test_a_bin_is_bit_identical_to_the_plain_gradient_survey_of_its_steps(eng, sym, K):
    """200 steps of config 1 in fp32, window (20, 190, 1), table (i - 20) % 3: bin b's gradient block is array_equal to the
    gradient sums of a plain survey with survey_steps = (20 + b, 190, 3), and so is its velocity block; the plain sums of the
    binned run are those of the run without bins."""
    kw = dict(CONFIG1, tf=10.0)
    pts = seeds_random(K)
    table = (np.arange(201) - 20) % 3
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=pts, survey_frame="tunnel", survey_gradient=True)
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


def test_the_sums_do_not_depend_on_the_chunking_or_on_a_resume_inside_the_window(eng, tmp_path):
    """All ten sums, plain and binned, bit for bit across _march_chunk = 32768 / 7 and a checkpoint after step 100 (inside the
    window) with a resume.  200 steps of config 1 in fp32 (overlapped: symmetric threshold 64), 600 points, window 20 .. 190
    every 3, five phase bins."""
    kw = dict(CONFIG1, tf=10.0)
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=seeds_random(600), survey_frame="tunnel",
                  survey_steps=(20, 190, 3), survey_bins=5, survey_period=4.3, survey_phase0=0.35, survey_gradient=True)
    eng.set_symmetric(64)
    try:
        base = _chunked(32768)(**kw, **common)
        assert base.nt == 201 and base.survey_count == 57 == base.survey_bin_count.sum()
        runs = {"chunk 7": _chunked(7)(**kw, **common)}
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, checkpoint_every=100, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 101 and R["survey_grad_sums"].shape == (5, 600)
        assert R["survey_bin_grad_sums"].shape == (5, 5, 600) and int(R["survey_samples"]) == 27
        assert (R["survey_grad_sums"][3] > 0.0).all() and not np.array_equal(R["survey_grad_sums"], base.survey_grad_sums)
        runs["resumed from 100"] = _ludvm().resume(ck, engine=eng, verbose=False)
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert r.survey_count == base.survey_count and np.array_equal(r.survey_bin_count, base.survey_bin_count), name
        assert np.array_equal(r.survey_sums, base.survey_sums) and np.array_equal(r.survey_bin_sums, base.survey_bin_sums), name
        assert np.array_equal(r.survey_grad_sums, base.survey_grad_sums), name
        assert np.array_equal(r.survey_bin_grad_sums, base.survey_bin_grad_sums), name
        assert np.array_equal(r.Cl, base.Cl), name
    assert (base.survey_bin_count > 0).all()


def test_marched_and_per_step_sums_agree(eng):
    """march=True (field_grad_f64) and march=False (pair_grad_f64 through Engine.gradient_field) in 'f64', steps 1-10, four bins,
    dense history: both against the long-double terms over the run's own sources and against each other, at the bounds of the
    by-value tests."""
    kw = dict(CONFIG1, tf=1.0)
    pts = probes32()
    common = dict(verbose=False, engine=eng, precision="f64", history="full", survey=pts, survey_frame="tunnel", survey_steps=(1, 11, 1),
                  survey_bins=4, survey_period=0.3, survey_gradient=True)
    a = _ludvm()(**kw, **common, march=True)
    b = _ludvm()(**kw, **common, march=False)
    steps = list(range(1, 11))
    _, gmax, per = _check_by_value(a, steps, "marched")
    _check_by_value(b, steps, "per-step")
    e_mean, e_sq = SG.sums_errors(a.survey_grad_sums, b.survey_grad_sums, 10, gmax)
    print(f"marched vs per-step: means {e_mean:.2e} of max|grad u|, squares {e_sq:.2e} of max|grad u|^2")
    assert e_mean <= SG.MEAN_BOUND and e_sq <= SG.SQUARE_BOUND
    assert np.array_equal(a.survey_bin_count, b.survey_bin_count) and a.survey_bin_count.sum() == 10 and (a.survey_bin_count > 0).all()
    for k in range(4):
        W = [i for i in steps if a.survey_bin_of_step[i] == k]
        ref = sum(per[i] for i in W)
        for sim in (a, b):
            e = SG.sums_errors(sim.survey_bin_grad_sums[k], ref, len(W), gmax)
            assert e[0] <= SG.MEAN_BOUND and e[1] <= SG.SQUARE_BOUND, (k, e)


def _ratios(mean_u, mean_w, ux, uz, wx, h1, h2, n):
    """Error ratios of the centred differences at h1 and h2 = h1 / 2 for ux, uz, wx at n centres.  Point layout: centre c at
    index c, then for each h the blocks x + h, x - h, z + h, z - h of n points each."""
    out = []
    for k, h in enumerate((h1, h2)):
        o = n + 4 * n * k
        xp, xm, zp, zm = (slice(o + j * n, o + (j + 1) * n) for j in range(4))
        c = slice(0, n)
        out.append(np.stack([np.abs((mean_u[xp] - mean_u[xm]) / (2 * h) - ux[c]), np.abs((mean_u[zp] - mean_u[zm]) / (2 * h) - uz[c]),
                             np.abs((mean_w[xp] - mean_w[xm]) / (2 * h) - wx[c])]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return out[0] / out[1]


def test_centred_differences_of_the_mean_velocity_converge_to_the_mean_gradient(eng):
    """Independent of the restated closed forms: a survey of point stencils x +- h, z +- h around 48 centres with h = v_core / 8
    and v_core / 16.  The mean is linear, so centred differences of survey_mean_u / _w converge to survey_mean_ux / _uz / _wx
    at second order: the error falls by about 4 per halving.  The ratio is asserted in [3.8, 4.2] for every (centre,
    component) at which the CPU reference -- the oracle's velocity and tests/gradient_common.py's gradient over the run's own
    sources, every centre at least 2 v_core from every source -- gives a ratio in [3.85, 4.15]: chosen by the reference, never
    by the code under test."""
    kw = dict(CONFIG1, tf=1.5)
    probe = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", run=False)
    vc = probe.v_core
    h1, h2 = vc / 8, vc / 16
    rng = np.random.default_rng(41)
    n = 48
    cx, cz = rng.uniform(-1.2, 1.0, n), 1.0 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.3, 0.6, n)
    xs, zs = [cx], [cz]
    for h in (h1, h2):
        xs += [cx + h, cx - h, cx, cx]
        zs += [cz, cz, cz + h, cz - h]
    pts = np.stack([np.concatenate(xs), np.concatenate(zs)])
    steps = list(range(20, 30, 3))
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="full", survey=pts, survey_steps=(20, 30, 3),
                   survey_gradient=True)
    assert sim.survey_count == len(steps) == 4
    # the CPU reference at the same points over the run's own sources
    mu, mw, g3, far = np.zeros(pts.shape[1]), np.zeros(pts.shape[1]), np.zeros([3, n]), np.full(n, np.inf)
    for i in steps:
        g, x, z = SG.all_sources(run_sources(sim, i))
        u, w = O.induced_velocity(g, x, z, pts[0], pts[1], vc)
        mu, mw = mu + u / 4, mw + w / 4
        vals, _ = GC.reference(g, x, z, cx, cz, vc)
        g3 += np.stack(vals) / 4
        far = np.minimum(far, np.hypot(cx[:, None] - x[None], cz[:, None] - z[None]).min(axis=1))
    ref_ratio = _ratios(mu, mw, g3[0], g3[1], g3[2], h1, h2, n)
    ok = (ref_ratio >= 3.85) & (ref_ratio <= 4.15) & (far >= 2 * vc)[None]
    got = _ratios(sim.survey_mean_u, sim.survey_mean_w, sim.survey_mean_ux[:n], sim.survey_mean_uz[:n], sim.survey_mean_wx[:n], h1, h2, n)
    print(f"{int(ok.sum())} of {3 * n} (centre, component) pairs chosen by the reference; ratios on the device "
          f"{got[ok].min():.3f} .. {got[ok].max():.3f} (reference {ref_ratio[ok].min():.3f} .. {ref_ratio[ok].max():.3f})")
    assert ok.sum() >= n                    # (most of them: the stencils are fine against the distance to the sources)
    assert ((got[ok] >= 3.8) & (got[ok] <= 4.2)).all(), (got[ok].min(), got[ok].max())


def test_the_largest_survey(eng):
    """K = 1 048 576 points, the last two steps of the README case (LUDVM() with its default arguments: 800 steps and one), dense history:
    1024 sampled points (observer_sources_common.survey_sample: the ends of every tile among them) by value, every point
    written."""
    rng = np.random.default_rng(23)
    pts = np.stack([rng.uniform(-1.0, 13.0, LIMIT), rng.uniform(-1.0, 3.0, LIMIT)])
    # (observer_sources_common.survey_sample takes both ends of EVERY tile: 4096 points here, over its 1024.  The same idea
    # within 1024: both ends of the first and the last tile and of 254 tiles drawn, the other 512 points drawn)
    tiles = np.concatenate([[0, LIMIT // TILE - 1], rng.choice(np.arange(1, LIMIT // TILE - 1), 254, replace=False)])
    pick = np.unique(np.concatenate([tiles * TILE, tiles * TILE + TILE - 1, rng.choice(LIMIT, 512, replace=False)]))
    assert 1000 <= len(pick) <= 1024 and pick[0] == 0 and pick[-1] == LIMIT - 1
    nt = _ludvm()(verbose=False, engine=eng, run=False).nt
    assert nt > 800
    sim = _ludvm()(verbose=False, engine=eng, history="full", survey=pts, survey_frame="tunnel", survey_steps=(nt - 2, nt, 1),
                   survey_gradient=True)
    assert sim.nt == nt and sim.survey_count == 2 and sim.survey_grad_sums.shape == (5, LIMIT)
    _check_by_value(sim, [nt - 2, nt - 1], f"K = {LIMIT}", pick=pick)
    assert np.isfinite(sim.survey_grad_sums).all() and (sim.survey_grad_sums[3] > 0.0).all()


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
    # LUDVM_E_STATE without a survey, and on read while the gradient sums are off
    _prepared(eng)
    assert _code_of(lambda: eng.march_set_survey_gradient(True)) == _ffi.E_STATE
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    # bin sums without bins, or without the plain sums: LUDVM_E_ARG
    assert _code_of(lambda: eng.march_set_survey_gradient(True, gsums=np.zeros([5, 5]), bin_gsums=np.zeros([2, 5, 5]))) == _ffi.E_ARG
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_bins(table, 2)
    assert _code_of(lambda: eng.march_set_survey_gradient(True, bin_gsums=np.zeros([2, 5, 5]))) == _ffi.E_ARG
    assert _code_of(lambda: eng.march_set_survey_gradient(2)) == _ffi.E_ARG
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    # an fp32 survey carries none, and the gradient sums refuse fp32 while they are on
    eng.march_set_survey_precision("f32")
    assert _code_of(lambda: eng.march_set_survey_gradient(True)) == _ffi.E_STATE
    eng.march_set_survey_precision("f64")
    eng.march_set_survey_gradient(True)
    g0, bg0 = eng.march_survey_gradient()                               # valid before any step: zeros
    assert g0.shape == (5, 5) and bg0.shape == (2, 5, 5) and not g0.any() and not bg0.any()
    assert _code_of(lambda: eng.march_set_survey_precision("f32")) == _ffi.E_STATE
    sim._march_call(S, 1, 7, False, 50)                                 # steps 1 .. 6: samples at 2 (bin 1), 4 (bin 0), 6 (none)
    g6, bg6 = eng.march_survey_gradient()
    sums6, m6 = eng.march_survey()
    assert m6 == 3 and (g6[3] > 0.0).all() and (bg6[:, 3] > 0.0).all()
    # (the survey still runs in float64: the refused precision changed nothing)
    plain, Sp = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table)
    plain._march_call(Sp, 1, 7, False, 50)
    assert np.array_equal(eng.march_survey()[0], sums6)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE          # (ludvm_march_setup reset it)
    # samples without sums: LUDVM_E_STATE; values that are not finite: LUDVM_E_ARG; a refused call changes nothing
    assert _code_of(lambda: eng.march_set_survey_gradient(True)) == _ffi.E_STATE
    eng.march_set_survey_gradient(True, gsums=g6, bin_gsums=bg6)
    bad_g, bad_bg = g6.copy(), bg6.copy()
    bad_g[2, 1], bad_bg[1, 4, 0] = np.nan, np.inf
    for bad in (lambda: eng.march_set_survey_gradient(True, gsums=bad_g, bin_gsums=bg6),
                lambda: eng.march_set_survey_gradient(True, gsums=g6, bin_gsums=bad_bg),
                lambda: eng.march_set_survey_gradient(True, bin_gsums=bg6),
                lambda: eng.march_set_survey_gradient(-1)):
        assert _code_of(bad) == _ffi.E_ARG
        g, bg = eng.march_survey_gradient()
        assert np.array_equal(g, g6) and np.array_equal(bg, bg6)
    assert _code_of(lambda: eng.march_set_survey_gradient(True)) == _ffi.E_STATE
    assert np.array_equal(eng.march_survey_gradient()[0], g6)
    with pytest.raises(ValueError):
        eng.march_set_survey_gradient(True, gsums=g6[:, :3])
    # carried over, the sums continue with the uninterrupted run's bits
    plain._march_call(Sp, 7, 13, False, 50)                             # steps 7 .. 12: samples at 8 (bin 1), 10 (bin 0), 12 (none)
    g12, bg12 = eng.march_survey_gradient()
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_bins=table, survey_gradient=True)
    whole._march_call(Sw, 1, 13, False, 50)
    gw, bgw = eng.march_survey_gradient()
    assert eng.march_survey()[1] == 6 and np.array_equal(g12, gw) and np.array_equal(bg12, bgw)
    # on = 0 removes it; ludvm_march_set_survey_bins and ludvm_march_set_survey reset it
    eng.march_set_survey_gradient(False)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_gradient(True, gsums=gw, bin_gsums=bgw)
    sb, nb = eng.march_survey_bins()
    eng.march_set_survey_bins(table, 2, sums=sb, counts=nb)
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_gradient(True, gsums=gw, bin_gsums=bgw)
    eng.march_set_survey(pts[0], pts[1])
    assert _code_of(eng.march_survey_gradient) == _ffi.E_STATE
    eng.march_set_survey_gradient(True)                                 # a fresh survey: no samples, sums from zero
    g, bg = eng.march_survey_gradient()
    assert not g.any() and bg is None
