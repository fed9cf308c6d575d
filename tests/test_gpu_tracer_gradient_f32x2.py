"""GPU tier: the tracers' deformation gradient in hi+lo fp32 (march_f32x2_grad_tracer_partial / march_grad_tracer_finish,
ludvm_march_set_tracer_gradient_f32x2; LUDVM(..., tracers=, tracer_precision='f32x2', tracer_gradient='f32x2'); DESIGN.md section
4.18) -- every recorded step by value against F_i = (I + dt G_i(start)) F_{i-1} over the sources the run itself names, the
release step against the np.longdouble gradient, passive on the plain hi+lo tracers' positions and on every other result,
independent of how a run is cut into calls, on both sides of every tile boundary, far from the origin with a small core, and the
codes of the entry point.

The tolerance is derived (tests/tracer_gradient_f32x2_common.py): component by component dt b (|F| + |F|) of the row before, b =
gradient_f32x2_common.bound at the start position, plus 1e-9 of max|F|; every by-value test asserts that it is below 1e-2 of the
largest single increment max|dt G F| of the checked steps -- a wake one step late is off by per cents of an increment."""
import signal

import numpy as np
import pytest

import gradient_f32x2_common as GF
import tracer_gradient_common as TG
import tracer_gradient_f32x2_common as C
from conftest import CONFIG1
from probes_common import probes32
from survey_f32_common import far_sheet, points_around
from test_gpu_tracer_gradient import first_step_sources
from tracers_common import releases_by_tile, run_sources, seeds37, seeds_random

pytestmark = pytest.mark.gpu

PLAN_TILE = 1024    # kTracerF32Tile of march_kernels.hpp: the tile of the launch plan (and of releases_by_tile here)
GROUP = 512         # kTracerGradF32Tile: the tracers of one workgroup of the fused kernel
F32 = dict(tracer_precision="f32x2", tracer_gradient="f32x2")


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
    class Chunked(_ludvm()):
        _march_chunk = chunk
    return Chunked


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


def _sources_of(sim):
    return lambda i: first_step_sources(sim) if i == 1 else run_sources(sim, i)


def test_the_tiles_are_what_the_tests_assume():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    per_lane = {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kTracerF32PerLane", "kTracerGradF32PerLane")}
    assert 256 * per_lane["kTracerF32PerLane"] == PLAN_TILE and 256 * per_lane["kTracerGradF32PerLane"] == GROUP


@pytest.mark.parametrize("case", ["f64_steps_2_50", "f32_overlapped_steps_70_200"])
def test_every_step_by_value_over_the_sources_of_its_own_roll_up(eng, case):
    """Dense history, every step recorded, 37 tracers.  'f64' over steps 2-50 (releases at 1, 7, 30); the overlapped fp32 run
    (symmetric threshold 64, probes set) over steps 70-200, where the sources pass 256 and 512 and the plan has more than one
    split."""
    seeds = seeds37()
    if case == "f64_steps_2_50":
        rel = np.array([1, 7, 30], dtype=np.int64)[np.arange(37) % 3]
        sim = _ludvm()(**dict(CONFIG1, tf=2.5), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                       tracer_release=rel, tracer_frame="tunnel", **F32)
        steps = range(2, 51)
    else:
        rel = np.array([1, 90, 150], dtype=np.int64)[np.arange(37) % 3]
        eng.set_symmetric(64)
        try:
            sim = _ludvm()(**CONFIG1, verbose=False, engine=eng, precision="f32", history="full", tracers=seeds, tracer_release=rel,
                           tracer_frame="tunnel", probes=probes32(), **F32)
        finally:
            eng.set_symmetric(1)
        steps = range(70, 201)
        ns = [len(run_sources(sim, s)[0]) + 80 for s in (70, 200)]
        print(f"sources of step 70: {ns[0]}, of step 200: {ns[1]}")
        assert ns[0] < 256 < ns[1]                          # (one source tile and split at first, several later)
    assert sim.tracer_gradient == "f32x2" and sim.tracer_precision == "f32x2"
    assert sim.tracer_F_path.steps() == sim.tracer_path.steps() == list(range(sim.nt))
    assert np.array_equal(sim.tracer_F_path[0], TG.identity(37))
    C.assert_rows(sim, rel, steps, _sources_of(sim), case)
    last = sim.nt - 1
    assert np.array_equal(sim.tracer_F_last, sim.tracer_F_path[last])
    ftle = sim.tracer_ftle()
    s = np.linalg.svd(np.moveaxis(sim.tracer_F_last.reshape(2, 2, -1), -1, 0), compute_uv=False)[:, 0]
    assert np.allclose(ftle, np.log(s) / (sim.dt * (last - rel + 1.0)), rtol=1e-12, atol=1e-13)
    early = sim.tracer_ftle(step=int(rel.max()) - 1)
    assert np.isnan(early[rel == rel.max()]).all() and np.isfinite(early[rel < rel.max()]).all()


def test_the_release_step_is_the_gradient_at_the_seed(eng):
    """At a tracer's release step r, (F - I) / dt is G at the seed: against the np.longdouble gradient over the sources of step r
    within gradient_f32x2_common's bound (+ the float64 rounding of I + dt G, 2^-52 (1 + dt |G|) / dt), r = 5 and r = 30, lab
    frame, 'f64', dense history.  `gradient_field(..., precision='f32x2')` at the same seeds against the same reference within
    the same bound: the marched kernel and the direct one each, not against each other (their source splits differ)."""
    seeds = seeds37()
    rel = np.array([5, 30], dtype=np.int64)[np.arange(37) % 2]
    sim = _ludvm()(**dict(CONFIG1, tf=2.0), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                   tracer_release=rel, **F32)
    for r in (5, 30):
        m = rel == r
        I = TG.identity(int(m.sum()))
        assert np.array_equal(sim.tracer_F_path[r - 1][:, m], I)
        gw, xs, zs, gf, xf, zf = run_sources(sim, r)
        g, x, z = np.concatenate([gw, gf]), np.concatenate([xs, xf]), np.concatenate([zs, zf])
        (ux, uz, wx), bound = GF.gradient_reference(g, x, z, seeds[0, m], seeds[1, m], sim.v_core)
        got = (sim.tracer_F_path[r][:, m] - I) / sim.dt
        scale = max(np.abs(ux).max(), np.abs(uz).max(), np.abs(wx).max())
        worst = 0.0
        for k, ref in enumerate((ux, uz, wx, -ux)):
            tol = bound + GF.EPS64 * (1.0 + sim.dt * np.abs(ref)) / sim.dt
            worst = max(worst, float((np.abs(got[k] - ref) / tol).max()))
        direct = eng.gradient_field(g, x, z, seeds[0, m], seeds[1, m], sim.v_core, precision="f32x2")
        dworst = max(float((np.abs(d - ref) / bound).max()) for d, ref in zip(direct, (ux, uz, wx)))
        print(f"release step {r}: (F - I) / dt vs the long double gradient at the seeds: {worst:.3f} of the bound; gradient_field "
              f"'f32x2': {dworst:.3f} of the bound (max|G| {scale:.3f}, largest bound {bound.max() / scale:.2e} of it)")
        assert 0.0 < worst <= 1.0 and dworst <= 1.0, (r, worst, dworst)


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
    assert a.tracer_path.steps() == b.tracer_path.steps()
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s]), ("tracer_path", s)
    assert np.array_equal(a.tracer_last, b.tracer_last)
    assert np.array_equal(a.probe_u, b.probe_u) and np.array_equal(a.probe_w, b.probe_w)


@pytest.mark.parametrize("case", ["f64_dense", "f32_sparse_overlapped"])
def test_the_gradient_is_passive_on_the_plain_f32x2_tracers(eng, case):
    """Three runs on one engine -- tracer_precision='f32x2' alone, with tracer_gradient='f32x2' added, plain again -- with 600 tracers
    released at 1, 40, 130 and never, and probes: `tracer_path` at every recorded step (every step in the dense case),
    `tracer_last`, Cl / Cd / Cm, every circulation[...], LEV_shed, the history rows, the final wake and the probe rows are the
    same arrays, bit for bit."""
    LUDVM = _ludvm()
    kw = dict(CONFIG1, tf=10.0)
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101])}[case]
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    common = dict(verbose=False, engine=eng, probes=probes32(), probe_frame="tunnel", tracers=seeds, tracer_release=rel,
                  tracer_frame="tunnel", tracer_precision="f32x2", **extra)
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**kw, **common)
        wake_plain = _final_wake(eng)
        grad = LUDVM(**kw, **common, tracer_gradient="f32x2")
        wake_grad = _final_wake(eng)
        again = LUDVM(**kw, **common)                       # (and a context that carried the gradient enqueues the plain kernel again)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "tracer_F_path") and plain.tracer_gradient is False and grad.tracer_gradient == "f32x2"
    if case == "f64_dense":
        assert grad.tracer_path.steps() == list(range(grad.nt))
    _same_run(plain, grad)
    _same_run(plain, again)
    for a, b in zip(wake_plain, wake_grad):
        assert np.array_equal(a, b)
    last = grad.nt - 1
    assert grad.tracer_F_path.steps() == grad.tracer_path.steps()
    F = grad.tracer_F_path[last]
    assert np.isfinite(F).all() and np.array_equal(F[:, rel > last], TG.identity(int((rel > last).sum())))
    assert np.abs(F[:, rel <= 130] - TG.identity(int((rel <= 130).sum()))).max(axis=0).min() > 0.0


def test_F_does_not_depend_on_the_chunking_or_on_a_resume_between_two_releases(eng, tmp_path):
    """The same F bits and positions across _march_chunk = 32768 / 7, dense or sparse history, the cap on one call's recorded rows
    (48 bytes per tracer and row), run to run, and across a checkpoint at step 100 -- between the releases at 40 and 130 -- with a
    resume, which continues on the route the file names.  200 steps of config 1 in fp32 (overlapped: symmetric threshold 64),
    600 tracers released at 1, 40, 130 and never."""
    import json
    kw = dict(CONFIG1, tf=10.0)
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    keep = [1, 39, 40, 41, 64, 128, 129, 130, 131, 192, 200]
    common = dict(verbose=False, engine=eng, precision="f32", tracers=seeds, tracer_release=rel, tracer_frame="tunnel",
                  tracer_steps=keep, **F32)
    calls = []

    class Capped(_ludvm()):
        _tracer_call_bytes = 48 * 600 * 2           # two recorded rows per call

        def _march_stretch(self, S, i, j, place, record=False):
            calls.append(int(np.count_nonzero((S.trec >= i) & (S.trec < j))))
            return super()._march_stretch(S, i, j, place, record=record)
    eng.set_symmetric(64)
    try:
        base = _chunked(32768)(**kw, **common, history="sparse")
        assert base.nt == 201 and base.tracer_F_path.steps() == [0] + keep
        runs = {
            "again": _chunked(32768)(**kw, **common, history="sparse"),
            "chunk 7": _chunked(7)(**kw, **common, history="sparse"),
            "dense": _ludvm()(**kw, **common, history="full"),
            "two rows per call": Capped(**kw, **common, history="sparse"),
        }
        assert max(calls) == 2 and sum(calls) == len(keep)
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, history="sparse", checkpoint_every=100, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 101 and R["tracer_F_cur"].shape == (4, 600)
        assert list(R["tracer_rows_steps"]) == [0] + keep[:5] and R["tracer_F_rows"].shape == (6, 4, 600)
        assert np.array_equal(R["tracer_F_cur"][:, rel > 100], TG.identity(int((rel > 100).sum())))
        ctor = json.loads(str(R["ctor"]))
        assert ctor["tracer_gradient"] == "f32x2" and ctor["tracer_precision"] == "f32x2"
        runs["resumed from 100"] = _ludvm().resume(ck, engine=eng, verbose=False)
        assert runs["resumed from 100"].tracer_gradient == "f32x2"
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert r.tracer_F_path.steps() == base.tracer_F_path.steps(), name
        for s in base.tracer_F_path.steps():
            assert np.array_equal(r.tracer_F_path[s], base.tracer_F_path[s]), (name, s)
            assert np.array_equal(r.tracer_path[s], base.tracer_path[s]), (name, s)
        assert np.array_equal(r.tracer_F_last, base.tracer_F_last) and np.array_equal(r.Cl, base.Cl), name
    assert np.array_equal(base.tracer_F_last, base.tracer_F_path[200])
    assert np.abs(base.tracer_F_last[:, rel <= 130] - TG.identity(int((rel <= 130).sum()))).max(axis=0).min() > 0.0


@pytest.mark.parametrize("M", [1, 255, 256, 257, GROUP - 1, GROUP, GROUP + 1, 1023, 1024, 1025, 2049])
def test_tracer_counts_on_both_sides_of_every_tile_boundary(eng, M):
    """M tracers over 30 steps in 'f64', dense history: every row within the tolerance; one lane, the second register set of a lane
    (256 / 257), one workgroup of the fused kernel and the next (511 / 512 / 513), one tile of the plan and the next (1023 / 1024 /
    1025), two tiles and one tracer.  Releases by tile of 1024: tile 0 free from step 1, tile 1 mixed (step 1, step 5, never: lane
    by lane), tile 2 wholly held.  A tracer not yet released keeps F exactly the identity at every step and has no exponent."""
    seeds = seeds_random(M, seed=17)
    rel = releases_by_tile(M, PLAN_TILE)
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                   tracer_release=rel, tracer_frame="tunnel", **F32)
    assert sim.nt == 31 and sim.tracer_F_path.steps() == list(range(31)) and sim.tracer_F_path[30].shape == (4, M)
    C.assert_rows(sim, rel, range(1, 31), _sources_of(sim), f"M = {M}")
    held = rel > 30
    for s in range(31):
        still = rel > s
        assert np.array_equal(sim.tracer_F_path[s][:, still], TG.identity(int(still.sum()))), s
    ftle = sim.tracer_ftle()
    assert np.array_equal(np.isnan(ftle), held)
    assert np.isnan(sim.tracer_ftle(step=4)[rel > 4]).all()
    if M > 2 * PLAN_TILE:
        assert held[2 * PLAN_TILE:].all() and not held[:PLAN_TILE].any()
    assert np.array_equal(sim.tracer_F_last, sim.tracer_F_path[30])


@pytest.mark.parametrize("x0", [-55.0, -5000.0])
def test_far_from_the_origin_with_a_small_core(eng, x0):
    """A 600-vortex sheet 1e-3 apart at x = x0 as free vortices, v_core = 1.3e-3 (dt = 1e-3): 600 tracers on the vortices, within
    one core of them and chords away, released at steps 1 and 3; rows 1 .. 8 within the tolerance -- the same one at x0 = -55 and
    at x0 = -5000: the bound knows nothing of the offset."""
    g, x, z = far_sheet(x0=x0)
    seeds = points_around(x, z, 1.3e-3)[:, ::3]
    M = seeds.shape[1]
    rel = np.array([1, 3], dtype=np.int64)[np.arange(M) % 2]
    sim = _ludvm()(**dict(CONFIG1, dt=1e-3, tf=8e-3, circulation_freevort=g, xy_freevort=np.stack([x, z])), verbose=False, engine=eng,
                   precision="f64", history="full", tracers=seeds, tracer_release=rel, **F32)
    assert abs(sim.v_core - 1.3e-3) < 1e-15 and sim.nt >= 9
    C.assert_rows(sim, rel, range(1, 9), _sources_of(sim), f"sheet at {x0}")


def _prepared(eng, **extra):
    """A 20-step 'f64' run set up for the march (ludvm_march_setup and, with tracers, ludvm_march_set_tracers done, no step run)."""
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
    from ludvm_amd import Engine, _ffi
    seeds = seeds37()[:, :5]
    trc = dict(tracers=seeds, tracer_release=np.array([1, 1, 3, 3, 99], dtype=np.int64), tracer_steps=[6, 12])
    fresh = Engine(0)
    try:
        fresh._march_ntracers = 5
        assert _code_of(fresh.march_set_tracer_gradient_f32x2) == _ffi.E_STATE            # (before ludvm_march_setup)
    finally:
        fresh.close()
    _prepared(eng)
    assert _code_of(eng.march_set_tracer_gradient_f32x2) == _ffi.E_STATE                  # (no tracers are set)
    # the plain hi+lo run of steps 1 .. 12, for its positions
    plain, Sp = _prepared(eng, **trc, tracer_precision="f32x2")
    plain._march_call(Sp, 1, 13, False, 50)
    state_plain = eng.march_tracer_state()
    # the new route through the class: the identity before any step
    sim, S = _prepared(eng, **trc, **F32)
    assert np.array_equal(eng.march_tracer_gradient_state(), TG.identity(5))
    sim._march_call(S, 1, 7, False, 50)
    state = eng.march_tracer_gradient_state()
    assert np.array_equal(state[:, 4], TG.identity(1)[:, 0]) and np.abs(state[:, :4] - TG.identity(4)).max(axis=0).min() > 0.0
    assert np.array_equal(state, sim.tracer_F_path[6])
    # an F that is not finite: E_ARG and nothing changes; not [4, M]: ValueError from the wrapper
    bad_F = state.copy()
    bad_F[2, 1] = np.nan
    for bad in (bad_F, np.where(np.isnan(bad_F), np.inf, bad_F)):
        assert _code_of(lambda: eng.march_set_tracer_gradient_f32x2(F=bad)) == _ffi.E_ARG
        assert np.array_equal(eng.march_tracer_gradient_state(), state)
    with pytest.raises(ValueError):
        eng.march_set_tracer_gradient_f32x2(F=state[:, :4])
    # the precision setter is refused for either value while the route is on, and changes nothing
    for prec in ("f64", "f32x2"):
        assert _code_of(lambda: eng.march_set_tracer_precision(prec)) == _ffi.E_STATE
        assert np.array_equal(eng.march_tracer_gradient_state(), state)
    assert _code_of(lambda: eng.march_set_tracer_gradient(True)) == _ffi.E_STATE          # (the float64 gradient needs float64 tracers)
    assert np.array_equal(eng.march_tracer_gradient_state(), state)
    sim._march_call(S, 7, 13, False, 50)
    assert np.array_equal(eng.march_tracer_state(), state_plain)                          # (the plain hi+lo tracers' positions)
    F12 = eng.march_tracer_gradient_state()
    assert np.array_equal(F12, sim.tracer_F_path[12]) and not np.array_equal(F12, state)
    # a given F is the state
    eng.march_set_tracer_gradient_f32x2(F=state)
    assert np.array_equal(eng.march_tracer_gradient_state(), state)
    # switched off by the older setter: plain hi+lo tracers are left, and the next run's positions are the plain route's
    off, So = _prepared(eng, **trc, **F32)
    off._march_call(So, 1, 7, False, 50)
    eng.march_set_tracer_gradient(False)
    assert _code_of(eng.march_tracer_gradient_state) == _ffi.E_STATE
    off.tracer_gradient = False                                                           # (the object reads no F rows either)
    off._march_call(So, 7, 13, False, 50)
    assert np.array_equal(eng.march_tracer_state(), state_plain)
    eng.march_set_tracer_precision("f32x2")                                               # (no longer refused)
    # from plain float64 tracers and from plain hi+lo tracers the entry switches both on
    for before in ({}, dict(tracer_precision="f32x2")):
        two, S2 = _prepared(eng, **trc, **before)
        eng.march_set_tracer_gradient_f32x2()
        two._march_call(S2, 1, 13, False, 50)
        assert np.array_equal(eng.march_tracer_state(), state_plain) and np.array_equal(eng.march_tracer_gradient_state(), F12)
    # ludvm_march_set_tracers resets everything (float64 tracers, no gradient), and so does ludvm_march_setup
    eng.march_set_tracers(seeds[0], seeds[1])
    assert _code_of(eng.march_tracer_gradient_state) == _ffi.E_STATE
    eng.march_set_tracer_gradient(True)                                                   # (float64 tracers: accepted)
    eng.march_set_tracer_gradient(False)
    eng.march_set_tracer_gradient_f32x2()
    eng.march_setup(two.Npoints - 1, two.Ncoeffs, *two._march_inputs(S2))
    assert _code_of(eng.march_tracer_gradient_state) == _ffi.E_STATE
    assert _code_of(eng.march_set_tracer_gradient_f32x2) == _ffi.E_STATE
