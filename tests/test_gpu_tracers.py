"""GPU tier: passive tracers advected inside the device-resident march (march_tracer_partial / march_tracer_finish,
ludvm_march_set_tracers / ludvm_march_read_tracers / ludvm_march_tracer_state) -- against the oracle, against the class's own
zero-circulation free vortices, against the probes, passive on every other result, independent of how a run is cut into
calls, on both sides of every tile boundary, and the codes of the three entry points."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from probes_common import probes32
from tracers_common import (TracedOracle, euler_step, gust_cloud, path_error, releases_1_7_50, releases_by_tile, run_sources,
                            seeds37, seeds_random)

pytestmark = pytest.mark.gpu

TILE = 512          # kTracerTile of march_kernels.hpp: 256 lanes x 2 tracers

# Marched 'f64' run against TracedOracle over steps 1-200 [MI355X]: the wake is no longer the oracle's to the bit there (the
# device solves with other summation orders; a rounding difference grows about 10x per 12 steps).
# Measured on the first GPU run: 2.42e-11 of the largest displacement (steps 1-50 of the same run: 2.5e-16).  Bound: 10x the
# measured maximum, never above 1e-7 of the largest displacement.
STEPS_1_200_MEASURED = 2.42e-11
STEPS_1_200_BOUND = 10 * STEPS_1_200_MEASURED
assert STEPS_1_200_BOUND <= 1e-7


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
    class Chunked(_ludvm()):
        _march_chunk = chunk
    return Chunked


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


@pytest.fixture(scope="module")
def oracle50():
    """TracedOracle over 50 steps per (method, frame): 37 seeds around the foil released at steps 1, 7 and 50."""
    made = {}

    def get(method, frame):
        if (method, frame) not in made:
            shift = (lambda o: o.xpiv) if frame == "tunnel" else None
            made[method, frame] = TracedOracle(seeds37(), release=releases_1_7_50(37), shift=shift, **dict(CONFIG1, tf=2.5, method=method))
        return made[method, frame]
    return get


@pytest.mark.parametrize("method", ["Faure", "Ramesh"])
@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_marched_paths_match_the_oracle(eng, oracle50, method, frame):
    """Check 2 of the CPU tier through the real march in 'f64', dense and sparse history: steps 1-50 at 1e-9 of the largest
    displacement; held tracers sit exactly on the seed of their step."""
    kw = dict(CONFIG1, tf=2.5, method=method)
    seeds, rel = seeds37(), releases_1_7_50(37)
    ref = oracle50(method, frame)
    for hist in ("full", "sparse"):
        sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history=hist, tracers=seeds, tracer_release=rel,
                       tracer_frame=frame, tracer_steps=range(51))
        assert sim.tracer_path.steps() == list(range(51))
        err = path_error(sim.tracer_path, ref, 1, 50)
        print(f"{method} {frame} ({hist}): marched tracer paths vs oracle, steps 1-50: {err:.2e} of the largest displacement")
        assert err <= 1e-9, (hist, err)
        assert np.array_equal(sim.tracer_path[0], ref.seeds_at(0)) and np.array_equal(sim.tracer_last, sim.tracer_path[50])
        for s in (1, 6, 7, 49):
            still = rel > s
            assert np.array_equal(sim.tracer_path[s][:, still], ref.seeds_at(s)[:, still]), s
    # the default of a sparse run: snapshot_steps and the last step
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="sparse", snapshot_steps=[7, 8, 30], tracers=seeds,
                   tracer_release=rel, tracer_frame=frame)
    assert sim.tracer_path.steps() == [0, 7, 8, 30, 50]
    assert path_error(sim.tracer_path, ref, 1, 50) <= 1e-9


def test_marched_paths_match_the_oracle_up_to_step_200(eng):
    """200 steps in 'f64' against TracedOracle: STEPS_1_200_BOUND (measured 2.42e-11 on the first GPU run; bound 2.42e-10 of the
    largest displacement)."""
    kw = dict(CONFIG1, tf=10.0)
    seeds, rel = seeds37(), np.array([1, 7, 120], dtype=np.int64)[np.arange(37) % 3]
    ref = TracedOracle(seeds, release=rel, shift=lambda o: o.xpiv, **kw)
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", tracers=seeds, tracer_release=rel, tracer_frame="tunnel")
    e50, e200 = path_error(sim.tracer_path, ref, 1, 50), path_error(sim.tracer_path, ref, 1, 200)
    print(f"marched tracer paths vs oracle: steps 1-50 {e50:.2e}, steps 1-200 {e200:.2e} of the largest displacement")
    assert e50 <= 1e-9, e50
    assert e200 <= STEPS_1_200_BOUND, e200


def test_overlapped_steps_advect_by_the_sources_of_their_own_roll_up(eng):
    """Overlapped steps (fp32, symmetric threshold lowered to 64: the tracer launch rides the second stream behind the solve
    and the probes, beside the symmetric kernel) checked by VALUE, as the probes' are: with the dense history the run itself
    says what the sources of step i were (tracers_common.run_sources).  Every recorded row i in 70-200 against the oracle's
    float64 Euler step from the run's OWN row i - 1 over exactly those sources: 1e-9 of the largest displacement -- both sums
    are float64 over sources that agree to an ulp, only the order of summation differs.  A launch placed behind the Euler
    finisher would see the wake a step later (per cents of the step)."""
    seeds, rel = seeds37(), np.array([1, 90, 150], dtype=np.int64)[np.arange(37) % 3]
    eng.set_symmetric(64)
    try:
        sim = _ludvm()(**CONFIG1, verbose=False, engine=eng, precision="f32", history="full", tracers=seeds, tracer_release=rel,
                       tracer_frame="tunnel", probes=probes32())
    finally:
        eng.set_symmetric(1)
    worst, step_max = 0.0, 0.0
    for i in range(70, 201):
        sd = sim._tracer_seeds(i)
        want = euler_step(sd, sim.tracer_path[i - 1], rel, i, sim.dt, sim.v_core, run_sources(sim, i))
        worst = max(worst, np.abs(sim.tracer_path[i] - want).max())
        step_max = max(step_max, np.abs(want - np.where(rel == i, sd, sim.tracer_path[i - 1]))[:, rel <= i].max())
    disp = max(np.abs(sim.tracer_path[i] - sim._tracer_seeds(i)).max() for i in range(70, 201))
    print(f"overlapped fp32 steps 70-200: tracer rows vs float64 Euler step over the run's own sources: {worst / disp:.2e} of the "
          f"largest displacement ({disp:.2f}), {worst / step_max:.2e} of the largest single step ({step_max:.3f})")
    assert worst <= 1e-9 * disp, worst / disp
    assert worst <= 1e-7 * step_max, worst / step_max     # (a wake one step late is off by per cents of a step)


def test_tracers_are_the_class_own_zero_circulation_free_vortices(eng):
    """37 seeds as zero-circulation free vortices appended to G5's cloud (dense history, 'f64': path['FREE']) against the same
    seeds as tracers of the run without them, 50 steps: 1e-9 of the largest displacement."""
    kw, gc, seeds = dict(CONFIG1, tf=2.5), gust_cloud(), seeds37()
    nf = len(gc["circulation_freevort"])
    a = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="full",
                 circulation_freevort=np.concatenate([gc["circulation_freevort"], np.zeros(37)]),
                 xy_freevort=np.concatenate([gc["xy_freevort"], seeds], axis=1))
    b = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", **gc, tracers=seeds)
    free = a.path["FREE"][:, :, nf:]
    rows = np.stack([b.tracer_path[s] for s in range(51)])
    disp = np.abs(free - seeds[None]).max()
    err = np.abs(free - rows).max() / disp
    print(f"tracers vs the class's zero-circulation free vortices, 50 steps: {err:.2e} of the largest displacement ({disp:.3f})")
    assert disp > 0.1 and err <= 1e-9, err


def test_first_free_step_is_the_probe_value(eng):
    """A tracer released at step r from a lab-frame seed: (position after r - seed) / dt is probe_u[r], probe_w[r] at that
    point, 1e-12 of max|u| -- r = 5 in a serial step, r = 150 in an overlapped one (fp32, symmetric threshold 64)."""
    seeds = seeds37()
    rel = np.array([5, 150], dtype=np.int64)[np.arange(37) % 2]
    eng.set_symmetric(64)
    try:
        sim = _ludvm()(**CONFIG1, verbose=False, engine=eng, precision="f32", history="sparse", tracers=seeds, tracer_release=rel,
                       probes=seeds, tracer_steps=[4, 5, 149, 150])
    finally:
        eng.set_symmetric(1)
    assert np.array_equal(sim.tracer_path[4], seeds) and np.array_equal(sim.tracer_path[149][:, rel == 150], seeds[:, rel == 150])
    for r in (5, 150):
        m = rel == r
        u = (sim.tracer_path[r][0, m] - seeds[0, m]) / sim.dt
        w = (sim.tracer_path[r][1, m] - seeds[1, m]) / sim.dt
        scale = max(np.abs(sim.probe_u[r]).max(), np.abs(sim.probe_w[r]).max())
        err = max(np.abs(u - sim.probe_u[r, m]).max(), np.abs(w - sim.probe_w[r, m]).max()) / scale
        print(f"release step {r}: first free step vs probe row: {err:.2e} of max|u|")
        assert err <= 1e-12, (r, err)


def test_marched_and_per_step_paths_agree(eng):
    """march=True and march=False in 'f64': 1e-12 of the largest displacement over steps 1-10."""
    kw = dict(CONFIG1, tf=1.0)
    seeds, rel = seeds37(), np.array([1, 3, 7], dtype=np.int64)[np.arange(37) % 3]
    common = dict(verbose=False, engine=eng, precision="f64", tracers=seeds, tracer_release=rel, tracer_frame="tunnel")
    a = _ludvm()(**kw, **common, march=True)
    b = _ludvm()(**kw, **common, march=False)
    worst = max(np.abs(a.tracer_path[s] - b.tracer_path[s]).max() for s in range(1, 11))
    disp = max(np.abs(b.tracer_path[s] - b._tracer_seeds(s)).max() for s in range(1, 11))
    print(f"march vs per-step: tracer paths, steps 1-10: {worst / disp:.2e} of the largest displacement ({disp:.3f})")
    assert np.array_equal(a.tracer_path[0], b.tracer_path[0])
    assert worst <= 1e-12 * disp, worst / disp


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
def test_tracers_are_passive(eng, case):
    """With and without 600 tracers (two tiles, staggered releases), with probes set in both runs: Cl, every
    circulation[...], LEV_shed, the history rows, the final wake and probe_u / probe_w are the same arrays, bit for bit --
    serial and overlapped steps (symmetric threshold lowered), dense and sparse history."""
    LUDVM = _ludvm()
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_dense_overlapped": dict(precision="f32", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101]),
             "f32_sparse_serial": dict(precision="f32", history="sparse", snapshot_steps=[64])}[case]
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    pts = probes32()
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**CONFIG1, verbose=False, engine=eng, probes=pts, probe_frame="tunnel", **extra)
        wake_plain = _final_wake(eng)
        traced = LUDVM(**CONFIG1, verbose=False, engine=eng, probes=pts, probe_frame="tunnel", tracers=seeds, tracer_release=rel,
                       tracer_frame="tunnel", **extra)
        wake_traced = _final_wake(eng)
        bare = LUDVM(**CONFIG1, verbose=False, engine=eng, tracers=seeds, tracer_release=rel, **extra)      # (and without probes)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "tracer_path")
    _same_run(plain, traced)
    _same_run(plain, bare)
    for a, b in zip(wake_plain, wake_traced):
        assert np.array_equal(a, b)
    assert np.array_equal(plain.probe_u, traced.probe_u) and np.array_equal(plain.probe_w, traced.probe_w)
    last = traced.nt - 1
    assert np.isfinite(traced.tracer_path[last]).all()
    assert np.abs(traced.tracer_path[last] - traced._tracer_seeds(last))[:, rel <= 130].min(axis=0).max() > 0.0


@pytest.mark.parametrize("sym", [1, 64])
def test_tracer_paths_do_not_depend_on_the_chunking(eng, tmp_path, sym):
    """The same bits across _march_chunk = 32768 / 100 / 7, snapshot_steps present or absent, dense or sparse history, the cap
    on one call's recorded rows, run to run, and across a checkpoint at step 300 with a resume -- serial steps
    (sym = 1) and overlapped ones (threshold 64).  400 steps of config 1 in fp32, 600 tracers released at 1, 40, 130 and never."""
    kw = dict(CONFIG1)
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    keep = [1, 39, 40, 41, 64, 128, 129, 130, 192, 193, 256, 399, 400]
    common = dict(verbose=False, engine=eng, precision="f32", tracers=seeds, tracer_release=rel, tracer_frame="tunnel", tracer_steps=keep)
    calls = []

    class Capped(_ludvm()):
        _tracer_call_bytes = 16 * 600 * 2           # two recorded rows per call

        def _march_stretch(self, S, i, j, place, record=False):
            calls.append(int(np.count_nonzero((S.trec >= i) & (S.trec < j))))
            return super()._march_stretch(S, i, j, place, record=record)
    eng.set_symmetric(sym)
    try:
        base = _chunked(32768)(**kw, **common, history="sparse")
        assert base.nt == 401 and base.tracer_path.steps() == [0] + keep
        runs = {
            "again": _chunked(32768)(**kw, **common, history="sparse"),
            "chunk 100 + snapshots": _chunked(100)(**kw, **common, history="sparse", snapshot_steps=[64, 192, 193, 300]),
            "chunk 7": _chunked(7)(**kw, **common, history="sparse"),
            "dense": _ludvm()(**kw, **common, history="full"),
            "dense, chunk 7": _chunked(7)(**kw, **common, history="full"),
            "two rows per call": Capped(**kw, **common, history="sparse"),
        }
        assert max(calls) == 2 and sum(calls) == len(keep)
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, history="sparse", checkpoint_every=300, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 301 and R["tracer_cur"].shape == (2, 600) and list(R["tracer_rows_steps"]) == [0] + keep[:11]
        runs["resumed from 300"] = _ludvm().resume(ck, engine=eng, verbose=False)
    finally:
        eng.set_symmetric(1)
    for name, r in runs.items():
        assert r.tracer_path.steps() == base.tracer_path.steps(), name
        for s in base.tracer_path.steps():
            assert np.array_equal(r.tracer_path[s], base.tracer_path[s]), (name, s)
        assert np.array_equal(r.tracer_last, base.tracer_last) and np.array_equal(r.Cl, base.Cl), name
    moved = np.abs(base.tracer_path[400] - base._tracer_seeds(400))
    assert moved[:, rel <= 130].min(axis=0).max() > 0.0 and not moved[:, rel > 400].any()


def test_resume_between_two_releases(eng, tmp_path):
    """Releases at 1, 7 and 50 in a 60-step 'f64' run, checkpoint after step 23 (and 46), resume from the file of step 46 and
    from a file of step 23: the same tracer_path, bit for bit."""
    kw = dict(CONFIG1, tf=3.0)
    seeds, rel = seeds37(), releases_1_7_50(37)
    common = dict(verbose=False, engine=eng, precision="f64", tracers=seeds, tracer_release=rel, tracer_frame="tunnel")
    base = _ludvm()(**kw, **common)
    for every, nxt in ((23, 47), (30, 31)):
        ck = str(tmp_path / f"ck{every}.npz")
        _ludvm()(**kw, **common, checkpoint_every=every, checkpoint_path=ck)
        assert int(np.load(ck)["next_step"]) == nxt
        c = _ludvm().resume(ck, engine=eng, verbose=False)
        assert c.tracer_path.steps() == list(range(61))
        for s in range(61):
            assert np.array_equal(c.tracer_path[s], base.tracer_path[s]), (every, s)
        assert np.array_equal(c.tracer_last, base.tracer_last)


@pytest.fixture(scope="module")
def oracle30():
    """TracedOracle over 30 steps (tunnel frame) for 3 x 1021 tracers: 1021 seeds, each released at step 1, at step 5 and never."""
    base = seeds_random(1021, seed=17)
    seeds = np.concatenate([base, base, base], axis=1)
    rel = np.repeat(np.array([1, 5, 10 ** 6], dtype=np.int64), 1021)
    return base, TracedOracle(seeds, release=rel, shift=lambda o: o.xpiv, **dict(CONFIG1, tf=1.5)).path_rows()


@pytest.mark.parametrize("M", [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1, 262144])
def test_tracer_counts_on_both_sides_of_every_tile_boundary(eng, oracle30, M):
    """M tracers over 30 steps in 'f64' against TracedOracle at 1e-9: one lane, the second register set of a lane (256 / 257),
    one tile and the next (511 / 512 / 513), three tiles and one tracer, and the limit.  Releases by tile: tile 0, 3, ... free
    from step 1, tile 1, 4, ... mixed (step 1, step 5, never: lane by lane), tile 2, 5, ... wholly held.  Seeds repeat with
    period 1021 (a prime: no tile sees the same lanes twice), so one oracle run of 3 x 1021 tracers serves every count."""
    base, rows = oracle30
    m = np.arange(M)
    seeds = base[:, m % 1021]
    rel = releases_by_tile(M, TILE)
    col = np.searchsorted([1, 5, 10 ** 6], rel) * 1021 + m % 1021
    keep = [1, 4, 5, 6, 30]
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="sparse", tracers=seeds,
                   tracer_release=rel, tracer_frame="tunnel", tracer_steps=keep)
    assert sim.tracer_path.steps() == [0] + keep and sim.tracer_path[30].shape == (2, M)
    seed30 = sim._tracer_seeds(30)
    disp = np.abs(rows[30][:, col] - seed30).max()
    worst = max(np.abs(sim.tracer_path[s] - rows[s][:, col]).max() for s in [0] + keep)
    print(f"M = {M}: {worst / disp:.2e} of the largest displacement ({disp:.3f})")
    assert worst <= 1e-9 * disp, worst / disp
    held = rel > 30
    assert np.array_equal(sim.tracer_path[30][:, held], seed30[:, held])
    if M > 2 * TILE:
        assert held[2 * TILE:min(M, 3 * TILE)].all() and not held[:TILE].any()
    assert np.array_equal(sim.tracer_last, sim.tracer_path[30])


def test_one_tracer_too_many_is_refused(eng):
    from ludvm_amd import LudvmHipError, _ffi
    with pytest.raises(ValueError, match="262144"):
        _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, tracers=np.zeros([2, 262145]))
    sim = _ludvm()(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64")      # (leaves the march set up)
    with pytest.raises(LudvmHipError) as e:
        eng.march_set_tracers(np.zeros(262145), np.zeros(262145))
    assert e.value.code == _ffi.E_ARG and sim.nt == 21


def _read(eng, cap, M):
    """ludvm_march_read_tracers itself -> (status code, rows, steps, x): what the library answers."""
    from ctypes import POINTER, byref, c_longlong, c_size_t
    from ludvm_amd.engine import _pd
    x, z = np.full([max(cap, 1), M], np.nan), np.full([max(cap, 1), M], np.nan)
    steps, n = np.zeros(max(cap, 1), dtype=np.int64), c_size_t(99)
    rc = eng._lib.ludvm_march_read_tracers(eng._ctx, _pd(x), _pd(z), cap, steps.ctypes.data_as(POINTER(c_longlong)), byref(n))
    return rc, int(n.value), steps, x


def test_entry_points_answer_the_documented_codes(eng):
    from ludvm_amd import Engine, LudvmHipError, _ffi
    LUDVM = _ludvm()
    fresh = Engine(0)
    try:
        with pytest.raises(LudvmHipError) as e:
            fresh.march_set_tracers([0.0], [0.0])                   # before ludvm_march_setup
        assert e.value.code == _ffi.E_STATE
    finally:
        fresh.close()
    seeds = seeds37()[:, :5]
    rel = np.array([1, 1, 3, 3, 99], dtype=np.int64)
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", tracers=seeds, tracer_release=rel,
                tracer_steps=[2, 4, 5, 9], run=False)
    S = sim._loop_begin()
    sim._free_slot = S.fslot
    S.fsl = slice(0, S.nf)
    sim._loop_prepare_engine(S)                                   # ludvm_march_setup + ludvm_march_set_tracers
    assert S.can_march
    assert np.array_equal(eng.march_tracer_state(), seeds)          # before any step: the seeds
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE                      # no ludvm_march_run call yet
    sim._march_call(S, 1, 7, False, 50)                             # steps 1 .. 6: rows of steps 2, 4, 5
    rc, n, steps, x = _read(eng, 8, 5)
    assert rc == _ffi.OK and n == 3 and list(steps[:3]) == [2, 4, 5]
    assert np.array_equal(x[:3], np.stack([sim.tracer_path[s][0] for s in (2, 4, 5)])) and np.isnan(x[3:]).all()
    rc, n, _, x_small = _read(eng, 2, 5)                            # rows_cap too small: the count, nothing copied
    assert rc == _ffi.E_ARG and n == 3 and np.isnan(x_small).all()
    assert _read(eng, 3, 5)[0] == _ffi.OK
    state = eng.march_tracer_state()
    assert np.array_equal(state[:, 4], seeds[:, 4]) and np.abs(state[:, :4] - seeds[:, :4]).min() > 0.0
    # malformed definitions change nothing
    for bad in (lambda: eng.march_set_tracers(np.zeros(262145), np.zeros(262145)),
                lambda: eng.march_set_tracers([0.0, np.nan], [0.0, 0.0]),
                lambda: eng.march_set_tracers([0.0, 1.0], [0.0, np.inf]),
                lambda: eng.march_set_tracers([0.0, 1.0], [0.0, 0.0], release=[1, 0]),
                lambda: eng.march_set_tracers([0.0, 1.0], [0.0, 0.0], release=[-2, 1]),
                lambda: eng.march_set_tracers([0.0], [0.0], shift_x=np.zeros(3)),
                lambda: eng.march_set_tracers([0.0], [0.0], cur=[[np.nan], [0.0]]),
                lambda: eng.march_set_tracers([0.0], [0.0], record_steps=[3, 3]),
                lambda: eng.march_set_tracers([0.0], [0.0], record_steps=[5, 4]),
                lambda: eng.march_set_tracers([0.0], [0.0], record_steps=[0]),
                lambda: eng.march_set_tracers([0.0], [0.0], record_steps=[21])):
        with pytest.raises(LudvmHipError) as e:
            bad()
        assert e.value.code == _ffi.E_ARG
    rc, n, steps, x2 = _read(eng, 3, 5)
    assert rc == _ffi.OK and n == 3 and np.array_equal(x2[:3], x[:3]) and np.array_equal(eng.march_tracer_state(), state)
    # a call that records nothing: OK with zero rows
    sim._march_call(S, 7, 9, False, 50)                             # steps 7, 8
    assert _read(eng, 0, 5)[:2] == (_ffi.OK, 0)
    # count = 0 removes them; ludvm_march_setup forgets them
    eng.march_set_tracers([], [])
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE
    with pytest.raises(LudvmHipError) as e:
        eng.march_tracer_state()
    assert e.value.code == _ffi.E_STATE
    eng.march_set_tracers(seeds[0], seeds[1])
    eng.march_setup(sim.Npoints - 1, sim.Ncoeffs, *sim._march_inputs(S))
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE
    # ... and a run after it leaves no tracer rows, and is the run it was
    S.tracers = None
    sim._march_call(S, 9, 14, False, 50)
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE
    plain = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64")
    assert np.array_equal(plain.Fn[1:14], sim.Fn[1:14])
