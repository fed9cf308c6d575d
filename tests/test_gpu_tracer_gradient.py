"""GPU tier: the deformation gradient carried by the marched tracers (march_grad_tracer_partial / march_grad_tracer_finish,
ludvm_march_set_tracer_gradient / ludvm_march_read_tracer_gradient / ludvm_march_tracer_gradient_state; LUDVM(..., tracers=,
tracer_gradient=True)) -- every recorded step by value against the definition F_i = (I + dt G_i(start)) F_{i-1} over the sources
the run itself names, the release step against the direct gradient sum, passive on the positions and on every other result,
independent of how a run is cut into calls, on both sides of every tile boundary, and the codes of the three entry points.

Tolerances of the by-value checks are the project's own for this construction (tests/test_gpu_tracers.py): 1e-9 of max |F| and
1e-7 of the largest single increment max |dt G F| -- both sides are float64 sums over sources that agree to an ulp; a wake one
step late is off by per cents of an increment."""
import signal

import numpy as np
import pytest

import tracer_gradient_common as TG
from conftest import CONFIG1
from probes_common import probes32
from tracers_common import releases_by_tile, run_sources, seeds37, seeds_random

pytestmark = pytest.mark.gpu

TILE = 512          # kTracerTile of march_kernels.hpp: 256 lanes x 2 tracers


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


def _check_rows(sim, rel, steps, what):
    worst, fmax, inc = TG.rows_against_the_recursion(sim, rel, steps, _sources_of(sim))
    print(f"{what}: F rows vs (I + dt G_ref) F_prev over the run's own sources: {worst / fmax:.2e} of max|F| ({fmax:.3f}), "
          f"{worst / inc:.2e} of the largest single increment ({inc:.3e})")
    assert inc > 1e-6                                       # (the steps deform: the check is not one of identities)
    assert worst <= 1e-9 * fmax, worst / fmax
    assert worst <= 1e-7 * inc, worst / inc


@pytest.mark.parametrize("case", ["f64_steps_2_50", "f32_overlapped_steps_70_200"])
def test_every_step_by_value_over_the_sources_of_its_own_roll_up(eng, case):
    """Dense history, every step recorded.  'f64' over steps 2-50; the overlapped fp32 run of
    test_gpu_tracers.py::test_overlapped_steps_advect_by_the_sources_of_their_own_roll_up (symmetric threshold 64, probes set)
    over steps 70-200."""
    seeds = seeds37()
    if case == "f64_steps_2_50":
        rel = np.array([1, 7, 30], dtype=np.int64)[np.arange(37) % 3]
        sim = _ludvm()(**dict(CONFIG1, tf=2.5), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                       tracer_release=rel, tracer_frame="tunnel", tracer_gradient=True)
        steps = range(2, 51)
    else:
        rel = np.array([1, 90, 150], dtype=np.int64)[np.arange(37) % 3]
        eng.set_symmetric(64)
        try:
            sim = _ludvm()(**CONFIG1, verbose=False, engine=eng, precision="f32", history="full", tracers=seeds, tracer_release=rel,
                           tracer_frame="tunnel", probes=probes32(), tracer_gradient=True)
        finally:
            eng.set_symmetric(1)
        steps = range(70, 201)
    assert sim.tracer_F_path.steps() == sim.tracer_path.steps() == list(range(sim.nt))
    assert np.array_equal(sim.tracer_F_path[0], TG.identity(37))
    _check_rows(sim, rel, steps, case)
    last = sim.nt - 1
    assert np.array_equal(sim.tracer_F_last, sim.tracer_F_path[last])
    # the exponent: numpy's SVD of the last row; NaN before a release
    ftle = sim.tracer_ftle()
    F = sim.tracer_F_last
    s = np.linalg.svd(np.moveaxis(F.reshape(2, 2, -1), -1, 0), compute_uv=False)[:, 0]
    assert np.allclose(ftle, np.log(s) / (sim.dt * (last - rel + 1.0)), rtol=1e-12, atol=1e-13)
    early = sim.tracer_ftle(step=int(rel.max()) - 1)
    assert np.isnan(early[rel == rel.max()]).all() and np.isfinite(early[rel < rel.max()]).all()


def test_the_release_step_is_the_direct_gradient_sum(eng):
    """At a tracer's release step r, (F - I) / dt is G at the seed: `velocity_gradient` (pair_grad_f64) over the sources of step
    r, to 1e-9 of max|G| -- the marched kernel and the direct one agree.  r = 5 and r = 30, lab frame, 'f64', dense history."""
    seeds = seeds37()
    rel = np.array([5, 30], dtype=np.int64)[np.arange(37) % 2]
    sim = _ludvm()(**dict(CONFIG1, tf=2.0), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                   tracer_release=rel, tracer_gradient=True)
    for r in (5, 30):
        m = rel == r
        assert np.array_equal(sim.tracer_F_path[r - 1][:, m], TG.identity(int(m.sum())))
        gw, xs, zs, gf, xf, zf = run_sources(sim, r)
        ux, uz, wx = sim.velocity_gradient(np.concatenate([gw, gf]), np.concatenate([xs, xf]), np.concatenate([zs, zf]),
                                           seeds[0, m], seeds[1, m])
        got = (sim.tracer_F_path[r][:, m] - TG.identity(int(m.sum()))) / sim.dt
        scale = max(np.abs(ux).max(), np.abs(uz).max(), np.abs(wx).max())
        err = max(np.abs(got[0] - ux).max(), np.abs(got[1] - uz).max(), np.abs(got[2] - wx).max(), np.abs(got[3] + ux).max())
        print(f"release step {r}: (F - I) / dt vs velocity_gradient at the seeds: {err / scale:.2e} of max|G| ({scale:.3f})")
        assert err <= 1e-9 * scale, (r, err / scale)


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
def test_the_gradient_is_passive(eng, case):
    """With and without tracer_gradient, 600 tracers (two tiles, staggered releases) and probes in both runs: the tracer
    positions, Cl, every circulation[...], LEV_shed, the history rows, the final wake and the probe rows are the same arrays,
    bit for bit."""
    LUDVM = _ludvm()
    kw = dict(CONFIG1, tf=10.0)
    extra = {"f64_dense": dict(precision="f64", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101])}[case]
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    common = dict(verbose=False, engine=eng, probes=probes32(), probe_frame="tunnel", tracers=seeds, tracer_release=rel,
                  tracer_frame="tunnel", **extra)
    if "overlapped" in case:
        eng.set_symmetric(64)
    try:
        plain = LUDVM(**kw, **common)
        wake_plain = _final_wake(eng)
        grad = LUDVM(**kw, **common, tracer_gradient=True)
        wake_grad = _final_wake(eng)
        again = LUDVM(**kw, **common)                       # (and a context that carried the gradient enqueues the plain pair again)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "tracer_F_path") and plain.tracer_gradient is False
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
    """The same F bits across _march_chunk = 32768 / 7, dense or sparse history, the cap on one call's recorded rows (48 bytes per
    tracer and row), run to run, and across a checkpoint at step 100 -- between the releases at 40 and 130 -- with a resume.
    200 steps of config 1 in fp32 (overlapped: symmetric threshold 64), 600 tracers released at 1, 40, 130 and never."""
    kw = dict(CONFIG1, tf=10.0)
    seeds = seeds_random(600)
    rel = np.array([1, 40, 130, 10 ** 6], dtype=np.int64)[np.arange(600) % 4]
    keep = [1, 39, 40, 41, 64, 128, 129, 130, 131, 192, 200]
    common = dict(verbose=False, engine=eng, precision="f32", tracers=seeds, tracer_release=rel, tracer_frame="tunnel",
                  tracer_steps=keep, tracer_gradient=True)
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
        assert "tracer_gradient" in str(R["ctor"])
        runs["resumed from 100"] = _ludvm().resume(ck, engine=eng, verbose=False)
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


@pytest.mark.parametrize("M", [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1])
def test_tracer_counts_on_both_sides_of_every_tile_boundary(eng, M):
    """M tracers over 30 steps in 'f64', dense history: every row against the NumPy recursion within the two tolerances; one
    lane, the second register set of a lane (256 / 257), one tile and the next (511 / 512 / 513), two and three tiles and one
    tracer.  Releases by tile: tile 0, 3, ... free from step 1, tile 1, 4, ... mixed (step 1, step 5, never: lane by lane),
    tile 2, 5, ... wholly held.  Held and never-released tracers keep F exactly the identity and have no exponent."""
    seeds = seeds_random(M, seed=17)
    rel = releases_by_tile(M, TILE)
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                   tracer_release=rel, tracer_frame="tunnel", tracer_gradient=True)
    assert sim.nt == 31 and sim.tracer_F_path.steps() == list(range(31)) and sim.tracer_F_path[30].shape == (4, M)
    _check_rows(sim, rel, range(1, 31), f"M = {M}")
    held = rel > 30
    for s in range(31):
        still = rel > s
        assert np.array_equal(sim.tracer_F_path[s][:, still], TG.identity(int(still.sum()))), s
    ftle = sim.tracer_ftle()
    assert np.isnan(ftle[held]).all() and np.isfinite(ftle[~held]).all()
    assert np.isnan(sim.tracer_ftle(step=4)[rel > 4]).all()
    if M > 2 * TILE:
        assert held[2 * TILE:min(M, 3 * TILE)].all() and not held[:TILE].any()
    assert np.array_equal(sim.tracer_F_last, sim.tracer_F_path[30])


def _read(eng, cap, M):
    """ludvm_march_read_tracer_gradient itself -> (status code, rows, steps, F): what the library answers."""
    from ctypes import POINTER, byref, c_longlong, c_size_t
    from ludvm_amd.engine import _pd
    F = np.full([max(cap, 1), 4, M], np.nan)
    steps, n = np.zeros(max(cap, 1), dtype=np.int64), c_size_t(99)
    rc = eng._lib.ludvm_march_read_tracer_gradient(eng._ctx, _pd(F), cap, steps.ctypes.data_as(POINTER(c_longlong)), byref(n))
    return rc, int(n.value), steps, F


def test_entry_points_answer_the_documented_codes(eng):
    from ludvm_amd import Engine, LudvmHipError, _ffi
    LUDVM = _ludvm()
    fresh = Engine(0)
    try:
        for call in (lambda: fresh.march_set_tracer_gradient(True), fresh.march_tracer_gradient_state):
            fresh._march_ntracers = 1
            with pytest.raises(LudvmHipError) as e:
                call()                                              # before ludvm_march_setup
            assert e.value.code == _ffi.E_STATE
    finally:
        fresh.close()
    seeds = seeds37()[:, :5]
    rel = np.array([1, 1, 3, 3, 99], dtype=np.int64)
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", tracers=seeds, tracer_release=rel,
                tracer_steps=[2, 4, 5, 9], tracer_gradient=True, run=False)
    S = sim._loop_begin()
    sim._free_slot = S.fslot
    S.fsl = slice(0, S.nf)
    sim._loop_prepare_engine(S)                                   # ludvm_march_setup, _set_tracers, _set_tracer_gradient
    assert S.can_march
    assert np.array_equal(eng.march_tracer_gradient_state(), TG.identity(5))      # before any step: the identity
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE                      # no ludvm_march_run call yet
    sim._march_call(S, 1, 7, False, 50)                             # steps 1 .. 6: rows of steps 2, 4, 5
    rc, n, steps, F = _read(eng, 8, 5)
    assert rc == _ffi.OK and n == 3 and list(steps[:3]) == [2, 4, 5]
    assert np.array_equal(F[:3], np.stack([sim.tracer_F_path[s] for s in (2, 4, 5)])) and np.isnan(F[3:]).all()
    rc, n, _, F_small = _read(eng, 2, 5)                            # rows_cap too small: the count, nothing copied
    assert rc == _ffi.E_ARG and n == 3 and np.isnan(F_small).all()
    state = eng.march_tracer_gradient_state()
    assert np.array_equal(state[:, 4], TG.identity(1)[:, 0]) and np.abs(state[:, :4] - TG.identity(4)).max(axis=0).min() > 0.0
    # a bad flag, an F that is not finite or not [4, M]: refused, nothing changes
    bad_F = state.copy()
    bad_F[2, 1] = np.nan
    for bad in (lambda: eng.march_set_tracer_gradient(2), lambda: eng.march_set_tracer_gradient(-1),
                lambda: eng.march_set_tracer_gradient(True, F=bad_F),
                lambda: eng.march_set_tracer_gradient(True, F=np.where(np.isnan(bad_F), np.inf, bad_F))):
        with pytest.raises(LudvmHipError) as e:
            bad()
        assert e.value.code == _ffi.E_ARG
    with pytest.raises(ValueError):
        eng.march_set_tracer_gradient(True, F=state[:, :3])
    rc, n, steps, F2 = _read(eng, 3, 5)
    assert rc == _ffi.OK and n == 3 and np.array_equal(F2, F[:3]) and np.array_equal(eng.march_tracer_gradient_state(), state)
    # the gradient needs float64 tracers: 'f32x2' is refused while it is on, and changes nothing
    with pytest.raises(LudvmHipError) as e:
        eng.march_set_tracer_precision("f32x2")
    assert e.value.code == _ffi.E_STATE and np.array_equal(eng.march_tracer_gradient_state(), state)
    # a call that records nothing: OK with zero rows
    sim._march_call(S, 7, 9, False, 50)                             # steps 7, 8
    assert _read(eng, 0, 5)[:2] == (_ffi.OK, 0)
    # switched off: no state and no rows; switched on again with an F: that F
    eng.march_set_tracer_gradient(False)
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE
    with pytest.raises(LudvmHipError) as e:
        eng.march_tracer_gradient_state()
    assert e.value.code == _ffi.E_STATE
    eng.march_set_tracer_gradient(True, F=state)
    assert np.array_equal(eng.march_tracer_gradient_state(), state)
    assert _read(eng, 8, 5)[0] == _ffi.E_STATE                      # (switched on after the last ludvm_march_run call)
    # ludvm_march_set_tracers resets it, and so does ludvm_march_setup
    eng.march_set_tracers(seeds[0], seeds[1])
    with pytest.raises(LudvmHipError) as e:
        eng.march_tracer_gradient_state()
    assert e.value.code == _ffi.E_STATE
    eng.march_set_tracer_precision("f32x2")
    with pytest.raises(LudvmHipError) as e:
        eng.march_set_tracer_gradient(True)                         # hi+lo fp32 tracers carry none
    assert e.value.code == _ffi.E_STATE
    eng.march_set_tracer_precision("f64")
    eng.march_set_tracer_gradient(True)
    eng.march_setup(sim.Npoints - 1, sim.Ncoeffs, *sim._march_inputs(S))
    with pytest.raises(LudvmHipError) as e:
        eng.march_tracer_gradient_state()
    assert e.value.code == _ffi.E_STATE
    eng.march_set_tracers([], [])
    with pytest.raises(LudvmHipError) as e:
        eng.march_set_tracer_gradient(True)                         # no tracers set
    assert e.value.code == _ffi.E_STATE
