"""GPU tier: the wake survey's pair sums in fp32 on local origins (march_f32_survey_partial, ludvm_march_set_survey_precision;
LUDVM(..., survey_precision='f32')) -- against the float64 survey of the same run on both sides of
every point-tile, origin-class and source-tile boundary, far from the coordinate origin, with every class guarded, passive on
every other result, independent of how a run is cut into calls, and the codes of the entry point."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import cloud
from probes_common import probes32
from survey_common import series_umax, sums_errors, window
from survey_f32_common import (GUARDED_VS_F64, MEAN_VS_F64, MOMENT_VS_F64, far_cloud, far_cloud_keywords, points_around,
                               sparse_cloud_keywords)
from tracers_common import seeds37, seeds_random

pytestmark = pytest.mark.gpu

NPAN = CONFIG1["Npoints"] - 1
V_CORE = 1.3 * CONFIG1["dt"]        # config 1: chord = Uinf = 1


def _tile():
    from ludvm_amd import _ffi
    return 256 * _ffi.SURVEY_F32_PER_LANE       # kSurveyF32Tile of march_kernels.hpp


@pytest.fixture(autouse=True)
def _time_limit():
    """A limit on every test's host-side time.  (The handler runs between Python instructions: a test stuck INSIDE a HIP call
    is ended by the time limit that wraps the pytest command, not by this.)"""
    def expired(signum, frame):
        raise TimeoutError("GPU test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
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


@pytest.fixture(scope="module")
def shed_wake(eng):
    """Where 100 steps of the README case leave their shed vortices (lab frame), and the pivot's x at the last step."""
    sim = _ludvm()(**dict(CONFIG1, tf=5.0), verbose=False, engine=eng, precision="f64", history="sparse")
    x, z, _ = _final_wake(eng)
    assert sim.nt == 101 and len(x) >= 100
    x.setflags(write=False); z.setflags(write=False)
    return x, z, float(sim.xpiv[sim.nt - 1])


def _points_on_the_wake(shed, K, frame):
    """K points, in turn ON a shed vortex of the prior run, within one core of one, and 3-8 chords from one ('tunnel': where they
    sit at the last step)."""
    x, z, xpiv_last = shed
    rng = np.random.default_rng(K)
    k = np.arange(K)
    v = (k // 3) % len(x)
    kind = k % 3
    ang = rng.uniform(0, 2 * np.pi, K)
    rad = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(0.05, 1.0, K) * V_CORE, rng.uniform(3.0, 8.0, K)))
    px, pz = x[v] + rad * np.cos(ang), z[v] + rad * np.sin(ang)
    return np.stack([px - xpiv_last if frame == "tunnel" else px, pz])


def _point_cases():
    T = 1024                        # (= _tile(): asserted in the test; collection does not import the package)
    counts = [1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]
    combos = [("Faure", "tunnel"), ("Ramesh", "lab"), ("Faure", "lab"), ("Ramesh", "tunnel")]
    cases = [(K, *combos[i % 4]) for i, K in enumerate(counts)]
    return cases + [(2 * T + 1, m, f) for m, f in combos if (2 * T + 1, m, f) not in cases]


@pytest.mark.parametrize("K,method,frame", _point_cases(), ids=lambda v: str(v))
def test_fp32_sums_match_the_float64_survey_of_the_same_run(eng, shed_wake, K, method, frame):
    """100 steps of the README case in 'f64', every step sampled, K points on / near / far from the shed sheet: the fp32 sums
    against the float64 survey of the same run -- means within 1e-5 of max|u| (the largest |u|, |w| of the run's own probe rows
    at the same points), raw second moments within 3e-5 of max|u|^2.  K on both sides of every point-tile boundary."""
    assert _tile() == 1024 and K in (1, 255, 256, 257, 1023, 1024, 1025, 2049)
    pts = _points_on_the_wake(shed_wake, K, frame)
    kw = dict(CONFIG1, tf=5.0, method=method)
    common = dict(verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame=frame)
    ref = _ludvm()(**kw, **common, probes=pts, probe_frame=frame)
    sim = _ludvm()(**kw, **common, survey_precision="f32")
    assert ref.survey_precision == "f64" and sim.survey_precision == "f32" and sim.survey_count == ref.survey_count == 100
    umax = series_umax(ref.probe_u, ref.probe_w, window(1, 101, 1, 101))
    e_mean, e_mom = sums_errors(sim.survey_sums, ref.survey_sums, 100, umax)
    print(f"K = {K} {method} {frame}: fp32 survey vs float64 survey, 100 steps: means {e_mean:.2e} of max|u|, raw second moments "
          f"{e_mom:.2e} of max|u|^2 (max|u| = {umax:.3f})")
    assert not np.array_equal(sim.survey_sums, ref.survey_sums)          # (the fp32 kernel ran)
    assert np.array_equal(sim.Cl, ref.Cl)
    assert e_mean <= MEAN_VS_F64, e_mean
    assert e_mom <= MOMENT_VS_F64, e_mom


@pytest.mark.parametrize("ns", [127, 128, 129, 255, 256, 257, 511, 512, 513])
def test_source_counts_at_the_class_and_tile_edges(eng, ns):
    """One sample, the window (3, 4, 1), with a cloud of free vortices sized so that step 3 walks exactly ns = nfree + 3 + 80
    sources (no leading-edge vortex is shed: asserted): half a class, a class, a tile and two tiles, each with one source
    less and one more -- at 300 points, and at K = 1 (one point tile, want = 64: chunk 256, so ns_ub = ns + 3 > 512 gives
    three source splits, the third holding 2 to 4 sources).  fp32 against the float64 sample: 1e-5 of the sample's max|u|."""
    i = 3
    nfree = ns - i - NPAN
    kw = dict(CONFIG1, tf=(i + 0.5) * CONFIG1["dt"], **cloud(nfree))
    for K in (300, 1):
        pts = seeds_random(300)[:, :K]
        common = dict(verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_steps=(i, i + 1, 1))
        ref = _ludvm()(**kw, **common)
        assert ref.nt == i + 2 and (ref.LEV_shed == -1).all()
        sim = _ludvm()(**kw, **common, survey_precision="f32")
        assert sim.survey_count == ref.survey_count == 1
        # the run goes one step past the sample: its wake then holds nfree + i + 1 vortices
        assert eng.wake_size() == nfree + i + 1, eng.wake_size()
        umax = np.abs(ref.survey_sums[:2]).max()
        e_mean, e_mom = sums_errors(sim.survey_sums, ref.survey_sums, 1, umax)
        print(f"ns = {ns}, K = {K}: one sample: (u, w) {e_mean:.2e} of max|u|, products {e_mom:.2e} of max|u|^2")
        assert not np.array_equal(sim.survey_sums, ref.survey_sums)
        assert e_mean <= MEAN_VS_F64 and e_mom <= MOMENT_VS_F64, (K, e_mean, e_mom)


@pytest.mark.parametrize("fill", [256, 0], ids=["one_whole_tile", "g5_alone"])
def test_far_from_the_coordinate_origin(eng, fill):
    """G5's free-vortex cloud moved to x = -55 and points on its vortices, within one core of them and 3-8 chords away, lab
    frame, 20 steps: the same bounds.  Filled up to 256 vortices -- one whole source tile, a dense cloud (256 vortices of
    |G| <= 0.16 in a unit box, 15 v_core across) -- its two classes hold nothing else and take the fp32 loop: the error is an fp32
    error (above 1e-12), and within the bounds.  Alone (61 vortices) it shares its tile with the shed and the bound vortices
    55 chords away: both classes are 850 v_core wide and take the guard."""
    g, x, z = far_cloud(fill=fill)
    pts = points_around(x, z, V_CORE)
    kw = dict(CONFIG1, tf=1.0, **far_cloud_keywords(fill=fill))
    common = dict(verbose=False, engine=eng, precision="f64", history="sparse", survey=pts)
    ref = _ludvm()(**kw, **common, probes=pts)
    sim = _ludvm()(**kw, **common, survey_precision="f32")
    assert sim.survey_count == 20
    umax = series_umax(ref.probe_u, ref.probe_w, window(1, 21, 1, 21))
    e_mean, e_mom = sums_errors(sim.survey_sums, ref.survey_sums, 20, umax)
    print(f"{len(g)} free vortices at x = -55, {pts.shape[1]} points: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of "
          f"max|u|^2 (max|u| = {umax:.3f})")
    assert not np.array_equal(sim.survey_sums, ref.survey_sums)
    assert e_mean <= MEAN_VS_F64 and e_mom <= MOMENT_VS_F64, (e_mean, e_mom)
    if fill:
        assert e_mean > GUARDED_VS_F64, e_mean          # (the cloud's classes took the fp32 loop)
    else:
        assert e_mean <= GUARDED_VS_F64, e_mean


def test_a_sparse_cloud_takes_the_guard_in_every_class(eng):
    """300 free vortices 1000 v_core apart (every origin class that holds one is far wider than 300 v_core; the tile that holds
    the last 44 also holds the shed and the bound vortices): every class is evaluated by the float64 loop, and the means are
    the float64 survey's to 1e-12 of max|u| -- the same arithmetic in another summation tree."""
    pts = np.concatenate([probes32(), seeds_random(300)], axis=1)
    kw = dict(CONFIG1, tf=1.0, **sparse_cloud_keywords(300, V_CORE))
    common = dict(verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel")
    ref = _ludvm()(**kw, **common, probes=pts, probe_frame="tunnel")
    sim = _ludvm()(**kw, **common, survey_precision="f32")
    umax = series_umax(ref.probe_u, ref.probe_w, window(1, 21, 1, 21))
    e_mean, e_mom = sums_errors(sim.survey_sums, ref.survey_sums, 20, umax)
    print(f"sparse cloud, every class guarded: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= GUARDED_VS_F64 and e_mom <= 3 * GUARDED_VS_F64, (e_mean, e_mom)


def _same_run(a, b):
    assert np.array_equal(a.Cl, b.Cl) and np.array_equal(a.Cd, b.Cd) and np.array_equal(a.Cm, b.Cm)
    for name in ("Fn", "Fs", "L", "D", "T", "M", "LESP", "fourier", "LEV_shed"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
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


@pytest.mark.parametrize("case", ["f64_dense_serial", "f64_sparse_serial", "f32_dense_overlapped", "f32_sparse_overlapped"])
def test_the_precision_of_the_survey_touches_nothing_else(eng, case):
    """200 steps with probes, tracers and a 600-point survey, survey_precision 'f64' against 'f32': loads, circulations, history
    rows, the resident wake, probe rows and tracer paths are the same arrays, bit for bit -- serial float64 steps and overlapped
    fp32 steps (symmetric threshold lowered to 64), dense and sparse history."""
    LUDVM = _ludvm()
    extra = {"f64_dense_serial": dict(precision="f64", history="full"),
             "f64_sparse_serial": dict(precision="f64", history="sparse", snapshot_steps=[64, 100]),
             "f32_dense_overlapped": dict(precision="f32", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101])}[case]
    kw = dict(CONFIG1, tf=10.0)
    others = dict(probes=probes32(), probe_frame="tunnel", tracers=seeds37(),
                  tracer_release=np.array([1, 40, 130], dtype=np.int64)[np.arange(37) % 3], tracer_steps=[1, 64, 128, 129, 200],
                  survey=seeds_random(600), survey_frame="tunnel", survey_steps=(5, 195, 3))
    eng.set_symmetric(64 if "overlapped" in case else 1)
    try:
        a = LUDVM(**kw, verbose=False, engine=eng, **others, **extra)
        wake_a = _final_wake(eng)
        b = LUDVM(**kw, verbose=False, engine=eng, survey_precision="f32", **others, **extra)
        wake_b = _final_wake(eng)
    finally:
        eng.set_symmetric(1)
    assert a.nt == 201 and a.survey_count == b.survey_count == 64
    _same_run(a, b)
    for p, q in zip(wake_a, wake_b):
        assert np.array_equal(p, q)
    assert np.array_equal(a.probe_u, b.probe_u) and np.array_equal(a.probe_w, b.probe_w)
    assert a.tracer_path.steps() == b.tracer_path.steps()
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s]), s
    assert np.array_equal(a.tracer_last, b.tracer_last)
    assert not np.array_equal(a.survey_sums, b.survey_sums) and np.isfinite(b.survey_sums).all()


@pytest.mark.parametrize("sym", [1, 64])
def test_fp32_sums_do_not_depend_on_the_chunking(eng, tmp_path, sym):
    """The cases of test_survey_sums_do_not_depend_on_the_chunking with survey_precision='f32': the same bits across _march_chunk =
    32768 / 100 / 7, snapshot_steps inside the window, run to run, and across a checkpoint after step 150 (a window step) with a
    resume, which takes the precision from the checkpoint -- serial steps (sym = 1) and overlapped ones (threshold 64).  300 steps
    of config 1 in fp32, 600 points, window 20 .. 290 every 5."""
    kw = dict(CONFIG1, tf=15.0)
    steps = (20, 290, 5)
    W = window(*steps, 301)
    assert 150 in W
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", survey=seeds_random(600), survey_frame="tunnel",
                  survey_steps=steps, survey_precision="f32")
    eng.set_symmetric(sym)
    try:
        base = _chunked(32768)(**kw, **common)
        assert base.nt == 301 and base.survey_count == len(W) == 54
        runs = {
            "again": _chunked(32768)(**kw, **common),
            "chunk 100 + snapshots": _chunked(100)(**kw, **dict(common, snapshot_steps=[27, 28, 64, 150, 192, 193])),
            "chunk 7": _chunked(7)(**kw, **common),
        }
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, checkpoint_every=150, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 151 and int(R["survey_samples"]) == len(window(20, 151, 5, 301)) == 27
        assert '"survey_precision": "f32"' in str(R["ctor"])
        runs["resumed from 150"] = _ludvm().resume(ck, engine=eng, verbose=False)
        f64 = _chunked(32768)(**kw, **dict(common, survey_precision="f64"))
    finally:
        eng.set_symmetric(1)
    assert runs["resumed from 150"].survey_precision == "f32"
    for name, r in runs.items():
        assert r.survey_count == base.survey_count, name
        assert np.array_equal(r.survey_sums, base.survey_sums), name
        assert np.array_equal(r.Cl, base.Cl), name
    assert not np.array_equal(R["survey_sums"], base.survey_sums) and np.abs(base.survey_sums[2]).min() > 0.0
    assert not np.array_equal(f64.survey_sums, base.survey_sums) and np.array_equal(f64.Cl, base.Cl)


def _prepared(eng, **extra):
    """A 20-step 'f64' run set up for the march (ludvm_march_setup and, with a survey, ludvm_march_set_survey done, no step run)."""
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
    pts = probes32()[:, :5]
    fresh = Engine(0)
    try:
        assert _code_of(lambda: fresh.march_set_survey_precision("f32")) == _ffi.E_STATE          # (before ludvm_march_setup)
    finally:
        fresh.close()
    _prepared(eng)
    assert _code_of(lambda: eng.march_set_survey_precision("f32")) == _ffi.E_STATE                # (no survey is set)
    assert _code_of(lambda: eng.march_set_survey_precision("f64")) == _ffi.E_STATE
    # the float64 run: steps 1 .. 12, samples at 2, 4, .. 12
    whole, Sw = _prepared(eng, survey=pts, survey_steps=(2, 20, 2))
    whole._march_call(Sw, 1, 13, False, 50)
    sums64, n64 = eng.march_survey()
    assert n64 == 6
    # the fp32 run of the same steps; a refused precision in the middle leaves the survey, its sums and its precision alone
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_precision="f32")
    sim._march_call(S, 1, 7, False, 50)
    sums6, n6 = eng.march_survey()
    for bad in (2, -1, 7):
        assert _code_of(lambda: eng.march_set_survey_precision(bad)) == _ffi.E_ARG
        again, n_again = eng.march_survey()
        assert n_again == n6 == 3 and np.array_equal(again, sums6)
    sim._march_call(S, 7, 13, False, 50)
    sums32, n32 = eng.march_survey()
    assert n32 == 6 and not np.array_equal(sums32, sums64)
    one, S1 = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_precision="f32")
    one._march_call(S1, 1, 13, False, 50)
    assert np.array_equal(eng.march_survey()[0], sums32)               # (so the refused calls had not switched to float64)
    umax = np.sqrt(sums64[2:4].max() / 6)                              # (the largest rms: a lower bound of max|u|)
    assert sums_errors(sums32, sums64, 6, umax)[0] <= MEAN_VS_F64
    # ludvm_march_set_survey resets to float64: a run after it is the float64 run, bit for bit
    two, S2 = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_precision="f32")
    eng.march_set_survey(pts[0], pts[1], steps=(2, 20, 2))
    two._march_call(S2, 1, 13, False, 50)
    again64, n = eng.march_survey()
    assert n == 6 and np.array_equal(again64, sums64)
    # ... and so does ludvm_march_setup, which forgets the survey
    eng.march_setup(two.Npoints - 1, two.Ncoeffs, *two._march_inputs(S2))
    assert _code_of(lambda: eng.march_set_survey_precision("f32")) == _ffi.E_STATE
