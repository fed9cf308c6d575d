"""GPU tier: passive tracers in hi+lo fp32 (march_f32x2_tracer_partial, ludvm_march_set_tracer_precision; LUDVM(...,
tracer_precision='f32x2')) -- every row by value against a float64 Euler step over the run's own sources in
serial and overlapped steps, the first free step against the probe row, on both sides of every source-tile, source-split and
tracer-tile boundary, where the survey's local origins give up, independent of how a run is cut into calls, passive on every
other result, and the codes of the entry point.

Two bounds (tests/tracers_f32x2_common.py): a velocity within 2e-6 of max|u| (the project's hi+lo tier), and a row within 2e-6
of the largest single step of that time step (dt max|u|: the same bound, times dt) plus 1e-9 of the largest displacement (the
float64 rounding of start + dt u in another summation order) of a float64 Euler step FROM THE SAME START.  Two trajectories
that have left one another are not bounded that way -- their distance grows by (1 + dt |grad u|) per step -- so every check
here starts both sides of a comparison from the same positions.

Largest values seen [MI355X], of the step's largest single step unless said otherwise: rows 2-200 of the README case 7.8e-7 in
serial float64 steps and 9.1e-7 in overlapped fp32 steps; first free step against the probe row 1.4e-7 and 4.9e-7 of max|u|;
source counts 127 .. 513: 2.6e-7 (a single tracer, of its own step: 1.1e-6); tracer counts 1 .. 262 144: 3.8e-7; the dense cloud
at x = -55 5.8e-7, the sparse cloud 6.1e-7."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import cloud
from probes_common import probes32
from survey_f32_common import far_cloud, far_cloud_keywords, points_around, sparse_cloud_keywords
from tracers_common import euler_step, releases_by_tile, run_sources, seeds37, seeds_random
from tracers_f32x2_common import STEP_ROUNDING, STEP_VS_F64, VELOCITY_VS_F64

pytestmark = pytest.mark.gpu

NPAN = CONFIG1["Npoints"] - 1
V_CORE = 1.3 * CONFIG1["dt"]        # config 1: chord = Uinf = 1
README200 = dict(CONFIG1, tf=10.0)  # the README case over 200 steps
T = 1024                            # kTracerF32Tile of march_kernels.hpp (asserted below: collection does not import the package)


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


def _chunked(chunk):
    return type("Chunked", (_ludvm(),), dict(_march_chunk=chunk))


def _final_wake(eng):
    return eng.wake_read(0, eng.wake_size(), gamma=True)


def test_the_tile_is_what_the_tests_assume():
    from ludvm_amd import _ffi
    assert 256 * _ffi.TRACER_F32X2_PER_LANE == T


@pytest.fixture(scope="module")
def wake_seeds(eng):
    """seeds37() and points on, within one core of and 3 - 8 chords from the vortices 200 steps of the README case leave behind
    (lab frame) -> [2, M], read-only."""
    sim = _ludvm()(**README200, verbose=False, engine=eng, precision="f64", history="sparse")
    x, z, _ = _final_wake(eng)
    assert sim.nt == 201 and len(x) >= 200
    seeds = np.concatenate([seeds37(), points_around(x, z, V_CORE)], axis=1)
    seeds.setflags(write=False)
    return seeds


def _rows_against_their_own_sources(sim, rel, steps, cols=None):
    """Every row i of `steps` against the float64 Euler step from the run's OWN row i - 1 over the sources the dense history
    says step i had -> (worst excess over the bound, worst |difference| / largest single step of its step, largest step,
    largest displacement).  cols: the tracers looked at (default: all)."""
    cols = np.arange(len(rel)) if cols is None else cols
    r = rel[cols]
    found = []
    for i in steps:
        sd = sim._tracer_seeds(i)[:, cols]
        prev = sim.tracer_path[i - 1][:, cols]
        want = euler_step(sd, prev, r, i, sim.dt, sim.v_core, run_sources(sim, i))
        free = r <= i
        if not free.any():
            assert np.array_equal(sim.tracer_path[i][:, cols], sd)
            continue
        start = np.where(r == i, sd, prev)
        found.append((np.abs(sim.tracer_path[i][:, cols] - want).max(), np.abs(want - start)[:, free].max(),
                      np.abs(sim.tracer_path[i][:, cols] - sd).max()))
        held = ~free
        assert np.array_equal(sim.tracer_path[i][:, cols][:, held], sd[:, held]), i
    diff, step, disp = (np.array(c) for c in zip(*found))
    bound = STEP_VS_F64 * step + STEP_ROUNDING * disp.max()
    return (diff - bound).max(), (diff / step).max(), step.max(), disp.max()


@pytest.mark.parametrize("case", ["f64_serial", "f32_overlapped"])
def test_every_row_is_a_float64_euler_step_of_the_row_before(eng, wake_seeds, case):
    """The README case over 200 steps with the dense history; tracers around the foil and on / near / far from where the wake
    will be, released at steps 1, 90 and 150; serial float64 steps, and overlapped fp32 steps (symmetric threshold lowered to
    64: the tracer launch rides the second stream beside the symmetric kernel).  Every row i in 2 .. 200 against the oracle's
    float64 Euler step from the run's own row i - 1 over the sources of step i (tracers_common.run_sources): 2e-6 of the
    step's largest single step + 1e-9 of the largest displacement.  The rows are not the 'f64'-tracer run's: the fp32 kernel
    ran; everything else of the run is."""
    seeds = wake_seeds
    rel = np.array([1, 90, 150], dtype=np.int64)[np.arange(seeds.shape[1]) % 3]
    extra = dict(precision="f64") if case == "f64_serial" else dict(precision="f32")
    common = dict(verbose=False, engine=eng, history="full", tracers=seeds, tracer_release=rel, **extra)
    eng.set_symmetric(64 if case == "f32_overlapped" else 1)
    try:
        sim = _ludvm()(**README200, **common, tracer_precision="f32x2")
        ref = _ludvm()(**README200, **common)
    finally:
        eng.set_symmetric(1)
    assert sim.tracer_precision == "f32x2" and ref.tracer_precision == "f64" and sim.nt == 201
    excess, rel_err, step, disp = _rows_against_their_own_sources(sim, rel, range(2, 201))
    print(f"{case}: {seeds.shape[1]} tracers, rows 2-200 vs float64 Euler step over the run's own sources: worst {rel_err:.2e} of "
          f"the step's largest single step (largest {step:.3f}, largest displacement {disp:.2f})")
    assert excess <= 0.0, rel_err
    assert np.array_equal(sim.tracer_path[0], ref.tracer_path[0]) and np.array_equal(sim.tracer_path[0], seeds)
    assert not any(np.array_equal(sim.tracer_path[i], ref.tracer_path[i]) for i in (1, 2, 100, 200))
    assert np.array_equal(sim.Cl, ref.Cl) and np.array_equal(sim.path["TEV"], ref.path["TEV"])


def test_first_free_step_is_the_probe_value(eng):
    """A tracer released at step r from a lab-frame seed: (position after r - seed) / dt against probe_u[r], probe_w[r] at that
    point, 2e-6 of max|u| -- r = 5 in a serial step, r = 150 in an overlapped one (fp32, symmetric threshold 64)."""
    seeds = seeds37()
    rel = np.array([5, 150], dtype=np.int64)[np.arange(37) % 2]
    eng.set_symmetric(64)
    try:
        sim = _ludvm()(**README200, verbose=False, engine=eng, precision="f32", history="sparse", tracers=seeds, tracer_release=rel,
                       probes=seeds, tracer_steps=[4, 5, 149, 150], tracer_precision="f32x2")
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
        assert 0.0 < err <= VELOCITY_VS_F64, (r, err)


def _one_step_against_f64(eng, kw, seeds, step):
    """All of `seeds` released at `step` in a run of `kw`, 'f32x2' against 'f64' tracers: both take the one free step from the
    same seeds -> (|difference| / largest single step, f32x2 run)."""
    rel = np.full(seeds.shape[1], step, dtype=np.int64)
    common = dict(verbose=False, engine=eng, precision="f64", history="sparse", tracers=seeds, tracer_release=rel,
                  tracer_steps=[step - 1, step])
    ref = _ludvm()(**kw, **common)
    sim = _ludvm()(**kw, **common, tracer_precision="f32x2")
    assert np.array_equal(sim.tracer_path[step - 1], seeds) and np.array_equal(ref.tracer_path[step - 1], seeds)
    moved = np.abs(ref.tracer_path[step] - seeds).max()
    diff = np.abs(sim.tracer_path[step] - ref.tracer_path[step]).max()
    assert not np.array_equal(sim.tracer_path[step], ref.tracer_path[step])
    assert diff <= STEP_VS_F64 * moved + STEP_ROUNDING * moved, diff / moved
    return diff / moved, sim


@pytest.mark.parametrize("ns", [127, 128, 129, 255, 256, 257, 511, 512, 513])
def test_source_counts_at_the_tile_and_split_edges(eng, ns):
    """One free step, step 3, with a cloud of free vortices sized so that it walks exactly ns = nfree + 3 + 80 sources (no
    leading-edge vortex is shed: asserted): half a tile, a tile and two tiles, each with one source less and one more.  One
    tracer tile has want = 64 and chunk 256, so ns_ub = ns + 3 makes one, two and three source splits, the last of them
    holding 1 to 4 sources or none.  Tracers ON the free vortices as step 3 finds them (a float64 run with the dense history
    says where) and within one core of them; at M = 1 as well.  Against the 'f64' tracers' step from the same seeds: 2e-6 of
    the largest single step."""
    i = 3
    nfree = ns - i - NPAN
    kw = dict(CONFIG1, tf=(i + 0.5) * CONFIG1["dt"], **cloud(nfree))
    look = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", history="full")
    assert look.nt == i + 2 and (look.LEV_shed == -1).all()
    assert eng.wake_size() == nfree + i + 1, eng.wake_size()      # (the run goes one step past step 3)
    fx, fz = look.path["FREE"][i - 1]
    assert len(fx) == nfree
    seeds = points_around(fx, fz, V_CORE)[:, :2 * nfree]           # on the vortices, and within one core of them
    for M in (seeds.shape[1], 1):
        err, sim = _one_step_against_f64(eng, kw, seeds[:, :M], i)
        assert (sim.LEV_shed == -1).all()
        print(f"ns = {ns}, M = {M}: one free step vs 'f64' tracers: {err:.2e} of the largest single step")


def _sampled(M, count=512, seed=5):
    """Every tracer of a small set; of a large one, sorted indices of `count` tracers: the first and the last tracer of both
    halves of tiles at the front, in the middle and at the back, the rest drawn."""
    if M <= 16 * T:
        return np.arange(M)
    tiles = np.array([0, 1, 2, 3, M // T // 2, M // T // 2 + 1, M // T - 3, M // T - 2, M // T - 1])
    edges = np.concatenate([tiles * T, tiles * T + T - 1, tiles * T + 255, tiles * T + 256])
    rng = np.random.default_rng(seed)
    rest = rng.choice(M, count - len(np.unique(edges)), replace=False)
    return np.unique(np.concatenate([edges, rest]))[:count]


@pytest.mark.parametrize("M", [1, T - 1, T, T + 1, 2 * T + 1, 262144])
def test_tracer_counts_on_both_sides_of_every_tile_boundary(eng, M):
    """M tracers over 30 steps: one lane, one tile and the next, two tiles and one tracer, and the limit.  Releases by tile of
    1024: tile 0, 3, ... free from step 1, tile 1, 4, ... mixed (step 1, step 5, never: lane by lane), tile 2, 5, ... wholly
    held -- a workgroup whose two tile_min entries both say "held" leaves at once.  Rows 5, 6 and 30 against the float64 Euler
    step from the run's own rows 4, 5 and 29 (at M = 262 144: 512 sampled tracers); held tracers equal seed + shift exactly;
    row 0 equals the seeds."""
    base = seeds_random(1021, seed=17)
    m = np.arange(M)
    seeds = base[:, m % 1021]
    rel = releases_by_tile(M, T)
    keep = [1, 4, 5, 6, 29, 30]
    sim = _ludvm()(**dict(CONFIG1, tf=1.5), verbose=False, engine=eng, precision="f64", history="full", tracers=seeds,
                   tracer_release=rel, tracer_frame="tunnel", tracer_steps=keep, tracer_precision="f32x2")
    assert sim.tracer_path.steps() == [0] + keep and sim.tracer_path[30].shape == (2, M)
    assert np.array_equal(sim.tracer_path[0], sim._tracer_seeds(0)) and np.array_equal(sim.tracer_last, sim.tracer_path[30])
    cols = _sampled(M)
    excess, rel_err, step, disp = _rows_against_their_own_sources(sim, rel, (5, 6, 30), cols)
    print(f"M = {M}: rows 5, 6, 30 of {len(cols)} tracers vs float64 Euler step: worst {rel_err:.2e} of the step's largest single "
          f"step (largest {step:.3f}, largest displacement {disp:.3f})")
    assert excess <= 0.0, rel_err
    for s in keep:
        still = rel > s
        assert np.array_equal(sim.tracer_path[s][:, still], sim._tracer_seeds(s)[:, still]), s
        assert np.isfinite(sim.tracer_path[s]).all()
    moved = np.abs(sim.tracer_path[30] - sim._tracer_seeds(30)).max(axis=0) > 0.0
    assert np.array_equal(moved, rel <= 30)
    if M > 2 * T:
        assert (rel[2 * T:min(M, 3 * T)] > 30).all() and (rel[:T] == 1).all()


@pytest.mark.parametrize("which", ["dense_cloud_at_-55", "sparse_cloud"])
def test_where_local_origins_give_up(eng, which):
    """G5's cloud filled to one whole source tile at x = -55, and 300 free vortices 1000 v_core apart (every origin class of the
    survey's fp32 scheme is wider than its guard there): tracers on the vortices, within one core of them and 3 - 8 chords away,
    released at steps 1 .. 10 in turn.  In each of the first 10 steps, the tracers released in it take their first free step
    from the same seed in the 'f32x2' and the 'f64'-tracer run: 2e-6 of that step's largest single step (+ 1e-9 of the largest
    displacement).  The accumulated distance of the two runs' rows is printed."""
    if which == "sparse_cloud":
        free = sparse_cloud_keywords(300, V_CORE)
        x, z = free["xy_freevort"]
    else:
        free = far_cloud_keywords(fill=256)
        _, x, z = far_cloud(fill=256)
    seeds = points_around(x, z, V_CORE)
    M = seeds.shape[1]
    rel = 1 + (np.arange(M) % 10).astype(np.int64)
    kw = dict(CONFIG1, tf=0.5, **free)
    common = dict(verbose=False, engine=eng, precision="f64", history="sparse", tracers=seeds, tracer_release=rel,
                  tracer_steps=range(11))
    ref = _ludvm()(**kw, **common)
    sim = _ludvm()(**kw, **common, tracer_precision="f32x2")
    assert sim.nt == 11
    disp = max(np.abs(ref.tracer_path[s] - seeds).max() for s in range(1, 11))
    worst = 0.0
    for s in range(1, 11):
        first = rel == s
        assert np.array_equal(sim.tracer_path[s - 1][:, first], seeds[:, first])
        step = np.abs(ref.tracer_path[s][:, first] - seeds[:, first]).max()
        diff = np.abs(sim.tracer_path[s][:, first] - ref.tracer_path[s][:, first]).max()
        worst = max(worst, diff / step)
        assert 0.0 < diff <= STEP_VS_F64 * step + STEP_ROUNDING * disp, (s, diff / step)
    apart = np.abs(sim.tracer_path[10] - ref.tracer_path[10]).max()
    print(f"{which}: {M} tracers, first free steps 1-10 vs 'f64' tracers: worst {worst:.2e} of the step's largest single step; rows "
          f"of step 10 are {apart / disp:.2e} of the largest displacement ({disp:.3f}) apart")
    assert np.array_equal(sim.Cl, ref.Cl)


@pytest.mark.parametrize("sym", [1, 64])
def test_paths_do_not_depend_on_the_chunking(eng, tmp_path, sym):
    """The same bits across _march_chunk = 32768 / 100 / 7, dense or sparse history, run to run, and across a checkpoint after
    step 200 -- between the releases at 130 and 250 -- with a resume, which takes the precision from the checkpoint: serial steps
    (sym = 1) and overlapped ones (threshold 64).  300 steps of config 1 in fp32, 1100 tracers (two tiles) released at 1, 40,
    130, 250 and never."""
    kw = dict(CONFIG1, tf=15.0)
    seeds = seeds_random(1100)
    rel = np.array([1, 40, 130, 250, 10 ** 6], dtype=np.int64)[np.arange(1100) % 5]
    keep = [1, 39, 40, 41, 64, 128, 129, 130, 192, 193, 249, 250, 251, 299, 300]
    common = dict(verbose=False, engine=eng, precision="f32", tracers=seeds, tracer_release=rel, tracer_frame="tunnel", tracer_steps=keep,
                  tracer_precision="f32x2")
    eng.set_symmetric(sym)
    try:
        base = _chunked(32768)(**kw, **common, history="sparse")
        assert base.nt == 301 and base.tracer_path.steps() == [0] + keep
        runs = {
            "again": _chunked(32768)(**kw, **common, history="sparse"),
            "chunk 100 + snapshots": _chunked(100)(**kw, **common, history="sparse", snapshot_steps=[64, 192, 193]),
            "chunk 7": _chunked(7)(**kw, **common, history="sparse"),
            "dense": _ludvm()(**kw, **common, history="full"),
        }
        ck = str(tmp_path / "ck.npz")
        _chunked(100)(**kw, **common, history="sparse", checkpoint_every=100, checkpoint_path=ck)
        R = np.load(ck)
        assert int(R["next_step"]) == 201 and R["tracer_cur"].shape == (2, 1100)
        assert '"tracer_precision": "f32x2"' in str(R["ctor"])
        runs["resumed from 200"] = _ludvm().resume(ck, engine=eng, verbose=False)
        f64 = _chunked(32768)(**kw, **dict(common, tracer_precision="f64"), history="sparse")
    finally:
        eng.set_symmetric(1)
    assert runs["resumed from 200"].tracer_precision == "f32x2"
    for name, r in runs.items():
        assert r.tracer_path.steps() == base.tracer_path.steps(), name
        for s in base.tracer_path.steps():
            assert np.array_equal(r.tracer_path[s], base.tracer_path[s]), (name, s)
        assert np.array_equal(r.tracer_last, base.tracer_last) and np.array_equal(r.Cl, base.Cl), name
    assert not np.array_equal(f64.tracer_path[300], base.tracer_path[300]) and np.array_equal(f64.Cl, base.Cl)
    moved = np.abs(base.tracer_path[300] - base._tracer_seeds(300))
    assert moved[:, rel <= 250].min(axis=0).min() > 0.0 and not moved[:, rel > 300].any()


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


@pytest.mark.parametrize("case", ["f64_dense_serial", "f32_sparse_overlapped"])
def test_the_precision_of_the_tracers_touches_nothing_else(eng, case):
    """200 steps with probes, 1100 tracers and a 600-point survey, tracer_precision 'f64' against 'f32x2': loads, circulations,
    history rows, the resident wake, probe rows and survey sums are the same arrays, bit for bit -- serial float64 steps with
    the dense history and overlapped fp32 steps (symmetric threshold lowered to 64) with the sparse one."""
    LUDVM = _ludvm()
    extra = {"f64_dense_serial": dict(precision="f64", history="full"),
             "f32_sparse_overlapped": dict(precision="f32", history="sparse", snapshot_steps=[100, 101])}[case]
    others = dict(probes=probes32(), probe_frame="tunnel", tracers=seeds_random(1100),
                  tracer_release=np.array([1, 40, 130], dtype=np.int64)[np.arange(1100) % 3], tracer_steps=[1, 64, 128, 129, 200],
                  survey=seeds_random(600), survey_frame="tunnel", survey_steps=(5, 195, 3))
    eng.set_symmetric(64 if "overlapped" in case else 1)
    try:
        a = LUDVM(**README200, verbose=False, engine=eng, **others, **extra)
        wake_a = _final_wake(eng)
        b = LUDVM(**README200, verbose=False, engine=eng, tracer_precision="f32x2", **others, **extra)
        wake_b = _final_wake(eng)
    finally:
        eng.set_symmetric(1)
    assert a.nt == 201 and a.survey_count == b.survey_count == 64
    _same_run(a, b)
    for p, q in zip(wake_a, wake_b):
        assert np.array_equal(p, q)
    assert np.array_equal(a.probe_u, b.probe_u) and np.array_equal(a.probe_w, b.probe_w)
    assert np.array_equal(a.survey_sums, b.survey_sums)
    assert a.tracer_path.steps() == b.tracer_path.steps()
    assert np.array_equal(a.tracer_path[0], b.tracer_path[0])
    assert not np.array_equal(a.tracer_path[200], b.tracer_path[200]) and np.isfinite(b.tracer_path[200]).all()


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
        assert _code_of(lambda: fresh.march_set_tracer_precision("f32x2")) == _ffi.E_STATE          # (before ludvm_march_setup)
    finally:
        fresh.close()
    _prepared(eng)
    assert _code_of(lambda: eng.march_set_tracer_precision("f32x2")) == _ffi.E_STATE                # (no tracers are set)
    assert _code_of(lambda: eng.march_set_tracer_precision("f64")) == _ffi.E_STATE
    # the float64 run: steps 1 .. 12
    whole, Sw = _prepared(eng, **trc)
    whole._march_call(Sw, 1, 13, False, 50)
    state64 = eng.march_tracer_state()
    # the fp32 run of the same steps; a refused precision in the middle leaves the tracers, their positions and their precision alone
    sim, S = _prepared(eng, **trc, tracer_precision="f32x2")
    sim._march_call(S, 1, 7, False, 50)
    state6 = eng.march_tracer_state()
    for bad in (1, 3, -1, 7):
        assert _code_of(lambda: eng.march_set_tracer_precision(bad)) == _ffi.E_ARG
        assert np.array_equal(eng.march_tracer_state(), state6)
    sim._march_call(S, 7, 13, False, 50)
    state32 = eng.march_tracer_state()
    assert not np.array_equal(state32, state64) and np.array_equal(state32[:, 4], seeds[:, 4])
    one, S1 = _prepared(eng, **trc, tracer_precision="f32x2")
    one._march_call(S1, 1, 13, False, 50)
    assert np.array_equal(eng.march_tracer_state(), state32)          # (so the refused calls had not switched to float64)
    # the precision may change between two calls: float64 from step 7 on is neither run
    mix, Sm = _prepared(eng, **trc, tracer_precision="f32x2")
    mix._march_call(Sm, 1, 7, False, 50)
    eng.march_set_tracer_precision("f64")
    mix._march_call(Sm, 7, 13, False, 50)
    mixed = eng.march_tracer_state()
    assert not np.array_equal(mixed, state32) and not np.array_equal(mixed, state64)
    # ludvm_march_set_tracers resets to float64: a run after it is the float64 run, bit for bit
    two, S2 = _prepared(eng, **trc, tracer_precision="f32x2")
    eng.march_set_tracers(seeds[0], seeds[1], release=trc["tracer_release"], record_steps=[6, 12])
    two._march_call(S2, 1, 13, False, 50)
    assert np.array_equal(eng.march_tracer_state(), state64)
    # ... and so does ludvm_march_setup, which forgets the tracers
    eng.march_set_tracer_precision("f32x2")
    eng.march_setup(two.Npoints - 1, two.Ncoeffs, *two._march_inputs(S2))
    assert _code_of(lambda: eng.march_set_tracer_precision("f32x2")) == _ffi.E_STATE
    three, S3 = _prepared(eng, **trc)
    three._march_call(S3, 1, 13, False, 50)
    assert np.array_equal(eng.march_tracer_state(), state64)
