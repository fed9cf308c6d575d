"""GPU tier of the wake integrals (march_integral_partial / _finish, march_energy_partial / _tiles / _finish behind march_solve,
ludvm_march_set_integrals / ludvm_march_read_integrals; LUDVM(..., wake_integrals=True, wake_energy_steps=); DESIGN.md section
4.22): by value against the long-double reference over the run's own dense history (tests/wake_integrals_common.py) at the
smallest shapes at which each part can go wrong, bit for bit however a run is cut, passive on every other result, and the
documented codes of the two entry points.

Worst |error| / bound per case [MI355X]: see each test's printed line; the figures are recorded in DESIGN.md section 4.22.
"""
import signal

import numpy as np
import pytest

import wake_integrals_common as WI
from conftest import CONFIG1
from observers_off_unit_common import case_keywords
from tracers_common import seeds37

pytestmark = pytest.mark.gpu


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


def _source_counts(sim):
    """S->n + nfoil behind the solve of every step 1 .. nt - 1, from the run's own shedding record"""
    shed = np.asarray(sim.LEV_shed) != -1
    i = np.arange(1, sim.nt)
    return sim.n_freevort + i + np.cumsum(shed)[1:] + (sim.Npoints - 1)


def test_config_1_by_value(eng):
    """Config 1's 400 steps in 'f64', dense history: the wake grows from 3 to 603, so with the 80 bound vortices the sources cross
    the 256-source tile and the 512-point tile; LEVs of both signs are shed.  The energy window begins at step 1, skips steps
    and ends before the run does."""
    win = (1, 380, 19)
    sim = _ludvm()(**CONFIG1, verbose=False, engine=eng, precision="f64", wake_integrals=True, wake_energy_steps=win)
    assert sim.history == "full"
    ns = _source_counts(sim)
    assert ns[0] < 256 < 512 < ns[-1]
    census = WI.class_census(sim, range(1, sim.nt))
    assert (census[[WI.TEV, WI.LEV, WI.BOUND]] > 0).all() and census[WI.FREE, 0] == 1
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps(win, sim.nt), "march, config 1")
    assert sim.integral_sums[0, WI.FREE, 0, 0] == 1.0 and not sim.integral_sums[0, 1:].any()


@pytest.mark.parametrize("edge", [256, 512, 2048])
def test_sources_on_and_around_an_edge(eng, edge):
    """245 panels, no LEV (LESPcrit out of reach) and edge - 255 free vortices: S->n + nfoil = edge - 10 + i behind step i, so
    steps 9, 10, 11 sit one below, on and one above the 256-source tile, the 512-point tile and the 2048-source chunk of the
    moments.  The energy is sampled at those three steps."""
    nf = edge - 255
    kw = dict(CONFIG1, tf=0.6, Npoints=246, LESPcrit=10.0)
    if nf > 1:
        kw.update(WI.mixed_cloud(nf, seed=edge))
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", wake_integrals=True, wake_energy_steps=(9, 12, 1))
    ns = _source_counts(sim)
    assert sim.nt == 13 and list(ns[8:11]) == [edge - 1, edge, edge + 1]
    WI.check_run(sim, sim, range(1, sim.nt), [9, 10, 11], f"march, sources across {edge}")
    if nf > 1:
        assert (WI.class_census(sim, [10])[WI.FREE] > nf // 4).all()


def test_free_cloud_many_tiles_and_splits(eng):
    """About 1100 free vortices of mixed sign in front of the foil: FREE in both slots, three point tiles, five source splits;
    a window that begins late and skips steps."""
    win = (5, 38, 4)
    kw = dict(CONFIG1, tf=2.0, **WI.mixed_cloud(1100))
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", wake_integrals=True, wake_energy_steps=win)
    assert 1024 < _source_counts(sim)[0] and _source_counts(sim)[-1] < 1536
    census = WI.class_census(sim, range(1, sim.nt))
    assert (census[WI.FREE] > 400).all() and census[WI.TEV].sum() == sim.nt - 1
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps(win, sim.nt), "march, 1100 free vortices")
    assert sim.integral_sums[0, WI.FREE, :, 0].sum() == 1100


def test_off_the_unit_point(eng):
    """G10's c4412d: chord 2, Uinf 3, rho 0.9, a cambered section, 'Ramesh' -- rho and the frame"""
    win = (1, 61, 7)
    kw = case_keywords("c4412d", steps=60)
    with pytest.warns(RuntimeWarning, match="mean line"):
        sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", wake_integrals=True, wake_energy_steps=win)
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps(win, sim.nt), "march, c4412d")
    tot = WI.reference(sim, 50, energy=False)["sums"].sum(axis=(0, 1))
    assert np.allclose(sim.wake_impulse[50], 0.9 * np.array([-tot[3], tot[2]]), rtol=1e-11)


def test_per_step_path_within_the_same_bounds(eng):
    """march=False: the rows the host forms, the energy from Engine.scalar_field at the step's sources"""
    win = (1, 100, 9)
    kw = dict(CONFIG1, tf=5.0)
    sim = _ludvm()(**kw, verbose=False, engine=eng, precision="f64", march=False, wake_integrals=True, wake_energy_steps=win)
    WI.check_run(sim, sim, range(1, sim.nt), WI.window_steps(win, sim.nt), "per-step path, config 1's first 100 steps")


def _same_rows(a, b):
    assert np.array_equal(a.integral_sums, b.integral_sums)
    assert np.array_equal(a.wake_energy, b.wake_energy, equal_nan=True)
    assert np.array_equal(a.Cl, b.Cl) and np.array_equal(a.LEV_shed, b.LEV_shed)


@pytest.mark.parametrize("sym", [1, 64])
def test_rows_do_not_depend_on_how_the_run_is_cut(eng, tmp_path, sym):
    """300 steps in 'f32', sparse history: one call; calls of 64 (on the sync period), 100 and 7 steps (off it); a repeat; a
    checkpoint at step 130 and a resume -- the same bits, serial steps (sym = 1) and overlapped ones (threshold 64)."""
    kw = dict(CONFIG1, tf=15.0)
    common = dict(verbose=False, engine=eng, precision="f32", history="sparse", wake_integrals=True, wake_energy_steps=(1, 290, 11))
    ck = str(tmp_path / "ck.npz")
    eng.set_symmetric(sym)
    try:
        one = _ludvm()(**kw, **common)
        assert one.nt == 301 and np.isfinite(one.wake_energy[1:290:11]).all() and one.integral_sums[-1, WI.LEV, :, 0].sum() > 0
        for chunk in (64, 100, 7):
            _same_rows(one, _chunked(chunk)(**kw, **common))
        _same_rows(one, _ludvm()(**kw, **common))
        _same_rows(one, _ludvm()(**kw, **common, snapshot_steps=[128, 129, 200], checkpoint_every=130, checkpoint_path=ck))
        assert int(np.load(ck)["next_step"]) == 261
        _same_rows(one, _ludvm().resume(ck, engine=eng, verbose=False))
    finally:
        eng.set_symmetric(1)


@pytest.mark.parametrize("case", ["f64_dense", "f32_overlapped"])
def test_the_observer_is_passive_and_composes(eng, case):
    """Cl, every circulation, the final wake, the probe rows, the tracer paths and the survey sums of a run WITH the observer are
    bit-identical to the same run without it."""
    kw = dict(CONFIG1, tf=6.0)
    extra = dict(precision="f64") if case == "f64_dense" else dict(precision="f32", history="sparse", snapshot_steps=[60, 61])
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(-6.0, 1.0, 40), rng.uniform(-1.0, 2.5, 40)])
    obs = dict(probes=pts, tracers=seeds37(), survey=pts[:, :24], survey_steps=(3, 110, 4))
    eng.set_symmetric(1 if case == "f64_dense" else 32)
    try:
        plain = _ludvm()(**kw, verbose=False, engine=eng, **extra, **obs)
        wake_plain = eng.wake_read(0, eng.wake_size(), gamma=True)
        both = _ludvm()(**kw, verbose=False, engine=eng, **extra, **obs, wake_integrals=True, wake_energy_steps=(1, 121, 5))
        wake_both = eng.wake_read(0, eng.wake_size(), gamma=True)
    finally:
        eng.set_symmetric(1)
    assert not hasattr(plain, "integral_sums") and np.isfinite(both.wake_energy[1::5]).all()
    assert np.array_equal(plain.Cl, both.Cl) and np.array_equal(plain.Cd, both.Cd) and np.array_equal(plain.LEV_shed, both.LEV_shed)
    for key in plain.circulation:
        assert np.array_equal(plain.circulation[key], both.circulation[key]), key
    for a, b in zip(wake_plain, wake_both):
        assert np.array_equal(a, b)
    assert np.array_equal(plain.probe_u, both.probe_u) and np.array_equal(plain.probe_w, both.probe_w)
    assert plain.tracer_path.steps() == both.tracer_path.steps()
    for s in plain.tracer_path.steps():
        assert np.array_equal(plain.tracer_path[s], both.tracer_path[s]), s
    assert plain.survey_count == both.survey_count and np.array_equal(plain.survey_sums, both.survey_sums)
    # ... and its own rows are those of a run that has nothing but the observer
    eng.set_symmetric(1 if case == "f64_dense" else 32)
    try:
        only = _ludvm()(**kw, verbose=False, engine=eng, **extra, wake_integrals=True, wake_energy_steps=(1, 121, 5))
    finally:
        eng.set_symmetric(1)
    _same_rows(only, both)


def _read(eng, rows):
    """ludvm_march_read_integrals itself -> (status code, sums, energy)"""
    from ludvm_amd.engine import _pd
    sums, energy = np.empty([rows, 4, 2, 6]), np.empty(rows)
    return eng._lib.ludvm_march_read_integrals(eng._ctx, _pd(sums), _pd(energy), rows), sums, energy


def _code(call):
    from ludvm_amd import LudvmHipError
    with pytest.raises(LudvmHipError) as e:
        call()
    return e.value.code


def test_entry_points_answer_the_documented_codes(eng):
    import torch
    from ludvm_amd import Engine, _ffi
    LUDVM = _ludvm()
    fresh = Engine(0)
    try:
        assert _code(lambda: fresh.march_set_integrals(True, [0])) == _ffi.E_STATE              # before ludvm_march_setup
    finally:
        fresh.close()
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", wake_integrals=True,
                wake_energy_steps=(2, 6, 2), run=False)
    S = sim._loop_begin()
    sim._free_slot = S.fslot
    S.fsl = slice(0, S.nf)
    sim._loop_prepare_engine(S)                                   # ludvm_march_setup + ludvm_march_set_integrals
    assert S.can_march and eng.wake_size() == 1
    assert _read(eng, 6)[0] == _ffi.E_STATE                       # no ludvm_march_run call yet
    sim._march_call(S, 1, 7, False, 50)                           # steps 1 .. 6
    for wrong in (5, 7, 0):
        assert _read(eng, wrong)[0] == _ffi.E_ARG
    rc, sums, energy = _read(eng, 6)
    assert rc == _ffi.OK and np.array_equal(sums, sim.integral_sums[1:7])
    assert np.isnan(energy[[0, 2, 4, 5]]).all() and np.isfinite(energy[[1, 3]]).all()       # steps 2 and 4; the window ends at 6
    n = eng.wake_size()
    tags = sim._wake_tags(S)
    assert n == len(tags) >= 7
    # refused calls leave the previous state, and its rows, as they were
    bad_tag = tags.copy()
    bad_tag[3] = 3
    for bad in (lambda: eng.march_set_integrals(True, bad_tag), lambda: eng.march_set_integrals(True, tags[:-1]),
                lambda: eng.march_set_integrals(True, np.append(tags, 0)), lambda: eng.march_set_integrals(True, tags, (0, 5, 1)),
                lambda: eng.march_set_integrals(True, tags, (3, 3, 1)), lambda: eng.march_set_integrals(True, tags, (1, 5, -1))):
        assert _code(bad) == _ffi.E_ARG
    acc = torch.zeros(64, dtype=torch.int64, device="cuda")
    eng.set_shard(0, 2, allreduce=lambda count, stream: None, d_acc=acc.data_ptr(), acc_bytes=acc.numel() * 8)
    try:
        assert _code(lambda: eng.march_set_integrals(True, tags)) == _ffi.E_STATE             # a sharded context
    finally:
        eng.set_shard(0, 1)
    rc, sums2, energy2 = _read(eng, 6)
    assert rc == _ffi.OK and np.array_equal(sums2, sums) and np.array_equal(energy2, energy, equal_nan=True)
    # set again (every = 0: no energy samples): the rows are gone until the next run, whose tags are the ones given here
    eng.march_set_integrals(True, tags)
    assert _read(eng, 6)[0] == _ffi.E_STATE
    sim.wake_energy_steps = None
    sim._march_call(S, 7, 12, False, 50)
    rc, sums3, energy3 = _read(eng, 5)
    assert rc == _ffi.OK and np.isnan(energy3).all() and np.array_equal(sums3, sim.integral_sums[7:12])
    plain = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", wake_integrals=True)
    assert np.array_equal(plain.integral_sums[1:12], sim.integral_sums[1:12])
    # on = 0 turns the observer off; ludvm_march_setup forgets it
    eng.march_set_integrals(False)
    assert _read(eng, 5)[0] == _ffi.E_STATE
