"""GPU tier of passive tracers in a sweep (ensemble_traced<PROBES>, ludvm_ensemble_run_traced): one set of seeds, paths for
every member, advected inside the one launch -- against the oracle, against solo marched runs on the same engine, at the
tracer counts where the kernel changes path, passive on every other result, independent of the batch, consistent with the
probe rows, and with the context left alone.  Bounds are the ones tests/test_gpu_tracers.py uses for the same comparisons on
the solo march."""
import ctypes
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from probes_common import probes32
from tracers_common import TracedOracle, gust_cloud, path_error, releases_1_7_50, releases_by_tile, seeds37, seeds_random

pytestmark = pytest.mark.gpu

TILE = 256          # kBlock of ensemble_kernels.hpp: tracers go in tiles of 256, one per lane
# A member against its solo precision='f64' marched run [MI355X], 300 tracers (a tile of 256 on the per-lane walk and one of 44
# on the sliced one), config 1's first 100 steps: 1e-12 of the largest displacement asserted over steps 1-10 (measured
# SOLO_1_10_MEASURED); up to step 100 measured SOLO_1_100_MEASURED (the two kernels sum the same pairs in different orders
# and the difference grows with the run): 10x the measured value is the bound, never above 1e-7.
SOLO_1_10_MEASURED = 0.0         # (the same bits: one source tile, the same order of summation)
SOLO_1_100_MEASURED = 6.14e-12
SOLO_1_100_BOUND = 10 * SOLO_1_100_MEASURED
assert SOLO_1_100_BOUND <= 1e-7

EDGE_M = (1, 64, 65, 85, 86, 128, 129, 256, 257, 513, 4096)


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


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_member_paths_match_the_oracle(eng, frame):
    """'Faure', 'Ramesh' and the free-vortex cloud of G5 as the members of one sweep, the 37 seeds released at steps 1, 7 and
    50: steps 1-50 at 1e-9 of the largest displacement against TracedOracle (the solo march measures 1.5e-15); row 0 is the
    seeds, held tracers sit exactly on the seed of their step."""
    from ludvm_amd import sweep
    seeds, rel = seeds37(), releases_1_7_50(37)
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2.5, method="Ramesh"), dict(CONFIG1, tf=2.5, **gust_cloud())]
    sims = sweep(cases, engine=eng, particles=seeds, particle_release=rel, particle_frame=frame, particle_steps=range(1, 51))
    for m, (kw, sim) in enumerate(zip(cases, sims)):
        ref = TracedOracle(seeds, release=rel, shift=(lambda o: o.xpiv) if frame == "tunnel" else None, **kw)
        assert sim.nt == 51 and sim.tracer_path.steps() == list(range(51)) and sim.tracer_path[50].shape == (2, 37)
        err = path_error(sim.tracer_path, ref, 1, 50)
        print(f"member {m} ({frame}): tracer paths vs oracle, steps 1-50: {err:.2e} of the largest displacement")
        assert err <= 1e-9, (m, err)
        assert np.array_equal(sim.tracer_path[0], ref.seeds_at(0)) and np.array_equal(sim.tracer_last, sim.tracer_path[50])
        assert np.array_equal(sim.tracer_xz, seeds) and np.array_equal(sim.tracer_release, rel) and sim.tracer_frame == frame
        for s in (1, 6, 7, 49):
            still = rel > s
            assert np.array_equal(sim.tracer_path[s][:, still], ref.seeds_at(s)[:, still]), (m, s)
            assert np.array_equal(sim.tracer_released(s), ~still)
    assert not np.array_equal(sims[0].tracer_path[50], sims[2].tracer_path[50])          # (the cloud moves them differently)


def _solo_error(sim, solo, first, last):
    steps = range(first, last + 1)
    worst = max(np.abs(sim.tracer_path[s] - solo.tracer_path[s]).max() for s in steps)
    disp = max(np.abs(solo.tracer_path[s] - solo._tracer_seeds(s)).max() for s in steps)
    assert disp > 0.0
    return worst / disp


def test_a_member_against_its_solo_march_on_the_same_engine(eng):
    """A member and its solo precision='f64' run with the same 300 tracers (tunnel frame, releases 1 / 7 / 50; config 1's
    first 100 steps, so n + npan passes 256: more than one source tile): 1e-12 of the largest displacement over steps 1-10,
    SOLO_1_100_BOUND up to step 100."""
    from ludvm_amd import LUDVM, sweep
    seeds, rel = seeds_random(300), releases_1_7_50(300)
    kw = dict(CONFIG1, tf=5)
    sim = sweep([dict(CONFIG1, tf=2, method="Ramesh"), kw], engine=eng, particles=seeds, particle_release=rel, particle_frame="tunnel",
                particle_steps=range(1, 101))[1]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", tracers=seeds, tracer_release=rel,
                 tracer_frame="tunnel", tracer_steps=range(1, 101))
    e10, e100 = _solo_error(sim, solo, 1, 10), _solo_error(sim, solo, 1, 100)
    print(f"sweep member vs solo march: tracer paths, steps 1-10 {e10:.2e}, steps 1-100 {e100:.2e} of the largest displacement")
    assert np.array_equal(sim.tracer_path[0], solo.tracer_path[0])
    assert e10 <= 1e-12, e10
    assert e100 <= SOLO_1_100_BOUND, e100
    held = rel > 100
    assert not held.any() and np.array_equal(sim.tracer_path[49][:, rel == 50], solo._tracer_seeds(49)[:, rel == 50])


@pytest.fixture(scope="module")
def oracle30():
    """TracedOracle over 30 steps (tunnel frame) for 3 x 1021 tracers: 1021 seeds, each released at step 1, at step 5 and never
    (the construction of tests/test_gpu_tracers.py)."""
    base = seeds_random(1021, seed=17)
    seeds = np.concatenate([base, base, base], axis=1)
    rel = np.repeat(np.array([1, 5, 10 ** 6], dtype=np.int64), 1021)
    rows = TracedOracle(seeds, release=rel, shift=lambda o: o.xpiv, **dict(CONFIG1, tf=1.5)).path_rows()
    rows.setflags(write=False)
    return base, rows


@pytest.mark.parametrize("M", EDGE_M)
def test_edge_tracer_counts(eng, oracle30, M):
    """M on both sides of 4 -> 3 (64 | 65), 3 -> 2 (85 | 86) and 2 -> 1 (128 | 129: the sliced-to-per-lane switch) lanes per
    tracer and of one tile to two and three (256 | 257, 513), the ends 1 and 4096.  30 steps in the tunnel frame as member 1 of
    two (its kin_off is 21), releases by tile of 256: tile 0, 3, ... free from step 1, tile 1, 4, ... mixed (step 1, step 5,
    never: lane by lane), tile 2, 5, ... wholly held (skipped).  Against the one oracle run of 3 x 1021 tracers at 1e-9 of the
    largest displacement; held tracers equal seed + shift exactly."""
    from ludvm_amd import sweep
    base, rows = oracle30
    m = np.arange(M)
    seeds = base[:, m % 1021]
    rel = releases_by_tile(M, TILE)
    col = np.searchsorted([1, 5, 10 ** 6], rel) * 1021 + m % 1021
    keep = [1, 4, 5, 6, 30]
    sims = sweep([dict(CONFIG1, tf=1, method="Ramesh"), dict(CONFIG1, tf=1.5)], engine=eng, particles=seeds, particle_release=rel,
                 particle_frame="tunnel", particle_steps=keep)
    short, sim = sims
    assert sim.tracer_path.steps() == [0] + keep and sim.tracer_path[30].shape == (2, M)
    assert short.tracer_path.steps() == [0, 1, 4, 5, 6] and short.tracer_last.shape == (2, M) and np.isfinite(short.tracer_last).all()
    seed30 = sim._tracer_seeds(30)
    disp = np.abs(rows[30][:, col] - seed30).max()
    worst = max(np.abs(sim.tracer_path[s] - rows[s][:, col]).max() for s in [0] + keep)
    print(f"M = {M}: {worst / disp:.2e} of the largest displacement ({disp:.3f})")
    assert worst <= 1e-9 * disp, worst / disp
    for s in keep:
        held = rel > s
        assert np.array_equal(sim.tracer_path[s][:, held], sim._tracer_seeds(s)[:, held]), s
    held = rel > 30
    assert np.abs(sim.tracer_path[30] - seed30)[:, ~held].min(axis=0).max() > 0.0
    if M > 2 * TILE:
        assert held[2 * TILE:min(M, 3 * TILE)].all() and not held[:TILE].any()
    assert np.array_equal(sim.tracer_last, sim.tracer_path[30])
    assert np.array_equal(short.tracer_last[:, rel > 20], short._tracer_seeds(20)[:, rel > 20])


class _Raw:
    """Keeps what the engine's three ensemble calls return."""
    NAMES = ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced")

    def __init__(self, eng):
        self.eng, self.out = eng, []
        for name in self.NAMES:
            inner = getattr(eng, name)

            def kept(*a, _inner=inner, _name=name, **k):
                res = _inner(*a, **k)
                self.out.append((_name, a[7], res, a))
                return res
            setattr(eng, name, kept)

    def close(self):
        for name in self.NAMES:
            delattr(self.eng, name)


def _same_raw(x, y, nsnap):
    """rows, wake_n and the filled part of every wake record of two ensemble calls, bit for bit."""
    (_, desc, a, _), (_, _, b, _) = x, y
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for m in range(desc.shape[0]):
        nt, _, nf, _, _, w0 = (int(v) for v in desc[m])
        cap = nf + 2 * (nt - 1)
        for r in range(nsnap + 1):
            n = int(a[2][m, r])
            for q in range(3):
                at = w0 + (3 * r + q) * cap
                assert n < 0 or np.array_equal(a[1][at:at + n], b[1][at:at + n]), (m, r, q)


def test_particles_are_passive(eng):
    """The same sweep without particles, with 300, and with 300 and 85 probes against the probes alone: loads, Fourier
    coefficients, every circulation, LEV_shed, the snapshot rows, the sizes of the wake records and the probe rows are the same
    arrays, bit for bit -- and so is everything ludvm_ensemble_run_traced returns with ntracer = 0 against
    ludvm_ensemble_run_probed."""
    from ludvm_amd import sweep
    cases = [dict(CONFIG1, tf=5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=6.5, alpha_m=5, alpha_max=15),
             dict(CONFIG1, tf=5, **gust_cloud())]
    snaps = (1, 2, 10, 50)
    pts = np.concatenate([probes32(), probes32()[:, ::-1] + 0.37, probes32()[:, :21] - 0.11], axis=1)
    seeds, rel = seeds_random(300), np.array([1, 40, 90, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    part = dict(particles=seeds, particle_release=rel, particle_frame="tunnel")
    raw = _Raw(eng)
    try:
        plain = sweep(cases, engine=eng, snapshot_steps=snaps)
        traced = sweep(cases, engine=eng, snapshot_steps=snaps, **part)
        probed = sweep(cases, engine=eng, snapshot_steps=snaps, probes=pts, probe_frame="tunnel")
        both = sweep(cases, engine=eng, snapshot_steps=snaps, probes=pts, probe_frame="tunnel", **part)
        shift = np.concatenate([s.xpiv for s in plain])
        eng.ensemble_run_traced(*raw.out[0][3], seed_x=[], seed_z=[], release=[], probe_x=pts[0], probe_z=pts[1], probe_shift_x=shift)
    finally:
        raw.close()
    assert [o[0] for o in raw.out] == ["ensemble_run", "ensemble_run_traced", "ensemble_run_probed", "ensemble_run_traced",
                                       "ensemble_run_traced"]
    for k in range(1, 5):
        _same_raw(raw.out[0], raw.out[k], len(snaps))
    pu, pw = raw.out[2][2][3], raw.out[2][2][4]
    assert pu.shape == (sum(s.nt for s in plain), 85) and np.abs(pw).max() > 0.0
    for k in (3, 4):                         # (rows, wakes, wake_n, tracer_rows, probe_u, probe_w)
        assert np.array_equal(raw.out[k][2][4], pu) and np.array_equal(raw.out[k][2][5], pw), k
    assert raw.out[4][2][3].shape == (4, 1, 2, 0)
    assert np.array_equal(raw.out[1][2][3], raw.out[3][2][3])            # (the paths do not depend on the probes either)
    for m, (a, b, c, d) in enumerate(zip(plain, traced, probed, both)):
        assert not hasattr(a, "tracer_path") and not hasattr(c, "tracer_path") and not hasattr(b, "probe_u")
        assert b.tracer_path.steps() == sorted({0, b.nt - 1} | {s for s in snaps if s <= b.nt - 1})
        last = b.nt - 1
        moved = np.abs(b.tracer_last - b._tracer_seeds(last))
        assert np.isfinite(b.tracer_last).all() and moved[:, rel <= 40].min(axis=0).max() > 0.0 and not moved[:, rel > last].any()
        assert np.array_equal(c.probe_u, d.probe_u) and np.array_equal(c.probe_w, d.probe_w)
        for other in (b, c, d):
            for name in ("Cl", "Cd", "Cm", "Fn", "Fs", "M", "LESP", "LESP_prev", "LEV_shed", "fourier"):
                assert np.array_equal(getattr(a, name), getattr(other, name)), (m, name)
            assert (a.nt, a.itev, a.ilev) == (other.nt, other.itev, other.ilev) and set(a.circulation) == set(other.circulation)
            for key in a.circulation:
                assert np.array_equal(a.circulation[key], other.circulation[key]), (m, key)
            for key in ("TEV", "LEV", "FREE"):
                assert a.path[key].steps() == other.path[key].steps()
                for s in a.path[key].steps():
                    assert np.array_equal(a.path[key][s], other.path[key][s]), (m, key, s)
        for s in b.tracer_path.steps():
            assert np.array_equal(b.tracer_path[s], d.tracer_path[s]), (m, s)


def test_path_bits_do_not_depend_on_the_batch_and_repeat(eng):
    """A member's paths alone, at index 0 and at index 39 of 40 members, and in a second call: the same bits."""
    from ludvm_amd import sweep
    seeds, rel = seeds_random(300), np.array([1, 40, 90, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    X = dict(CONFIG1, tf=5)
    others = [dict(CONFIG1, tf=3 + (q % 5), LESPcrit=0.1 + 0.01 * (q % 17), alpha_max=5 + (q % 11),
                   method="Ramesh" if q % 7 == 0 else "Faure") for q in range(38)]
    kw = dict(engine=eng, particles=seeds, particle_release=rel, particle_frame="tunnel", particle_steps=[1, 39, 40, 41, 90, 100])
    alone = sweep([X], **kw)[0]
    first = sweep([X] + others + [X], **kw)
    again = sweep([X] + others + [X], **kw)
    assert len(first) == 40 and alone.tracer_path.steps() == [0, 1, 39, 40, 41, 90, 100]
    assert np.abs(alone.tracer_path[100] - alone._tracer_seeds(100))[:, rel <= 90].min(axis=0).max() > 0.0
    for other in (first[0], first[39]):
        assert other.tracer_path.steps() == alone.tracer_path.steps() and np.array_equal(alone.tracer_last, other.tracer_last)
        for s in alone.tracer_path.steps():
            assert np.array_equal(alone.tracer_path[s], other.tracer_path[s]), s
    for a, b in zip(first, again):
        assert a.tracer_path.steps() == b.tracer_path.steps() and np.array_equal(a.tracer_last, b.tracer_last)
        for s in a.tracer_path.steps():
            assert np.array_equal(a.tracer_path[s], b.tracer_path[s]), s
    assert not np.array_equal(first[1].tracer_path[39], first[2].tracer_path[39])      # (the other members are different cases)
    short = [s for s in first if s.nt - 1 < 90]
    assert short and all(s.tracer_path.steps() == [0, 1, 39, 40, 41] for s in short)      # (no row for a step a member has not)


def test_first_free_step_is_the_probe_value(eng):
    """A tracer released at step r from a lab-frame seed that is also a probe of the same sweep: (position after r - seed) /
    dt is the member's probe_u[r], probe_w[r] at that point, 1e-12 of max|u| -- r = 5 and r = 30, a 'Faure' and a 'Ramesh'
    member."""
    from ludvm_amd import sweep
    seeds = seeds37()
    rel = np.array([5, 30], dtype=np.int64)[np.arange(37) % 2]
    sims = sweep([dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh")], engine=eng, particles=seeds, particle_release=rel,
                 probes=seeds, particle_steps=[4, 5, 29, 30])
    for m, sim in enumerate(sims):
        assert np.array_equal(sim.tracer_path[4], seeds) and np.array_equal(sim.tracer_path[29][:, rel == 30], seeds[:, rel == 30])
        for r in (5, 30):
            k = rel == r
            u = (sim.tracer_path[r][0, k] - seeds[0, k]) / sim.dt
            w = (sim.tracer_path[r][1, k] - seeds[1, k]) / sim.dt
            scale = max(np.abs(sim.probe_u[r]).max(), np.abs(sim.probe_w[r]).max())
            err = max(np.abs(u - sim.probe_u[r, k]).max(), np.abs(w - sim.probe_w[r, k]).max()) / scale
            print(f"member {m}, release step {r}: first free step vs probe row: {err:.2e} of max|u|")
            assert err <= 1e-12, (m, r, err)


def _arrays(members, npan=80, ncoef=30, nt=3):
    T = 8 * npan + ncoef * npan + (ncoef - 1) * npan
    scalars = np.ones([members, 12])
    scalars[:, 8:] = 0.0
    desc = np.array([[nt, m * nt, 1, m, m * (nt - 1), m * 3 * (1 + 2 * (nt - 1))] for m in range(members)], dtype=np.int64)
    return (npan, ncoef, scalars, np.zeros([members, T]), np.zeros([members * nt, 7 + 2 * npan]), np.zeros([members, 8 + ncoef]),
            np.zeros(3 * members), desc)


def test_the_library_answers_the_documented_codes_and_leaves_the_context_alone(eng):
    """What ludvm_ensemble_run_traced refuses on the host (LUDVM_E_ARG) launches nothing; a traced sweep leaves the resident
    wake and the state of a march -- tracers of its own included -- as they were."""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    cases = [dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=5, alpha_m=5, alpha_max=15)]
    seeds, rel = seeds37(), releases_1_7_50(37)
    part = dict(engine=eng, particles=seeds[:, ::-1] + 0.25, particle_release=rel, particle_frame="tunnel")

    # a hand-placed resident wake
    rng = np.random.default_rng(3)
    x, z, g = rng.uniform(-3, 0, 500), rng.uniform(-1, 1, 500), rng.standard_normal(500)
    eng.wake_clear()
    eng.wake_append(x, z, g)
    sweep(cases, snapshot_steps=(3,), **part)

    packed = _arrays(2)
    one = dict(seed_x=[0.0], seed_z=[0.0], release=[1])
    for word, kw in (("at most", dict(seed_x=np.zeros(4097), seed_z=np.zeros(4097), release=np.ones(4097, dtype=np.int64))),
                     ("one per kinematics row", dict(one, shift_x=np.zeros(5))),
                     ("finite", dict(seed_x=[0.0, np.inf], seed_z=[0.0, 0.0], release=[1, 1])),
                     ("finite", dict(seed_x=[0.0, 1.0], seed_z=[np.nan, 0.0], release=[1, 1])),
                     ("finite", dict(one, shift_x=[0.0, 0.0, np.inf, 0.0, 0.0, 0.0])),
                     (">= 1", dict(seed_x=[0.0, 1.0], seed_z=[0.0, 0.0], release=[1, 0])),
                     ("strictly increasing", dict(one, record_steps=[2, 2])),
                     ("strictly increasing", dict(one, record_steps=[2, 1])),
                     ("strictly increasing", dict(one, record_steps=[0, 1]))):
        with pytest.raises(LudvmHipError) as e:
            eng.ensemble_run_traced(*packed, **kw)
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))
    # tracer_doubles too small, a null record array, records over 1 GiB
    from ludvm_amd.engine import _pd
    npan, ncoef, sc, tb, kin, ini, fr, desc = packed
    pll = ctypes.POINTER(ctypes.c_longlong)
    rows, wakes, wake_n = np.zeros([4, 12 + 2 * ncoef + 2 * npan]), np.zeros(30), np.zeros([2, 1], dtype=np.int64)
    sx, r1, trows = np.zeros(4), np.ones(4, dtype=np.int64), np.zeros([2, 1, 2, 4])

    def call(tr, tdoubles, ntrec=0, trec=None):
        return eng._lib.ludvm_ensemble_run_traced(eng._ctx, 2, npan, ncoef, _pd(sc), sc.size, _pd(tb), _pd(kin), 6, _pd(ini), _pd(fr), 2,
                                                  desc.ctypes.data_as(pll), None, 0, _pd(rows), 4, _pd(wakes), 30,
                                                  wake_n.ctypes.data_as(pll), None, None, 0, None, 0, None, None, _pd(sx), _pd(sx),
                                                  r1.ctypes.data_as(pll), 4, None, 0, trec, ntrec, tr, tdoubles)
    def last_error():
        return eng._lib.ludvm_last_error(eng._ctx).decode()
    assert call(_pd(trows), trows.size - 1) == _ffi.E_ARG and "outside the array" in last_error()
    assert call(None, trows.size) == _ffi.E_ARG
    many = np.arange(1, 2 ** 23 + 1, dtype=np.int64)                      # 2 members x (2^23 + 1) records x 64 bytes > 1 GiB
    assert call(_pd(trows), trows.size, len(many), many.ctypes.data_as(pll)) == _ffi.E_ARG and "1 GiB" in last_error()
    assert not rows.any() and not trows.any()
    assert eng.wake_size() == 500
    xr, zr, gr = eng.wake_read(0, 500, gamma=True)
    assert np.array_equal(xr, x) and np.array_equal(zr, z) and np.array_equal(gr, g)

    # a traced sweep between two march_run calls of a chunked solo run that has tracers of its own
    class Chunked(LUDVM):
        _march_chunk = 96
        between = None

        def _march_call(self, S, i, j, rec_i, print_dt):
            super()._march_call(S, i, j, rec_i, print_dt)
            if self.between is not None and j < self.nt:
                self.between()

    def chunked(between):
        Chunked.between = staticmethod(between) if between else None
        s = Chunked(**CONFIG1, verbose=False, engine=eng, precision="f32", history="sparse", tracers=seeds, tracer_release=rel,
                    tracer_steps=[50, 100, 200, 400])
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.path["LEV"][s.nt - 1], s.tracer_last] + \
               [s.tracer_path[q] for q in (50, 100, 200, 400)]
    count = []
    plain = chunked(None)
    mixed = chunked(lambda: count.append(len(sweep(cases, **part))))
    assert len(count) >= 3
    assert all(np.array_equal(a, b) for a, b in zip(plain, mixed))
    sim = sweep([dict(CONFIG1, tf=1)], **part)[0]               # a following sweep works
    assert sim.tracer_last.shape == (2, 37) and np.isfinite(sim.tracer_last).all()


def test_a_sharded_context_answers_e_state():
    """ludvm_ensemble_run_traced on a context sharded through ludvm_set_shard: LUDVM_E_STATE, nothing launched (the hook is
    never called)."""
    import torch
    from ludvm_amd import Engine, LudvmHipError, _ffi
    called = []
    other = Engine(0)
    try:
        acc = torch.zeros([64], dtype=torch.int64, device=torch.device("cuda", other.device))
        other.set_shard(0, 2, lambda count, stream: called.append(count), acc.data_ptr(), 64 * 8)
        with pytest.raises(LudvmHipError) as e:
            other.ensemble_run_traced(*_arrays(2), seed_x=[0.0], seed_z=[0.0], release=[1])
        assert e.value.code == _ffi.E_STATE and "sharded" in str(e.value) and not called
        other.set_shard(0, 1)
    finally:
        other.close()
