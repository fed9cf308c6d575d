"""GPU tier of the wake survey in a sweep (ensemble_surveyed<PROBES, TRACERS>, ludvm_ensemble_run_surveyed): one set of points,
the five raw sums of every member accumulated inside the one launch -- against the oracle, against the probe rows of the same
launch, at the point counts where the kernel changes path, against solo marched runs on the same engine, passive on every
other result, independent of the batch, with members of unequal length, over many source tiles, and with the context left
alone.  Bounds are survey_common.py's, the ones tests/test_gpu_survey.py uses for the same comparisons on the solo march."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import case_keywords as source_case_keywords
from probes_common import ProbedOracle, probes32
from survey_common import (MEAN_VS_ORACLE, MEAN_VS_PROBES, MOMENT_VS_ORACLE, MOMENT_VS_PROBES, case_keywords, check_derived,
                           oracle_series, series_sums, series_umax, sums_errors, window)
from tracers_common import gust_cloud, seeds37, seeds_random

pytestmark = pytest.mark.gpu

TILE = 256          # kBlock of ensemble_kernels.hpp: points go in tiles of 256, one per lane
# A member against its solo precision='f64' marched run [MI355X], 300 points (a tile of 256 on the per-lane walk and one of 44
# on the sliced one), config 1's first 100 steps: means 1e-12 of max|u| and raw second moments 3e-12 of max|u|^2 asserted over
# the window 1-10; over the window 1-100 measured SOLO_1_100_MEASURED (the two kernels sum the same pairs in different orders
# and the difference grows with the run): 10x the measured values are the bounds, never above 1e-7 / 3e-7.
SOLO_1_100_MEASURED = (7.23e-15, 3.50e-15)         # (means of max|u|, raw second moments of max|u|^2; window 1-10: 4.1e-17, 5.7e-17)
SOLO_1_100_BOUND = tuple(10 * v for v in SOLO_1_100_MEASURED)
assert SOLO_1_100_BOUND[0] <= 1e-7 and SOLO_1_100_BOUND[1] <= 3e-7

EDGE_K = (1, 64, 65, 85, 86, 128, 129, 256, 257, 513, 4096)


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
def test_member_sums_match_the_oracle(eng, frame):
    """'Faure', 'Ramesh' and the free-vortex cloud of G5 as the members of one sweep, probes32()'s points, every step of
    tf = 2.5: means at 1e-9 of max|u|, raw second moments at 3e-9 of max|u|^2 against the sums of ProbedOracle's series."""
    from ludvm_amd import sweep
    pts = probes32()
    members = [("Faure", False), ("Ramesh", False), ("Faure", True)]
    sims = sweep([case_keywords(m, c) for m, c in members], engine=eng, survey=pts, survey_frame=frame)
    for k, ((method, cloud), sim) in enumerate(zip(members, sims)):
        nt = sim.nt
        assert nt == 51 and sim.survey_count == 50 and sim.survey_steps == (1, 51, 1) and sim.survey_frame == frame
        ou, ow = oracle_series(pts, method, frame, cloud)
        steps = window(1, nt, 1, nt)
        ref, umax = series_sums(ou, ow, steps), series_umax(ou, ow, steps)
        e_mean, e_mom = sums_errors(sim.survey_sums, ref, 50, umax)
        print(f"member {k} ({method}, cloud={cloud}, {frame}): survey vs oracle, steps 1-50: means {e_mean:.2e} of max|u|, raw "
              f"second moments {e_mom:.2e} of max|u|^2")
        assert e_mean <= MEAN_VS_ORACLE, (k, e_mean)
        assert e_mom <= MOMENT_VS_ORACLE, (k, e_mom)
        assert np.array_equal(sim.survey_x, pts[0]) and np.array_equal(sim.survey_z, pts[1])
        check_derived(sim)
    assert not np.array_equal(sims[0].survey_sums, sims[2].survey_sums)           # (the cloud changes the field)


@pytest.mark.parametrize("steps", [(1, 51, 1), (7, 40, 3), (3, 1000, 2), (5, 30, 100), (40, 1000, 1)],
                         ids=["all", "7-40-3", "stop>nt", "every>window", "last-step-alone"])
def test_sums_are_the_reduction_of_the_probe_rows_of_the_same_launch(eng, steps):
    """The same points as `probes=` and `survey=` (tunnel frame) in a sweep of a 50-step 'Faure' and a 40-step 'Ramesh' member:
    the sums against the reduction of the member's own probe rows over its sampled steps -- means at 1e-12 of max|u|, raw second
    moments at 3e-12 of max|u|^2.  (40, 1000, 1) is the shorter member's last step alone.  Phase 2s forms (u, w) in
    ens_probe_row's order and the terms as series_sums does up to the fused multiply-add: measured [MI355X] exactly 0 for the
    means in every window and at most 3.2e-16 of max|u|^2 for the raw second moments."""
    from ludvm_amd import sweep
    pts = probes32()
    sims = sweep([dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh")], engine=eng, probes=pts, probe_frame="tunnel",
                 survey=pts, survey_frame="tunnel", survey_steps=steps)
    for k, sim in enumerate(sims):
        W = window(*steps, sim.nt)
        assert sim.nt == (51, 41)[k] and sim.survey_count == len(W) >= 1 and sim.survey_steps == (steps[0], min(steps[1], sim.nt), steps[2])
        ref, umax = series_sums(sim.probe_u, sim.probe_w, W), series_umax(sim.probe_u, sim.probe_w, W)
        e_mean, e_mom = sums_errors(sim.survey_sums, ref, len(W), umax)
        print(f"member {k}, window {steps}: survey vs the launch's own probe rows over {len(W)} steps: means {e_mean:.2e} of "
              f"max|u|, raw second moments {e_mom:.2e} of max|u|^2")
        assert e_mean <= MEAN_VS_PROBES, (k, e_mean)
        assert e_mom <= MOMENT_VS_PROBES, (k, e_mom)
        check_derived(sim)
    if steps == (40, 1000, 1):
        assert sims[1].survey_count == 1 and sims[0].survey_count == 11


@pytest.fixture(scope="module")
def oracle30():
    """ProbedOracle's series over 30 steps (tunnel frame) at 4096 points."""
    pts = seeds_random(4096, seed=17)
    u, w = ProbedOracle(pts, shift=lambda o: o.xpiv, **dict(CONFIG1, tf=1.5)).series()
    u.setflags(write=False); w.setflags(write=False); pts.setflags(write=False)
    return pts, u, w


@pytest.mark.parametrize("K", EDGE_K)
def test_edge_point_counts(eng, oracle30, K):
    """K on both sides of 4 -> 3 (64 | 65), 3 -> 2 (85 | 86) and 2 -> 1 (128 | 129: the sliced-to-per-lane switch) lanes per
    point and of one tile to two and three (256 | 257, 513), the ends 1 and 4096.  30 steps in the tunnel frame as member 1 of
    two (its kin_off is 21).  Every point against the one oracle series at the two oracle bounds."""
    from ludvm_amd import sweep
    pts, u, w = oracle30
    short, sim = sweep([dict(CONFIG1, tf=1, method="Ramesh"), dict(CONFIG1, tf=1.5)], engine=eng, survey=pts[:, :K], survey_frame="tunnel")
    assert sim.nt == 31 and sim.survey_count == 30 and short.survey_count == 20 and sim.survey_sums.shape == (5, K)
    steps = window(1, 31, 1, 31)
    ref, umax = series_sums(u[:, :K], w[:, :K], steps), series_umax(u[:, :K], w[:, :K], steps)
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, 30, umax)
    print(f"K = {K}: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE, e_mean
    assert e_mom <= MOMENT_VS_ORACLE, e_mom
    assert np.isfinite(short.survey_sums).all() and (short.survey_sums[2] > 0.0).all() and (sim.survey_sums[2:4] > 0.0).all()
    check_derived(sim)


def test_a_member_against_its_solo_march_on_the_same_engine(eng):
    """A member and its solo precision='f64' run with the same 300 points (tunnel frame; config 1's first 100 steps, so
    n + npan passes 256: more than one source tile): 1e-12 / 3e-12 over the window 1-10, SOLO_1_100_BOUND over 1-100.  The
    scale max|u| is that of the member's own probe rows at the same points."""
    from ludvm_amd import LUDVM, sweep
    pts = seeds_random(300)
    kw = dict(CONFIG1, tf=5)
    got = {}
    for name, steps in (("1-10", (1, 11, 1)), ("1-100", (1, 101, 1))):
        sim = sweep([dict(CONFIG1, tf=2, method="Ramesh"), kw], engine=eng, probes=pts, probe_frame="tunnel", survey=pts,
                    survey_frame="tunnel", survey_steps=steps)[1]
        solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel",
                     survey_steps=steps)
        W = window(*steps, sim.nt)
        assert sim.nt == 101 and sim.survey_count == solo.survey_count == len(W) and sim.survey_steps == solo.survey_steps
        got[name] = sums_errors(sim.survey_sums, solo.survey_sums, len(W), series_umax(sim.probe_u, sim.probe_w, W))
        print(f"sweep member vs solo march, window {name}: means {got[name][0]:.2e} of max|u|, raw second moments "
              f"{got[name][1]:.2e} of max|u|^2")
    assert got["1-10"][0] <= 1e-12 and got["1-10"][1] <= 3e-12, got
    assert got["1-100"][0] <= SOLO_1_100_BOUND[0] and got["1-100"][1] <= SOLO_1_100_BOUND[1], got


class _Raw:
    """Keeps what the engine's ensemble calls return."""
    NAMES = ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed")

    def __init__(self, eng):
        self.eng, self.out = eng, []
        for name in self.NAMES:
            inner = getattr(eng, name)

            def kept(*a, _inner=inner, _name=name, **k):
                res = _inner(*a, **k)
                self.out.append((_name, a[7], res))
                return res
            setattr(eng, name, kept)

    def close(self):
        for name in self.NAMES:
            delattr(self.eng, name)


def _same_raw(x, y, nsnap):
    """rows, wake_n and the filled part of every wake record of two ensemble calls, bit for bit."""
    (_, desc, a), (_, _, b) = x, y
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for m in range(desc.shape[0]):
        nt, _, nf, _, _, w0 = (int(v) for v in desc[m])
        cap = nf + 2 * (nt - 1)
        for r in range(nsnap + 1):
            n = int(a[2][m, r])
            for q in range(3):
                at = w0 + (3 * r + q) * cap
                assert n < 0 or np.array_equal(a[1][at:at + n], b[1][at:at + n]), (m, r, q)


def test_a_survey_is_passive(eng):
    """A sweep with 85 probes and 300 particles, with and without a survey of 300 points: rows, wake records, probe rows and
    tracer records as the engine returns them, and every member's loads, Fourier coefficients, circulations, LEV_shed, snapshot
    rows, probe rows and tracer paths are the same arrays, bit for bit; so is a sweep with the survey alone against the plain
    one."""
    from ludvm_amd import sweep
    cases = [dict(CONFIG1, tf=5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=6.5, alpha_m=5, alpha_max=15),
             dict(CONFIG1, tf=5, **gust_cloud())]
    snaps = (1, 2, 10, 50)
    rake = np.concatenate([probes32(), probes32()[:, ::-1] + 0.37, probes32()[:, :21] - 0.11], axis=1)
    seeds, rel = seeds_random(300), np.array([1, 40, 90, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    obs = dict(probes=rake, probe_frame="tunnel", particles=seeds, particle_release=rel, particle_frame="tunnel")
    sv = dict(survey=seeds_random(300, seed=9), survey_frame="tunnel", survey_steps=(5, 120, 3))
    raw = _Raw(eng)
    try:
        without = sweep(cases, engine=eng, snapshot_steps=snaps, **obs)
        with_ = sweep(cases, engine=eng, snapshot_steps=snaps, **obs, **sv)
        plain = sweep(cases, engine=eng, snapshot_steps=snaps)
        alone = sweep(cases, engine=eng, snapshot_steps=snaps, **sv)
    finally:
        raw.close()
    assert [o[0] for o in raw.out] == ["ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run", "ensemble_run_surveyed"]
    for k in (1, 2, 3):
        _same_raw(raw.out[0], raw.out[k], len(snaps))
    a, b = raw.out[0][2], raw.out[1][2]          # (rows, wakes, wake_n, tracer_rows, probe_u, probe_w[, survey_sums])
    assert len(a) == 6 and len(b) == 7 and b[6].shape == (4, 5, 300)
    for q in (3, 4, 5):
        assert np.array_equal(a[q], b[q]), q
    assert np.abs(a[3]).max() > 0.0 and np.abs(a[5]).max() > 0.0
    assert np.array_equal(b[6], raw.out[3][2][4])            # (the sums do not depend on the probes and tracers either)
    for m, (s0, s1, s2, s3) in enumerate(zip(without, with_, plain, alone)):
        assert not hasattr(s0, "survey_sums") and not hasattr(s2, "survey_sums") and not hasattr(s3, "probe_u")
        assert s1.survey_count == len(window(5, 120, 3, s1.nt)) and np.isfinite(s1.survey_sums).all() and (s1.survey_sums[2] > 0).all()
        assert np.array_equal(s1.survey_sums, s3.survey_sums)
        assert np.array_equal(s0.probe_u, s1.probe_u) and np.array_equal(s0.probe_w, s1.probe_w)
        assert s0.tracer_path.steps() == s1.tracer_path.steps() and np.array_equal(s0.tracer_last, s1.tracer_last)
        for s in s0.tracer_path.steps():
            assert np.array_equal(s0.tracer_path[s], s1.tracer_path[s]), (m, s)
        for other in (s1, s2, s3):
            for name in ("Cl", "Cd", "Cm", "Fn", "Fs", "M", "LESP", "LESP_prev", "LEV_shed", "fourier"):
                assert np.array_equal(getattr(s0, name), getattr(other, name)), (m, name)
            assert (s0.nt, s0.itev, s0.ilev) == (other.nt, other.itev, other.ilev) and set(s0.circulation) == set(other.circulation)
            for key in s0.circulation:
                assert np.array_equal(s0.circulation[key], other.circulation[key]), (m, key)
            for key in ("TEV", "LEV", "FREE"):
                assert s0.path[key].steps() == other.path[key].steps()
                for s in s0.path[key].steps():
                    assert np.array_equal(s0.path[key][s], other.path[key][s]), (m, key, s)


def test_sums_do_not_depend_on_the_batch_and_repeat(eng):
    """A member's sums alone, at index 0 and at index 39 of 40 members, and in a second call: the same bits."""
    from ludvm_amd import sweep
    X = dict(CONFIG1, tf=5)
    others = [dict(CONFIG1, tf=3 + (q % 5), LESPcrit=0.1 + 0.01 * (q % 17), alpha_max=5 + (q % 11),
                   method="Ramesh" if q % 7 == 0 else "Faure") for q in range(38)]
    kw = dict(engine=eng, survey=seeds_random(300), survey_frame="tunnel", survey_steps=(5, 90, 4))
    alone = sweep([X], **kw)[0]
    first = sweep([X] + others + [X], **kw)
    again = sweep([X] + others + [X], **kw)
    assert len(first) == 40 and alone.survey_count == 22 and (alone.survey_sums[2] > 0.0).all()
    for other in (first[0], first[39]):
        assert other.survey_count == 22 and np.array_equal(alone.survey_sums, other.survey_sums)
    for a, b in zip(first, again):
        assert a.survey_count == b.survey_count and np.array_equal(a.survey_sums, b.survey_sums)
    assert not np.array_equal(first[1].survey_sums, first[2].survey_sums)          # (the other members are different cases)


def test_members_of_unequal_length_sample_their_own_steps(eng):
    """tf = 1, 2.5 and 5 under the window (5, 60, 4): each member's count is the number of the window's steps it has, and the
    short member's sums are those of a sweep holding it alone."""
    from ludvm_amd import sweep
    pts = seeds37()
    cases = [dict(CONFIG1, tf=1), dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=5)]
    kw = dict(engine=eng, survey=pts, survey_steps=(5, 60, 4))
    sims = sweep(cases, **kw)
    assert [s.nt for s in sims] == [21, 51, 101]
    for sim in sims:
        assert sim.survey_count == len(window(5, 60, 4, sim.nt)) and sim.survey_steps == (5, min(60, sim.nt), 4)
        check_derived(sim)
    assert [s.survey_count for s in sims] == [4, 12, 14]
    short = sweep(cases[:1], **kw)[0]
    assert short.survey_count == 4 and np.array_equal(short.survey_sums, sims[0].survey_sums)
    assert not np.array_equal(sims[1].survey_sums, sims[2].survey_sums)


def test_many_source_tiles(eng):
    """A member with 1180 free vortices (five 256-source tiles from its first step on; observer_sources_common.py's case A)
    behind another member, 600 points (two per-lane tiles and a sliced one of 88), every one of its 24 steps: against the
    oracle at the oracle bounds."""
    from ludvm_amd import sweep
    pts = seeds_random(600)
    kw = source_case_keywords("A")
    sim = sweep([dict(CONFIG1, tf=1), kw], engine=eng, survey=pts)[1]
    assert sim.nt == 25 and sim.survey_count == 24 and sim.n_freevort == 1180
    ou, ow = ProbedOracle(pts, **kw).series()
    steps = window(1, 25, 1, 25)
    ref, umax = series_sums(ou, ow, steps), series_umax(ou, ow, steps)
    e_mean, e_mom = sums_errors(sim.survey_sums, ref, 24, umax)
    print(f"1180 free vortices, 600 points: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE, e_mean
    assert e_mom <= MOMENT_VS_ORACLE, e_mom


def _arrays(members, npan=80, ncoef=30, nt=3):
    T = 8 * npan + ncoef * npan + (ncoef - 1) * npan
    scalars = np.ones([members, 12])
    scalars[:, 8:] = 0.0
    desc = np.array([[nt, m * nt, 1, m, m * (nt - 1), m * 3 * (1 + 2 * (nt - 1))] for m in range(members)], dtype=np.int64)
    return (npan, ncoef, scalars, np.zeros([members, T]), np.zeros([members * nt, 7 + 2 * npan]), np.zeros([members, 8 + ncoef]),
            np.zeros(3 * members), desc)


def test_the_library_answers_the_documented_codes_and_leaves_the_context_alone(eng):
    """What ludvm_ensemble_run_surveyed refuses on the host (LUDVM_E_ARG) launches nothing; a solo marched run with a survey of
    its own gives the same results before and after a surveyed sweep on the same engine, the resident wake of the first is
    still there after the sweep, and ensemble_limits() is unchanged."""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    pts = seeds37()

    def solo():
        s = LUDVM(**dict(CONFIG1, tf=3), verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel",
                  survey_steps=(3, 55, 2))
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.survey_sums, np.array(s.survey_count)]
    limits = eng.ensemble_limits()
    before = solo()
    size = eng.wake_size()
    wake = eng.wake_read(0, size, gamma=True) if size else ()
    sims = sweep([dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=5, alpha_m=5, alpha_max=15)], engine=eng, snapshot_steps=(3,),
                 survey=pts[:, ::-1] + 0.25, survey_frame="tunnel", probes=pts, particles=pts)
    assert all(np.isfinite(s.survey_sums).all() and s.survey_count == s.nt - 1 for s in sims)

    packed = _arrays(2)
    one = dict(survey_x=[0.0], survey_z=[0.0], survey_steps=(1, 3, 1))
    for word, kw in (("at most", dict(one, survey_x=np.zeros(4097), survey_z=np.zeros(4097))),
                     ("one per kinematics row", dict(one, survey_shift_x=np.zeros(5))),
                     ("finite", dict(one, survey_x=[0.0, np.inf], survey_z=[0.0, 0.0])),
                     ("finite", dict(one, survey_x=[0.0, 1.0], survey_z=[np.nan, 0.0])),
                     ("finite", dict(one, survey_shift_x=[0.0, 0.0, np.inf, 0.0, 0.0, 0.0])),
                     ("first >= 1", dict(one, survey_steps=(0, 3, 1))),
                     ("every >= 1", dict(one, survey_steps=(1, 3, 0)))):
        with pytest.raises(LudvmHipError) as e:
            eng.ensemble_run_surveyed(*packed, **kw)
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))

    assert eng.wake_size() == size and eng.ensemble_limits() == limits
    for a, b in zip(wake, eng.wake_read(0, size, gamma=True) if size else ()):
        assert np.array_equal(a, b)
    after = solo()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
