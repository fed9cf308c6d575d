"""GPU tier of the phase-locked wake survey in a sweep (ensemble_binned<PROBES, TRACERS>, ludvm_ensemble_run_surveyed_binned;
DESIGN.md section 4.19): every member's bin sums accumulated inside the one launch -- against the step-ordered reduction of the
launch's own probe rows, bit for bit against plain surveys of each bin's steps, passive on every other result, independent of
the batch, against the solo marched run with survey_bins, at the edges, and with the context left alone.

Bounds.  The bin means against the probe rows are asserted EXACTLY: phase 2s forms (u, w) with the bits of a probe row at the
same points and the lane that owns a point adds them in step order, which is what a sequential NumPy sum does.  The raw second
moments are fused multiply-adds where NumPy rounds the product first: 3e-12 of max|u|^2 per sample, survey_common.py's bound,
the one tests/test_gpu_ensemble_survey.py uses.  A member against its solo float64 march over steps 1-10: 1e-12 of max|u| and
3e-12 of max|u|^2, the bounds of that file's solo comparison.  Measured [MI355X]: the products against the probe rows at most
1.9e-16 of max|u|^2; the member against its solo march 9.0e-15 of max|u| and 6.4e-15 of max|u|^2; K = 4096, bin 0 + bin 1
against the plain sums 2.6e-16 / 1.9e-16; the 63 tests take 1.3 s."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import case_keywords as source_case_keywords
from probes_common import probes32
from survey_bins_common import check_bin_derived
from survey_common import MOMENT_VS_PROBES, check_derived, series_sums, series_umax, window
from tracers_common import gust_cloud, seeds_random

pytestmark = pytest.mark.gpu

PI = np.pi


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


def four_members():
    """'Faure', 'Ramesh', G5's free-vortex cloud and a member of another k (a period of 20 steps), 50 / 40 / 50 / 50 steps."""
    return [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=2.5, **gust_cloud()),
            dict(CONFIG1, tf=2.5, k=2 * PI)]


def check_bins_are_the_reduction_of_the_probe_rows(sim, label):
    """Every bin block against the sequential sum, in step order, of the member's own probe rows (probes at the survey's
    points) over that bin's steps: sum u and sum w exactly, the three products at MOMENT_VS_PROBES of max|u|^2 per sample; an
    empty bin holds zeros; the counts are the table's."""
    table, B = sim.survey_bin_of_step, sim.survey_nbins
    K = sim.probe_u.shape[1]
    sums = sim.survey_bin_sums.reshape(B, 5, K)
    sampled = [int(i) for i in np.flatnonzero(table >= 0)]
    umax = series_umax(sim.probe_u, sim.probe_w, sampled)
    worst = 0.0
    for b in range(B):
        W = [int(i) for i in np.flatnonzero(table == b)]
        assert sim.survey_bin_count[b] == len(W), (label, b)
        ref = series_sums(sim.probe_u, sim.probe_w, W)
        assert np.array_equal(sums[b, :2], ref[:2]), (label, b, np.abs(sums[b, :2] - ref[:2]).max())
        if W:
            worst = max(worst, np.abs(sums[b, 2:] - ref[2:]).max() / len(W) / umax ** 2)
        else:
            assert not sums[b].any(), (label, b)
    print(f"{label}: bins vs the launch's own probe rows: means exact, raw second moments {worst:.2e} of max|u|^2")
    assert worst <= MOMENT_VS_PROBES, (label, worst)


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
@pytest.mark.parametrize("steps", [(1, 51, 1), (7, 40, 3), (3, 1000, 2)], ids=["all", "7-40-3", "stop>nt"])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("K", [1, 129, 257])
def test_bin_sums_are_the_step_ordered_reduction_of_the_launchs_own_probe_rows(eng, K, B, steps, frame):
    """K = 1: a sliced tile; 129: a per-lane tile; 257: two tiles.  survey_phases=B bins every member by its own period (200 steps
    for config 1, 20 for the member with k = 2 pi), so the tables differ under one B."""
    from ludvm_amd import sweep
    pts = seeds_random(K, seed=11)
    sims = sweep(four_members(), engine=eng, probes=pts, probe_frame=frame, survey=pts, survey_frame=frame, survey_steps=steps,
                 survey_phases=B)
    assert [s.nt for s in sims] == [51, 41, 51, 51]
    for m, sim in enumerate(sims):
        W = window(*steps, sim.nt)
        assert sim.survey_nbins == B and sim.survey_count == len(W) == sim.survey_bin_count.sum()
        assert np.array_equal(np.flatnonzero(sim.survey_bin_of_step >= 0), W)
        check_bins_are_the_reduction_of_the_probe_rows(sim, f"member {m}, K = {K}, B = {B}, window {steps}, {frame}")
        check_derived(sim)
        check_bin_derived(sim)
    assert not np.array_equal(sims[0].survey_bin_of_step, sims[3].survey_bin_of_step) or B == 1


def test_a_bin_block_is_bit_for_bit_a_plain_survey_of_that_bins_steps(eng):
    """table[i] = i % 8 inside the window (3, nt, 1) for two members of 50 and 40 steps, 300 points (a per-lane tile and a
    sliced one of 44): block b of each member equals all five plain sums of the surveyed sweep that samples (first_b, nt, 8),
    first_b the first i >= 3 with i % 8 == b; and the plain sums are those of the sweep without bins."""
    from ludvm_amd import sweep
    pts = seeds_random(300)
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh")]
    first = 3
    kw = dict(engine=eng, survey=pts, survey_frame="tunnel")
    binned = sweep(cases, **kw, survey_steps=(first, 51, 1), survey_phases=[np.arange(51) % 8, np.arange(41) % 8])
    whole = sweep(cases, **kw, survey_steps=(first, 51, 1))
    for sim, plain in zip(binned, whole):
        assert sim.survey_nbins == 8 and sim.survey_phase is None and np.array_equal(sim.survey_sums, plain.survey_sums)
    for b in range(8):
        first_b = next(i for i in range(first, first + 8) if i % 8 == b)
        plain = sweep(cases, **kw, survey_steps=(first_b, 51, 8))
        for m, (sim, ref) in enumerate(zip(binned, plain)):
            assert sim.survey_bin_count[b] == ref.survey_count == len(window(first_b, 51, 8, sim.nt)) >= 4, (m, b)
            assert (ref.survey_sums[2] > 0.0).all()
            assert np.array_equal(sim.survey_bin_sums[b], ref.survey_sums), (m, b)


class _Raw:
    """Keeps what the engine's ensemble calls return."""
    NAMES = ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned")

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


def test_nothing_else_moves(eng):
    """A sweep with 85 probes, 300 particles and a survey of 300 points, with and without survey_phases: rows, wake records,
    wake_n, probe rows, tracer records and the plain survey sums as the engine returns them, and every member's loads, paths,
    probe rows, tracer paths and survey attributes, are the same arrays bit for bit."""
    from ludvm_amd import sweep
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15, k=2 * PI),
             dict(CONFIG1, tf=2.5, **gust_cloud())]
    snaps = (1, 2, 10, 45)
    rake = np.concatenate([probes32(), probes32()[:, ::-1] + 0.37, probes32()[:, :21] - 0.11], axis=1)
    seeds, rel = seeds_random(300), np.array([1, 20, 35, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    obs = dict(snapshot_steps=snaps, probes=rake, probe_frame="tunnel", particles=seeds, particle_release=rel, particle_frame="tunnel",
               survey=seeds_random(300, seed=9), survey_frame="tunnel", survey_steps=(5, 120, 3))
    raw = _Raw(eng)
    try:
        without = sweep(cases, engine=eng, **obs)
        with_ = sweep(cases, engine=eng, **obs, survey_phases=6)
    finally:
        raw.close()
    assert [o[0] for o in raw.out] == ["ensemble_run_surveyed", "ensemble_run_surveyed_binned"]
    desc, a, b = raw.out[0][1], raw.out[0][2], raw.out[1][2]
    # (rows, wakes, wake_n, tracer_rows, probe_u, probe_w, survey_sums[, bin_sums])
    assert len(a) == 7 and len(b) == 8 and b[7].shape == (4, 6, 5, 300) and np.abs(b[7]).max() > 0.0
    for q in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(a[q], b[q]), q
    assert np.abs(a[3]).max() > 0.0 and np.abs(a[5]).max() > 0.0 and np.abs(a[6]).max() > 0.0
    for m in range(desc.shape[0]):
        nt, _, nf, _, _, w0 = (int(v) for v in desc[m])
        cap = nf + 2 * (nt - 1)
        for r in range(len(snaps) + 1):
            n = int(a[2][m, r])
            for q in range(3):
                at = w0 + (3 * r + q) * cap
                assert n < 0 or np.array_equal(a[1][at:at + n], b[1][at:at + n]), (m, r, q)
    for m, (s0, s1) in enumerate(zip(without, with_)):
        assert not hasattr(s0, "survey_bin_sums") and s1.survey_bin_count.sum() == s1.survey_count
        for name in ("Cl", "Cd", "Cm", "Fn", "Fs", "M", "LESP", "LESP_prev", "LEV_shed", "fourier", "probe_u", "probe_w", "tracer_last",
                     "survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw"):
            assert np.array_equal(getattr(s0, name), getattr(s1, name)), (m, name)
        assert s0.survey_count == s1.survey_count and s0.survey_steps == s1.survey_steps
        assert s0.tracer_path.steps() == s1.tracer_path.steps()
        for s in s0.tracer_path.steps():
            assert np.array_equal(s0.tracer_path[s], s1.tracer_path[s]), (m, s)
        for key in s0.circulation:
            assert np.array_equal(s0.circulation[key], s1.circulation[key]), (m, key)
        for key in ("TEV", "LEV", "FREE"):
            assert s0.path[key].steps() == s1.path[key].steps()
            for s in s0.path[key].steps():
                assert np.array_equal(s0.path[key][s], s1.path[key][s]), (m, key, s)
        # the bins of the sampled steps add up to the plain sums (a different order of the same terms)
        tot = s1.survey_bin_sums.sum(axis=0)
        assert np.abs(tot - s1.survey_sums).max() <= 1e-12 * np.abs(s1.survey_sums).max()


def test_bin_sums_do_not_depend_on_the_batch_and_repeat(eng):
    """A member's bin sums alone, at index 0 and at index 39 of 40 members, and in a second call: the same bits."""
    from ludvm_amd import sweep
    X = dict(CONFIG1, tf=2.5, k=2 * PI)
    others = [dict(CONFIG1, tf=1 + 0.5 * (q % 4), LESPcrit=0.1 + 0.01 * (q % 17), alpha_max=5 + (q % 11), k=PI * (1 + q % 3),
                   method="Ramesh" if q % 7 == 0 else "Faure") for q in range(38)]
    kw = dict(engine=eng, survey=seeds_random(300), survey_frame="tunnel", survey_steps=(2, 48, 1), survey_phases=8)
    alone = sweep([X], **kw)[0]
    first = sweep([X] + others + [X], **kw)
    again = sweep([X] + others + [X], **kw)
    assert len(first) == 40 and alone.survey_bin_count.sum() == 46 and (alone.survey_bin_count >= 4).all()
    assert (alone.survey_bin_sums[:, 2] > 0.0).all()
    for other in (first[0], first[39]):
        assert np.array_equal(alone.survey_bin_of_step, other.survey_bin_of_step)
        assert np.array_equal(alone.survey_bin_sums, other.survey_bin_sums) and np.array_equal(alone.survey_sums, other.survey_sums)
    for a, b in zip(first, again):
        assert np.array_equal(a.survey_bin_count, b.survey_bin_count) and np.array_equal(a.survey_bin_sums, b.survey_bin_sums)
    assert not np.array_equal(first[1].survey_bin_sums, first[2].survey_bin_sums)      # (the other members are different cases)


def test_a_member_against_its_solo_march_with_survey_bins(eng):
    """A member (k = 4 pi: a period of 10 steps) and its solo precision='f64' marched run with survey_bins=5, 300 points, tunnel
    frame, steps 1-10: the same table and counts, bin means within 1e-12 of max|u| and raw second moments within 3e-12 of
    max|u|^2 (per sample; max|u| from the member's own probe rows) -- the two kernels sum the same pairs in different orders."""
    from ludvm_amd import LUDVM, sweep
    pts = seeds_random(300)
    kw = dict(CONFIG1, tf=2.5, k=4 * PI)
    steps = (1, 11, 1)
    sim = sweep([dict(CONFIG1, tf=2, method="Ramesh"), kw], engine=eng, probes=pts, probe_frame="tunnel", survey=pts,
                survey_frame="tunnel", survey_steps=steps, survey_phases=5)[1]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_frame="tunnel",
                 survey_steps=steps, survey_bins=5)
    assert np.array_equal(sim.survey_bin_of_step, solo.survey_bin_of_step) and np.array_equal(sim.survey_bin_count, solo.survey_bin_count)
    assert np.array_equal(sim.survey_bin_count, [2, 2, 2, 2, 2]) and np.array_equal(sim.survey_phase, solo.survey_phase)
    umax = series_umax(sim.probe_u, sim.probe_w, window(*steps, sim.nt))
    n = sim.survey_bin_count.reshape(5, 1, 1).astype(float)
    d = np.abs(sim.survey_bin_sums - solo.survey_bin_sums) / n
    e_mean, e_mom = d[:, :2].max() / umax, d[:, 2:].max() / umax ** 2
    print(f"sweep member vs solo march with survey_bins=5, steps 1-10: bin means {e_mean:.2e} of max|u|, raw second moments "
          f"{e_mom:.2e} of max|u|^2")
    assert e_mean <= 1e-12 and e_mom <= 3e-12, (e_mean, e_mom)
    assert np.abs(sim.survey_bin_mean_u - solo.survey_bin_mean_u).max() <= 1e-12 * umax


def test_gaps_and_an_empty_bin_give_nan_like_a_solo_run(eng):
    """A table with -1 entries inside the window and bin 1 never used: counts from the table, zeros in the empty block, nan for its
    mean and moments -- as the solo marched run with the same table gives -- and the gaps are in the plain sums only."""
    from ludvm_amd import LUDVM, sweep
    pts = seeds_random(129, seed=5)
    kw = dict(CONFIG1, tf=1.5)
    i = np.arange(31)
    table = np.where(i % 3 == 1, -1, np.where(i % 2 == 0, 0, 2))
    sim = sweep([kw], engine=eng, probes=pts, survey=pts, survey_steps=(2, 31, 1), survey_phases=[table])[0]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", survey=pts, survey_steps=(2, 31, 1), survey_bins=table)
    assert sim.survey_nbins == 3 and np.array_equal(sim.survey_bin_of_step, solo.survey_bin_of_step)
    assert np.array_equal(sim.survey_bin_count, solo.survey_bin_count) and sim.survey_bin_count[1] == 0
    assert sim.survey_bin_count.sum() == (table[2:] >= 0).sum() == 20 < sim.survey_count == 29
    for name in ("survey_bin_mean_u", "survey_bin_mean_w", "survey_bin_uu", "survey_bin_ww", "survey_bin_uw"):
        assert np.isnan(getattr(sim, name)[1]).all() and np.isnan(getattr(solo, name)[1]).all(), name
        assert np.isfinite(getattr(sim, name)[[0, 2]]).all(), name
    assert np.isfinite(sim.survey_coherent_uu).all() and np.isfinite(sim.survey_random_uw).all()
    check_bins_are_the_reduction_of_the_probe_rows(sim, "gaps and an empty bin")
    check_bin_derived(sim)


def test_a_short_member_whose_window_holds_one_step(eng):
    """The window (20, 1000, 1) is the 20-step member's last step alone: one sample in one bin, the probe row of that step."""
    from ludvm_amd import sweep
    pts = seeds_random(85, seed=21)
    short, long_ = sweep([dict(CONFIG1, tf=1, k=2 * PI), dict(CONFIG1, tf=2.5, k=2 * PI)], engine=eng, probes=pts, survey=pts,
                         survey_steps=(20, 1000, 1), survey_phases=4)
    assert short.nt == 21 and short.survey_count == 1 and np.array_equal(short.survey_bin_count, [1, 0, 0, 0])
    assert long_.survey_count == 31 and (long_.survey_bin_count >= 5).all()
    assert np.array_equal(short.survey_bin_sums[0, 0], short.probe_u[20]) and np.array_equal(short.survey_bin_sums[0, 1], short.probe_w[20])
    assert np.array_equal(short.survey_bin_sums[0], short.survey_sums)
    for sim in (short, long_):
        check_bins_are_the_reduction_of_the_probe_rows(sim, f"window (20, 1000, 1), nt = {sim.nt}")


def test_many_source_tiles(eng):
    """A member with 1180 free vortices (five 256-source tiles from its first step on; observer_sources_common.py's case A)
    behind another member, 600 points (two per-lane tiles and a sliced one of 88), B = 3 over its 24 steps, against the
    reduction of its probe rows at the same 600 points (one chunk: a sweep takes up to 1024 probes)."""
    from ludvm_amd import sweep
    pts = seeds_random(600)
    kw = source_case_keywords("A")
    table = np.arange(25) % 3
    sim = sweep([dict(CONFIG1, tf=1), kw], engine=eng, probes=pts, survey=pts, survey_phases=[np.arange(21) % 3, table])[1]
    assert sim.nt == 25 and sim.n_freevort == 1180 and sim.survey_count == 24 and np.array_equal(sim.survey_bin_count, [8, 8, 8])
    check_bins_are_the_reduction_of_the_probe_rows(sim, "1180 free vortices, 600 points, B = 3")


def test_4096_points_two_bins_add_up_to_the_plain_sums(eng):
    """K = 4096 (sixteen tiles), B = 2 over 10 steps: bin 0 + bin 1 against the plain sums of the same launch, the means within
    1e-12 of max|u| per sample.  max|u| is taken as the largest root mean square over the points, sqrt(max(sum u^2, sum w^2) /
    n) <= max|u|: the smaller scale makes the bound the tighter one."""
    from ludvm_amd import sweep
    pts = seeds_random(4096, seed=17)
    sim = sweep([dict(CONFIG1, tf=1, method="Ramesh"), dict(CONFIG1, tf=0.5)], engine=eng, survey=pts, survey_frame="tunnel",
                survey_phases=[np.arange(21) % 2, np.arange(11) % 2])[1]
    assert sim.nt == 11 and sim.survey_count == 10 and np.array_equal(sim.survey_bin_count, [5, 5]) and sim.survey_bin_sums.shape == (2, 5, 4096)
    scale = np.sqrt(sim.survey_sums[2:4].max() / 10)
    tot = sim.survey_bin_sums[0] + sim.survey_bin_sums[1]
    e_mean = np.abs(tot[:2] - sim.survey_sums[:2]).max() / 10 / scale
    e_mom = np.abs(tot[2:] - sim.survey_sums[2:]).max() / 10 / scale ** 2
    print(f"K = 4096, B = 2: bin 0 + bin 1 vs the plain sums: means {e_mean:.2e} of rms|u|, raw second moments {e_mom:.2e} of rms|u|^2")
    assert e_mean <= 1e-12 and e_mom <= 3e-12, (e_mean, e_mom)
    assert (sim.survey_bin_sums[:, 2] > 0.0).all() and not np.array_equal(sim.survey_bin_sums[0], sim.survey_bin_sums[1])
    check_bin_derived(sim)


def _arrays(members, npan=80, ncoef=30, nt=3):
    T = 8 * npan + ncoef * npan + (ncoef - 1) * npan
    scalars = np.ones([members, 12])
    scalars[:, 8:] = 0.0
    desc = np.array([[nt, m * nt, 1, m, m * (nt - 1), m * 3 * (1 + 2 * (nt - 1))] for m in range(members)], dtype=np.int64)
    return (npan, ncoef, scalars, np.zeros([members, T]), np.zeros([members * nt, 7 + 2 * npan]), np.zeros([members, 8 + ncoef]),
            np.zeros(3 * members), desc)


def test_the_library_answers_the_documented_codes_and_leaves_the_context_alone(eng):
    """What ludvm_ensemble_run_surveyed_binned refuses on the host (LUDVM_E_ARG) launches nothing; a solo marched run with
    survey_bins gives the same results before and after a binned sweep on the same engine, the resident wake of the first is
    still there after the sweep, and ensemble_limits() is unchanged."""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    pts = seeds_random(37, seed=2)

    def solo():
        s = LUDVM(**dict(CONFIG1, tf=2.5, k=2 * PI), verbose=False, engine=eng, precision="f64", history="sparse", survey=pts,
                  survey_frame="tunnel", survey_steps=(3, 45, 2), survey_bins=4)
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.survey_sums, s.survey_bin_sums, s.survey_bin_count]
    limits = eng.ensemble_limits()
    before = solo()
    size = eng.wake_size()
    wake = eng.wake_read(0, size, gamma=True) if size else ()
    sims = sweep([dict(CONFIG1, tf=2, method="Ramesh", k=PI), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15)], engine=eng,
                 snapshot_steps=(3,), survey=pts[:, ::-1] + 0.25, survey_frame="tunnel", probes=pts, particles=pts, survey_phases=7)
    assert all(np.isfinite(s.survey_bin_sums).all() and s.survey_bin_count.sum() == s.nt - 1 for s in sims)

    packed = _arrays(2)
    one = dict(survey_x=[0.0], survey_z=[0.0], survey_steps=(1, 3, 1), bin_of_step=np.zeros(6, dtype=np.int32), nbins=2)
    for word, kw in (("one per kinematics row", dict(one, bin_of_step=np.zeros(5, dtype=np.int32))),
                     ("-1 (none) or 0 .. bins - 1", dict(one, bin_of_step=[0, 1, 2, 0, 0, 0])),
                     ("-1 (none) or 0 .. bins - 1", dict(one, bin_of_step=[0, 1, -2, 0, 0, 0])),
                     ("survey bins <= 64", dict(one, nbins=65)),
                     ("need survey points", dict(one, survey_x=[], survey_z=[])),
                     ("first >= 1", dict(one, survey_steps=(0, 3, 1)))):
        with pytest.raises(LudvmHipError) as e:
            eng.ensemble_run_surveyed_binned(*packed, **kw)
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))

    assert eng.wake_size() == size and eng.ensemble_limits() == limits
    for a, b in zip(wake, eng.wake_read(0, size, gamma=True) if size else ()):
        assert np.array_equal(a, b)
    after = solo()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
