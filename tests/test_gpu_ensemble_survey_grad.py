"""GPU tier of the wake survey's gradient sums in a sweep (ensemble_graded<PROBES, TRACERS>, ludvm_ensemble_run_surveyed_graded;
DESIGN.md section 4.21): every member's five gradient sums accumulated inside the one launch -- by value against the
long-double closed forms over the sources of the member's solo twin, at the point counts where the walk changes its path,
passive on every other result, a bin bit for bit against the gradient sums of its steps, independent of the batch, against the
solo marched run with survey_gradient=True, against centred differences of the launch's own mean velocity, and the entry
point's codes with the context left alone.

Bounds (tests/survey_gradient_common.py, the project's for this construction): means of ux, e, omega within MEAN_BOUND = 1e-9 of
max|grad u| over the sampled steps and points, means of omega^2 and Q within SQUARE_BOUND = 3e-9 of max|grad u|^2.  The twin
-- LUDVM(..., precision='f64', history='full') -- and the member are first asserted to agree in Cl / Cd / Cm and the final wake
to 1e-12: the twin's sources are then the member's to summation order.  Before a comparison counts, the same reference summed
over the sources of step i - 1 is asserted to be off by more than ten tolerances somewhere: a wake taken one step late cannot
pass.  Measured [MI355X]: by value at most 1.6e-15 of max|grad u| and 3.1e-15 of max|grad u|^2 (the 'Ramesh' member of the
three-member sweep; every other case below 7e-16 / 1.2e-15); the member against its solo march 4.1e-15 / 8.9e-15, bins 2.0e-14 /
4.4e-14; the centred differences converge with ratios 3.987 .. 4.020; the 22 tests take 6.9 s."""
import signal

import numpy as np
import pytest

import gradient_common as GC
import survey_gradient_common as SG
from conftest import CONFIG1
from ensemble_survey_grad_common import BIN_GRAD_ATTRS, GRAD_ATTRS, member_window, reference_of, sources_of
from observer_sources_common import case_keywords as source_case_keywords
from oracle import ludvm_oracle as O
from oracle.g10_cases import DHALF
from probes_common import probes32
from survey_bins_common import check_bin_derived
from survey_common import check_derived, window
from tracers_common import gust_cloud, run_sources, seeds_random

pytestmark = pytest.mark.gpu

PI = np.pi
DT = CONFIG1["dt"]


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


def steps_kw(steps, dt=DT, **over):
    """Keywords of a run of `steps` time steps (tf half a step short of the last level)."""
    return dict(CONFIG1, dt=dt, tf=(steps - 0.5) * dt, **over)


def _twin(eng, kw):
    from ludvm_amd import LUDVM
    return LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="full")


def assert_twin_and_member_agree(sim, twin, label):
    """Cl / Cd / Cm and the final wake to 1e-12: the twin's sources are the member's to summation order."""
    assert sim.nt == twin.nt and np.array_equal(sim.LEV_shed, twin.LEV_shed), label
    for name in ("Cl", "Cd", "Cm"):
        assert np.abs(getattr(sim, name) - getattr(twin, name)).max() <= 1e-12, (label, name)
    last, nlev = sim.nt - 1, int((sim.LEV_shed != -1).sum())
    assert sim.itev == twin.itev
    assert np.abs(sim.path["TEV"][last][:, :sim.itev + 1] - twin.path["TEV"][last][:, :sim.itev + 1]).max() <= 1e-12, label
    if nlev:
        assert np.abs(sim.path["LEV"][last][:, :nlev] - twin.path["LEV"][last][:, :nlev]).max() <= 1e-12, label
    if np.size(sim.path["FREE"][last]):
        assert np.abs(np.asarray(sim.path["FREE"][last]) - np.asarray(twin.path["FREE"][last])).max() <= 1e-12, label


def check_by_value(sim, twin, label, pick=None, late=True):
    """The member's gradient sums (and bins) at the points `pick` against the long-double terms over the twin's sources, added
    in step order; first the reference over the sources of step i - 1 must miss by more than ten tolerances."""
    steps = member_window(sim.survey_steps, sim.nt)
    assert sim.survey_count == len(steps)
    K = sim._survey_xz.shape[1]
    pick = np.arange(K) if pick is None else pick
    B = getattr(sim, "survey_nbins", 0)
    table = sim.survey_bin_of_step if B else None
    ref, gmax, bref = reference_of(twin, sim._survey_xz, sim.survey_frame, steps, table, B, pick)
    assert gmax > 0.0
    if late:
        wrong = reference_of(twin, sim._survey_xz, sim.survey_frame, steps, pick=pick, lag=1)[0]
        l_mean, l_sq = SG.sums_errors(wrong, ref, len(steps), gmax)
        assert l_mean > 10 * SG.MEAN_BOUND and l_sq > 10 * SG.SQUARE_BOUND, (label, l_mean, l_sq)
    got = sim.survey_grad_sums.reshape(5, -1)[:, pick]
    e_mean, e_sq = SG.sums_errors(got, ref, len(steps), gmax)
    print(f"{label}: {len(steps)} steps, {len(pick)} points: means of ux, e, omega {e_mean:.2e} of max|grad u| ({gmax:.3f}) = "
          f"{e_mean / SG.MEAN_BOUND:.1e} of the bound; means of omega^2, Q {e_sq:.2e} of max|grad u|^2 = {e_sq / SG.SQUARE_BOUND:.1e} of the bound")
    assert e_mean <= SG.MEAN_BOUND, (label, e_mean)
    assert e_sq <= SG.SQUARE_BOUND, (label, e_sq)
    assert (got[3] > 0.0).all(), label                  # every point was written
    for b in range(B):
        n = int(sim.survey_bin_count[b])
        if n == 0:
            assert not sim.survey_bin_grad_sums[b].any(), (label, b)
            continue
        e = SG.sums_errors(sim.survey_bin_grad_sums[b].reshape(5, -1)[:, pick], bref[b], n, gmax)
        assert e[0] <= SG.MEAN_BOUND and e[1] <= SG.SQUARE_BOUND, (label, b, e)
    return steps


def three_members(steps=28):
    """'Faure' and 'Ramesh' members of different k and one off the unit point (chord 0.5, Uinf 2, rho = 1000, its own dt; v_core
    follows them), `steps` steps each."""
    return [steps_kw(steps), steps_kw(steps, method="Ramesh", k=0.4 * PI), steps_kw(steps, **DHALF)]


@pytest.fixture(scope="module")
def twins(eng):
    """The solo twins of three_members(), computed once."""
    return [_twin(eng, kw) for kw in three_members()]


# ---- 1. by value -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_by_value_over_the_twins_own_sources(eng, twins, frame):
    """Three members in one sweep, 28 steps, 300 points (a point-per-lane tile of 256 and a sliced one of 44), every step
    sampled, both frames."""
    from ludvm_amd import sweep
    pts = seeds_random(300)
    sims = sweep(three_members(), engine=eng, survey=pts, survey_frame=frame, survey_grad=True)
    assert len({s.v_core for s in sims}) >= 2 and sims[2].chord == 0.5 and sims[2].rho == 1000
    for m, (sim, twin) in enumerate(zip(sims, twins)):
        assert sim.nt == 29 and sim.survey_gradient is True and sim.v_core == twin.v_core
        assert_twin_and_member_agree(sim, twin, f"member {m}")
        check_by_value(sim, twin, f"member {m} ({frame})")
        check_derived(sim)
        SG.check_derived(sim)
        for name in GRAD_ATTRS:
            assert np.isfinite(getattr(sim, name)).all(), (m, name)
        for name in BIN_GRAD_ATTRS:
            assert not hasattr(sim, name), name


# ---- 2. shapes where the walk can go wrong -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 64, 65, 85, 86, 128, 129, 256, 257, 513])
def test_point_counts_where_the_walk_changes_its_path(eng, twins, K):
    """4 -> 3 -> 2 -> 1 lanes per point (64 | 65, 85 | 86, 128 | 129: the sliced tile against the point-per-lane one), one tile
    to two (256 | 257) and to three (513); 28 steps, tunnel frame, bins of 3 so that the bin blocks are checked too.  The sources
    of the 'Faure' member number i + 80 in step i: every remainder of four, the pad group at work."""
    from ludvm_amd import sweep
    pts = seeds_random(K, seed=17)
    sims = sweep(three_members()[:2], engine=eng, survey=pts, survey_frame="tunnel", survey_grad=True,
                 survey_phases=[np.arange(29) % 3, np.arange(29) % 3])
    src = sources_of(twins[0])
    assert {len(SG.all_sources(src(i))[0]) % 4 for i in range(1, 29)} == {0, 1, 2, 3}
    for m in (0, 1):
        assert sims[m].survey_grad_sums.shape == (5, K) and sims[m].survey_bin_grad_sums.shape == (3, 5, K)
        check_by_value(sims[m], twins[m], f"K = {K}, member {m}", late=K >= 64)
        SG.check_bin_derived(sims[m])


def test_4096_points(eng):
    """K = 4096 (sixteen tiles) over 10 steps behind a 20-step member: 256 picked points by value, every point written."""
    from ludvm_amd import sweep
    pts = seeds_random(4096, seed=17)
    kw = steps_kw(10)
    sim = sweep([steps_kw(20, method="Ramesh"), kw], engine=eng, survey=pts, survey_frame="tunnel", survey_grad=True)[1]
    twin = _twin(eng, kw)
    assert_twin_and_member_agree(sim, twin, "K = 4096")
    rng = np.random.default_rng(5)
    pick = np.unique(np.concatenate([[0, 255, 256, 4095], rng.choice(4096, 252, replace=False)]))
    check_by_value(sim, twin, "K = 4096", pick=pick)
    assert sim.survey_grad_sums.shape == (5, 4096) and (sim.survey_grad_sums[3] > 0.0).all() and np.isfinite(sim.survey_grad_sums).all()


def test_many_source_tiles(eng):
    """A member with 1180 free vortices (five 256-source tiles from its first step on; observer_sources_common.py's case A)
    behind another member, 600 points (two point-per-lane tiles and a sliced one of 88), 24 steps."""
    from ludvm_amd import sweep
    pts = seeds_random(600)
    kw = source_case_keywords("A")
    sim = sweep([steps_kw(20), kw], engine=eng, survey=pts, survey_grad=True)[1]
    twin = _twin(eng, kw)
    assert sim.nt == 25 and sim.n_freevort == 1180 and sim.survey_count == 24
    assert_twin_and_member_agree(sim, twin, "1180 free vortices")
    check_by_value(sim, twin, "1180 free vortices, 600 points")


# ---- 3. passive ---------------------------------------------------------------------------------------------------------------

class _Raw:
    """Keeps what the engine's ensemble calls return."""
    NAMES = ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
             "ensemble_run_surveyed_graded")

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


@pytest.mark.parametrize("phases", [None, 5], ids=["plain", "binned"])
def test_nothing_else_moves(eng, phases):
    """A sweep of four members with 85 probes, 300 particles and a survey of 300 points, with and without survey_grad (and with
    survey_phases=5 in both): rows, wake records, wake_n, probe rows, tracer records, the velocity sums and their bins as the
    engine returns them, and every member's attributes, are the same arrays bit for bit."""
    from ludvm_amd import sweep
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15, k=2 * PI),
             dict(CONFIG1, tf=2.5, **gust_cloud())]
    snaps = (1, 2, 10, 45)
    rake = np.concatenate([probes32(), probes32()[:, ::-1] + 0.37, probes32()[:, :21] - 0.11], axis=1)
    seeds, rel = seeds_random(300), np.array([1, 20, 35, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    obs = dict(snapshot_steps=snaps, probes=rake, probe_frame="tunnel", particles=seeds, particle_release=rel, particle_frame="tunnel",
               survey=seeds_random(300, seed=9), survey_frame="tunnel", survey_steps=(5, 120, 3))
    if phases:
        obs.update(survey_phases=phases)
    raw = _Raw(eng)
    try:
        without = sweep(cases, engine=eng, **obs)
        with_ = sweep(cases, engine=eng, **obs, survey_grad=True)
    finally:
        raw.close()
    assert [o[0] for o in raw.out] == ["ensemble_run_surveyed_binned" if phases else "ensemble_run_surveyed", "ensemble_run_surveyed_graded"]
    desc, a, b = raw.out[0][1], raw.out[0][2], raw.out[1][2]
    # (rows, wakes, wake_n, tracer_rows, probe_u, probe_w, survey_sums[, bin_sums]); graded: ..., bin_sums, grad_sums, bin_grad_sums
    assert len(a) == (8 if phases else 7) and len(b) == 10 and b[8].shape == (4, 5, 300) and np.abs(b[8]).max() > 0.0
    for q in (0, 2, 3, 4, 5, 6) + ((7,) if phases else ()):
        assert np.array_equal(a[q], b[q]), q
    if phases:
        assert b[9].shape == (4, 5, 5, 300) and np.abs(b[9]).max() > 0.0 and np.abs(a[7]).max() > 0.0
    else:
        assert b[7] is None and b[9] is None
    assert np.abs(a[3]).max() > 0.0 and np.abs(a[5]).max() > 0.0 and np.abs(a[6]).max() > 0.0
    for m in range(desc.shape[0]):
        nt, _, nf, _, _, w0 = (int(v) for v in desc[m])
        cap = nf + 2 * (nt - 1)
        for r in range(len(snaps) + 1):
            n = int(a[2][m, r])
            for q in range(3):
                at = w0 + (3 * r + q) * cap
                assert n < 0 or np.array_equal(a[1][at:at + n], b[1][at:at + n]), (m, r, q)
    names = ("Cl", "Cd", "Cm", "Fn", "Fs", "M", "LESP", "LESP_prev", "LEV_shed", "fourier", "probe_u", "probe_w", "tracer_last",
             "survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw")
    if phases:
        names += ("survey_bin_sums", "survey_bin_count", "survey_bin_of_step", "survey_bin_mean_u", "survey_bin_uw", "survey_coherent_uu")
    for m, (s0, s1) in enumerate(zip(without, with_)):
        assert not hasattr(s0, "survey_grad_sums") and not hasattr(s0, "survey_gradient") and s1.survey_gradient is True
        for name in names:
            assert np.array_equal(getattr(s0, name), getattr(s1, name), equal_nan=True), (m, name)
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
        assert (s1.survey_grad_sums[3] > 0.0).all()
        SG.check_derived(s1)
        if phases:
            SG.check_bin_derived(s1)
            tot = s1.survey_bin_grad_sums.sum(axis=0)
            assert np.abs(tot - s1.survey_grad_sums).max() <= 1e-12 * np.abs(s1.survey_grad_sums).max()


# ---- 4. bins -------------------------------------------------------------------------------------------------------------------

def test_a_bin_block_is_bit_for_bit_the_gradient_sums_of_that_bins_steps(eng):
    """table[i] = i % 8 inside the window (3, nt, 1) for two members of 50 and 40 steps, 300 points: block b of each member's
    bin gradient sums equals the gradient sums of the graded sweep that samples (first_b, nt, 8), first_b the first i >= 3 with
    i % 8 == b, and so does its velocity block; the plain gradient sums are those of the graded sweep without bins."""
    from ludvm_amd import sweep
    pts = seeds_random(300)
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh")]
    first = 3
    kw = dict(engine=eng, survey=pts, survey_frame="tunnel", survey_grad=True)
    binned = sweep(cases, **kw, survey_steps=(first, 51, 1), survey_phases=[np.arange(51) % 8, np.arange(41) % 8])
    whole = sweep(cases, **kw, survey_steps=(first, 51, 1))
    for sim, plain in zip(binned, whole):
        assert sim.survey_nbins == 8 and np.array_equal(sim.survey_grad_sums, plain.survey_grad_sums)
        assert np.array_equal(sim.survey_sums, plain.survey_sums) and not hasattr(plain, "survey_bin_grad_sums")
        SG.check_bin_derived(sim)
        check_bin_derived(sim)
    for b in range(8):
        first_b = next(i for i in range(first, first + 8) if i % 8 == b)
        plain = sweep(cases, **kw, survey_steps=(first_b, 51, 8))
        for m, (sim, ref) in enumerate(zip(binned, plain)):
            assert sim.survey_bin_count[b] == ref.survey_count == len(window(first_b, 51, 8, sim.nt)) >= 4, (m, b)
            assert (ref.survey_grad_sums[3] > 0.0).all()
            assert np.array_equal(sim.survey_bin_grad_sums[b], ref.survey_grad_sums), (m, b)
            assert np.array_equal(sim.survey_bin_sums[b], ref.survey_sums), (m, b)


def test_gaps_and_an_empty_bin_give_a_zero_block_and_nan_means(eng):
    from ludvm_amd import sweep
    pts = seeds_random(129, seed=5)
    i = np.arange(31)
    table = np.where(i % 3 == 1, -1, np.where(i % 2 == 0, 0, 2))
    sim = sweep([dict(CONFIG1, tf=1.5)], engine=eng, survey=pts, survey_steps=(2, 31, 1), survey_phases=[table], survey_grad=True)[0]
    assert sim.survey_nbins == 3 and sim.survey_bin_count[1] == 0 and sim.survey_bin_count.sum() == 20 < sim.survey_count == 29
    assert not sim.survey_bin_grad_sums[1].any() and (sim.survey_bin_grad_sums[[0, 2], 3] > 0.0).all()
    for name in ("survey_bin_mean_ux", "survey_bin_mean_strain", "survey_bin_mean_omega", "survey_bin_mean_q", "survey_bin_omega2"):
        assert np.isnan(getattr(sim, name)[1]).all() and np.isfinite(getattr(sim, name)[[0, 2]]).all(), name
    assert np.isfinite(sim.survey_coherent_omega2).all() and np.isfinite(sim.survey_random_omega2).all()
    SG.check_derived(sim)
    SG.check_bin_derived(sim)


# ---- 5. batch and repeat ------------------------------------------------------------------------------------------------------

def test_the_sums_do_not_depend_on_the_batch_and_repeat(eng):
    """A member's ten sums and their bins alone, at index 0 and at index 39 of 40 members, and in a second call: the same bits."""
    from ludvm_amd import sweep
    X = dict(CONFIG1, tf=2.5, k=2 * PI)
    others = [dict(CONFIG1, tf=1 + 0.5 * (q % 4), LESPcrit=0.1 + 0.01 * (q % 17), alpha_max=5 + (q % 11), k=PI * (1 + q % 3),
                   method="Ramesh" if q % 7 == 0 else "Faure") for q in range(38)]
    kw = dict(engine=eng, survey=seeds_random(300), survey_frame="tunnel", survey_steps=(2, 48, 1), survey_phases=8, survey_grad=True)
    alone = sweep([X], **kw)[0]
    first = sweep([X] + others + [X], **kw)
    again = sweep([X] + others + [X], **kw)
    assert len(first) == 40 and (alone.survey_bin_count >= 4).all() and (alone.survey_bin_grad_sums[:, 3] > 0.0).all()
    for other in (first[0], first[39]):
        for name in ("survey_grad_sums", "survey_bin_grad_sums", "survey_sums", "survey_bin_sums"):
            assert np.array_equal(getattr(alone, name), getattr(other, name)), name
    for a, b in zip(first, again):
        for name in ("survey_grad_sums", "survey_bin_grad_sums", "survey_sums", "survey_bin_sums"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert not np.array_equal(first[1].survey_grad_sums, first[2].survey_grad_sums)      # (the other members are different cases)


# ---- 6. against the solo march -----------------------------------------------------------------------------------------------

def test_a_member_against_its_solo_march_with_survey_gradient(eng):
    """A member and its solo precision='f64' marched run with survey_gradient=True, 300 points, tunnel frame, steps 1-10, five
    bins: the bounds of the by-value tests with max|grad u| from the long-double reference; the two kernels sum the same pairs in
    different orders, so the measured ratio lies orders below the bounds."""
    from ludvm_amd import LUDVM, sweep
    pts = seeds_random(300)
    kw = dict(CONFIG1, tf=2.5, k=4 * PI)
    steps = (1, 11, 1)
    sim = sweep([dict(CONFIG1, tf=2, method="Ramesh"), kw], engine=eng, survey=pts, survey_frame="tunnel", survey_steps=steps,
                survey_phases=5, survey_grad=True)[1]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="full", survey=pts, survey_frame="tunnel",
                 survey_steps=steps, survey_bins=5, survey_gradient=True)
    assert np.array_equal(sim.survey_bin_of_step, solo.survey_bin_of_step) and np.array_equal(sim.survey_bin_count, [2, 2, 2, 2, 2])
    _, gmax, _ = reference_of(solo, pts, "tunnel", list(range(1, 11)))
    e_mean, e_sq = SG.sums_errors(sim.survey_grad_sums, solo.survey_grad_sums, 10, gmax)
    worst = [SG.sums_errors(sim.survey_bin_grad_sums[b], solo.survey_bin_grad_sums[b], 2, gmax) for b in range(5)]
    b_mean, b_sq = max(w[0] for w in worst), max(w[1] for w in worst)
    print(f"sweep member vs solo march with survey_gradient, steps 1-10: means {e_mean:.2e} of max|grad u| ({gmax:.3f}) = "
          f"{e_mean / SG.MEAN_BOUND:.1e} of the bound, squares {e_sq:.2e} of max|grad u|^2 = {e_sq / SG.SQUARE_BOUND:.1e} of the bound; "
          f"bins {b_mean:.2e} / {b_sq:.2e}")
    assert e_mean <= SG.MEAN_BOUND and e_sq <= SG.SQUARE_BOUND, (e_mean, e_sq)
    assert b_mean <= SG.MEAN_BOUND and b_sq <= SG.SQUARE_BOUND, (b_mean, b_sq)
    assert np.abs(sim.survey_mean_omega - solo.survey_mean_omega).max() <= SG.MEAN_BOUND * gmax


# ---- 7. physics without any reference run ------------------------------------------------------------------------------------

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
    """tests/test_gpu_survey_gradient.py's test of the same name on a sweep member: a survey of point stencils x +- h, z +- h
    around 48 centres with h = v_core / 8 and v_core / 16.  Centred differences of the launch's own survey_mean_u / _w converge
    to its survey_mean_ux / _uz / _wx at second order: the ratio is asserted in [3.8, 4.2] for every (centre, component) at
    which the CPU reference over the twin's sources gives a ratio in [3.85, 4.15] with every centre at least 2 v_core from
    every source -- chosen by the reference, never by the code under test."""
    from ludvm_amd import LUDVM, sweep
    kw = dict(CONFIG1, tf=1.5)
    vc = LUDVM(**kw, verbose=False, engine=eng, precision="f64", run=False).v_core
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
    sim = sweep([dict(CONFIG1, tf=1, method="Ramesh"), kw], engine=eng, survey=pts, survey_steps=(20, 30, 3), survey_grad=True)[1]
    twin = _twin(eng, kw)
    assert sim.survey_count == len(steps) == 4
    assert_twin_and_member_agree(sim, twin, "stencils")
    mu, mw, g3, far = np.zeros(pts.shape[1]), np.zeros(pts.shape[1]), np.zeros([3, n]), np.full(n, np.inf)
    for i in steps:
        g, x, z = SG.all_sources(run_sources(twin, i))
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
    assert ok.sum() >= n
    assert ((got[ok] >= 3.8) & (got[ok] <= 4.2)).all(), (got[ok].min(), got[ok].max())


# ---- 8. entry point ------------------------------------------------------------------------------------------------------------

NAME = "ludvm_ensemble_run_surveyed_graded"


class _Tampered:
    """The engine's library with the arguments of the graded call changed on their way in (what Engine never sends)."""

    def __init__(self, lib, change):
        self._lib, self._change = lib, change

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != NAME:
            return fn
        return lambda *a: fn(*self._change(list(a)))


def _arrays(members, npan=80, ncoef=30, nt=3):
    T = 8 * npan + ncoef * npan + (ncoef - 1) * npan
    scalars = np.ones([members, 12])
    scalars[:, 8:] = 0.0
    desc = np.array([[nt, m * nt, 1, m, m * (nt - 1), m * 3 * (1 + 2 * (nt - 1))] for m in range(members)], dtype=np.int64)
    return (npan, ncoef, scalars, np.zeros([members, T]), np.zeros([members * nt, 7 + 2 * npan]), np.zeros([members, 8 + ncoef]),
            np.zeros(3 * members), desc)


def _set(index, value):
    def change(a):
        a[index] = value(a) if callable(value) else value
        return a
    return change


def _prepared(eng, **extra):
    """A 20-step 'f64' run set up for the march (ludvm_march_setup and the survey's set calls done, no step run)."""
    from ludvm_amd import LUDVM
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", run=False, **extra)
    S = sim._loop_begin()
    sim._free_slot = S.fslot
    S.fsl = slice(0, S.nf)
    sim._loop_prepare_engine(S)
    assert S.can_march
    return sim, S


def test_the_library_answers_the_documented_codes_and_leaves_the_context_alone(eng):
    """What ludvm_ensemble_run_surveyed_graded refuses on the host (LUDVM_E_ARG) launches nothing: the resident wake of a solo
    run is still there, a prepared solo march runs on with the bits of an undisturbed one, and a solo survey_gradient=True run
    gives the same bits before and after a graded sweep on the same engine.  (LUDVM_E_STATE of a sharded context needs two
    devices: not reached here.)"""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    pts = seeds_random(37, seed=2)

    def solo():
        s = LUDVM(**dict(CONFIG1, tf=2.5, k=2 * PI), verbose=False, engine=eng, precision="f64", history="sparse", survey=pts,
                  survey_frame="tunnel", survey_steps=(3, 45, 2), survey_bins=4, survey_gradient=True)
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.survey_sums, s.survey_bin_sums, s.survey_bin_count,
                s.survey_grad_sums, s.survey_bin_grad_sums]
    limits = eng.ensemble_limits()
    before = solo()
    size = eng.wake_size()
    wake = eng.wake_read(0, size, gamma=True) if size else ()
    sims = sweep([dict(CONFIG1, tf=2, method="Ramesh", k=PI), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15)], engine=eng,
                 snapshot_steps=(3,), survey=pts[:, ::-1] + 0.25, survey_frame="tunnel", probes=pts, particles=pts, survey_phases=7,
                 survey_grad=True)
    assert all(np.isfinite(s.survey_bin_grad_sums).all() and (s.survey_grad_sums[3] > 0.0).all() for s in sims)
    assert eng.wake_size() == size
    after = solo()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))

    packed = _arrays(2)
    one = dict(survey_x=[0.0], survey_z=[0.0], survey_steps=(1, 3, 1))
    two = dict(one, bin_of_step=np.zeros(6, dtype=np.int32), nbins=2)
    lib = eng._lib
    # grad_doubles = 0 with both arrays null is the binned call itself
    kw = dict(CONFIG1, tf=1)
    plain = sweep([kw], engine=eng, survey=pts, survey_phases=3)[0]
    eng._lib = _Tampered(lib, lambda a: a[:-4] + [None, 0, None, 0])
    try:
        same = sweep([kw], engine=eng, survey=pts, survey_phases=3, survey_grad=True)[0]
    finally:
        eng._lib = lib
    assert np.array_equal(same.survey_sums, plain.survey_sums) and np.array_equal(same.survey_bin_sums, plain.survey_bin_sums)
    assert not same.survey_grad_sums.any() and not same.survey_bin_grad_sums.any()

    # a prepared solo march, then every refusal, then its steps: the bits of an undisturbed one
    sim, S = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_gradient=True)
    refusals = (
        ("gradient sums need survey points", dict(one, survey_x=[], survey_z=[]), None),
        ("must hold members x 5 x points", one, _set(-3, lambda a: a[-3] + 1)),
        ("must hold members x bins x 5 x points", two, _set(-1, lambda a: a[-1] - 1)),
        ("null array", one, _set(-4, None)),
        ("null array", two, _set(-2, None)),
        ("bin gradient sums need survey bins", one, _set(-2, lambda a: a[-4])),
        ("bin gradient sums need survey bins", one, _set(-1, 10)),
        ("-1 (none) or 0 .. bins - 1", dict(two, bin_of_step=[0, 1, 2, 0, 0, 0]), None),
        ("survey bins <= 64", dict(two, nbins=65), None),
        ("first >= 1", dict(one, survey_steps=(0, 3, 1)), None),
    )
    for word, kw, change in refusals:
        if change is not None:
            eng._lib = _Tampered(lib, change)
        try:
            with pytest.raises(LudvmHipError) as e:
                eng.ensemble_run_surveyed_graded(*packed, **kw)
        finally:
            eng._lib = lib
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))
    # 3277 members x 4096 points x 80 bytes of plain and gradient sums: over 1 GiB, and the message gives the size
    with pytest.raises(LudvmHipError) as e:
        eng.ensemble_run_surveyed_graded(*_arrays(3277, npan=2, ncoef=4, nt=2), survey_x=np.zeros(4096), survey_z=np.zeros(4096),
                                         survey_steps=(1, 2, 1))
    assert e.value.code == _ffi.E_ARG and "over 1 GiB" in str(e.value) and "1024.06" in str(e.value), str(e.value)
    assert eng.ensemble_limits() == limits
    sim._march_call(S, 1, 7, False, 50)
    g6, _ = eng.march_survey_gradient()
    sums6, m6 = eng.march_survey()
    fresh, Sf = _prepared(eng, survey=pts, survey_steps=(2, 20, 2), survey_gradient=True)
    fresh._march_call(Sf, 1, 7, False, 50)
    assert m6 == 3 and (g6[3] > 0.0).all() and np.array_equal(eng.march_survey_gradient()[0], g6) and np.array_equal(eng.march_survey()[0], sums6)
    size = eng.wake_size()
    wake = eng.wake_read(0, size, gamma=True)
    with pytest.raises(LudvmHipError):
        eng.ensemble_run_surveyed_graded(*packed, **dict(one, survey_steps=(0, 3, 1)))
    assert eng.wake_size() == size
    for a, b in zip(wake, eng.wake_read(0, size, gamma=True)):
        assert np.array_equal(a, b)
