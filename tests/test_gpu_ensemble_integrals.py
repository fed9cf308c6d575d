"""GPU tier of the wake integrals in a sweep (ensemble_integrals<PROBES, TRACERS, SURVEY>, ludvm_ensemble_run_integrals; DESIGN.md
section 4.23): every member's class moments of every step and its energy W at the sampled steps, accumulated inside the one
launch -- by value against the long-double reference over the member's OWN sources (the sweep is run with
snapshot_steps=range(1, nt), tests/ensemble_integrals_common.py) at the source counts where the walks change tiles, passive on
every other result, independent of the batch and of the window, against the solo marched run with wake_integrals=True, and the
entry point's codes with the context left alone.

Bounds (tests/wake_integrals_common.py, imported): moments within (ns + 16) 2^-52 sum |term| with exact counts, W within
1/2 sum |G_a| B_a plus the summation term.  Before the three-member comparison counts, the reference over the sources of step
i - 1 is asserted to miss both bounds by more than ten times.  Each test prints its worst |error| / bound; DESIGN.md section 4.23
records the table."""
import signal

import numpy as np
import pytest

import ensemble_integrals_common as EI
from conftest import CONFIG1
from probes_common import probes32
from test_gpu_ensemble_survey_grad import assert_twin_and_member_agree, steps_kw, three_members
from oracle.g10_cases import DHALF
from tracers_common import gust_cloud, seeds_random

pytestmark = pytest.mark.gpu

PI = np.pi
NAME = "ludvm_ensemble_run_integrals"


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


def _sweep(*a, **k):
    from ludvm_amd import sweep
    return sweep(*a, **k)


def _source_counts(sim):
    """n + npan behind the solve of every step 1 .. nt - 1, from the member's own rows"""
    return sim.integral_sums[1:, :, :, 0].sum(axis=(1, 2)).astype(int)


# ---- 1. by value -------------------------------------------------------------------------------------------------------------------

def members_with_both_lev_signs(steps=28):
    """three_members() -- 'Faure', 'Ramesh' of another k, the off-unit DHALF (chord 0.5, Uinf 2, rho 1000, its own dt and v_core) --
    with DHALF pitching about alpha_m = -8 degrees: in 28 steps the first two shed LEVs of positive circulation only (3 and 23
    of them), this one twelve of negative circulation, so the batch fills both LEV slots."""
    return three_members(steps)[:2] + [steps_kw(steps, **dict(DHALF, alpha_m=-8))]


def test_three_members_by_value_over_their_own_sources(eng):
    """'Faure', 'Ramesh' and the off-unit DHALF in one sweep, 28 steps, every step sampled for the energy."""
    win = (1, 29, 1)
    sims = _sweep(members_with_both_lev_signs(), engine=eng, snapshot_steps=EI.dense_snapshots(29), integrals=True, energy_steps=win)
    assert len({s.v_core for s in sims}) >= 2 and sims[2].chord == 0.5 and sims[2].rho == 1000
    census = np.zeros([4, 2], dtype=int)
    for m, sim in enumerate(sims):
        assert sim.nt == 29 and sim.wake_integrals is True and sim.wake_energy_steps == win
        assert sim.integral_sums.shape == (29, 4, 2, 6) and sim.path["TEV"].steps() == list(range(29))
        steps = range(1, 29)
        # the planted fault first: a wake taken one step late cannot pass
        lag_m, lag_w = EI.lagged_misses(sim, steps, steps)
        print(f"member {m}: the sources of step i - 1 miss the moment bound {lag_m:.1e} times, the energy bound {lag_w:.1e} times")
        assert lag_m > 10 and lag_w > 10, (m, lag_m, lag_w)
        EI.check_member(sim, steps, f"sweep, member {m}")
        census = np.maximum(census, EI.class_census(sim, steps))
        assert sim.integral_sums[0, EI.FREE, 0, 0] == 1.0 and not sim.integral_sums[0, 1:].any() and np.isnan(sim.wake_energy[0])
    print("largest counts [class, sign] over the batch:", census.tolist())
    assert (census[[EI.TEV, EI.LEV, EI.BOUND]] > 0).all(), census


# ---- 2. tile edges of the source walk ----------------------------------------------------------------------------------------------

EDGES = (256, 512, 2048)


@pytest.fixture(scope="module")
def edge_sweep(eng):
    """245 panels, no LEV (LESPcrit out of reach), 14 steps, and edge - 255 free vortices -- the constructor's single zero-strength
    one for 256, mixed clouds of 257 and 1793 -- in ONE sweep: n + npan = edge - 10 + i behind step i of each member, so steps 9,
    10, 11 sit one below, on and one above the edge (the window is common to a sweep, hence the common steps)."""
    cases = []
    for edge in EDGES:
        kw = steps_kw(14, Npoints=246, LESPcrit=10.0)
        if edge > 256:
            kw.update(EI.mixed_cloud(edge - 255, seed=edge))
        cases.append(kw)
    return _sweep(cases, engine=eng, snapshot_steps=EI.dense_snapshots(15), integrals=True, energy_steps=(9, 12, 1))


@pytest.mark.parametrize("m", range(3), ids=[str(e) for e in EDGES])
def test_sources_on_and_around_an_edge(edge_sweep, m):
    sim, edge = edge_sweep[m], EDGES[m]
    assert sim.nt == 15 and sim.n_freevort == edge - 255 and not (sim.LEV_shed[1:] != -1).any()
    assert list(_source_counts(sim)[8:11]) == [edge - 1, edge, edge + 1]
    EI.check_member(sim, [9, 10, 11], f"sweep, sources across {edge}")
    if edge > 256:
        assert (EI.class_census(sim, [10])[EI.FREE] > (edge - 255) // 4).all()


# ---- 3. a mixed-sign cloud over five source tiles -------------------------------------------------------------------------------

def test_mixed_cloud_five_tiles_and_a_zero_strength_vortex(eng):
    cloud = EI.mixed_cloud(1100)
    cloud["circulation_freevort"][7] = 0.0
    g = cloud["circulation_freevort"]
    sim = _sweep([steps_kw(3, **cloud)], engine=eng, snapshot_steps=EI.dense_snapshots(4), integrals=True, energy_steps=(1, 4, 1))[0]
    ns = _source_counts(sim)
    assert sim.nt == 4 and 1024 < ns[0] and ns[-1] <= 1280
    EI.check_member(sim, [1, 2, 3], "sweep, 1100 free vortices")
    # Gamma = 0 counts in slot 0
    assert (g == 0.0).sum() == 1 and (g > 0.0).sum() > 400 and (g < 0.0).sum() > 400
    for i in range(4):
        assert sim.integral_sums[i, EI.FREE, 0, 0] == (g >= 0.0).sum() and sim.integral_sums[i, EI.FREE, 1, 0] == (g < 0.0).sum()


# ---- 4. the cap ------------------------------------------------------------------------------------------------------------------

def test_the_wake_cap(eng):
    """8190 free vortices and one step: cap = 8192 = LUDVM_ENSEMBLE_MAX_WAKE, the tag buffer's largest size; 8271 sources, 33
    strides of a lane.  Moments only: the long-double reference of one energy sample there (6.8e7 pairs, with their bound) is
    about 16 s of host work, more than a test of this suite may take, so the largest energy cases are the 2049 sources of the edge
    test and the mixed cloud above."""
    from ludvm_amd import _ffi
    sim = _sweep([steps_kw(1, **EI.mixed_cloud(8190, seed=3))], engine=eng, snapshot_steps=EI.dense_snapshots(2), integrals=True)[0]
    assert sim.nt == 2 and sim.n_freevort + 2 * (sim.nt - 1) == _ffi.ENSEMBLE_MAX_WAKE
    assert _source_counts(sim)[0] == 8190 + 1 + 80 and np.isnan(sim.wake_energy).all()
    EI.check_member(sim, (), "sweep, the 8192-vortex cap")
    assert sim.integral_sums[0, EI.FREE, :, 0].sum() == 8190 and (sim.integral_sums[1, EI.FREE, :, 0] > 3000).all()


# ---- 5. members of different nt, dt, nfree -----------------------------------------------------------------------------------------

class _Raw:
    """Keeps what the engine's ensemble calls return."""
    NAMES = ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
             "ensemble_run_surveyed_graded", "ensemble_run_integrals")

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


def test_ragged_members_land_at_their_own_offsets(eng):
    cases = [steps_kw(20), steps_kw(12, dt=0.03, method="Ramesh", k=0.4 * PI), steps_kw(16, **EI.mixed_cloud(300, seed=4))]
    win = (2, 18, 3)
    raw = _Raw(eng)
    try:
        sims = _sweep(cases, engine=eng, snapshot_steps=EI.dense_snapshots(21), integrals=True, energy_steps=win)
    finally:
        raw.close()
    assert [o[0] for o in raw.out] == ["ensemble_run_integrals"]
    desc, out = raw.out[0][1], raw.out[0][2]
    isums, energy = out[-2], out[-1]
    assert [s.nt for s in sims] == [21, 13, 17] and isums.shape == (51, 4, 2, 6) and energy.shape == (51,)
    for m, sim in enumerate(sims):
        nt, k0 = int(desc[m][0]), int(desc[m][1])
        assert sim.integral_sums.shape == (nt, 4, 2, 6) and sim.wake_energy.shape == (nt,)          # rows past nt do not exist
        assert not isums[k0].any() and np.isnan(energy[k0])                                        # row 0 is the host's
        assert np.array_equal(sim.integral_sums[1:], isums[k0 + 1:k0 + nt])
        assert np.array_equal(sim.wake_energy[1:], energy[k0 + 1:k0 + nt], equal_nan=True)
        assert sim.wake_energy_steps == (2, min(18, nt), 3)
        assert (_source_counts(sim) >= sim.n_freevort + np.arange(1, nt) + 80).all()
        EI.check_member(sim, EI.window_steps(win, nt), f"ragged sweep, member {m}")


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "plain", "binned", "graded"])
def test_nothing_else_moves(eng, mode):
    """A sweep of four members with 85 probes, 300 particles and -- but for 'none' -- a survey of 300 points (plain, with
    survey_phases=5, and with survey_grad=True as well), with and without integrals: every array the engine returns and every
    member's attributes are the same bit for bit."""
    cases = [dict(CONFIG1, tf=2.5), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15, k=2 * PI),
             dict(CONFIG1, tf=2.5, **gust_cloud())]
    snaps = (1, 2, 10, 45)
    rake = np.concatenate([probes32(), probes32()[:, ::-1] + 0.37, probes32()[:, :21] - 0.11], axis=1)
    seeds, rel = seeds_random(300), np.array([1, 20, 35, 10 ** 6], dtype=np.int64)[np.arange(300) % 4]
    obs = dict(snapshot_steps=snaps, probes=rake, probe_frame="tunnel", particles=seeds, particle_release=rel, particle_frame="tunnel")
    if mode != "none":
        obs.update(survey=seeds_random(300, seed=9), survey_frame="tunnel", survey_steps=(5, 120, 3))
    if mode in ("binned", "graded"):
        obs.update(survey_phases=5)
    if mode == "graded":
        obs.update(survey_grad=True)
    raw = _Raw(eng)
    try:
        without = _sweep(cases, engine=eng, **obs)
        with_ = _sweep(cases, engine=eng, **obs, integrals=True, energy_steps=(5, 120, 3))
    finally:
        raw.close()
    old = dict(none="ensemble_run_traced", plain="ensemble_run_surveyed", binned="ensemble_run_surveyed_binned",
               graded="ensemble_run_surveyed_graded")[mode]
    assert [o[0] for o in raw.out] == [old, "ensemble_run_integrals"]
    desc, a, b = raw.out[0][1], raw.out[0][2], raw.out[1][2]
    # (rows, wakes, wake_n, tracer_rows, probe_u, probe_w[, survey_sums[, bin_sums[, grad_sums, bin_grad_sums]]]); the new entry:
    # all ten of them (None where there is none), then integral_sums and energy
    assert len(a) == dict(none=6, plain=7, binned=8, graded=10)[mode] and len(b) == 12
    for q in range(len(a)):
        if q != 1:
            assert a[q] is not None and np.array_equal(a[q], b[q]) and np.abs(a[q]).max() > 0.0, q
    for q in range(len(a), 10):
        assert b[q] is None, q
    for m in range(desc.shape[0]):
        nt, _, nf, _, _, w0 = (int(v) for v in desc[m])
        cap = nf + 2 * (nt - 1)
        for r in range(len(snaps) + 1):
            n = int(a[2][m, r])
            for q in range(3):
                at = w0 + (3 * r + q) * cap
                assert n < 0 or np.array_equal(a[1][at:at + n], b[1][at:at + n]), (m, r, q)
    names = ("Cl", "Cd", "Cm", "Fn", "Fs", "M", "LESP", "LESP_prev", "LEV_shed", "fourier", "probe_u", "probe_w", "tracer_last")
    if mode != "none":
        names += ("survey_sums", "survey_mean_u", "survey_mean_w", "survey_uu", "survey_ww", "survey_uw")
    if mode in ("binned", "graded"):
        names += ("survey_bin_sums", "survey_bin_count", "survey_bin_of_step", "survey_bin_mean_u", "survey_bin_uw", "survey_coherent_uu")
    if mode == "graded":
        names += ("survey_grad_sums", "survey_bin_grad_sums", "survey_mean_omega", "survey_bin_mean_omega")
    for m, (s0, s1) in enumerate(zip(without, with_)):
        assert not hasattr(s0, "integral_sums") and s0.wake_integrals is False and s1.wake_integrals is True
        for name in names:
            assert np.array_equal(getattr(s0, name), getattr(s1, name), equal_nan=True), (m, name)
        if mode != "none":
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
        sampled = EI.window_steps((5, 120, 3), s1.nt)
        assert np.isfinite(s1.wake_energy[sampled]).all() and np.isnan(s1.wake_energy).sum() == s1.nt - len(sampled)
        assert (s1.integral_sums[1:, EI.BOUND, :, 0].sum(axis=1) == 80).all() and (s1.integral_sums[1:, EI.TEV, :, 0].sum(axis=1) > 0).all()


# ---- 7. bits -----------------------------------------------------------------------------------------------------------------------

def test_a_members_rows_do_not_depend_on_the_batch_or_the_window_and_repeat(eng):
    kw = steps_kw(24, **EI.mixed_cloud(200, seed=8))
    others = [steps_kw(12 + (q % 9), k=(0.1 + 0.01 * q) * PI, method="Ramesh" if q % 3 == 0 else "Faure") for q in range(63)]
    every = dict(engine=eng, integrals=True, energy_steps=(1, 25, 1))
    alone = _sweep([kw], **every)[0]
    assert alone.nt == 25 and np.isfinite(alone.wake_energy[1:]).all() and np.isnan(alone.wake_energy[0])
    for sim in (_sweep([kw] + others[:3], **every)[0], _sweep(others + [kw], **every)[-1], _sweep([kw], **every)[0]):
        assert np.array_equal(sim.integral_sums, alone.integral_sums) and np.array_equal(sim.wake_energy, alone.wake_energy, equal_nan=True)
    third = _sweep([others[0], kw], engine=eng, integrals=True, energy_steps=(1, 25, 3))[1]
    on = np.zeros(25, bool)
    on[1::3] = True
    assert np.array_equal(third.wake_energy[on], alone.wake_energy[on]) and np.isnan(third.wake_energy[~on]).all()
    assert np.array_equal(third.integral_sums, alone.integral_sums)
    none = _sweep([kw], engine=eng, integrals=True)[0]
    assert np.array_equal(none.integral_sums, alone.integral_sums) and np.isnan(none.wake_energy).all()


# ---- 8. against the solo march -----------------------------------------------------------------------------------------------------

def test_a_member_against_its_solo_march(eng):
    """The member and LUDVM(..., precision='f64', wake_integrals=True) differ by summation order only: each sum within the sum of
    the two runs' own bounds plus the twin term for wakes that agree to 1e-12 (asserted first)."""
    from ludvm_amd import LUDVM
    kw, win = steps_kw(28), (1, 29, 4)
    sim = _sweep([kw], engine=eng, snapshot_steps=EI.dense_snapshots(29), integrals=True, energy_steps=win)[0]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="full", wake_integrals=True, wake_energy_steps=win)
    assert_twin_and_member_agree(sim, solo, "solo march")
    EI.assert_circulations_agree(sim, solo, "solo march")
    assert sim.wake_energy_steps == solo.wake_energy_steps and np.array_equal(sim.integral_sums[0], solo.integral_sums[0])
    sampled = set(EI.window_steps(win, sim.nt))
    worst_m = worst_w = 0.0
    for i in range(1, sim.nt):
        e = i in sampled
        rm, rs = EI.reference(sim, i, energy=e), EI.reference(solo, i, energy=e)
        tm, tw = EI.twin_term(sim, i, e)
        assert np.array_equal(sim.integral_sums[i, :, :, 0], solo.integral_sums[i, :, :, 0])
        tol = (EI.moment_bound(rm) + EI.moment_bound(rs) + tm)[:, :, 1:]
        err = np.abs(sim.integral_sums[i] - solo.integral_sums[i])[:, :, 1:]
        assert not (err[tol == 0.0] != 0.0).any()
        worst_m = max(worst_m, float(np.max(np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), 0.0))))
        if e:
            worst_w = max(worst_w, abs(sim.wake_energy[i] - solo.wake_energy[i]) / (EI.W_bound(rm) + EI.W_bound(rs) + tw))
    print(f"member against its solo march: worst |difference| / (both bounds + twin term): moments {worst_m:.2e}, energy {worst_w:.2e}")
    assert worst_m <= 1.0 and worst_w <= 1.0
    assert np.array_equal(np.isnan(sim.wake_energy), np.isnan(solo.wake_energy))


# ---- 9. entry point ----------------------------------------------------------------------------------------------------------------

class _Tampered:
    """The engine's library with the arguments of the integrals call changed on their way in (what Engine never sends)."""

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


def _then(*changes):
    def change(a):
        for c in changes:
            a = c(a)
        return a
    return change


def test_the_library_answers_the_documented_codes_and_leaves_the_context_alone(eng):
    """What ludvm_ensemble_run_integrals refuses on the host (LUDVM_E_ARG) launches nothing: the resident wake of a solo run is
    still there and readable, and a solo wake_integrals=True run gives the same bits before and after a sweep with integrals on
    the same engine.  integral_doubles = 0 with both arrays null is the graded call itself.  (LUDVM_E_STATE of a sharded context
    needs two devices: not reached here.)"""
    from ludvm_amd import LUDVM, LudvmHipError, _ffi
    pts = seeds_random(37, seed=2)

    def solo():
        s = LUDVM(**dict(CONFIG1, tf=2.5, k=2 * PI), verbose=False, engine=eng, precision="f64", history="sparse", wake_integrals=True,
                  wake_energy_steps=(3, 45, 6))
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.integral_sums, np.nan_to_num(s.wake_energy)]
    limits = eng.ensemble_limits()
    before = solo()
    size = eng.wake_size()
    sims = _sweep([dict(CONFIG1, tf=2, method="Ramesh", k=PI), dict(CONFIG1, tf=2.5, alpha_m=5, alpha_max=15)], engine=eng,
                  snapshot_steps=(3,), survey=pts[:, ::-1] + 0.25, survey_frame="tunnel", probes=pts, particles=pts, survey_phases=7,
                  survey_grad=True, integrals=True, energy_steps=(2, 40, 5))
    assert all(np.isfinite(s.wake_energy[2:s.nt:5][:7]).all() and (s.survey_grad_sums[3] > 0.0).all() for s in sims)
    assert eng.wake_size() == size
    assert all(np.array_equal(a, b) for a, b in zip(before, solo()))

    lib = eng._lib
    # integral_doubles = 0 with both arrays null (and no window) is the graded call itself
    kw = dict(CONFIG1, tf=1)
    plain = _sweep([kw], engine=eng, survey=pts, survey_phases=3, survey_grad=True)[0]
    eng._lib = _Tampered(lib, lambda a: a[:-7] + [None, 0, None, 0, 0, 0, 0])
    try:
        same = _sweep([kw], engine=eng, survey=pts, survey_phases=3, survey_grad=True, integrals=True, energy_steps=(1, 9, 2))[0]
    finally:
        eng._lib = lib
    for name in ("Cl", "survey_sums", "survey_bin_sums", "survey_grad_sums", "survey_bin_grad_sums"):
        assert np.array_equal(getattr(same, name), getattr(plain, name)), name
    assert not same.integral_sums[1:].any()

    # a solo run's resident wake, then every refusal: the wake is still there and readable
    LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng, precision="f64", history="sparse")
    size = eng.wake_size()
    wake = eng.wake_read(0, size, gamma=True)
    assert size >= 20
    packed = _arrays(2)                 # 6 kinematics rows
    some, none = dict(energy_steps=(1, 3, 1)), dict()
    refusals = (
        ("null array", none, _set(-7, None)),                                               # sums null, count given
        ("null array", some, _set(-5, None)),                                               # energy null, count given
        ("kinematics rows x 48", none, _set(-6, lambda a: a[-6] + 1)),
        ("kinematics rows x 48", none, _set(-6, 0)),                                        # sums given, count 0
        ("one double per kinematics row", some, _set(-4, lambda a: a[-4] - 1)),
        ("one double per kinematics row", some, _set(-4, 0)),                               # energy given, count 0
        ("needs the integral sums", some, _then(_set(-7, None), _set(-6, 0))),              # energy without integrals
        ("needs the integral sums", none, _then(_set(-7, None), _set(-6, 0), _set(-1, 1))),
        ("first >= 1 and every >= 1", dict(energy_steps=(0, 3, 1)), None),
        ("first >= 1 and every >= 1", dict(energy_steps=(1, 3, 0)), None),                  # an energy array and every = 0
        ("null array", none, _set(-1, -1)),                                                 # every < 0 without an array
        ("first >= 1 and every >= 1", dict(energy_steps=(1, 3, -1)), None),
        ("holds no time step", dict(energy_steps=(3, 3, 1)), None),
        ("holds no time step", dict(energy_steps=(2, 1, 1)), None),
    )
    for word, kw, change in refusals:
        if change is not None:
            eng._lib = _Tampered(lib, change)
        try:
            with pytest.raises(LudvmHipError) as e:
                eng.ensemble_run_integrals(*packed, **kw)
        finally:
            eng._lib = lib
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))
        assert eng.wake_size() == size
    # 2 739 200 kinematics rows x 49 x 8 bytes of rows and energy: over 1 GiB, and the message gives the size (the count alone is
    # changed on its way in: the check comes before any array is read)
    eng._lib = _Tampered(lib, _then(_set(8, 2739200), _set(-6, 2739200 * 48)))
    try:
        with pytest.raises(LudvmHipError) as e:
            eng.ensemble_run_integrals(*packed)
    finally:
        eng._lib = lib
    assert e.value.code == _ffi.E_ARG and "over 1 GiB" in str(e.value) and "1024.0" in str(e.value), str(e.value)
    assert eng.ensemble_limits() == limits and eng.wake_size() == size
    for a, b in zip(wake, eng.wake_read(0, size, gamma=True)):
        assert np.array_equal(a, b)
