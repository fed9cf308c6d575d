"""GPU tier of G11 (tests/observers_off_unit_common.py): the observer kernels -- probes, passive tracers (float64 and 'f32x2'), the
tracers' deformation gradient, the wake survey (float64 and 'f32') with its gradient sums and phase bins in the solo march,
phases 2p / 2t / 2s of a sweep member -- on G10's cases, where chord, Uinf, dt and v_core differ from config 1's and sections
are cambered.  Every other GPU test of an observer builds its run from CONFIG1: there a sweep member's dt, vc4 and shift row
equal every other member's, v_core is 0.065 wherever a rule is stated in cores, xpiv is -t, and the bound vortices lie on the
chord line.

Every bound is one the project already states, imported from the module that defines it; the CPU tier
(tests/test_observers_off_unit_host.py) shows that the host loop stays 10 x inside the oracle bounds over the compared steps
and that a kernel reading a foreign dt, v_core, shift row, chord-line section or unit-point frequency would miss them by at
least 100 x."""
import signal
import warnings

import numpy as np
import pytest

import survey_gradient_common as SG
import tracer_gradient_common as TG
from observer_sources_common import MEMBER_VS_SOLO, PROBE_VS_SOURCES, ROW0_VS_ORACLE, TRACER_VS_SOURCES, field
from observers_off_unit_common import (BIN_CASES, F_ROW_VS_INCREMENT, FP32_CASES, FRAMES, GUARD_STEP, PROBE_VS_ORACLE, SOLO_CASES,
                                       SOURCES_CASES, STEPS, SWEEP, SWEEP_F, SWEEP_PAIRS, TRACER_VS_ORACLE, WINDOW, OracleRun, bin_settings,
                                       case_keywords, errors, exact_bin_table, guard_case, observers, of_run, reference, run_keywords,
                                       stored_sources, sweep_observers)
from oracle import g10_cases as G10
from oracle import ludvm_oracle as O
from survey_bins_common import check_bin_derived, check_bins_against_probes
from survey_common import (MEAN_VS_ORACLE, MEAN_VS_PROBES, MOMENT_VS_ORACLE, MOMENT_VS_PROBES, check_derived, series_sums, series_umax,
                           sums_errors, window)
from survey_f32_common import GUARDED_VS_F64, MAX_EXTENT, MEAN_VS_F64, MOMENT_VS_F64, local_f32_field
from tracers_common import euler_step, run_sources
from tracers_f32x2_common import STEP_ROUNDING, STEP_VS_F64

pytestmark = pytest.mark.gpu

ORACLE_BOUNDS = (PROBE_VS_ORACLE, TRACER_VS_ORACLE, MEAN_VS_ORACLE, MOMENT_VS_ORACLE)
WINDOWS = {"lab": (2, STEPS + 1, 1), "tunnel": (3, STEPS + 1, 4)}       # the survey windows (2, nt, 1) and (3, nt, 4) of a 50-step run


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


@pytest.fixture(scope="module")
def oracle():
    """(name, method or None) -> OracleRun over 50 steps, made once."""
    made = {}

    def get(name, method=None):
        if (name, method) not in made:
            made[name, method] = OracleRun(name) if method is None else OracleRun(name, method=method)
        return made[name, method]
    return get


def _solo(eng, kw, **extra):
    from ludvm_amd import LUDVM
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered section's "mean line unpinned" warning
        return LUDVM(**kw, verbose=False, engine=eng, **extra)


def _against_the_oracle(label, sim, ref, n):
    e = errors(of_run(sim), ref, 1, n)
    print(f"G11 {label} vs oracle, steps 1-{n}: probes {e[0]:.2e} of max|u|, tracers {e[1]:.2e} of the largest displacement, "
          f"survey means {e[2]:.2e} of max|u|, raw second moments {e[3]:.2e} of max|u|^2")
    for v, bound in zip(e, ORACLE_BOUNDS):
        assert v <= bound, (label, e)
    return e


def _frames_are_exact(sim, obs, frame, Uinf):
    """probe_positions, _tracer_seeds and tracer_released against xpiv = -Uinf t, exactly."""
    assert np.array_equal(sim.xpiv, -Uinf * sim.t) and (Uinf == 1 or not np.array_equal(sim.xpiv, -sim.t))
    for s in (0, 1, 7, STEPS):
        sh = sim.xpiv[s] if frame == "tunnel" else 0.0
        assert np.array_equal(sim.probe_positions(s), np.stack([obs["probes"][0] + sh, obs["probes"][1]])), s
        assert np.array_equal(sim._tracer_seeds(s), np.stack([obs["tracers"][0] + sh, obs["tracers"][1]])), s
        assert np.array_equal(sim.tracer_released(s), obs["release"] <= s), s
        if s:                   # a held tracer sits on the seed of its step
            held = obs["release"] > s
            assert np.array_equal(sim.tracer_path[s][:, held], sim._tracer_seeds(s)[:, held]), s


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", SOLO_CASES)
def test_solo_observers_match_the_oracle(eng, oracle, name, frame):
    """A 50-step precision='f64' march of the case carrying probes32(), seeds37() (released at 1, 7, 50) and a 600-point survey,
    all in the case's chords and in `frame`, against the oracle over steps 1-50: probe rows at 1e-9 of max|u|, tracer rows at
    1e-9 of the largest displacement, the survey (window (2, nt, 1) in the lab frame, (3, nt, 4) in the tunnel's) at
    MEAN_VS_ORACLE / MOMENT_VS_ORACLE; row 0 at 1e-12; probe_positions, _tracer_seeds and tracer_released exactly, with
    xpiv = -Uinf t.
    Measured [MI355X], worst of the eight runs: probes 4.0e-15 (c2412, lab), tracers 1.6e-15, survey means 1.2e-15 / raw second
    moments 1.4e-15 (d23, tunnel); row 0: 0."""
    run, obs = oracle(name), observers(name)
    sim = _solo(eng, case_keywords(name, STEPS), precision="f64", history="full", **run_keywords(obs, frame, WINDOWS[frame]))
    ref = reference(run, obs, frame, WINDOWS[frame])
    assert sim.nt == STEPS + 1 and sim.v_core == run.v_core and sim.dt == run.dt and sim.survey_count == len(ref["W"])
    assert sim.tracer_path.steps() == list(range(sim.nt))
    _against_the_oracle(f"{name} solo march ({frame})", sim, ref, WINDOW[name])
    scale = max(np.abs(ref["u"][1:]).max(), np.abs(ref["w"][1:]).max())
    e0 = max(np.abs(sim.probe_u[0] - ref["u"][0]).max(), np.abs(sim.probe_w[0] - ref["w"][0]).max()) / scale
    print(f"G11 {name} solo march ({frame}): row 0 {e0:.2e} of max|u|")
    assert e0 <= ROW0_VS_ORACLE and np.array_equal(sim.tracer_path[0], ref["seeds"][0])
    _frames_are_exact(sim, obs, frame, run.Uinf)
    check_derived(sim)


@pytest.mark.parametrize("mode", ["f64", "f32_overlapped"])
@pytest.mark.parametrize("name", SOURCES_CASES)
def test_every_step_over_the_runs_own_sources(eng, name, mode):
    """The case's full run (200 steps; `c2412f`: 100, the 127-point section with 120 free vortices) with the dense history,
    every step 2 .. nt - 1 against float64 sums over the sources the run states itself (tracers_common.run_sources): probe rows
    -- at probes32() and at the survey's 600 points -- at PROBE_VS_SOURCES of the step's max|u|; tracer rows as the Euler step
    from the run's own row before at TRACER_VS_SOURCES of the largest displacement; the survey as the reduction of the run's
    own probe rows at MEAN_VS_PROBES / MOMENT_VS_PROBES; the deformation gradient by rows_against_the_recursion (1e-9 of max|F|,
    1e-7 of the largest increment); the survey's gradient sums at every sixth point against the long-double terms at MEAN_BOUND
    / SQUARE_BOUND.  'f64': serial steps, tunnel frame, window (2, nt, 1).  'f32_overlapped': precision='f32' with the symmetric
    threshold at 64 (overlapped steps from about step 50 on), lab frame, window (3, nt, 4).
    Measured [MI355X], worst of the six runs: probes 2.6e-15, tracers 2.3e-16 (largest displacement 1.9 .. 19.8), survey vs probe
    rows 0 / 3.5e-17, F rows 1.8e-16 of max|F| and 3.9e-15 of the largest increment, gradient sums 8.8e-17 / 1.4e-16."""
    obs = observers(name)
    kw = case_keywords(name)
    nt = G10.BY_NAME[name]["steps"] + 1
    frame, steps = ("tunnel", (2, nt, 1)) if mode == "f64" else ("lab", (3, nt, 4))
    probes = np.concatenate([obs["probes"], obs["survey"]], axis=1)
    extra = dict(history="full", tracer_gradient=True, survey_gradient=True,
                 **run_keywords(dict(obs, probes=probes), frame, steps))
    if mode == "f64":
        sim = _solo(eng, kw, precision="f64", **extra)
    else:
        eng.set_symmetric(64)
        try:
            sim = _solo(eng, kw, precision="f32", **extra)
        finally:
            eng.set_symmetric(1)
    rel = obs["release"]
    W = window(*steps, nt)
    assert sim.nt == nt and nt in (101, 201) and sim.survey_count == len(W) and sim.tracer_path.steps() == list(range(nt))
    src = {i: run_sources(sim, i) for i in range(2, nt)}
    e_probe = e_tracer = disp = 0.0
    for i in range(2, nt):
        pos = sim.probe_positions(i)
        u, w = field(O.induced_velocity, src[i], pos[0], pos[1], sim.v_core)
        scale = max(np.abs(u).max(), np.abs(w).max())
        e_probe = max(e_probe, max(np.abs(sim.probe_u[i] - u).max(), np.abs(sim.probe_w[i] - w).max()) / scale)
        sd = sim._tracer_seeds(i)
        want = euler_step(sd, sim.tracer_path[i - 1], rel, i, sim.dt, sim.v_core, src[i])
        e_tracer = max(e_tracer, np.abs(sim.tracer_path[i] - want).max())
        disp = max(disp, np.abs(sim.tracer_path[i] - sd).max())
        assert np.array_equal(sim.tracer_path[i][:, rel > i], sd[:, rel > i]), i
    e_tracer /= disp
    su, sw = sim.probe_u[:, 32:], sim.probe_w[:, 32:]
    e_mean, e_mom = sums_errors(sim.survey_sums, series_sums(su, sw, W), len(W), series_umax(su, sw, W))
    f_worst, fmax, inc = TG.rows_against_the_recursion(sim, rel, range(2, nt), lambda i: src[i])
    pick = np.arange(0, 600, 6)
    gref, gmax, _ = SG.reference_sums(W, lambda i: tuple(c[pick] for c in sim._survey_points(i)), lambda i: src[i], sim.v_core)
    g_mean, g_sq = SG.sums_errors(sim.survey_grad_sums.reshape(5, -1)[:, pick], gref, len(W), gmax)
    print(f"G11 {name} {mode}, steps 2-{nt - 1} over the run's own sources: probes {e_probe:.2e} of max|u|, tracers {e_tracer:.2e} of the "
          f"largest displacement ({disp:.3f}), survey vs probe rows {e_mean:.2e} / {e_mom:.2e}, F rows {f_worst / fmax:.2e} of max|F| "
          f"and {f_worst / inc:.2e} of the largest increment, gradient sums {g_mean:.2e} of max|grad u| / {g_sq:.2e} of its square")
    assert e_probe <= PROBE_VS_SOURCES, e_probe
    assert disp > 0.0 and e_tracer <= TRACER_VS_SOURCES, e_tracer
    assert e_mean <= MEAN_VS_PROBES and e_mom <= MOMENT_VS_PROBES, (e_mean, e_mom)
    assert inc > 1e-6 and f_worst <= SG.MEAN_BOUND * fmax and f_worst <= F_ROW_VS_INCREMENT * inc, (f_worst, fmax, inc)
    assert gmax > 0.0 and g_mean <= SG.MEAN_BOUND and g_sq <= SG.SQUARE_BOUND, (g_mean, g_sq)
    check_derived(sim)
    SG.check_derived(sim)


def _f32x2_rows(sim, rel):
    """Every row i >= 2 of an 'f32x2' run against the float64 Euler step from the run's OWN row i - 1 over the step's own sources
    (the construction of tests/test_gpu_tracers_f32x2.py) -> (worst excess over STEP_VS_F64 x the step's largest single step +
    STEP_ROUNDING x the largest displacement, worst |difference| / the largest single step of its step)."""
    found = []
    for i in range(2, sim.nt):
        sd, prev = sim._tracer_seeds(i), sim.tracer_path[i - 1]
        want = euler_step(sd, prev, rel, i, sim.dt, sim.v_core, run_sources(sim, i))
        free = rel <= i
        start = np.where(rel == i, sd, prev)
        found.append((np.abs(sim.tracer_path[i] - want).max(), np.abs(want - start)[:, free].max(), np.abs(sim.tracer_path[i] - sd).max()))
        assert np.array_equal(sim.tracer_path[i][:, ~free], sd[:, ~free]), i
    diff, step, disp = (np.array(c) for c in zip(*found))
    return (diff - (STEP_VS_F64 * step + STEP_ROUNDING * disp.max())).max(), (diff / step).max()


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_observers_at_other_core_radii(eng, name):
    """v_core = 0.13 (`d23`) and 0.0325 (`dhalf`): the rules stated in cores have run at 0.065 only.  100 steps, tunnel frame:
    survey_precision='f32' against the float64 survey of the same run at MEAN_VS_F64 / MOMENT_VS_F64 (max|u| from the run's
    probe rows at the survey's points), and tracer_precision='f32x2' with every row a float64 Euler step of the row before at
    STEP_VS_F64 of the step's largest single step (+ STEP_ROUNDING of the largest displacement).
    The guard: a 4-step run whose every origin class at the sampled step 3 is 14.08 wide on `dhalf` (between 300 x 0.0325 and
    300 x 0.065) and 28.16 wide on `d23` (between 300 x 0.065 and 300 x 0.13) -- observers_off_unit_common.guard_case.  The
    model local_f32_field with the run's v_core says: every class guarded on `dhalf`, none on `d23`.  So on `dhalf` the fp32
    survey is the float64 survey, and the model, to GUARDED_VS_F64; on `d23` it is within MEAN_VS_F64 of both and MORE than
    GUARDED_VS_F64 from the float64 survey (the fp32 loop ran).  A kernel that took 0.065 for the core would fail one or the
    other (the CPU tier: the model at 0.065 decides the opposite way).
    Measured [MI355X]: d23 survey 1.4e-8 / 1.5e-8, tracer rows 6.8e-7 of the step's largest single step; guard run: no class
    guarded, 5.4e-8 / 7.2e-8 from the model, 1.6e-7 / 7.9e-8 from the float64 survey.  dhalf survey 1.4e-8 / 1.7e-8, tracer rows
    5.5e-7; guard run: 4 of 4 classes guarded, 3.3e-16 / 3.3e-16 from the model, 4.9e-16 / 9.6e-16 from the float64 survey."""
    obs = observers(name)
    kw = case_keywords(name, 100)
    common = dict(precision="f64", history="full", probes=obs["survey"], probe_frame="tunnel", survey=obs["survey"], survey_frame="tunnel",
                  survey_steps=(2, 101, 1), tracers=obs["tracers"], tracer_release=obs["release"], tracer_frame="tunnel")
    ref = _solo(eng, kw, **common)
    sim = _solo(eng, kw, survey_precision="f32", tracer_precision="f32x2", **common)
    assert sim.nt == 101 and sim.survey_count == ref.survey_count == 99 and np.array_equal(sim.Cl, ref.Cl)
    umax = series_umax(ref.probe_u, ref.probe_w, window(2, 101, 1, 101))
    e_mean, e_mom = sums_errors(sim.survey_sums, ref.survey_sums, 99, umax)
    excess, worst = _f32x2_rows(sim, obs["release"])
    print(f"G11 {name} v_core = {sim.v_core:.4f}: fp32 survey vs float64 survey {e_mean:.2e} of max|u| / {e_mom:.2e} of max|u|^2; "
          f"f32x2 tracer rows vs a float64 Euler step of the row before {worst:.2e} of the step's largest single step")
    assert not np.array_equal(sim.survey_sums, ref.survey_sums) and not np.array_equal(sim.tracer_last, ref.tracer_last)
    assert e_mean <= MEAN_VS_F64 and e_mom <= MOMENT_VS_F64, (e_mean, e_mom)
    assert excess <= 0.0, (excess, worst)

    gkw, pts = guard_case(name)
    gcommon = dict(precision="f64", history="full", survey=pts, survey_steps=(GUARD_STEP, GUARD_STEP + 1, 1))
    gref = _solo(eng, gkw, **gcommon)
    gsim = _solo(eng, gkw, survey_precision="f32", **gcommon)
    assert gsim.survey_count == gref.survey_count == 1 and gsim.nt == GUARD_STEP + 2
    g, x, z = stored_sources(gref, GUARD_STEP)
    u, w, guarded, classes = local_f32_field(g, x, z, pts[0], pts[1], gsim.v_core, max_extent=MAX_EXTENT)
    model = np.stack([u, w, u * u, w * w, u * w])
    gmax = np.abs(gref.survey_sums[:2]).max()
    m_mean, m_mom = sums_errors(gsim.survey_sums, model, 1, gmax)
    f_mean, f_mom = sums_errors(gsim.survey_sums, gref.survey_sums, 1, gmax)
    print(f"G11 {name} guard run: {guarded} of {classes} classes guarded by the model; fp32 survey vs the model {m_mean:.2e} / {m_mom:.2e}, "
          f"vs the float64 survey {f_mean:.2e} / {f_mom:.2e} (of max|u| / max|u|^2)")
    assert classes == 4
    if name == "dhalf":
        assert guarded == classes
        assert m_mean <= GUARDED_VS_F64 and m_mom <= 3 * GUARDED_VS_F64, (m_mean, m_mom)
        assert f_mean <= GUARDED_VS_F64 and f_mom <= 3 * GUARDED_VS_F64, (f_mean, f_mom)
    else:
        assert guarded == 0
        assert m_mean <= MEAN_VS_F64 and m_mom <= MOMENT_VS_F64, (m_mean, m_mom)
        assert GUARDED_VS_F64 < f_mean <= MEAN_VS_F64 and f_mom <= MOMENT_VS_F64, (f_mean, f_mom)


@pytest.mark.parametrize("setting", bin_settings(), ids=["B8", "B5_phase0"])
@pytest.mark.parametrize("name", BIN_CASES)
def test_integer_bins_off_the_unit_point(eng, name, setting):
    """survey_bins = 8 (window (2, nt, 1)) and 5 with survey_phase0 (window (3, nt, 4)) over the case's 200 steps -- `d23`: 200
    steps per period; `k45`: 133 1/3, the first use of the integer rule on a period that is no whole number of steps, and the first
    with chord and Uinf in f.  The table is the exact-arithmetic one of the CPU tier at every sampled step; every bin is the
    reduction of the run's own probe rows at MEAN_VS_PROBES / MOMENT_VS_PROBES; the derived attributes hold; bin 3 is
    bit-identical to the survey of a run given bin 3's steps through an explicit table.
    Measured [MI355X]: bins vs the run's own probe rows: means 0, raw second moments at most 1.1e-16 of max|u|^2; counts d23
    24 + 7 x 25 | 5 x 10, k45 31, 34, 33, 33, 18, 16, 17, 17 | 13, 14, 7, 7, 9."""
    kw = case_keywords(name)
    pts = observers(name)["survey"]
    B = setting["survey_bins"]
    steps = (2, 201, 1) if B == 8 else (3, 201, 4)
    common = dict(precision="f64", history="sparse", probes=pts, probe_frame="tunnel", survey=pts, survey_frame="tunnel", survey_steps=steps)
    sim = _solo(eng, kw, **common, **setting)
    table, decided = exact_bin_table(sim.t, kw, B, setting.get("survey_phase0"))
    sampled = sim.survey_bin_of_step >= 0
    assert sim.nt == 201 and sampled.sum() == len(window(*steps, 201)) == sim.survey_count and decided[sampled].all()
    assert np.array_equal(sim.survey_bin_of_step[sampled], table[sampled])
    assert (sim.survey_bin_count > 0).all() and np.array_equal(sim.survey_phase, (np.arange(B) + 0.5) / B)
    check_bins_against_probes(sim, f"G11 {name} B = {B}")
    check_bin_derived(sim)
    only3 = np.where(sim.survey_bin_of_step == 3, 0, -1).astype(np.int64)
    one = _solo(eng, kw, **common, survey_bins=only3)
    assert one.survey_nbins == 1 and one.survey_bin_count[0] == sim.survey_bin_count[3] > 0
    assert np.array_equal(one.survey_bin_sums[0], sim.survey_bin_sums[3])
    assert np.array_equal(one.survey_sums, sim.survey_sums)
    print(f"G11 {name} B = {B}: counts {sim.survey_bin_count.tolist()}; bin 3 repeats bit for bit through an explicit table")


def _sweep(eng, batch, obs, frame):
    from ludvm_amd import sweep
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered sections' "mean line unpinned" warning
        return sweep(batch, engine=eng, probes=obs["probes"], probe_frame=frame, particles=obs["tracers"], particle_release=obs["release"],
                     particle_frame=frame, particle_steps=range(1, STEPS + 1), survey=obs["survey"], survey_frame=frame,
                     survey_steps=WINDOWS[frame])


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("which", ["seven_81_point_cases", "c2412f_faure_ramesh"])
def test_mixed_sweep_observers(eng, oracle, which, frame):
    """ONE sweep of d23, c2412, d23r, dhalf, k45, c6409, c4412d -- three chords, three speeds, three dts, three core radii, 100
    and 200 steps, both methods, cambered and symmetric sections, every member differing from both neighbours in dt, Uinf and
    v_core -- with probes, particles (released at 1, 7, 50) and a survey common to the sweep, the points one set in chords of
    2, 1 and 0.5; and a second sweep of the 127-point `c2412f`, 'Faure' beside 'Ramesh'.  Each member's dt, vc4 and shift row
    are its own (ens_probe_row, ens_tracer_step, ens_survey_step): each member against ITS oracle over steps 1-50 at 1e-9 /
    1e-9 / MEAN_VS_ORACLE / MOMENT_VS_ORACLE, against its solo 'f64' march over steps 1-10 at MEMBER_VS_SOLO (probe rows of
    max|u|, particle rows of the largest displacement), and the batch reversed gives every member the same bits.
    Measured [MI355X]: against the oracle, worst member k45 in the lab frame: probes 6.0e-13, particles 5.1e-14, survey
    5.2e-14 / 3.3e-14 (c6409: 5.1e-14, 6.5e-15, 2.8e-15 / 1.1e-15; every other member below 5e-15); against the solo march:
    probes at most 1.0e-15, particles at most 7.1e-16 (c2412f 'Ramesh': 1.4e-14).  No member read a neighbour's dt, vc4 or
    shift row: the CPU tier puts each of those at 3.7e-3 .. 2.7 of the same scales."""
    obs = sweep_observers() if which.startswith("seven") else observers("c2412f")
    members = [(n, None) for n in SWEEP] if which.startswith("seven") else [(SWEEP_F[0], None), (SWEEP_F[1], "Ramesh")]
    batch = [case_keywords(n) if m is None else case_keywords(n, method=m) for n, m in members]
    sims = _sweep(eng, batch, obs, frame)
    back = _sweep(eng, batch[::-1], obs, frame)[::-1]
    if which.startswith("seven"):
        for a, b in SWEEP_PAIRS:
            assert sims[a].xpiv[7] != sims[b].xpiv[7] and sims[a].dt != sims[b].dt and sims[a].v_core != sims[b].v_core, (a, b)
        assert {s.nt for s in sims} == {101, 201}
    else:
        assert sims[0].Npoints == 127 and sims[0].n_freevort == 120 and not np.array_equal(sims[0].Cl, sims[1].Cl)
    for k, ((name, method), sim, rev) in enumerate(zip(members, sims, back)):
        label = f"{name}{'' if method is None else ' ' + method} as member {k} ({frame})"
        run = oracle(name, method)
        ref = reference(run, obs, frame, WINDOWS[frame])
        assert sim.survey_count == len(ref["W"]) and sim.tracer_path.steps()[:STEPS + 1] == list(range(STEPS + 1))
        _against_the_oracle(label, sim, ref, WINDOW[name])
        assert np.array_equal(sim.tracer_path[0], ref["seeds"][0])
        check_derived(sim)
        # the same bits wherever the member stands
        assert np.array_equal(sim.probe_u, rev.probe_u) and np.array_equal(sim.probe_w, rev.probe_w), label
        assert all(np.array_equal(sim.tracer_path[s], rev.tracer_path[s]) for s in sim.tracer_path.steps()), label
        assert np.array_equal(sim.survey_sums, rev.survey_sums) and np.array_equal(sim.tracer_last, rev.tracer_last), label
        # its solo march over 10 steps
        kw10 = case_keywords(name, 10) if method is None else case_keywords(name, 10, method=method)
        solo = _solo(eng, kw10, precision="f64", history="full", probes=obs["probes"], probe_frame=frame, tracers=obs["tracers"],
                     tracer_release=obs["release"], tracer_frame=frame)
        sl = slice(1, 11)
        scale = max(np.abs(solo.probe_u[sl]).max(), np.abs(solo.probe_w[sl]).max())
        e_probe = max(np.abs(sim.probe_u[sl] - solo.probe_u[sl]).max(), np.abs(sim.probe_w[sl] - solo.probe_w[sl]).max()) / scale
        disp = max(np.abs(solo.tracer_path[s] - solo._tracer_seeds(s)).max() for s in range(1, 11))
        e_path = max(np.abs(sim.tracer_path[s] - solo.tracer_path[s]).max() for s in range(1, 11)) / disp
        print(f"G11 {label} vs its solo march, steps 1-10: probes {e_probe:.2e} of max|u|, particles {e_path:.2e} of the largest "
              f"displacement")
        assert e_probe <= MEMBER_VS_SOLO and e_path <= MEMBER_VS_SOLO, (label, e_probe, e_path)
