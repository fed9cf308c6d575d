"""GPU tier: the observer kernels behind march_solve -- march_probe_partial / _finish, march_tracer_partial / _finish,
march_survey_partial / _finish of the solo march, phases 2p and 2t of a sweep member -- checked BY VALUE at many source tiles:
splits that walk several 256-source tiles, up to 81 splits, ragged and empty last splits, a source count at a multiple of 256
and one either side of it, the probe finisher's strided leg, and the steps at which a launch plan changes form inside a run.
The cases, their arithmetic and the two observer sets are in tests/observer_sources_common.py; what the references rest on is
checked on the CPU in tests/test_observer_sources_host.py.

Case A is compared with the full Python oracle (the bounds of test_marched_series_matches_the_oracle, of
test_marched_paths_match_the_oracle and of survey_common); cases B and C with float64 sums over the sources the run's own dense
history states (the construction and bounds of test_overlapped_steps_probe_the_sources_of_their_own_roll_up and of its tracer
twin).  Every run asserts what its shapes rest on: no leading-edge vortex is shed, and the wake holds nfree + nt - 1 vortices
afterwards.

Measured worst values [MI355X] -- probe rows of max|u|, tracer rows of the largest displacement, survey means of max|u| /
raw second moments of max|u|^2 -- for the few | many set; the boundary steps named in the case table are printed by every test
and lie within these:
  case A vs the oracle           probes 8.5e-16 | 2.0e-15 (row 0: 5.8e-16 | 2.1e-15), tracers 2.0e-15 | 4.5e-15,
                                 survey 1.2e-16 / 1.2e-16 | 1.3e-15 / 1.2e-15; per-step path (few): 6.6e-16, 4.0e-15, 9.3e-17 / 8.7e-17
  case B vs its own sources      probes 9.8e-15 | 9.8e-15, tracers 1.8e-15 | 2.6e-15, survey 6.1e-16 / 4.2e-16 | 4.3e-15 / 3.5e-15
  case C vs its own sources      probes 9.3e-15 | 1.1e-14, tracers 5.6e-15 | 5.4e-15, survey 1.5e-15 / 1.4e-15 | 2.3e-15 / 2.8e-15
  case A as a sweep member       probes 5.7e-16 (row 0: 7.5e-16), particles 2.0e-15
  sweep member, 8000 vortices    probes 1.2e-15 of max|u| against the solo march, particles 7.8e-15 of the largest displacement
Every bound taken from the project holds at these source counts with five orders to spare; none was widened."""
import signal

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import (CASES, MEMBER_VS_SOLO, NPAN, PROBE_VS_SOURCES, ROW0_VS_ORACLE, SETS, TRACER_VS_SOURCES, CaseAOracle,
                                     case_keywords, cloud, euler_step_by, fast_iv, field, observers, probes4096, run_keywords)
from probes_common import probes32, series_error
from survey_common import MEAN_VS_ORACLE, MOMENT_VS_ORACLE, series_sums, series_umax, sums_errors, window
from tracers_common import releases_1_7_50, releases_by_tile, run_sources, seeds37, seeds_random

pytestmark = pytest.mark.gpu

ORACLE_SERIES = 1e-9            # of max|u| over steps 1 .. nt - 1: test_marched_series_matches_the_oracle
ORACLE_PATHS = 1e-9             # of the largest displacement: test_marched_paths_match_the_oracle


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
def oracle_a():
    return CaseAOracle()


def _run(eng, case, which, march=True):
    """One 'f64' run of `case` with the observers of set `which`, dense history; asserts what the case's shapes rest on."""
    from ludvm_amd import LUDVM
    nfree, steps = CASES[case][:2]
    obs = observers(case, which)
    sim = LUDVM(**case_keywords(case), verbose=False, engine=eng, precision="f64", history="full", march=march, **run_keywords(obs))
    size = eng.wake_size()
    print(f"case {case} ({which}{'' if march else ', per-step path'}): nt = {sim.nt}, LEV_shed == -1: {bool((sim.LEV_shed == -1).all())}, "
          f"wake size after the run {size} (nfree + nt - 1 = {nfree + sim.nt - 1})")
    assert sim.nt == steps + 1
    assert (sim.LEV_shed == -1).all(), "a leading-edge vortex was shed: ns(i) = nfree + i + 80 no longer holds (repair the cloud)"
    assert size == nfree + sim.nt - 1
    assert sim.tracer_path.steps() == list(range(sim.nt)) and sim.survey_count == len(window(*obs["window"], sim.nt))
    return sim, obs


@pytest.fixture(scope="module")
def runs(eng):
    """(case, set) -> (run, observers), made once."""
    made = {}

    def get(case, which):
        if (case, which) not in made:
            made[case, which] = _run(eng, case, which)
        return made[case, which]
    return get


def _report(label, case, per_step):
    """Prints the worst step and the case's boundary steps on their own -> the worst value."""
    worst = max(per_step, key=per_step.get)
    at = ", ".join(f"step {s}: {per_step[s]:.2e}" for s in CASES[case][2] if s in per_step)
    print(f"{label}: worst {per_step[worst]:.2e} (step {worst}); {at}")
    return per_step[worst]


# ---- case A: against the full oracle -------------------------------------------------------------------------------------------

def _check_a_probes(label, sim, oracle_a, which):
    ou, ow = oracle_a.series(which)
    steps = range(1, sim.nt)
    scale = max(np.abs(ou[1:]).max(), np.abs(ow[1:]).max())
    err = {i: max(np.abs(sim.probe_u[i] - ou[i]).max(), np.abs(sim.probe_w[i] - ow[i]).max()) / scale for i in steps}
    e0 = series_error(sim, ou, ow, 0, 0)
    _report(f"{label}: probe rows vs oracle / max|u|, row 0 {e0:.2e}", "A", err)
    for i in steps:
        assert err[i] <= ORACLE_SERIES, (i, err[i])
    assert e0 <= ROW0_VS_ORACLE, e0


def _check_a_tracers(label, sim, oracle_a, which, obs):
    rows, seeds, rel = oracle_a.tracer_rows(which), obs["tracers"], obs["release"]
    steps = range(1, sim.nt)
    disp = max(np.abs(rows[i] - seeds).max() for i in steps)
    err = {i: np.abs(sim.tracer_path[i] - rows[i]).max() / disp for i in steps}
    _report(f"{label}: tracer paths vs oracle / the largest displacement ({disp:.3f})", "A", err)
    assert disp > 0.0 and np.array_equal(sim.tracer_path[0], seeds)
    for i in steps:
        assert err[i] <= ORACLE_PATHS, (i, err[i])
        assert np.array_equal(sim.tracer_path[i][:, rel > i], seeds[:, rel > i]), i
    assert np.array_equal(sim.tracer_last, sim.tracer_path[sim.nt - 1])


def _check_a_survey(label, sim, oracle_a, which, obs):
    ou, ow = oracle_a.series(which, "survey")
    W = window(*obs["window"], sim.nt)
    ref, umax = series_sums(ou, ow, W), series_umax(ou, ow, W)
    e_mean, e_mom = sums_errors(sim.survey_sums[:, obs["pick"]], ref, len(W), umax)
    print(f"{label}: survey sums over steps {W[0]}-{W[-1]} at {len(obs['pick'])} of {sim.survey_sums.shape[1]} points vs oracle: means "
          f"{e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE, e_mean
    assert e_mom <= MOMENT_VS_ORACLE, e_mom
    assert np.isfinite(sim.survey_sums).all() and np.abs(sim.survey_sums[2]).min() > 0.0          # every point was written


@pytest.mark.parametrize("which", SETS)
def test_case_a_matches_the_oracle(runs, oracle_a, which):
    """Case A (nfree = 1180, 24 steps: five full splits, a sixth that is empty in steps 11-20 and holds one source from step 21,
    ns = 1280 exactly at step 20) with both observer sets against the full Python oracle: probe rows of steps 1-24 at 1e-9 of
    max|u| and row 0 at 1e-12, tracer paths at 1e-9 of the largest displacement, survey sums at survey_common's two bounds.
    Steps 10, 11, 20 and 21 are reported on their own."""
    sim, obs = runs("A", which)
    label = f"case A ({which})"
    _check_a_probes(label, sim, oracle_a, which)
    _check_a_tracers(label, sim, oracle_a, which, obs)
    _check_a_survey(label, sim, oracle_a, which, obs)


def test_case_a_on_the_per_step_path(eng, oracle_a):
    """march=False on the small set: the engine's per-step calls (other kernels) against the same oracle at the same bounds."""
    sim, obs = _run(eng, "A", "few", march=False)
    label = "case A (few, per-step path)"
    _check_a_probes(label, sim, oracle_a, "few")
    _check_a_tracers(label, sim, oracle_a, "few", obs)
    _check_a_survey(label, sim, oracle_a, "few", obs)


# ---- cases B and C: against the run's own sources ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def own_sources(runs):
    """(case, set) -> the errors of the run against float64 sums (the C oracle, at most 16 threads) over the sources its own dense
    history states for every step i >= 2, computed once: probe rows / the step's max|u|; tracer rows against the Euler step
    from the run's OWN previous row; the survey's five sums at the checked points."""
    made = {}

    def get(case, which):
        if (case, which) in made:
            return made[case, which]
        sim, obs = runs(case, which)
        iv, rel, pick = fast_iv(), obs["release"], obs["pick"]
        W = window(*obs["window"], sim.nt)
        assert W[0] >= 2
        su, sw = np.zeros([sim.nt, len(pick)]), np.zeros([sim.nt, len(pick)])
        probe, tracer, step_max, disp = {}, {}, 0.0, 0.0
        for i in range(2, sim.nt):
            src = run_sources(sim, i)
            assert len(src[0]) + len(src[3]) == CASES[case][0] + i + NPAN       # ns(i)
            u, w = field(iv, src, obs["probes"][0], obs["probes"][1], sim.v_core)
            scale = max(np.abs(u).max(), np.abs(w).max())
            probe[i] = max(np.abs(sim.probe_u[i] - u).max(), np.abs(sim.probe_w[i] - w).max()) / scale
            sd, before = sim._tracer_seeds(i), sim.tracer_path[i - 1]
            want = euler_step_by(iv, sd, before, rel, i, sim.dt, sim.v_core, src)
            tracer[i] = np.abs(sim.tracer_path[i] - want).max()
            assert np.array_equal(sim.tracer_path[i][:, rel > i], sd[:, rel > i]), i
            step_max = max(step_max, np.abs(want - np.where(rel == i, sd, before))[:, rel <= i].max())
            disp = max(disp, np.abs(sim.tracer_path[i] - sd).max())
            if i in W:
                su[i], sw[i] = field(iv, src, obs["survey"][0, pick], obs["survey"][1, pick], sim.v_core)
        made[case, which] = dict(probe=probe, tracer=tracer, step_max=step_max, disp=disp,
                                 survey=sums_errors(sim.survey_sums[:, pick], series_sums(su, sw, W), len(W), series_umax(su, sw, W)),
                                 window=W, points=(len(pick), sim.survey_sums.shape[1]))
        return made[case, which]
    return get


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("case", ["B", "C"])
def test_probe_rows_are_the_field_of_the_runs_own_sources(own_sources, case, which):
    """Every probe row i >= 2 against the float64 sum over the sources of step i: 1e-9 of the step's max|u|.  B: 64 splits
    at step 12, 65 from step 13 (the finisher's strided leg), the 65th empty until step 24 and with one source in step 25;
    with 4096 probes 16 splits of 1024, then 13 of 1280.  C: 80 / 81 splits; with 4096 probes 16 splits of 1280 (five tiles per workgroup), then 14 of 1536."""
    err = own_sources(case, which)["probe"]
    _report(f"case {case} ({which}): probe rows vs the run's own sources / max|u|", case, err)
    for i, e in err.items():
        assert e <= PROBE_VS_SOURCES, (i, e)


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("case", ["B", "C"])
def test_tracer_rows_are_the_euler_step_over_the_runs_own_sources(own_sources, case, which):
    """Every tracer row i >= 2 against the Euler step from the run's own row i - 1 over the sources of step i: 1e-9 of the
    largest displacement and 1e-7 of the largest single step (the two bounds of
    test_overlapped_steps_advect_by_the_sources_of_their_own_roll_up).  B: 64 splits of 256 at step 12, 33 of 512 from step 13.
    C: 40 splits of 512, 41 from step 6 with the last one empty until step 11."""
    got = own_sources(case, which)
    disp, step_max = got["disp"], got["step_max"]
    err = {i: e / disp for i, e in got["tracer"].items()}
    worst = _report(f"case {case} ({which}): tracer rows vs the Euler step over the run's own sources / the largest displacement "
                    f"({disp:.3e}; largest single step {step_max:.3e})", case, err)
    assert disp > 0.0 and step_max > 0.0
    for i, e in err.items():
        assert e <= TRACER_VS_SOURCES, (i, e)
    assert worst * disp <= 1e-7 * step_max, worst * disp / step_max


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("case", ["B", "C"])
def test_survey_sums_are_the_sums_of_the_field_of_the_runs_own_sources(own_sources, case, which):
    """The five sums over the window against the same sums of the float64 field of each step's sources, at every point of the
    600-point survey and at the sample of the 20481-point one (both ends of every 512-point tile): survey_common's bounds."""
    got = own_sources(case, which)
    (e_mean, e_mom), W = got["survey"], got["window"]
    print(f"case {case} ({which}): survey sums over steps {W[0]}-{W[-1]} at {got['points'][0]} of {got['points'][1]} points vs the "
          f"run's own sources: means {e_mean:.2e} of max|u|, raw second moments {e_mom:.2e} of max|u|^2")
    assert e_mean <= MEAN_VS_ORACLE, e_mean
    assert e_mom <= MOMENT_VS_ORACLE, e_mom


# ---- exact zeros: a split past the end of the sources ----------------------------------------------------------------------------

@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("case", list(CASES))
def test_an_empty_last_split_adds_exact_zeros(eng, runs, case, which):
    """A second run of the same case gives the same probe rows, tracer rows and survey sums, bit for bit -- in particular
    over the steps whose last split lies wholly past the end of the sources (A: 11-20; B: 13-24 for 32 probes; C: 6-10): the
    slab row of such a split still holds what the previous run's last steps left there, unless the kernel writes its zeros."""
    first, _ = runs(case, which)
    again, _ = _run(eng, case, which)
    for i in range(first.nt):
        assert np.array_equal(first.probe_u[i], again.probe_u[i]) and np.array_equal(first.probe_w[i], again.probe_w[i]), i
        assert np.array_equal(first.tracer_path[i], again.tracer_path[i]), i
    assert np.array_equal(first.survey_sums, again.survey_sums)
    print(f"case {case} ({which}): a second run repeats every probe row, tracer row and survey sum bit for bit")


# ---- sweep: phases 2p and 2t over many source tiles ----------------------------------------------------------------------------------

def test_a_sweep_member_with_the_cloud_matches_the_oracle(eng, oracle_a):
    """Case A as member 1 of a sweep (its arrays start at non-zero offsets behind a 20-step member), probes32() and seeds37()
    released at 1, 7 and 50: the member's probe rows and particle paths against the case-A oracle at the bounds of the solo run
    (six source tiles, ns = 1280 | 1281 at steps 20 | 21)."""
    from ludvm_amd import sweep
    seeds, rel = seeds37(), releases_1_7_50(37)
    sims = sweep([dict(CONFIG1, tf=1), case_keywords("A")], engine=eng, probes=probes32(), particles=seeds, particle_release=rel,
                 particle_steps=range(1, 25))
    sim = sims[1]
    assert sims[0].nt == 21 and sim.nt == 25 and (sim.LEV_shed == -1).all()
    assert sim.tracer_path.steps() == list(range(25))
    _check_a_probes("case A as a sweep member", sim, oracle_a, "few")
    _check_a_tracers("case A as a sweep member", sim, oracle_a, "few", dict(tracers=seeds, release=rel))


def test_a_sweep_member_at_32_source_tiles_against_its_solo_march(eng):
    """One member with 8000 free vortices over 10 steps (8081 .. 8090 sources: 32 tiles), 1024 probes and 4096 particles
    (released by tile of 256) against its solo precision='f64' march with the same points -- whose kernels cases B and C check
    by value: MEMBER_VS_SOLO of max|u| over steps 1-10 for the probe rows, of the largest displacement for the paths."""
    from ludvm_amd import LUDVM, sweep
    kw = dict(CONFIG1, tf=9.5 * CONFIG1["dt"], **cloud(8000))
    pts, seeds = probes4096()[:, :1024], seeds_random(4096, seed=5)
    rel = releases_by_tile(4096, 256, steps=(1, 5, 10 ** 6))
    sim = sweep([kw], engine=eng, probes=pts, particles=seeds, particle_release=rel, particle_steps=range(1, 11))[0]
    solo = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", probes=pts, tracers=seeds, tracer_release=rel,
                 tracer_steps=range(1, 11))
    assert sim.nt == solo.nt == 11 and np.array_equal(sim.LEV_shed, solo.LEV_shed)
    e_probe = series_error(sim, solo.probe_u, solo.probe_w, 1, 10)
    steps = range(1, 11)
    worst = max(np.abs(sim.tracer_path[s] - solo.tracer_path[s]).max() for s in steps)
    disp = max(np.abs(solo.tracer_path[s] - solo._tracer_seeds(s)).max() for s in steps)
    print(f"sweep member (8000 free vortices) vs solo march, steps 1-10: probe rows {e_probe:.2e} of max|u|, particle paths "
          f"{worst / disp:.2e} of the largest displacement ({disp:.3e}); LEV shed: {bool((sim.LEV_shed != -1).any())}")
    e0 = series_error(sim, solo.probe_u, solo.probe_w, 0, 0)          # (8000 free vortices: the two sum row 0 in orders of their own)
    assert e0 <= ROW0_VS_ORACLE and np.array_equal(sim.tracer_path[0], seeds) and np.array_equal(solo.tracer_path[0], seeds), e0
    assert e_probe <= MEMBER_VS_SOLO, e_probe
    assert disp > 0.0 and worst <= MEMBER_VS_SOLO * disp, worst / disp
    for s in steps:
        assert np.array_equal(sim.tracer_path[s][:, rel > s], seeds[:, rel > s]), s
