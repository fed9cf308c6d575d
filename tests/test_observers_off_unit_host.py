"""CPU tier of G11 (tests/observers_off_unit_common.py): the observers off the unit point, on the fake engine and the oracle.
It licenses the bounds the GPU tier (tests/test_gpu_observers_off_unit.py) asserts -- the host loop, which differs from the
oracle by summation order only, stays 10 x inside each over the compared window -- and proves that the inputs can tell a
subtly wrong kernel from a right one: every mutation of the list below moves the quantity it touches by at least 100 x the
bound the GPU tier applies to it.  The bin table is checked against the rule in exact rational arithmetic, and the fp32
survey's model makes the opposite guard decision at config 1's core radius."""
import warnings

import numpy as np
import pytest

from observers_off_unit_common import (BIN_CASES, CASES, FP32_CASES, FRAMES, GUARD_EXTENT, GUARD_STEP, MARGIN, PROBE_VS_ORACLE,
                                       SENSITIVITY, STEPS, SWEEP, SWEEP_PAIRS, TRACER_VS_ORACLE, WINDOW, OracleRun, bin_settings,
                                       case_keywords, errors, exact_bin_table, guard_case, observers, of_run, reference, run_keywords,
                                       stored_sources, sweep_observers, unit_frequency, v_core_of)
from oracle import g10_cases as G10
from survey_common import MEAN_VS_ORACLE, MEAN_VS_PROBES, MOMENT_VS_ORACLE, series_sums
from survey_f32_common import MAX_EXTENT, local_f32_field

BOUNDS = (PROBE_VS_ORACLE, TRACER_VS_ORACLE, MEAN_VS_ORACLE, MOMENT_VS_ORACLE)
NAMES = ("probes", "tracers", "survey means", "survey moments")
UNIT = dict(dt=0.05, v_core=0.065)


@pytest.fixture(scope="module")
def oracle():
    """name -> OracleRun over 50 steps, made once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = OracleRun(name)
        return made[name]
    return get


def _host(kw, **extra):
    from fake_engine import FakeEngine
    from ludvm_amd import LUDVM
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered section's "mean line unpinned" warning
        return LUDVM(**kw, verbose=False, engine=FakeEngine(), **extra)


def test_the_cases_are_off_the_unit_point():
    """What the tiers rest on: the point sets are config 1's in chords, and the table gives the scales the issue names."""
    got = {n: case_keywords(n) for n in CASES}
    assert (got["d23"]["chord"], got["d23"]["Uinf"], got["d23"]["method"]) == (2, 3, "Faure")
    assert (got["dhalf"]["chord"], got["dhalf"]["Uinf"], got["dhalf"]["dt"]) == (0.5, 2, 0.0125)
    assert (got["c4412d"]["Naca"], got["c4412d"]["chord"], got["c4412d"]["Uinf"], got["c4412d"]["method"]) == ("4412", 2, 3, "Ramesh")
    assert (got["c2412"]["Naca"], got["c2412"]["chord"], got["c2412"]["Uinf"], got["c2412"]["dt"]) == ("2412", 1, 1, 0.05)
    assert got["c2412f"]["Npoints"] == 127 and len(got["c2412f"]["circulation_freevort"]) == 120
    assert abs(v_core_of(got["d23"]) - 0.13) < 1e-15 and abs(v_core_of(got["dhalf"]) - 0.0325) < 1e-15
    steps_per_period = {n: 2 * np.pi * got[n]["chord"] / (got[n].get("k", 0.2 * np.pi) * got[n]["Uinf"]) / got[n]["dt"] for n in BIN_CASES}
    assert abs(steps_per_period["d23"] - 200) < 1e-9 and abs(steps_per_period["k45"] - 400 / 3) < 1e-9
    sw = [case_keywords(n) for n in SWEEP]
    assert len({k["chord"] for k in sw}) == 3 and len({k["Uinf"] for k in sw}) == 3 and len({k["dt"] for k in sw}) == 3
    assert len({round(v_core_of(k), 12) for k in sw}) == 3 and {k["method"] for k in sw} == {"Faure", "Ramesh"}
    assert {G10.BY_NAME[n]["steps"] for n in SWEEP} == {100, 200} and {G10.is_cambered(G10.BY_NAME[n]) for n in SWEEP} == {True, False}
    for a, b in SWEEP_PAIRS:        # neighbours in the list share none of dt, Uinf and v_core
        ka, kb = sw[a], sw[b]
        assert ka["dt"] != kb["dt"] and ka["Uinf"] != kb["Uinf"] and abs(v_core_of(ka) - v_core_of(kb)) > 0.03, (a, b)


@pytest.mark.parametrize("name", CASES + ("d23r", "c6409"))
def test_host_loop_matches_the_oracle(oracle, name):
    """2a.  The host loop carrying probes + tracers + survey at once, in both frames, against the oracle over steps 1 .. WINDOW:
    MARGIN = 10 x inside 1e-9 of max|u| (probes), 1e-9 of the largest displacement (tracers), MEAN_VS_ORACLE / MOMENT_VS_ORACLE
    (survey, window (2, nt, 1) in the lab frame and (3, nt, 4) in the tunnel's) -- the condition under which the GPU tier asserts
    those bounds; row 0 and the seeds exactly.  The measured values stand next to WINDOW in the common module.  (`d23r` and
    `c6409` run in the mixed sweep only.)"""
    run = oracle(name)
    obs = observers(name) if name in CASES else sweep_observers()
    n = WINDOW[name]
    assert 30 <= n <= STEPS
    for frame, steps in zip(FRAMES, ((2, STEPS + 1, 1), (3, STEPS + 1, 4))):
        sim = _host(case_keywords(name, STEPS), history="full", **run_keywords(obs, frame, steps))
        ref = reference(run, obs, frame, steps)
        assert sim.nt == run.nt == STEPS + 1 and sim.v_core == run.v_core and np.array_equal(sim.xpiv, -run.Uinf * sim.t)
        assert sim.tracer_path.steps() == list(range(sim.nt)) and sim.survey_count == len(ref["W"])
        e = errors(of_run(sim), ref, 1, n)
        print(f"G11 {name} host loop vs oracle ({frame}), steps 1-{n}: probes {e[0]:.2e} of max|u|, tracers {e[1]:.2e} of the largest "
              f"displacement, survey means {e[2]:.2e} of max|u|, raw second moments {e[3]:.2e} of max|u|^2")
        for what, v, bound in zip(NAMES, e, BOUNDS):
            assert v <= bound / MARGIN, (name, frame, what, v)
        assert np.array_equal(sim.tracer_path[0], ref["seeds"][0])
        assert np.abs(sim.probe_u[0] - ref["u"][0]).max() <= 1e-12 * max(1.0, np.abs(ref["u"][0]).max())


def _moved(label, run, obs, frame, what, **mutation):
    """Asserts that the mutation moves each quantity of `what` by SENSITIVITY bounds within the compared window."""
    steps = (2, STEPS + 1, 1)
    e = errors(reference(run, obs, frame, steps, **mutation), reference(run, obs, frame, steps), 1, WINDOW[run.name])
    print(f"G11 {label}: probes {e[0]:.2e}, tracers {e[1]:.2e}, survey means {e[2]:.2e}, raw second moments {e[3]:.2e}")
    for k in what:
        assert e[k] >= SENSITIVITY * BOUNDS[k], (label, NAMES[k], e[k])


@pytest.mark.parametrize("name", CASES)
def test_mutations_of_a_solo_run_are_seen(oracle, name):
    """2b.  What a subtly wrong observer would give, on the CPU, against the true oracle values: config 1's v_core = 0.065 in
    the sums (probes, tracers, survey), config 1's dt = 0.05 in the tracers' Euler step, the tunnel frame's shift -t for
    -Uinf t (all three), and the bound vortices on the chord line for a cambered case (all three) -- each at least 100 x the
    bound the GPU tier applies.  A mutation is skipped only where the case has config 1's own value (`c2412`: unit scales)."""
    run, obs = oracle(name), observers(name)
    everything = (0, 1, 2, 3)
    tried = 0
    if abs(run.v_core - UNIT["v_core"]) > 1e-12:
        _moved(f"{name}: v_core = 0.065 for {run.v_core:.4f}", run, obs, "lab", everything, v_core=UNIT["v_core"])
        tried += 1
    if run.dt != UNIT["dt"]:
        _moved(f"{name}: dt = 0.05 for {run.dt:.4f} in the Euler step", run, obs, "lab", (1,), dt=UNIT["dt"])
        tried += 1
    if run.Uinf != 1:
        _moved(f"{name}: xpiv = -t for -{run.Uinf} t", run, obs, "tunnel", everything, shift=-run.t)
        tried += 1
    if run.cambered:
        _moved(f"{name}: bound vortices on the chord line", run, obs, "lab", everything, sources=run.flat_sources)
        _moved(f"{name}: bound vortices on the chord line (tunnel)", run, obs, "tunnel", everything, sources=run.flat_sources)
        tried += 1
    assert tried >= (1 if name == "c2412" else 3), (name, tried)


def test_mutations_of_the_mixed_sweep_are_seen(oracle):
    """2b, the sweep.  Every member evaluated with the dt, with the v_core, and with the shift row of a neighbour in the list
    (the member before it, and -- the batch runs reversed too -- the one after it): each moves the member's probe rows,
    particle rows (dt: those alone) and survey sums at least 100 x the bounds test_mixed_sweep_observers asserts.  The neighbour's
    shift row is its own xpiv at the same step index: what a kernel reads that takes the member's step at the wrong offset of
    the concatenated table."""
    obs = sweep_observers()
    for m, other in SWEEP_PAIRS:
        run, nb = oracle(SWEEP[m]), oracle(SWEEP[other])
        label = f"sweep member {m} ({SWEEP[m]}) with member {other}'s ({SWEEP[other]})"
        _moved(f"{label} v_core", run, obs, "tunnel", (0, 1, 2, 3), v_core=nb.v_core)
        _moved(f"{label} dt", run, obs, "lab", (1,), dt=nb.dt)
        _moved(f"{label} shift row", run, obs, "tunnel", (0, 1, 2, 3), shift=nb.xpiv)
        assert run.xpiv[7] != nb.xpiv[7]


@pytest.mark.parametrize("name", BIN_CASES)
def test_the_bin_table_is_the_exact_rule(oracle, name):
    """2c.  survey_bins = 8, and 5 with survey_phase0, over the case's full 200 steps (`d23`: 200 steps per period; `k45`:
    133 1/3): the table against floor(B frac(tau) + 1e-9) in exact rational arithmetic from sim.t and the keywords k, Uinf,
    chord -- at every step whose phase is farther than 1e-6 from a bin edge, and at the steps that sit ON an edge (8 of `d23`'s
    200 with B = 8, 4 %: leaving them out would break the 2 % cap, and the rule's 1e-9 decides them); what remains undecided is
    counted and at most 2 % of the window (measured: none).  survey_phase is the bin centres.  The mutation f = k / 2 pi gives
    another table (more than a quarter of the steps change bin), and over the oracle's 50 steps the mean of the bin that holds
    step 30 differs under it from the true one by more than 100 x MEAN_VS_PROBES of max|u| (measured 0.38 and 0.23)."""
    kw = case_keywords(name)
    pts = observers(name)["survey"][:, :8]
    run = oracle(name)
    ou, ow = None, None
    for setting in bin_settings():
        for steps in ((2, 201, 1), (3, 201, 4)):
            sim = _host(kw, survey=pts, survey_steps=steps, run=False, **setting)
            B = setting["survey_bins"]
            assert sim.nt == 201 and sim.survey_nbins == B and np.array_equal(sim.survey_phase, (np.arange(B) + 0.5) / B)
            table, decided = exact_bin_table(sim.t, kw, B, setting.get("survey_phase0"))
            sampled = np.zeros(sim.nt, dtype=bool)
            sampled[steps[0]:steps[1]:steps[2]] = True
            assert np.array_equal(sim.survey_bin_of_step >= 0, sampled)
            left_out = int((sampled & ~decided).sum())
            v = ((sim.t - setting.get("survey_phase0", 0.0)) * sim.f * B) % 1.0
            on_edge = int((sampled & (np.minimum(v, 1.0 - v) < 1e-6 * B)).sum())
            print(f"G11 {name} B = {B} window {steps}: {int(sampled.sum())} steps, {on_edge} within 1e-6 of an edge, {left_out} undecided")
            assert left_out <= 0.02 * sampled.sum(), (name, setting, left_out)
            ok = sampled & decided
            assert np.array_equal(sim.survey_bin_of_step[ok], table[ok]), (name, setting)
            assert len(np.unique(table[ok])) == B
            wrong, _ = exact_bin_table(sim.t, kw, B, setting.get("survey_phase0"), frequency=unit_frequency(kw))
            assert (wrong[ok] != table[ok]).mean() > 0.25, (name, setting)
            if steps[2] == 1 and B == 8:        # the sums of bin 3 under the two tables, over the oracle's 50 steps
                if ou is None:
                    from observers_off_unit_common import probe_series
                    ou, ow = probe_series(run, pts, run.shift("lab"))
                first = slice(2, STEPS + 1)
                umax = max(np.abs(ou[first]).max(), np.abs(ow[first]).max())
                means = []
                for tb in (table, wrong):
                    W = [i for i in range(2, STEPS + 1) if tb[i] == tb[30]]
                    means.append(series_sums(ou, ow, W)[:2] / len(W))
                moved = np.abs(means[0] - means[1]).max() / umax
                print(f"G11 {name}: the bin of step 30 under f = k / 2 pi: its mean moves {moved:.2e} of max|u|")
                assert moved >= SENSITIVITY * MEAN_VS_PROBES, moved


@pytest.mark.parametrize("name", FP32_CASES)
def test_the_guard_model_decides_by_the_cases_own_core(name):
    """2 (for 3c).  The 4-step guard run of the case on the fake engine, its step-3 sources in the device's stored order, in the
    NumPy model of the fp32 survey: with the case's v_core the guard takes every class on `dhalf` (extent 14.08 > 300 x 0.0325)
    and none on `d23` (28.16 < 300 x 0.13); with config 1's 0.065 the model makes the opposite choice for every class."""
    kw, pts = guard_case(name)
    sim = _host(kw, history="full")
    g, x, z = stored_sources(sim, GUARD_STEP)
    nf = kw["xy_freevort"].shape[1]
    assert nf == 258 and np.array_equal(x[:nf], sim.path["FREE"][GUARD_STEP - 1][0]) and len(g) == nf + GUARD_STEP + int((sim.LEV_shed[1:4] != -1).sum()) + 80
    vc = v_core_of(kw)
    assert sim.v_core == vc and MAX_EXTENT * min(vc, 0.065) < GUARD_EXTENT[name] < MAX_EXTENT * max(vc, 0.065)
    few = pts[:, ::16]
    _, _, own, classes = local_f32_field(g, x, z, few[0], few[1], vc, max_extent=MAX_EXTENT)
    _, _, unit, _ = local_f32_field(g, x, z, few[0], few[1], 0.065, max_extent=MAX_EXTENT)
    print(f"G11 {name} guard model: {classes} classes, guarded with v_core = {vc:.4f}: {own}, with 0.065: {unit}")
    assert classes == 4
    assert (own, unit) == ((classes, 0) if name == "dhalf" else (0, classes))
