"""CPU tier of the step-local solve check (tests/solve_steps_common.py): the float64 oracle and the product's host loop (on
tests/fake_engine.py) pass it at every step, with the sources evaluated in given and in reversed order; the largest residual
per quantity over those runs is the host floor the GPU bounds are derived from; the case table goes through every branch of
the solve; and the check sees each of a list of planted faults at the step that made it.

`python tests/test_solve_steps_host.py` prints the floor table of profiles/solve_steps_residuals.txt.
"""
import numpy as np
import pytest

from observer_sources_common import fast_iv
from oracle import ludvm_oracle as O
import solve_steps_common as S

# (case, method) of the oracle's runs and of the product's host loop
ORACLE_RUNS = [("config1", "Faure"), ("config1", "Ramesh"), ("d23", "Faure"), ("d23", "Ramesh"), ("c4412d", "Ramesh"),
               ("c2412f", "Faure"), ("c150", "Faure")]
HOST_RUNS = [("config1", "Faure"), ("config1", "Ramesh"), ("c4412d", "Ramesh"), ("c2412f", "Faure")]


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


class Runs:
    """Runs and their checked steps, each made once."""

    def __init__(self, iv):
        self.iv, self.kw = iv, S.small_cases()
        self._sims, self._steps = {}, {}

    def sim(self, kind, case, method):
        key = (kind, case, method)
        if key not in self._sims:
            if kind == "oracle":
                sim = O.OracleLUDVM(**self.kw[case], method=method)
            else:
                from fake_engine import FakeEngine
                from ludvm_amd import LUDVM
                sim = LUDVM(**self.kw[case], method=method, verbose=False, engine=FakeEngine())
            for a in (*sim.path.values(), sim.LEV_shed, sim.fourier):
                a.setflags(write=False)
            self._sims[key] = sim
        return self._sims[key]

    def steps(self, kind, case, method, order="given"):
        key = (kind, case, method, order)
        if key not in self._steps:
            sim = self.sim(kind, case, method)
            f = self.iv if order == "given" else S.reversed_iv(self.iv)
            self._steps[key] = {i: S.step_solve_residuals(sim, i, f) for i in range(1, sim.nt)}
        return self._steps[key]

    def all_steps(self):
        for kind, runs in (("oracle", ORACLE_RUNS), ("host", HOST_RUNS)):
            for case, method in runs:
                for order in ("given", "reversed"):
                    yield (kind, case, method, order), self.steps(kind, case, method, order)


@pytest.fixture(scope="module")
def runs(iv):
    return Runs(iv)


def measured_floors(runs):
    """quantity -> (largest residual / scale beyond the Newton allowance, where) over every run of the tier."""
    floor = {q: (0.0, None) for q in S.QUANTITIES}
    for key, steps in runs.all_steps():
        for i, s in steps.items():
            for q, r in s.res.items():
                v = max(r - s.allow.get(q, 0.0), 0.0) / s.scale[q]
                if v > floor[q][0]:
                    floor[q] = (v, key + (i,))
    return floor


def test_every_run_passes_at_every_step_and_the_floors_are_the_recorded_ones(runs):
    """The oracle's runs (both methods; config 1 over all 400 steps; off-unit, cambered and free-vortex cases) and the product's
    host loop: every residual of every step within its bound, the shedding decision identical, Ramesh's two conditions at the
    run's circulations within `maxerror`.  The largest residual over its scale is at most the floor recorded in the common
    module, and every bound is 64 x its floor inside [1e-12, 1e-9]."""
    for key, steps in runs.all_steps():
        assert len(steps) == runs.sim(*key[:3]).nt - 1
        for i, s in steps.items():
            assert s.shed == s.shed_run, (key, i, s.margin)
            assert not S.over_bound(s), (key, i, S.over_bound(s))
            if s.newton:
                assert s.newton["kelvin"] <= 1e-10 and s.newton["lesp_cond"] <= 1e-10, (key, i, s.newton)
    assert runs.sim("oracle", "config1", "Faure").nt == 401
    floor = measured_floors(runs)
    # (a floor is a handful of ulps of one sum: another libm or thread count may move it by an ulp or two, hence the factor 2;
    # 64 x the largest floor is 9e-14, so every bound sits at the 1e-12 contract with a decade to spare)
    for q in S.QUANTITIES:
        assert floor[q][0] <= 2 * S.HOST_FLOOR[q], (q, floor[q])
        assert floor[q][0] >= S.HOST_FLOOR[q] / 4, (q, floor[q], "the recorded floor is stale")
        assert S.BOUND[q] == min(max(64 * S.HOST_FLOOR[q], 1e-12), 1e-9)
        assert 64 * 2 * S.HOST_FLOOR[q] < 1e-12 and S.BOUND[q] == 1e-12


def test_the_cases_go_through_every_branch_of_the_solve(runs):
    """Asserted on the oracle's runs: step 1, a first LEV, a consecutive one, one after a gap, shedding with A0 > 0 and with
    A0 < 0, a non-shedding step after shedding ones, both methods, a cambered section, chord, Uinf, rho != 1, free vortices --
    and config 1 alone goes through all the events.  No decision of any case is closer than 1e-6 to LESPcrit, so it is
    checked at every step with no exemption."""
    seen = set()
    for case, method in ORACLE_RUNS:
        steps = runs.steps("oracle", case, method)
        ev = set().union(*(s.events for s in steps.values()))
        seen |= ev
        if case == "config1":
            assert ev == S.EVENTS, (method, S.EVENTS - ev)
        margin = min(s.margin for s in steps.values())
        assert margin >= S.MIN_MARGIN, (case, method, margin)
    assert seen == S.EVENTS
    assert {m for _, m in ORACLE_RUNS} == {"Faure", "Ramesh"}
    kw = runs.kw
    assert any(kw[c]["Naca"][:2] != "00" and kw[c]["chord"] != 1 and kw[c]["Uinf"] != 1 and kw[c]["rho"] != 1 for c, _ in ORACLE_RUNS)
    assert any("circulation_freevort" in kw[c] for c, _ in ORACLE_RUNS)
    shed = runs.sim("oracle", "config1", "Faure").LEV_shed != -1
    assert 150 < shed.sum() < 250                       # about half of config 1's steps shed


def test_config_1_margin_and_counts(runs):
    """The figures the tier was planned with, from the oracle's config 1 ('Faure')."""
    steps = runs.steps("oracle", "config1", "Faure")
    count = lambda e: sum(e in s.events for s in steps.values())       # noqa: E731
    assert count("shed A0 < 0") + count("shed A0 > 0") == count("first LEV") + count("consecutive LEV") + count("LEV after a gap")
    assert count("first LEV") == 1 and count("LEV after a gap") >= 2 and count("consecutive LEV") > 150
    assert min(count("shed A0 < 0"), count("shed A0 > 0")) > 80
    assert 1e-4 < min(s.margin for s in steps.values()) < 3e-4


# ---- sensitivity ------------------------------------------------------------------------------------------------------
def pick(steps, event, after=20):
    """A step of the run with `event`, not among its first ones."""
    return next(i for i, s in sorted(steps.items()) if i > after and event in s.events)


def scaled(name, factor):
    def f(h, k, runs):
        itev, ilev, _ = S.counts(h, k)
        h.circulation[name][itev if name == "TEV" else ilev] *= factor
    return f


def coefficient_off(h, k, runs):
    h.fourier[k, 0, 5] += 1e-9


def derivatives_from_the_post_lev_coefficients(h, k, runs):
    h.fourier[k, 1, :] = (h.fourier[k, 0, :] - h.fourier[k - 1, 0, :]) / h.dt


def bound_of_the_other_method(h, k, runs):
    h.circulation["bound"][k - 1] = S.model_step(h, k, runs.iv, fault="bound_other")["bound"]


def row_of(fault):
    def f(h, k, runs):
        S.plant_row(h, k, S.model_step(h, k, runs.iv, fault=fault))
    f.__name__ = str(fault)
    return f


# (name, case, method, the event the planted step must have, the fault, does it change what LATER steps start from)
PLANTS = [
    ("gamma_tev", "config1", "Faure", "no LEV after shedding", scaled("TEV", 1 + 1e-8), True),
    ("gamma_tev_ramesh", "config1", "Ramesh", "consecutive LEV", scaled("TEV", 1 + 1e-8), True),
    ("gamma_lev", "config1", "Faure", "consecutive LEV", scaled("LEV", 1 + 1e-8), True),
    ("fourier_1e-9", "config1", "Faure", "consecutive LEV", coefficient_off, False),
    ("derivatives_post_lev", "config1", "Faure", "consecutive LEV", derivatives_from_the_post_lev_coefficients, False),
    ("derivatives_post_lev_ramesh", "config1", "Ramesh", "consecutive LEV", derivatives_from_the_post_lev_coefficients, False),
    ("bound_other_faure", "d23", "Faure", "LEV after a gap", bound_of_the_other_method, False),
    ("bound_other_ramesh", "d23", "Ramesh", "no LEV after shedding", bound_of_the_other_method, False),
    # (a case with free vortices: the last source of config 1's wake is its one zero-strength free vortex)
    ("last_source_dropped", "c150", "Faure", "consecutive LEV", row_of("drop_last"), True),
    ("row_i_for_row_i-1", "config1", "Faure", "consecutive LEV", row_of("row_i"), True),
    ("lev_at_the_leading_edge", "config1", "Faure", "consecutive LEV", row_of("lev_le"), True),
    ("lev_by_the_third_rule", "config1", "Faure", "LEV after a gap", row_of("lev_third"), True),
    ("lev_by_the_third_rule_ramesh", "config1", "Ramesh", "LEV after a gap", row_of("lev_third"), True),
    ("lespcrit_not_flipped", "config1", "Faure", "shed A0 < 0", row_of("no_flip"), True),
    ("lespcrit_not_flipped_ramesh", "config1", "Ramesh", "shed A0 < 0", row_of("no_flip"), True),
    ("loads_without_the_new_vortices", "config1", "Faure", "consecutive LEV", row_of("loads_old_wake"), False),
    ("loads_without_the_new_vortices_ramesh", "c4412d", "Ramesh", "no LEV after shedding", row_of("loads_old_wake"), False),
]


@pytest.mark.parametrize("name,case,method,event,fault,feeds_later", PLANTS, ids=[p[0] for p in PLANTS])
def test_the_check_sees_a_planted_fault_at_its_step(name, case, method, event, fault, feeds_later, runs):
    """Each fault, planted into a copy of an oracle run's arrays at one step k, pushes a residual of step k over its bound and
    none of an untouched step.  Untouched: every step before k, and -- for a fault that changes only what step k stores, not
    a circulation or a shedding that later wakes are made of -- every step after k + 1 (step k + 1 takes its derivatives from
    row k).  A fault of the first kind is followed to step k + 3 (later wakes hold what it wrote); one of the second kind over
    the whole run."""
    sim = runs.sim("oracle", case, method)
    clean = runs.steps("oracle", case, method)
    k = pick(clean, event)
    assert 3 < k < sim.nt - 4
    h = S.history_copy(sim)
    fault(h, k, runs)
    flagged = {i for i in range(1, k + 4 if feeds_later else sim.nt) if S.over_bound(S.step_solve_residuals(h, i, runs.iv))}
    assert k in flagged, name
    assert not {i for i in flagged if i < k}, (name, flagged)
    if not feeds_later:
        assert flagged <= {k, k + 1}, (name, flagged)


def test_the_row_the_model_chains_is_the_oracles_row(runs):
    """Control of the planted rows: the row model_step solves from the old wake alone, with no fault, written over the oracle's
    own leaves every step within its bounds -- so what the faults above change is the fault."""
    for case, method, event in (("config1", "Faure", "consecutive LEV"), ("config1", "Ramesh", "LEV after a gap"),
                                ("c4412d", "Ramesh", "no LEV after shedding")):
        sim = runs.sim("oracle", case, method)
        k = pick(runs.steps("oracle", case, method), event)
        h = S.history_copy(sim)
        S.plant_row(h, k, S.model_step(h, k, runs.iv))
        for i in range(k - 1, k + 3):
            s = S.step_solve_residuals(h, i, runs.iv)
            assert not S.over_bound(s), (case, method, i, S.over_bound(s))


def floor_table(runs):
    lines = ["quantity         host floor   bound (x scale)   where the floor was met (tier, case, method, source order, step)"]
    for q, (v, where) in measured_floors(runs).items():
        lines.append(f"{q:<16} {v:.2e}     {S.bound_from_floor(v):.0e}             {where}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(floor_table(Runs(fast_iv())))
