"""CPU tier of the step-local roll-up check (tests/rollup_common.py): the float64 oracle passes it at every step of the
README case, the check sees a wrong row at the step that made it, and the cases of tests/test_gpu_rollup_steps.py go through
the wake sizes they are listed for."""
import copy
import types

import numpy as np
import pytest

from conftest import CONFIG1
from observer_sources_common import fast_iv
from oracle import ludvm_oracle as O
from rollup_common import CASES, CLOUDS, NPAN, case_keywords, check_alignments, step_residuals, worst

ORACLE_BOUND = 1e-12        # of the scale: float64 against float64 (placement (a - b) / 3 against 1 / 3 * (a - b): one ulp)
FAULT_BOUND = 1e-5          # of the scale: what the fp32 tier allows, so what a fault must exceed to be seen


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


@pytest.fixture(scope="module")
def config1():
    sim = O.OracleLUDVM(**CONFIG1)
    for a in (*sim.path.values(), sim.LEV_shed):
        a.setflags(write=False)
    return sim


@pytest.fixture(scope="module")
def clean(config1, iv):
    """step -> residual / scale of the oracle's own run (the worst family)."""
    return {i: worst(step_residuals(config1, i, iv))[0] for i in range(2, config1.nt)}


def history_copy(sim):
    """The attributes step_residuals reads, the path rows writable copies."""
    return types.SimpleNamespace(path={k: np.array(v) for k, v in sim.path.items()}, circulation=copy.deepcopy(sim.circulation),
                                 LEV_shed=np.array(sim.LEV_shed), v_core=sim.v_core, dt=sim.dt, nt=sim.nt)


def test_the_oracle_passes_the_check_at_every_step(config1, iv):
    """Family mapping, placement of the shed vortices, shed bookkeeping and the zero-strength LEV slot: float64 against
    float64, every family of every step 2 .. 400."""
    assert config1.nt == 401
    seen = set()
    for i in range(2, config1.nt):
        s = step_residuals(config1, i, iv)
        seen.update(s.res)
        for fam, r in s.res.items():
            assert r <= ORACLE_BOUND * s.scale, (i, fam, r / s.scale)
        assert ("PHANTOM" in s.res) == (config1.LEV_shed[i] == -1)
    assert seen == {"TEV", "LEV", "FREE", "PHANTOM"}


def flagged(sim, iv, clean, around):
    """Steps over FAULT_BOUND.  Every step is computed near `around`; elsewhere a step whose rows the corruption did not
    touch is the clean run's (step i reads rows i - 1 and i only)."""
    out = set()
    for i in range(2, sim.nt):
        r = worst(step_residuals(sim, i, iv))[0] if abs(i - around) <= 3 else clean[i]
        if r > FAULT_BOUND:
            out.add(i)
    return out


def test_the_check_sees_a_fault_at_its_step(config1, iv, clean):
    """Three corruptions of a copy of the oracle's history, each at the run's last row -- the result of step 400 and the start
    of none -- raise that step's residual above 1e-5 of the scale and no other's.  The same corruptions of an inner row k are
    seen at step k and, because row k is also where step k + 1 starts, at k + 1: nowhere else."""
    shed = config1.LEV_shed != -1
    last = config1.nt - 1
    pair = max(i for i in range(2, last) if shed[i])                 # the last inner step that sheds a pair
    inner = 200
    assert max(clean.values()) <= ORACLE_BOUND

    def displaced(h, k):
        s = step_residuals(config1, k, iv)
        h.path["TEV"][k, 0, 17] += h.dt * 1e-4 * s.scale

    def newest_tev_without_the_foil(h, k):
        from tracers_common import run_sources
        gw, xs, zs, *_ = run_sources(config1, k)
        n_new = 2 if shed[k] else 1
        u, w = iv(gw, xs, zs, xs[-n_new:-n_new + 1 or None], zs[-n_new:-n_new + 1 or None], h.v_core)
        h.path["TEV"][k, :, k - 1] = [xs[-n_new] + h.dt * u[0], zs[-n_new] + h.dt * w[0]]

    def pair_swapped(h, k):
        ilev = int(shed[:k].sum())
        t, l = h.path["TEV"][k, :, k - 1].copy(), h.path["LEV"][k, :, ilev].copy()
        h.path["TEV"][k, :, k - 1], h.path["LEV"][k, :, ilev] = l, t

    for corrupt, k in ((displaced, last), (newest_tev_without_the_foil, last), (pair_swapped, last if shed[last] else None)):
        if k is None:
            continue
        h = history_copy(config1)
        corrupt(h, k)
        assert flagged(h, iv, clean, k) == {k}, corrupt.__name__
    for corrupt, k in ((displaced, inner), (newest_tev_without_the_foil, inner), (pair_swapped, pair)):
        h = history_copy(config1)
        corrupt(h, k)
        assert flagged(h, iv, clean, k) == {k, k + 1}, corrupt.__name__
        # ... and with the rows up to k alone (the run as it stood after step k) exactly step k
        h.nt = k + 1
        assert flagged(h, iv, clean, k) == {k}, corrupt.__name__


def test_config1_goes_through_its_alignments(config1):
    """The steps the README case is listed for, with the oracle's shedding."""
    shed = config1.LEV_shed != -1
    n0 = {i: 1 + (i - 1) + int(shed[:i].sum()) for i in range(2, config1.nt)}
    new = {i: 2 if shed[i] else 1 for i in n0}
    assert (n0[2] + new[2], n0[400] + new[400]) == (3, 603)    # the wake the roll-ups of steps 2 .. 400 move
    assert not shed[400]                                    # (604 entries with the zero-strength LEV slot of the last step)
    assert (n0[167], new[167]) == (255, 2)                  # a shed pair straddles the first origin-block edge
    assert (n0[346], new[346]) == (512, 2)                  # 512 reached exactly: the pair opens block 2 and the second tile
    for i, k in ((122, 1), (280, 2)):                       # the last bound vortex is the first entry of a block
        assert new[i] == k and (n0[i] + new[i] + NPAN - 1) % 256 == 0, i
    check_alignments("config1", config1)


assert set(CLOUDS) == {"c150", "c151", "c396", "c397"}


@pytest.mark.parametrize("name,step,n0", [("c150", 66, 256), ("c151", 71, 255), ("c396", 69, 511), ("c397", 72, 512)])
def test_cloud_cases_go_through_their_alignments(name, step, n0, iv):
    """A free-vortex cloud sets the wake size of step 1, so 100 steps reach an edge with a shed pair on it; the oracle passes
    the check there as well."""
    sim = O.OracleLUDVM(**case_keywords(name))
    assert sim.nt == 101 and sim.path["FREE"].shape[2] == CASES[name][0]
    check_alignments(name, sim)
    s = step_residuals(sim, step, iv)
    assert s.align == (n0, 2)
    if name == "c151":
        t = step_residuals(sim, 26, iv)
        assert t.align[1] == 1 and (sum(t.align) + NPAN - 1) % 256 == 0
    for i in range(2, sim.nt):
        s = step_residuals(sim, i, iv)
        for fam, r in s.res.items():
            assert r <= ORACLE_BOUND * s.scale, (name, i, fam, r / s.scale)
