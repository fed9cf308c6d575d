"""Shared by tests/test_rollup_steps_host.py and tests/test_gpu_rollup_steps.py: ONE wake roll-up step of a run, checked by
value against the run's own state.  A run with the dense history says the sources of step i's roll-up itself
(tracers_common.run_sources: the wake of row i - 1, the vortices shed in step i at their placement, the bound vortices of
step i); the float64 pair sums of those sources at the wake's own positions (LUDVM.py:1105-1106) and one explicit Euler
update (:1108-1127) are the row i the run must hold.  No step depends on an earlier one, so the flow's divergence -- which
opens the windows of every test that follows a run against the golden one -- does not enter: the residual of step 400 is
as sharp as that of step 2.

Host only (NumPy and the oracle's pair sum); nothing here knows how a kernel is launched.  The case table's comments name the
kernel constants the cases are chosen for:

    256   vortices per origin block (two origin classes per block, by index parity)
    512   vortices per tile of the symmetric kernel at 8 vortices per lane (two origin blocks)
    80    bound vortices of config 1, staged behind the wake: entry n0 + n_new + 80 - 1 is the last staged one
"""
from collections import namedtuple

import numpy as np

from conftest import CONFIG1
from oracle import g9_cases
from tracers_common import run_sources

FAMILIES = ("TEV", "LEV", "FREE")
BLOCK = 256

# What step_residuals returns.  `res`: family -> max |row i - expected| / dt (a velocity), 'PHANTOM' among them on a step that
# sheds no LEV; `scale`: max(|u|, |w|) over the step's targets; `align`: (n0, n_new); `xmax`: max |coordinate| of the
# expected row (what the float64 Euler update rounds at).
Step = namedtuple("Step", "res scale align xmax")


def step_residuals(sim, i, iv):
    """Residual of step i >= 2 of `sim` (anything with path, circulation, LEV_shed, v_core, dt of a dense history).
    `iv(g, xs, zs, xp, zp, v_core) -> (u, w)`: observer_sources_common.fast_iv()."""
    assert i >= 2
    P, dt, vc = sim.path, sim.dt, sim.v_core
    gw, xs, zs, gf, xf, zf = run_sources(sim, i)
    uw, ww = iv(gw, xs, zs, xs, zs, vc)
    uf, wf = iv(gf, xf, zf, xs, zs, vc)
    u, w = uw + uf, ww + wf
    ex, ez = xs + dt * u, zs + dt * w
    shed = np.asarray(sim.LEV_shed) != -1
    itev, ilev, nfree = i - 1, int(shed[:i].sum()), P["FREE"].shape[2]
    n_new = 2 if shed[i] else 1
    old = itev + ilev + nfree                       # run_sources' order: TEV[:itev] | LEV[:ilev] | FREE | shed in step i
    tev = np.r_[np.arange(itev), old]
    lev = np.r_[itev:itev + ilev, old + 1] if shed[i] else np.arange(itev, itev + ilev)
    free = np.arange(itev + ilev, old)
    res = {}
    for fam, cols in (("TEV", tev), ("LEV", lev), ("FREE", free)):
        row = np.asarray(P[fam][i])[:, :len(cols)]
        res[fam] = max(np.abs(row[0] - ex[cols]).max(), np.abs(row[1] - ez[cols]).max()) / dt if len(cols) else 0.0
    if not shed[i]:
        # the zero-strength LEV slot of a non-shedding step: column ilev of row i starts at the origin (the array's
        # zeros, LUDVM.py:1112-1118) and is convected like any target; a source of strength 0 at (0, 0) adds exactly 0
        o = np.zeros(1)
        pu, pw = iv(gw, xs, zs, o, o, vc)
        qu, qw = iv(gf, xf, zf, o, o, vc)
        got = np.asarray(P["LEV"][i])[:, ilev]
        res["PHANTOM"] = max(abs(got[0] - dt * (pu[0] + qu[0])), abs(got[1] - dt * (pw[0] + qw[0]))) / dt
    scale = max(np.abs(u).max(), np.abs(w).max())
    n0 = max(nfree, 1) + (i - 1) + ilev
    return Step(res, scale, (n0, n_new), max(np.abs(ex).max(), np.abs(ez).max()))


def worst(step, families=None):
    """(residual / scale, family) of the worst family of a step (of `families`, default all it has)."""
    fams = [f for f in step.res if families is None or f in families]
    f = max(fams, key=lambda k: step.res[k])
    return step.res[f] / step.scale, f


def euler_slack(step, dt):
    """What the float64 Euler update itself may round: 4 ulp(max |x|) / dt, a velocity."""
    return 4 * np.spacing(step.xmax) / dt


def alignments(sim, first=2):
    """{(n0 % 256, n_new)} over the steps first .. nt - 1 of a run, from its own shedding."""
    shed = np.asarray(sim.LEV_shed) != -1
    nfree = sim.path["FREE"].shape[2]
    before = np.concatenate([[0], np.cumsum(shed)])            # LEVs shed before step i
    return {(int(max(nfree, 1) + (i - 1) + before[i]) % BLOCK, 2 if shed[i] else 1) for i in range(first, len(shed))}


def foil_tail_opens_a_block(sim, npan, first=2):
    """{n_new} of the steps whose last staged bound vortex is the first entry of an origin block:
    (n0 + n_new + npan - 1) % 256 == 0."""
    shed = np.asarray(sim.LEV_shed) != -1
    nfree = sim.path["FREE"].shape[2]
    before = np.concatenate([[0], np.cumsum(shed)])
    out = set()
    for i in range(first, len(shed)):
        n0, n_new = max(nfree, 1) + (i - 1) + int(before[i]), 2 if shed[i] else 1
        if (n0 + n_new + npan - 1) % BLOCK == 0:
            out.add(n_new)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------
# name -> (nfree, tf, alignments (n0 % 256, n_new) the run must go through, n_new of a step whose foil tail opens a block)
#   config1   wake 3 -> 604: a shed pair straddles 256 (n0 = 255), 512 is reached exactly and a pair opens the block
#             (n0 = 512: also the 512 tile edge); the last bound vortex opens a block with one and with two new vortices
#   c150      n0 = 256 with a pair: the pair opens block 1
#   c151      n0 = 255 with a pair: straddles the edge; the foil tail opens a block early in the run
#   c396      n0 = 511 with a pair: straddles the 512 tile edge
#   c397      n0 = 512 with a pair: opens block 2 / the second tile
CASES = {
    "config1": (0, 20, {(255, 2), (0, 2)}, {1, 2}),
    "c150": (150, 5, {(0, 2)}, set()),
    "c151": (151, 5, {(255, 2)}, {1}),
    "c396": (396, 5, {(255, 2)}, set()),
    "c397": (397, 5, {(0, 2)}, set()),
}
CLOUDS = ("c150", "c151", "c396", "c397")
NPAN = CONFIG1["Npoints"] - 1


def case_keywords(name):
    nfree, tf = CASES[name][:2]
    kw = dict(CONFIG1, tf=tf)
    if nfree:
        g, xy = g9_cases.free_cloud(9900 + nfree, nfree)
        kw.update(circulation_freevort=g, xy_freevort=xy)
    return kw


def check_alignments(name, sim):
    """The run went through the alignments the case is listed for."""
    _, _, want, tails = CASES[name]
    got = alignments(sim)
    assert want <= got, (name, sorted(want - got))
    got_t = foil_tail_opens_a_block(sim, NPAN)
    assert tails <= got_t, (name, tails, got_t)
