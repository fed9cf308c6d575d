"""What the two tiers of G9 share (tests/test_g9_fixture.py, tests/test_gpu_g9.py): the fixture by run, the oracle's run of a
case (once per session), and the comparison of a run with the reference's."""
import warnings

import numpy as np

from conftest import grouped, load_golden
from oracle import g9_cases as G9
from oracle import ludvm_oracle as O

RUNS = [(c, m) for c in G9.CASES for m in c["methods"] if G9.in_fixture(c, m)]

_FIXTURE = {}
_ORACLE = {}


def fixture():
    """{run key: named arrays} of tests/golden/g9_edge_runs.npz (read once, never written to)."""
    if not _FIXTURE:
        _FIXTURE.update({k: G9.unpack(v) for k, v in grouped(load_golden("g9_edge_runs.npz")).items()})
    return _FIXTURE


def oracle_run(c, method):
    """OracleLUDVM on (case, method) as named arrays, run once per session."""
    k = G9.key(c, method)
    if k not in _ORACLE:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _ORACLE[k] = G9.unpack(G9.pack(O.OracleLUDVM(**G9.kwargs(c, method)), c))
    return _ORACLE[k]


def reference_run(c, method):
    """The reference's run of (case, method): from the fixture, or -- 'Ramesh' at the panel counts the fixture leaves out --
    the oracle's, which equals the reference bit for bit on every stored run (tests/test_g9_fixture.py)."""
    return fixture()[G9.key(c, method)] if G9.in_fixture(c, method) else oracle_run(c, method)


def compare_dense(got, ref, tol, what):
    """A dense-history run packed like the fixture against the reference's: identical LEV_shed and counts, every series and
    wake row within tol of the row's maximum (1 where it is zero).  -> the worst ratio."""
    assert np.array_equal(got["LEV_shed"], ref["LEV_shed"]), what
    assert (got["nt"], got["itev"], got["ilev"]) == (ref["nt"], ref["itev"], ref["ilev"]), what
    worst = 0.0
    for k in G9.SERIES[:-1] + ("TEV", "LEV", "FREE"):
        assert got[k].shape == ref[k].shape, (what, k)
        scale = np.abs(ref[k]).max() or 1.0
        d = np.abs(got[k] - ref[k]).max() / scale
        assert d <= tol, (what, k, d)
        worst = max(worst, d)
    return worst


def product_errors(sim, ref, c):
    """A product run with sparse history (a sweep member, a marched or a per-step solo run; the case's snapshot step stored)
    against the reference's run: asserts identical LEV_shed, nt, itev, ilev, the shapes of the stored wake rows and that
    everything is finite; -> {what: max |difference|} for the loads over steps 0-99, the circulations, the wake rows at the
    snapshot step and Kelvin's sum."""
    what = c["name"]
    if not np.array_equal(sim.LEV_shed, ref["LEV_shed"]):
        s = int(np.argmax(sim.LEV_shed != ref["LEV_shed"]))
        raise AssertionError(f"{what}: LEV_shed differs first at step {s}: |A0| {abs(sim.LESP_prev[s - 1])!r}, LESPcrit {sim.LESPcrit}")
    assert (sim.nt, sim.itev, sim.ilev) == (ref["nt"], ref["itev"], ref["ilev"]), what
    err = {}
    for name in ("Cl", "Cd", "Cm"):
        a = getattr(sim, name)
        assert a.shape == ref[name].shape and np.isfinite(a).all(), (what, name)
        err[name] = float(np.abs(a - ref[name])[:100].max())
    assert np.isfinite(sim.LESP).all() and np.isfinite(sim.fourier).all(), what
    err["LESP"] = float(np.abs(sim.LESP - ref["LESP"])[:100].max())
    C = sim.circulation
    for k in ("TEV", "LEV", "bound"):
        assert C[k].shape == ref["circ_" + k].shape and np.isfinite(C[k]).all(), (what, k)
        err["circ_" + k] = float(np.abs(C[k] - ref["circ_" + k]).max())
    s = c["snap"]
    nlev = int((ref["LEV_shed"][:s + 1] != -1).sum())
    shed_now = ref["LEV_shed"][s] != -1
    cols = {"TEV": s, "LEV": nlev if shed_now else nlev + 1, "FREE": max(c["nfree"], 1)}
    for k in ("TEV", "LEV", "FREE"):
        row = np.asarray(sim.path[k][s])
        assert row.shape == (2, cols[k]) and np.isfinite(row).all(), (what, k, row.shape, cols[k])
        err["row_" + k] = float(np.abs(row - ref[k][:, :cols[k]]).max())
    assert abs(float(C["IC"]) - ref["circ_IC"]) <= 1e-12 * max(1.0, abs(ref["circ_IC"])), what
    err["kelvin"] = float(abs(C["bound"][sim.itev] + C["TEV"].sum() + C["LEV"].sum() + np.sum(C["FREE"]) - C["IC"]))
    return err


def show(label, err):
    print(f"G9 {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
