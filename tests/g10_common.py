"""What the two tiers of G10 share (tests/test_g10_fixture.py, tests/test_gpu_g10.py): the fixture by case, the oracle's run of
a case (once per session), the windows, and the comparison of a run with the reference's.

Windows (tier T3): every load, LESP and circulation series within 1e-9 of the series' own maximum over the first 100 steps and
within 1e-7 over the first 200; the wake rows after step G10.SNAP = 100 within 1e-9 of the largest wake coordinate.  WINDOW[name] is the number of steps a case is compared over: the CPU
tier licenses it (the host loop, which differs from the reference by summation order only, stays 10 x inside)."""
import warnings

import numpy as np

from conftest import grouped, load_golden
from oracle import g10_cases as G10
from oracle import ludvm_oracle as O
from oracle.g9_cases import SERIES

T3_100, T3_200 = 1e-9, 1e-7
MARGIN = 10.0
WINDOW = {c["name"]: c["steps"] for c in G10.CASES}        # 200 steps (both windows) or 100 (`dhalf`, `c2412f`: the first only)
SHED_MARGIN = 1e-4              # | |A0| - |LESPcrit| | above this: an fp32 rounding of A0 cannot turn the shedding decision
SHED_MIN_STEPS = 50

_FIXTURE = {}
_ORACLE = {}


def raw():
    """{group: {key: array}} of tests/golden/g10_off_unit_runs.npz (read once, never written to)."""
    if not _FIXTURE:
        _FIXTURE.update(grouped(load_golden("g10_off_unit_runs.npz")))
        for g in _FIXTURE.values():
            for a in g.values():
                a.setflags(write=False)
    return _FIXTURE


def fixture():
    """{case name: named arrays}."""
    return {c["name"]: G10.unpack(raw()[c["name"]]) for c in G10.CASES}


def downwash_calls():
    d = raw()["downwash"]
    return [{k: d[f"{n}_{k}"] for k in ("step", "g", "xw", "zw", "W")} for n in range(int(d["ncalls"]))]


def oracle_sim(c, **over):
    """OracleLUDVM on the case (with constructor keywords replaced by `over`), run once per session."""
    k = (c["name"], tuple(sorted(over.items())))
    if k not in _ORACLE:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _ORACLE[k] = O.OracleLUDVM(**G10.kwargs(c, **over))
    return _ORACLE[k]


def safe_shedding_steps(ref):
    """The number N of leading steps over which the reference's | |A0| - |LESPcrit| | at the shedding decision stays above
    SHED_MARGIN: LEV_shed[: N + 1] of an fp32 run must equal the reference's."""
    a0 = np.abs(ref["LESP_prev"][:ref["nt"] - 1])          # LESP_prev[itev] belongs to step itev + 1
    close = np.abs(a0 - abs(float(ref["params"][G10.PARAM_KEYS.index("LESPcrit")]))) <= SHED_MARGIN
    return int(np.argmax(close)) if close.any() else ref["nt"] - 1


def _rel(got, ref, n):
    scale = np.abs(ref).max() or 1.0
    return float(np.abs(got[:n] - ref[:n]).max() / scale)


def window_errors(got, ref, name):
    """A run as named arrays (G10.unpack's keys; a product run through `product_arrays`) against the reference's: identical
    LEV_shed and counts; -> {series: (error over the first 100 steps, over the first 200 or None)} relative to the series'
    maximum, and 'rows': the wake rows after step G10.SNAP relative to the largest wake coordinate."""
    if not np.array_equal(got["LEV_shed"], ref["LEV_shed"]):
        s = int(np.argmax(got["LEV_shed"] != ref["LEV_shed"]))
        raise AssertionError(f"{name}: LEV_shed differs first at step {s}: |A0| {abs(got['LESP_prev'][s - 1])!r} "
                             f"(reference {abs(ref['LESP_prev'][s - 1])!r})")
    assert (got["nt"], got["itev"], got["ilev"]) == (ref["nt"], ref["itev"], ref["ilev"]), name
    assert abs(got["circ_IC"] - ref["circ_IC"]) <= 1e-12 * max(1.0, abs(ref["circ_IC"])), name
    both = WINDOW[name] > 100
    err = {}
    for k in SERIES[:-1]:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (name, k)
        err[k] = (_rel(got[k], ref[k], 100), _rel(got[k], ref[k], 200) if both else None)
    for i in range(4):
        a, b = got["fourier4"][:, 0, i], ref["fourier4"][:, 0, i]
        err[f"A{i}"] = (_rel(a, b, 100), _rel(a, b, 200) if both else None)
    top = max(np.abs(ref[k]).max() for k in ("TEV", "LEV", "FREE"))
    rows = 0.0
    for k in ("TEV", "LEV", "FREE"):
        n = got[k].shape[1]
        # (a product run stores the live columns; the reference carries one zero-strength LEV slot more on a step that sheds none)
        assert n in (ref[k].shape[1], ref[k].shape[1] - 1) and np.isfinite(got[k]).all(), (name, k, got[k].shape, ref[k].shape)
        rows = max(rows, float(np.abs(got[k] - ref[k][:, :n]).max() / top))
    err["rows"] = (rows, None)
    return err


def worst(err):
    """-> (worst over the 100-step window, worst over the 200-step window or None)."""
    a = [v[0] for v in err.values() if v[0] is not None]
    b = [v[1] for v in err.values() if v[1] is not None]
    return max(a), (max(b) if b else None)


def show(label, err):
    w100, w200 = worst(err)
    tail = "" if w200 is None else f", first 200 steps {w200:.2e} (window {T3_200:.0e})"
    print(f"G10 {label}: first 100 steps {w100:.2e} (window {T3_100:.0e}){tail}")
    return w100, w200


def assert_within(label, err, factor=1.0):
    """Every figure inside its window divided by `factor` (the CPU tier's margin)."""
    show(label, err)
    for k, (e100, e200) in err.items():
        assert e100 is None or e100 <= T3_100 / factor, (label, k, e100)
        assert e200 is None or e200 <= T3_200 / factor, (label, k, e200)


def product_arrays(sim):
    """A product run (dense history, or sparse with step G10.SNAP stored) as G10.unpack names it."""
    s = G10.SNAP
    C = sim.circulation
    out = dict(Cl=sim.Cl, Cd=sim.Cd, Cm=sim.Cm, LESP=sim.LESP, LESP_prev=sim.LESP_prev, circ_TEV=C["TEV"], circ_LEV=C["LEV"],
               circ_bound=C["bound"], LEV_shed=np.asarray(sim.LEV_shed, dtype=np.float64), nt=sim.nt, itev=sim.itev, ilev=sim.ilev,
               circ_IC=float(C["IC"]), fourier4=sim.fourier[:, :, :4])
    nlev = int((out["LEV_shed"][:s + 1] != -1).sum())
    for k, n in (("TEV", s), ("LEV", nlev + 1), ("FREE", None)):
        out[k] = np.asarray(sim.path[k][s])[:, :n]
    return out
