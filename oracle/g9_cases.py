"""G9 case table: sweep members and marched runs at edge panel and wake counts (TEST INFRASTRUCTURE ONLY).

The one source of truth of fixture group G9.  oracle/gen_golden.py (g9) runs the unmodified reference on these cases and writes
tests/golden/g9_edge_runs.npz; tests/test_g9_fixture.py (CPU) checks that the inputs regenerate, that the oracle and the host
loop reproduce the fixture and that every pair of neighbouring panel counts still straddles the kernel constant it is named
after; tests/test_gpu_g9.py runs each case through `sweep` and through the solo march.  This module does not import the
reference.

Three groups:
  A  panel and coefficient counts: 100 steps, 120 free vortices (the wake grows from 120 to ~275 vortices: past 128, where the
     solo march gets its second source split and pair_f64_few starts, and past 256, the sweep's second source tile); Npoints - 1
     on both sides of every edge of npan + 1 (the sweep's chord targets) and of npan + 3 (the march's); 'Faure' and 'Ramesh'
  B  free-vortex counts around the source tiles, 30 steps, 'Faure'
  C  the capacity edge: nfree + 2 (nt - 1) = ENSEMBLE_MAX_WAKE exactly, one step
Free-vortex clouds come from g8_cases' counter-based generators, so the fixture regenerates bit for bit on any machine.
"""
import hashlib

import numpy as np

from oracle.g8_cases import normal12, uniform24

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")

A_NPAN = (2, 61, 62, 63, 64, 82, 83, 84, 85, 125, 126, 127, 128, 253, 254, 255, 256)
A_NCOEF = (4, 5, 30, 63, 64)                   # cycled over A_NPAN in this order
A_EXTRA = ((256, 64), (2, 64))
A_NFREE, A_TF, A_SNAP = 120, 5, 50
B_NFREE = (2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025)
B_TF, B_SNAP = 1.5, 30
C_NFREE, C_SNAP = 8190, 1
C_OVER = C_NFREE + 1                           # one vortex too many for a sweep member (refused; not in the fixture)

# (npan below, npan above, constants the edge is made of, what the edge is): the first count on the far side is `hi`
#   sweep: ntt = npan + 1 chord targets, slices = min(kBlock / ntt, kEnsSlicesMax); a second pass from ntt > kBlock
#   march: nt = npan + 3 chord targets, groups = min(kBlock / nt, kFewGroupsMax), pair_f64_few while 2 nt <= kBlock and
#          nt <= kFewTargets
PAIRS = [(63, 64, "sweep slices 4|3"), (84, 85, "sweep slices 3|2"), (127, 128, "sweep slices 2|1"),
         (255, 256, "sweep second pass"),
         (61, 62, "march groups 4|3"), (82, 83, "march groups 3|2"), (125, 126, "march few|plain"),
         (253, 254, "march kFewTargets")]


def free_cloud(seed, n):
    """(gamma[n], xy[2, n]) of a free-vortex cloud in [-3, -1] x [-0.5, 0.5]."""
    x = -3.0 + 2.0 * uniform24(seed, 1, n)
    z = -0.5 + uniform24(seed, 2, n)
    g = 0.02 * normal12(seed, 3, n)
    return g, np.stack([x, z])


def _case(name, group, npan, ncoef, nfree, seed, tf, methods, snap):
    return dict(name=name, group=group, npan=npan, ncoef=ncoef, nfree=nfree, seed=seed, tf=tf, methods=tuple(methods), snap=snap)


def _build():
    cases = []
    pairs = [(npan, A_NCOEF[i % len(A_NCOEF)]) for i, npan in enumerate(A_NPAN)] + list(A_EXTRA)
    for npan, ncoef in pairs:
        cases.append(_case(f"a{npan}-{ncoef}", "A", npan, ncoef, A_NFREE, 9000 + npan, A_TF, ("Faure", "Ramesh"), A_SNAP))
    for nf in B_NFREE:
        cases.append(_case(f"b{nf}", "B", 80, 30, nf, 9500 + nf, B_TF, ("Faure",), B_SNAP))
    cases.append(_case("b-default", "B", 80, 30, 0, 0, B_TF, ("Faure",), B_SNAP))       # no free vortices given
    cases.append(_case(f"c{C_NFREE}", "C", 80, 30, C_NFREE, 9000 + 80, CONFIG1["dt"], ("Faure",), C_SNAP))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
GROUP_A = [c for c in CASES if c["group"] == "A"]
GROUP_B = [c for c in CASES if c["group"] == "B"]
GROUP_C = [c for c in CASES if c["group"] == "C"]

PARAM_KEYS = ("npan", "ncoef", "nfree", "seed", "tf", "snap")


def params(c):
    """float64[len(PARAM_KEYS)]: the numbers a case is made of (stored in the fixture, compared with the table)."""
    return np.array([float(c[k]) for k in PARAM_KEYS])


def inputs(c):
    """(gamma, xy) of the case's free vortices, or None where none are given (the default: one zero-strength vortex)."""
    return free_cloud(c["seed"], c["nfree"]) if c["nfree"] else None


def kwargs(c, method="Faure", **over):
    """Constructor keywords of the case (reference, oracle and product alike)."""
    kw = dict(CONFIG1, tf=c["tf"], Npoints=c["npan"] + 1, Ncoeffs=c["ncoef"], method=method)
    inp = inputs(c)
    if inp is not None:
        kw.update(circulation_freevort=inp[0], xy_freevort=inp[1])
    kw.update(over)
    return kw


def over_capacity_kwargs():
    """Group C with one free vortex more: nfree + 2 (nt - 1) = ENSEMBLE_MAX_WAKE + 1."""
    g, xy = free_cloud(GROUP_C[0]["seed"], C_OVER)
    return dict(CONFIG1, tf=CONFIG1["dt"], circulation_freevort=g, xy_freevort=xy)


def key(c, method):
    return f"{c['name']}-{method}"


def digest(c):
    """uint8[32]: sha256 of the case's free vortices (float64, little-endian; of nothing where there are none)."""
    h = hashlib.sha256()
    inp = inputs(c)
    if inp is not None:
        for name, a in (("g", inp[0]), ("xy", inp[1])):
            h.update(name.encode())
            h.update(np.ascontiguousarray(a, dtype="<f8").tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


SERIES = ("Cl", "Cd", "Cm", "LESP", "circ_TEV", "circ_LEV", "circ_bound", "LEV_shed")
META_KEYS = PARAM_KEYS + ("nt", "itev", "ilev", "circ_IC", "cols_TEV", "cols_LEV", "cols_FREE")


def in_fixture(c, method):
    """Whether the fixture holds the reference's run of (case, method).  'Ramesh' runs only in the sweep, so the fixture keeps
    it at the panel counts next to an edge of the sweep's lane arithmetic; at the others (the march's edges, npan = 2) the
    'Ramesh' member is compared with OracleLUDVM at test time.  This keeps the fixture small."""
    return method == "Faure" or c["npan"] in SWEEP_EDGE_NPAN


SWEEP_EDGE_NPAN = frozenset(n for lo, hi, what in PAIRS if what.startswith("sweep") for n in (lo, hi))


def pack(sim, c):
    """What the fixture keeps of one run (a reference or oracle object, dense history), four arrays: `meta` (META_KEYS),
    `sha256` of the free vortices, `series` [len(SERIES), nt] over all steps, and `wake` [2, TEV | LEV | FREE columns]: the
    live columns of the three wake rows at the case's snapshot step, side by side (LEV: one column more, the zero-strength
    slot the reference convects on a step that sheds no LEV)."""
    s = c["snap"]
    shed = np.asarray(sim.LEV_shed, dtype=np.float64)
    nlev = int((shed[:s + 1] != -1).sum())
    rows = [np.asarray(sim.path["TEV"][s])[:, :s], np.asarray(sim.path["LEV"][s])[:, :nlev + 1], np.asarray(sim.path["FREE"][s])]
    C = sim.circulation
    series = np.zeros([len(SERIES), sim.nt])       # (the circulations have nt - 1 entries: their rows end in a 0 that unpack drops)
    for i, a in enumerate((sim.Cl, sim.Cd, sim.Cm, sim.LESP, C["TEV"], C["LEV"], C["bound"], shed)):
        series[i, :len(a)] = a
    meta = np.concatenate([params(c), [sim.nt, sim.itev, sim.ilev, float(C["IC"])], [r.shape[1] for r in rows]])
    return dict(meta=meta, sha256=digest(c), series=series, wake=np.concatenate(rows, axis=1).astype(np.float64))


def unpack(d):
    """A fixture entry (or pack()'s dict) as named arrays: the SERIES, nt / itev / ilev / circ_IC, TEV / LEV / FREE rows."""
    meta = dict(zip(META_KEYS, d["meta"]))
    nt = int(meta["nt"])
    out = {k: d["series"][i, :nt - 1 if k.startswith("circ_") else nt] for i, k in enumerate(SERIES)}
    for k in ("nt", "itev", "ilev"):
        out[k] = int(meta[k])
    out["circ_IC"] = float(meta["circ_IC"])
    a = 0
    for k in ("TEV", "LEV", "FREE"):
        n = int(meta["cols_" + k])
        out[k] = d["wake"][:, a:a + n]
        a += n
    out["params"], out["sha256"] = d["meta"][:len(PARAM_KEYS)], d["sha256"]
    return out
