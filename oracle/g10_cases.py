"""G10 case table: time loops off the unit point -- chord, Uinf, rho != 1 and cambered sections (TEST INFRASTRUCTURE ONLY).

The one source of truth of fixture group G10.  oracle/gen_golden.py (g10) runs the unmodified reference on these cases and
writes tests/golden/g10_off_unit_runs.npz; tests/test_g10_fixture.py (CPU) checks that the table is the fixture, that the
oracle and the host loop reproduce it, how many steps of each case the shedding decision is safe from an fp32 rounding, and
that no case can be met by a run that ignores chord, Uinf, rho or the camber; tests/test_gpu_g10.py runs each case through
the per-step path, the march (serial and overlapped) and `sweep`.  This module does not import the reference.

Every other time-loop fixture runs chord = 1, Uinf = 1, a symmetric section: there the camber product of the downwash row,
every power of chord and Uinf in the solve and the loads, and the mean line in the bound-vortex positions are multiplied by
1 or by 0.  The rules of the dimensional cases:
  chord, Uinf, rho pairwise different, none equal to 1; chord = 2 with Uinf = 3 makes every monomial c^a U^b distinct, so a
  wrong exponent cannot cancel; dt keeps dt Uinf / chord = 0.05, so the wake density per chord is config 1's.
The cambered sections use the published NACA 4-digit mean line on linspace(0, 1, Npoints) stations (the stand-in's opt-in,
oracle/airfoils_standin): everything downstream of the mean line is the reference's, the mean line itself is not pinned.

The reference has no similarity property in these variables (h_max, the pivot and the core radius do not scale together
with its dt): only its own numbers are the contract, there is no scale-the-result test.
"""
import numpy as np

from oracle.g9_cases import SERIES, free_cloud

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")

D23 = dict(chord=2, Uinf=3, rho=0.9, dt=0.05 * 2 / 3, h_max=2)
DHALF = dict(chord=0.5, Uinf=2, rho=1000, dt=0.05 * 0.5 / 2, h_max=0.5)
F_NFREE, F_SEED = 120, 10127
# the step whose wake rows the fixture keeps: the last one of the tight window (and of the 100-step cases).  The rows after step
# 200 are no contract: there the product's host loop, which differs from the reference by summation order only, is itself
# 1.5e-7 of the largest coordinate away on d23r.
SNAP = 100


def _case(name, steps, method="Faure", nfree=0, seed=0, **over):
    return dict(name=name, steps=steps, method=method, nfree=nfree, seed=seed, over=over)


CASES = [
    _case("d23", 200, **D23),
    _case("d23r", 200, method="Ramesh", **D23),
    _case("dhalf", 100, **DHALF),
    # (alpha_m = 6: with 5, |A0| passes within 7e-5 of LESPcrit at step 47, inside the margin an fp32 run is allowed)
    _case("k45", 200, **dict(D23, k=0.3 * np.pi, phi=45, alpha_m=6, alpha_max=15)),
    # (alpha_max = 12: at config 1's 10, |A0| passes within 1e-4 of LESPcrit at step 26)
    _case("c2412", 200, Naca="2412", alpha_max=12),
    _case("c6409", 200, Naca="6409", alpha_m=4),
    _case("c4412d", 200, method="Ramesh", **dict(D23, Naca="4412")),
    # 126 panels: the far side of the march's pair_f64_few | pair_f64 edge (oracle/g9_cases.py: "march few|plain")
    _case("c2412f", 100, nfree=F_NFREE, seed=F_SEED, **dict(D23, Naca="2412", Npoints=127)),
]
BY_NAME = {c["name"]: c for c in CASES}


def is_cambered(c):
    return c["over"].get("Naca", "0012")[:2] != "00"


CAMBERED = [c for c in CASES if is_cambered(c)]
SPY_CASE, SPY_STEPS = "c4412d", (1, 2, 50)
# the flow field of c4412d: one box around the foil and its near wake per step (the foil travels 10 chords in 100 steps),
# 32 x 24 and 40 x 24 points
FIELD_CASE = "c4412d"
FIELD_BOXES = {1: (-1.5, 2.5, 0.5, 3.5, 0.125), 100: (-11.0, -6.0, -3.5, -0.5, 0.125)}      # step: xmin, xmax, zmin, zmax, dr

# what a case is made of, as numbers (stored in the fixture, compared with the table)
KW_DEFAULTS = dict(alpha_m=0, alpha_max=10, k=0.2 * np.pi, phi=90, h_max=1)
PARAM_KEYS = ("chord", "Uinf", "rho", "dt", "h_max", "k", "phi", "alpha_m", "alpha_max", "Npoints", "Ncoeffs", "LESPcrit",
              "naca", "ramesh", "steps", "nfree", "seed")


def kwargs(c, **over):
    """Constructor keywords of the case (reference, oracle and product alike).  tf lies half a step short of the last level:
    t = arange(t0, tf + dt, dt) then has steps + 1 entries whatever the rounding of dt."""
    kw = dict(CONFIG1, method=c["method"])
    kw.update(c["over"])
    if c["nfree"]:
        g, xy = free_cloud(c["seed"], c["nfree"])
        kw.update(circulation_freevort=g, xy_freevort=xy)
    kw.update(over)
    kw["tf"] = (c["steps"] - 0.5) * kw["dt"]
    return kw


def params(c):
    """float64[len(PARAM_KEYS)]: the numbers a case is made of."""
    kw = dict(KW_DEFAULTS, **kwargs(c))
    kw.update(naca=int(kw["Naca"]), ramesh=c["method"] == "Ramesh", steps=c["steps"], nfree=c["nfree"], seed=c["seed"])
    return np.array([float(kw[k]) for k in PARAM_KEYS])


def key(c):
    return c["name"]


FOIL_KEYS = ("eta", "eta_panel", "detadx_panel", "x_panel")
META_KEYS = ("nt", "itev", "ilev", "circ_IC", "v_core", "cols_TEV", "cols_LEV", "cols_FREE")


def pack(sim, c):
    """What the fixture keeps of one run (a reference, oracle or product object with the dense history): `params`, `meta`
    (META_KEYS), `series` [len(SERIES), nt] over all steps, `fourier4` = fourier[:, :, :4], `lesp_prev` (A0 before
    the shedding decision of each step), `wake` [2, TEV | LEV | FREE
    columns], the live columns of the three wake rows after step SNAP side by side (LEV: one column more, the zero-strength
    slot the reference convects on a step that sheds no LEV), and for a cambered case the section's tables `foil`
    [eta | eta_panel | detadx_panel | x_panel]."""
    s = SNAP
    shed = np.asarray(sim.LEV_shed, dtype=np.float64)
    nlev = int((shed[:s + 1] != -1).sum())
    rows = [np.asarray(sim.path["TEV"][s])[:, :s], np.asarray(sim.path["LEV"][s])[:, :nlev + 1], np.asarray(sim.path["FREE"][s])]
    C = sim.circulation
    series = np.zeros([len(SERIES), sim.nt])       # (the circulations have nt - 1 entries: their rows end in a 0 that unpack drops)
    for i, a in enumerate((sim.Cl, sim.Cd, sim.Cm, sim.LESP, C["TEV"], C["LEV"], C["bound"], shed)):
        series[i, :len(a)] = a
    meta = np.array([sim.nt, sim.itev, sim.ilev, float(C["IC"]), sim.v_core] + [r.shape[1] for r in rows], dtype=np.float64)
    d = dict(params=params(c), meta=meta, series=series, fourier4=np.array(sim.fourier[:, :, :4], dtype=np.float64),
             lesp_prev=np.array(sim.LESP_prev, dtype=np.float64),
             wake=np.concatenate(rows, axis=1).astype(np.float64))
    if is_cambered(c):
        d["foil"] = np.concatenate([np.asarray(sim.airfoil[k], dtype=np.float64) for k in FOIL_KEYS])
    return d


def unpack(d):
    """A fixture entry (or pack()'s dict) as named arrays: the SERIES, fourier4, nt / itev / ilev / circ_IC / v_core, the TEV /
    LEV / FREE rows after step SNAP, params and (cambered cases) the section's tables."""
    meta = dict(zip(META_KEYS, d["meta"]))
    nt = int(meta["nt"])
    out = {k: d["series"][i, :nt - 1 if k.startswith("circ_") else nt] for i, k in enumerate(SERIES)}
    for k in ("nt", "itev", "ilev"):
        out[k] = int(meta[k])
    out["circ_IC"], out["v_core"] = float(meta["circ_IC"]), float(meta["v_core"])
    a = 0
    for k in ("TEV", "LEV", "FREE"):
        n = int(meta["cols_" + k])
        out[k] = d["wake"][:, a:a + n]
        a += n
    out["params"], out["fourier4"], out["LESP_prev"] = d["params"], d["fourier4"], d["lesp_prev"]
    if "foil" in d:
        npts = int(d["params"][PARAM_KEYS.index("Npoints")])
        cuts = np.cumsum([0, npts, npts - 1, npts - 1, npts - 1])
        for i, k in enumerate(FOIL_KEYS):
            out[k] = d["foil"][cuts[i]:cuts[i + 1]]
    return out
