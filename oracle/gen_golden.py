#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by importing and running the reference.

TEST INFRASTRUCTURE ONLY.  Runs in the build container, where /root/reference exists; the GPU box
never sees the reference, only the .npz files this script writes (inputs + expected outputs).

    python oracle/gen_golden.py            # writes tests/golden/*.npz

Fixture groups:
  G1 kernel KATs      -- LUDVM.induced_velocity (LUDVM.py:549-570) called unbound on seeded inputs;
                         needs no stand-in of any kind.
  G2 config-1 run     -- the README example (LUDVM.py:161-162): loads, Fourier coefficients, LESP,
                         circulations, wake snapshots.
  G3 boundary trace   -- every induced_velocity call (arguments and returns) of selected steps.
  G4 flowfield        -- coarse grid at three time steps (LUDVM.py:1186-1298).
  G5 variants         -- method='Ramesh', user free vortices, alpha_m != 0.
  G6 generators       -- the deterministic free-vortex cloud builders (LUDVM.py:53-96).
  G7 config-2 regime  -- BASELINE config 2's parameters (dt = 1e-3, v_core = 1.3e-3) run by the reference itself for the
                         first 1500 steps (the full 50 000 do not fit its dense history): loads, circulations, LESP, the
                         onset of LEV shedding (step 1335) and three wake rows.
  G8 fp32 routes      -- LUDVM.induced_velocity called unbound on sampled targets of the cases of oracle/g8_cases.py, which
                         straddle every routing threshold of the fp32 pair kernels (direct / symmetric, T = 4 / 8, quad,
                         tile sizes, targets per lane, grid patches, float64, hi+lo, Morton order).  Only outputs are
                         stored: the inputs regenerate from the case table (its digest is kept per case).
                             python oracle/gen_golden.py g8    # this group alone
  G9 edge runs        -- the unmodified reference class run on the cases of oracle/g9_cases.py: panel counts on both sides of
                         every edge of the sweep's and the march's chord-sum lane arithmetic, 4 .. 64 Fourier coefficients,
                         free-vortex counts around the source tiles, and a wake that fills a sweep member's slab exactly.
                             python oracle/gen_golden.py g9    # this group alone
  G10 off-unit runs   -- the unmodified reference class run on the cases of oracle/g10_cases.py: chord, Uinf and rho pairwise
                         different and none of them 1, other kinematics, and cambered NACA 4-digit sections; every
                         airfoil_downwash call of three steps and a flow field of one cambered dimensional case.
                             python oracle/gen_golden.py g10   # this group alone
G2-G5 and G9 run the unmodified reference class with oracle/airfoils_standin on sys.path (zero camber,
valid for the symmetric NACA0012 all BASELINE configs use).  G10 alone switches the stand-in's opt-in mean line on
(airfoils.MEAN_LINE = oracle.ludvm_oracle.naca4_camber, the published NACA 4-digit mean line): this pins everything the
reference does downstream of the mean line, not the mean line the PyPI package would hand over, and not .dat sections.
"""
import os
import sys
import io
import types
import contextlib
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "airfoils_standin"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

warnings.simplefilter("ignore", DeprecationWarning)
import LUDVM as REF  # noqa: E402  (the reference module)

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------- G1
def g1_kernel_kats():
    rng = np.random.default_rng(20260101)
    cases = {}

    def wake_like(n, offset=0.0):
        return rng.uniform(-10, 0, n) + offset, rng.uniform(-2, 2, n), rng.standard_normal(n)

    def add(name, g, xw, zw, xp, zp, v_core, viscous=True):
        ns = types.SimpleNamespace(v_core=v_core)
        u, w = REF.LUDVM.induced_velocity(ns, g, xw, zw, xp, zp, viscous=viscous)
        cases[name] = dict(g=np.asarray(g), xw=np.asarray(xw, float), zw=np.asarray(zw, float),
                           xp=np.asarray(xp, float), zp=np.asarray(zp, float),
                           v_core=float(v_core), viscous=bool(viscous), u=u, w=w)

    for vc, tag in ((0.065, "vc065"), (1.3e-3, "vc0013")):
        # single pair
        add(f"p1x1_{tag}", np.array([0.7]), np.array([-1.0]), np.array([0.25]), np.array([-0.4]), np.array([-0.1]), vc)
        # unit new TEV -> 80 chord points, integer circulation [1] (LUDVM.py:751)
        xa = np.linspace(-1.0, 0.0, 80) - 3.0
        za = 0.05 * np.sin(np.linspace(0, 3, 80))
        add(f"p80x1_int_{tag}", np.array([1]), np.array([0.012 - 3.0]), np.array([0.001]), xa, za, vc)
        # wake -> chord
        x, z, g = wake_like(603)
        add(f"p80x603_{tag}", g, x, z, xa, za, vc)
        # TEV slice of the wake as targets (targets are a subset of the sources: self pairs)
        x, z, g = wake_like(604)
        add(f"p400x604_self_{tag}", g, x, z, x[:400], z[:400], vc)
        add(f"p1x604_{tag}", g, x, z, x[603:], z[603:], vc)
        # odd sizes, disjoint sets
        xs, zs, gs = wake_like(1023)
        xt, zt, _ = wake_like(257)
        add(f"p257x1023_{tag}", gs, xs, zs, xt, zt, vc)
        # coordinates offset by -50 (late-time wake)
        xs, zs, gs = wake_like(1023, offset=-50.0)
        add(f"p257x1023_off50_{tag}", gs, xs, zs, xs[:257] + 1e-3, zs[:257] - 2e-3, vc)
        # non-contiguous views, as time_loop passes them (path[...][i,0,:k])
        big = rng.uniform(-5, 0, (3, 2, 700))
        gam = rng.standard_normal(700)
        add(f"p300x650_strided_{tag}", gam[:650], big[1, 0, :650], big[1, 1, :650], big[2, 0, :300], big[2, 1, :300], vc)
    # inviscid on disjoint sets (viscous != True -> v_core = 0, LUDVM.py:562-563)
    xs, zs, gs = wake_like(333)
    xt, zt, _ = wake_like(129)
    add("p129x333_inviscid", gs, xs, zs, xt, zt, 0.065, viscous=False)
    # inviscid with a coincident pair: the reference returns NaN there (0/0)
    with np.errstate(all="ignore"):
        add("p3x3_inviscid_self", np.array([1.0, -2.0, 0.5]), np.array([0.0, 1.0, 2.0]), np.array([0.0, 0.5, -0.5]),
            np.array([0.0, 1.5, 2.0]), np.array([0.0, 0.25, -0.5]), 0.065, viscous=False)
    # a medium all-pairs case
    x, z, g = wake_like(2048)
    add("p2048x2048_self_vc065", g / 2048, x, z, x, z, 0.065)

    flat = {}
    for name, c in cases.items():
        for k, v in c.items():
            flat[f"{name}/{k}"] = v
    np.savez_compressed(os.path.join(OUT, "g1_kernel_kats.npz"), **flat)
    print("G1:", len(cases), "cases")


# ------------------------------------------------------------------------------------------- runs
CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")


class Spy:
    """Records every induced_velocity call (G3) and every airfoil_downwash call (G10) of selected time steps."""

    def __init__(self, steps):
        self.steps = set(steps)
        self.calls = []
        self.downwash = []
        self.step = None


def run_reference(kwargs, spy=None):
    cls = REF.LUDVM
    if spy is None:
        return quiet(cls, **kwargs)
    orig_iv = cls.induced_velocity
    orig_dw = cls.airfoil_downwash

    def iv(self, circulation, xw, zw, xp, zp, viscous=True):
        u, w = orig_iv(self, circulation, xw, zw, xp, zp, viscous)
        # the current step is recovered from the wake-copy already done for row i (LUDVM.py:664-666):
        # spy.step is set by the downwash wrapper below, which receives i explicitly
        if spy.step in spy.steps:
            spy.calls.append(dict(step=spy.step, g=np.array(circulation), xw=np.array(xw), zw=np.array(zw),
                                  xp=np.array(xp), zp=np.array(zp), viscous=bool(viscous), u=u.copy(), w=w.copy()))
        return u, w

    def dw(self, circulation, xw, zw, i):
        spy.step = i
        W = orig_dw(self, circulation, xw, zw, i)
        if i in spy.steps:
            spy.downwash.append(dict(step=i, g=np.array(circulation, dtype=float), xw=np.array(xw), zw=np.array(zw), W=W.copy()))
        return W

    cls.induced_velocity = iv
    cls.airfoil_downwash = dw
    try:
        return quiet(cls, **kwargs)
    finally:
        cls.induced_velocity = orig_iv
        cls.airfoil_downwash = orig_dw


def pack_run(sim, snaps):
    d = dict(
        nt=sim.nt, itev=sim.itev, ilev=sim.ilev, v_core=sim.v_core,
        Cl=sim.Cl, Cd=sim.Cd, Cm=sim.Cm, Cn=sim.Cn, Cs=sim.Cs, Ct=sim.Ct,
        Fn=sim.Fn, Fs=sim.Fs, L=sim.L, D=sim.D, T=sim.T, M=sim.M,
        LESP=sim.LESP, LESP_prev=sim.LESP_prev, LEV_shed=sim.LEV_shed,
        circ_TEV=sim.circulation["TEV"], circ_LEV=sim.circulation["LEV"], circ_bound=sim.circulation["bound"],
        circ_FREE=np.asarray(sim.circulation["FREE"], float), circ_IC=float(sim.circulation["IC"]),
        circ_airfoil_last=sim.circulation["airfoil"][sim.itev], fourier=sim.fourier,
        alpha=sim.alpha, alpha_dot=sim.alpha_dot, h_dot=sim.h_dot, t=sim.t,
        airfoil_x=sim.airfoil["x"], airfoil_theta_panel=sim.airfoil["theta_panel"],
        path_airfoil_last=sim.path["airfoil"][-1], path_gamma_points_1=sim.path["airfoil_gamma_points"][1],
        snap_steps=np.array(snaps),
    )
    for s in snaps:
        d[f"TEV_{s}"] = sim.path["TEV"][s]
        d[f"LEV_{s}"] = sim.path["LEV"][s]
        d[f"FREE_{s}"] = sim.path["FREE"][s]
    return d


def g2_g3_g4_config1():
    spy = Spy(steps=[1, 2, 3, 4, 5, 100, 400])
    sim = run_reference(CONFIG1, spy)
    d = pack_run(sim, [1, 2, 10, 50, 100, 400])
    np.savez_compressed(os.path.join(OUT, "g2_config1.npz"), **d)
    print("G2: nt", sim.nt, "itev", sim.itev, "ilev", sim.ilev, "Cl[-3:]", sim.Cl[-3:])

    flat = {"ncalls": len(spy.calls)}
    for k, c in enumerate(spy.calls):
        for key, v in c.items():
            flat[f"{k}/{key}"] = v
    np.savez_compressed(os.path.join(OUT, "g3_boundary_trace.npz"), **flat)
    print("G3:", len(spy.calls), "calls")

    tsteps = [0, 50, 200]
    quiet(sim.flowfield, xmin=-10, xmax=0, zmin=-4, zmax=4, dr=0.25, tsteps=tsteps)
    np.savez_compressed(os.path.join(OUT, "g4_flowfield.npz"), tsteps=np.array(tsteps), dr=0.25,
                        box=np.array([-10.0, 0.0, -4.0, 4.0]), x_ff=sim.x_ff, z_ff=sim.z_ff,
                        u_ff=sim.u_ff, w_ff=sim.w_ff, ome_ff=sim.ome_ff)
    print("G4: grid", sim.x_ff.shape)


def g5_variants():
    # (a) Ramesh (Newton) method, short run
    kw = dict(CONFIG1, tf=2, method="Ramesh")
    sim = run_reference(kw)
    np.savez_compressed(os.path.join(OUT, "g5_ramesh.npz"), **pack_run(sim, [1, 10, sim.nt - 1]))
    print("G5a Ramesh: nt", sim.nt, "ilev", sim.ilev)
    # (b) user free vortices: the reference's own deterministic cloud (LUDVM.py:53-71)
    xy, gam = REF.generate_free_single_vortex()
    kw = dict(CONFIG1, tf=5, circulation_freevort=gam, xy_freevort=np.transpose(xy))
    sim = run_reference(kw)
    d = pack_run(sim, [1, 10, sim.nt - 1])
    d["xy_freevort"] = np.transpose(xy)
    d["gamma_freevort"] = gam
    np.savez_compressed(os.path.join(OUT, "g5_freevort.npz"), **d)
    print("G5b free vortices: n_free", sim.n_freevort, "ilev", sim.ilev)
    # (c) non-zero mean pitch
    kw = dict(CONFIG1, tf=5, alpha_m=5, alpha_max=15)
    sim = run_reference(kw)
    np.savez_compressed(os.path.join(OUT, "g5_alpham.npz"), **pack_run(sim, [1, 10, sim.nt - 1]))
    print("G5c alpha_m: ilev", sim.ilev)


def g6_generators():
    """Deterministic free-vortex generators (LUDVM.py:53-96)."""
    xy1, g1 = REF.generate_free_single_vortex()
    xy2, g2 = REF.generate_flowfield_vortices()
    np.savez_compressed(os.path.join(OUT, "g6_generators.npz"), single_xy=xy1, single_gamma=g1, lattice_xy=xy2,
                        lattice_gamma=g2)
    print("G6: single", xy1.shape, "lattice", xy2.shape)


def g7_config2_regime():
    """The reference at config 2's parameters over the first 1500 steps (LUDVM.py:597-1171 at dt = 1e-3)."""
    import time
    kw = dict(CONFIG1, dt=1e-3, tf=1.5)
    t0 = time.time()
    sim = run_reference(kw)
    shed = sim.LEV_shed != -1
    d = dict(nt=sim.nt, itev=sim.itev, ilev=sim.ilev, v_core=sim.v_core, Cl=sim.Cl, Cd=sim.Cd, Cm=sim.Cm, LESP=sim.LESP,
             LEV_shed=sim.LEV_shed, circ_TEV=sim.circulation["TEV"], circ_LEV=sim.circulation["LEV"],
             circ_bound=sim.circulation["bound"], circ_IC=float(sim.circulation["IC"]), fourier4=sim.fourier[:, :, :4],
             first_lev_step=int(np.argmax(shed)) if shed.any() else -1)
    for s_ in (300, 1000, 1500):
        d[f"TEV_{s_}"] = sim.path["TEV"][s_][:, :s_ + 1]
        d[f"LEV_{s_}"] = sim.path["LEV"][s_][:, :max(1, sim.ilev + 1)]
    np.savez_compressed(os.path.join(OUT, "g7_config2_first1500.npz"), **d)
    print("G7: nt", sim.nt, "itev", sim.itev, "ilev", sim.ilev, "first LEV at step", d["first_lev_step"],
          "reference wall %.0f s" % (time.time() - t0))


def g8_fp32_routes():
    """The G8 cases (oracle/g8_cases.py): the reference's pair sum on each case's sampled targets x all its sources."""
    import time
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from oracle import g8_cases as G8
    t0 = time.time()

    def ref(vc, g, xw, zw, xp, zp):
        ns = types.SimpleNamespace(v_core=vc)
        rows = max(1, (1 << 24) // max(len(xw), 1))          # ~8 temporaries of rows x len(xw) float64: <= ~1 GB
        u, w = np.empty(len(xp)), np.empty(len(xp))
        for a in range(0, len(xp), rows):
            u[a:a + rows], w[a:a + rows] = REF.LUDVM.induced_velocity(ns, g, xw, zw, xp[a:a + rows], zp[a:a + rows])
        return u, w

    flat = {}
    for c in G8.CASES:
        inp = G8.inputs(c)
        idx = G8.sample(c)
        xp, zp = G8.targets(c, inp, idx)
        u, w = ref(c["v_core"], inp["g"], inp["xs"], inp["zs"], xp, zp)
        name = c["name"]
        flat[f"{name}/idx"] = idx
        flat[f"{name}/u"] = u
        flat[f"{name}/w"] = w
        flat[f"{name}/params"] = G8.params(c)
        flat[f"{name}/sha256"] = G8.digest(inp)
        if "foil_x" in inp:        # the second call of :1105-1106: the bound vortices on the same wake points
            flat[f"{name}/u_foil"], flat[f"{name}/w_foil"] = ref(c["v_core"], inp["foil_g"], inp["foil_x"], inp["foil_z"], xp, zp)
        print(f"G8 {name}: {len(idx)} x {c['ns']}  ({time.time() - t0:.0f} s)", flush=True)
    path = os.path.join(OUT, "g8_fp32_routes.npz")
    np.savez_compressed(path, **flat)
    print("G8:", len(G8.CASES), "cases,", os.path.getsize(path), "bytes")


def g9_edge_runs():
    """The G9 cases (oracle/g9_cases.py): loads, LESP, circulations and one set of wake rows per case and method."""
    import time
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from oracle import g9_cases as G9
    t0 = time.time()
    flat = {}
    for c in G9.CASES:
        for method in c["methods"]:
            if not G9.in_fixture(c, method):
                continue
            sim = run_reference(G9.kwargs(c, method))
            for k, v in G9.pack(sim, c).items():
                flat[f"{G9.key(c, method)}/{k}"] = v
            print(f"G9 {G9.key(c, method)}: nt {sim.nt} itev {sim.itev} ilev {sim.ilev}  ({time.time() - t0:.0f} s)", flush=True)
    path = os.path.join(OUT, "g9_edge_runs.npz")
    np.savez_compressed(path, **flat)
    print("G9:", len(G9.CASES), "cases,", os.path.getsize(path), "bytes")


def g10_off_unit_runs():
    """The G10 cases (oracle/g10_cases.py): loads, LESP, circulations, A0 .. A3 and the wake after the last step per case, the
    section's tables of the cambered ones; every airfoil_downwash call of three steps and the flow field of c4412d."""
    import time
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    import airfoils
    from oracle import g10_cases as G10
    from oracle.ludvm_oracle import naca4_camber
    t0 = time.time()
    flat = {}
    airfoils.MEAN_LINE = naca4_camber
    try:
        for c in G10.CASES:
            spy = Spy(G10.SPY_STEPS) if c["name"] == G10.SPY_CASE else None
            sim = run_reference(G10.kwargs(c), spy)
            for k, v in G10.pack(sim, c).items():
                flat[f"{G10.key(c)}/{k}"] = v
            if spy is not None:
                flat["downwash/ncalls"] = np.array(len(spy.downwash))
                for n, call in enumerate(spy.downwash):
                    for k, v in call.items():
                        flat[f"downwash/{n}_{k}"] = v
            if c["name"] == G10.FIELD_CASE:
                for s, (xmin, xmax, zmin, zmax, dr) in G10.FIELD_BOXES.items():
                    quiet(sim.flowfield, xmin=xmin, xmax=xmax, zmin=zmin, zmax=zmax, dr=dr, tsteps=[s])
                    flat[f"field/{s}"] = np.stack([sim.x_ff, sim.z_ff, sim.u_ff[0], sim.w_ff[0], sim.ome_ff[0]])
            print(f"G10 {G10.key(c)}: nt {sim.nt} itev {sim.itev} ilev {sim.ilev}  ({time.time() - t0:.0f} s)", flush=True)
    finally:
        airfoils.MEAN_LINE = None
    path = os.path.join(OUT, "g10_off_unit_runs.npz")
    np.savez_compressed(path, **flat)
    print("G10:", len(G10.CASES), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "g10":
        g10_off_unit_runs()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g9":
        g9_edge_runs()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g7":
        g7_config2_regime()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "g8":
        g8_fp32_routes()
        sys.exit(0)
    g1_kernel_kats()
    g2_g3_g4_config1()
    g5_variants()
    g6_generators()
    g7_config2_regime()
    g8_fp32_routes()
    g9_edge_runs()
    g10_off_unit_runs()
    tot = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("total fixture bytes:", tot)
