"""Shared by tests/test_solve_steps_host.py and tests/test_gpu_solve_steps.py: ONE time-step SOLVE of a run, checked by value
against the run's own state (the companion of tests/rollup_common.py, which does the same for the step's roll-up).

A run that holds the wake before step i (row i - 1 of a dense history, or of a sparse one that records every step) says
everything step i's solve starts from.  From it the host rebuilds, as the reference writes them (citations are file:line into
LUDVM.py, as in oracle/ludvm_oracle.py): the placements of the new vortices (:672-681, :788-800), the three downwash terms
(:743-754, :924-934; T1 from a float64 pair sum of the old wake at the step's chord points, T2 and T3 from unit vortices), the
solution before the leading-edge test (Faure's closed form :758-760; for Ramesh the exact root of the Kelvin residual, which
is linear in Gamma_TEV), the test itself (:781) and the sign LESPcrit takes (:802-805), on a shedding step the exact 2 x 2
solution for (Gamma_TEV, Gamma_LEV) (:944-954, and Ramesh's two conditions :807-914, linear as well: no Newton is replayed),
the Fourier coefficients of the final W with the derivatives of the pre-LEV ones (:963-966), the bound vorticity (:987-1010)
and the loads with the chord velocity from a direct pair sum over the wake INCLUDING the step's new vortices (:1035-1090).
No step depends on an earlier one, so the flow's divergence does not enter: step 400 is checked as sharply as step 2.

How the pieces are chained.  `model_step(..., adopt=False)` solves the whole step from the old wake alone (what a correct
implementation computes; with `fault=` what a named wrong one computes: the sensitivity tests plant those rows).
`step_solve_residuals` runs it with adopt=True: the circulations, then the Fourier rows, are taken from the RUN once they have
been compared, so every later quantity is checked against its own inputs and a residual names the stage that is wrong.  The
one thing a run does not hold is the pre-LEV Gamma_TEV of a shedding step: there LESP_prev and the derivative row are checked
against the exact root, and for Ramesh (whose Newton stops at its own `maxerror`) they get the allowance `Step.allow` states.

Host only (NumPy and the oracle's pair sum); nothing here knows how a kernel is launched.
"""
import copy
import types
from collections import namedtuple

import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz

# every quantity of a step that has a residual and a scale
QUANTITIES = ("G_TEV", "G_LEV", "bound", "kelvin", "lesp_cond", "LESP_prev", "LESP", "fourier", "fourier_dot",
              "gamma_airfoil", "airfoil", "Gamma_airfoil", "Fn", "Fs", "L", "D", "M", "Cl", "Cd", "Cm")

# What step_solve_residuals returns.  `res`: quantity -> |run - expected| (max over a row); `scale`: quantity -> the sum of the
# magnitudes of the terms the quantity is made of (what float64 rounds at); `allow`: quantity -> what Ramesh's Newton may
# leave on top of the float64 bound (empty for Faure); `margin`: | |A0 before the LEV test| - |LESPcrit| |; `shed`: the
# checker's decision, `shed_run`: the run's; `events`: names of what the step went through; `n_wake`: wake size before the
# step; `newton`: for Ramesh dict(kelvin, lesp_cond, jinv) -- |residuals| of its two conditions at the run's circulations and
# the inf-norm of the inverse of the linear system the step solved.
Step = namedtuple("Step", "res scale allow margin shed shed_run events n_wake newton")

CONTRACT = 1e-12            # per-call float64 contract of include/ludvm_hip.h: no bound below it
LOADS_BOUND = 1e-9          # the suite's float64 bound for loads: no bound above it
DEVICE_FACTOR = 64          # the device partitions the sums differently (thousands of 128-source splits) and takes its
                            # reciprocal root by v_rsq_f64 + Newton: neither is modelled on the host

# ---- the host floors (tests/test_solve_steps_host.py measures and asserts them; profiles/solve_steps_residuals.txt) -----
# Largest residual / scale of each quantity over: the oracle's runs of config 1, d23, c4412d, c2412f and c150 ('Faure' and
# 'Ramesh', sources in given and in reversed order) and the product's host loop on tests/fake_engine.py.
HOST_FLOOR = {
    "G_TEV": 1.3e-16, "G_LEV": 1.6e-16, "bound": 4.2e-16, "kelvin": 2.7e-16, "lesp_cond": 3.3e-16, "LESP_prev": 1.4e-15,
    "LESP": 1.2e-15, "fourier": 1.2e-15, "fourier_dot": 5.6e-16, "gamma_airfoil": 5.6e-16, "airfoil": 7.6e-16,
    "Gamma_airfoil": 7.1e-16, "Fn": 2.0e-16, "Fs": 0.0, "L": 1.8e-16, "D": 3.2e-17, "M": 1.1e-16, "Cl": 1.8e-16, "Cd": 3.2e-17,
    "Cm": 1.1e-16,
}


def bound_from_floor(floor):
    return min(max(DEVICE_FACTOR * floor, CONTRACT), LOADS_BOUND)


BOUND = {q: bound_from_floor(HOST_FLOOR[q]) for q in QUANTITIES}


def _row(P, fam, i):
    return np.asarray(P[fam][i])


def counts(sim, i):
    """(itev, ilev, shed[]) before step i, from LEV_shed."""
    shed = np.asarray(sim.LEV_shed) != -1
    return i - 1, int(shed[:i].sum()), shed


def old_wake(sim, i, row=None):
    """(g, x, z) of the wake before step i in the reference's order TEV | LEV | FREE (:743-745), positions of row i - 1."""
    itev, ilev, _ = counts(sim, i)
    r = i - 1 if row is None else row
    P, C = sim.path, sim.circulation
    t, l, f = _row(P, "TEV", r)[:, :itev], _row(P, "LEV", r)[:, :ilev], _row(P, "FREE", r)
    g = np.concatenate([np.asarray(C["TEV"])[:itev], np.asarray(C["LEV"])[:ilev], np.atleast_1d(np.asarray(C["FREE"], dtype=float))])
    return g, np.concatenate([t[0], l[0], f[0]]), np.concatenate([t[1], l[1], f[1]])


def placements(sim, i, lev_rule=None):
    """-> (tev_xy, lev_xy) of step i.  lev_rule: None (the reference's), 'le' or 'third' (forced: a fault)."""
    itev, ilev, shed = counts(sim, i)
    P, foil = sim.path, sim.path["airfoil"]
    te, le = foil[i, :, -1], foil[i, :, 0]
    if itev == 0:
        tev = foil[0, :, -1] + np.array([0.5 * sim.Uinf * sim.dt, 0])                       # :672-676
    else:
        tev = te + 1 / 3 * (_row(P, "TEV", i - 1)[:, itev - 1] - te)                        # :678-681
    third = ilev > 0 and shed[i - 1] if lev_rule is None else (lev_rule == "third")
    lev = le + 1 / 3 * (_row(P, "LEV", i - 1)[:, ilev - 1] - le) if third else np.array(le, dtype=float)   # :788-800
    return tev, lev


def model_step(sim, i, iv, adopt=False, fault=None):
    """Step i >= 1 of `sim` solved on the host from the wake before it.  -> dict of everything the step stores (under the
    names of QUANTITIES, rows as arrays) plus what the checker reports.  adopt: take Gamma_TEV, Gamma_LEV, the shedding decision
    and the Fourier rows from the run once they are compared.  fault (adopt=False): one of 'drop_last', 'row_i', 'lev_le',
    'lev_third', 'no_flip', 'loads_old_wake', 'bound_other' -- what a named wrong implementation computes."""
    assert i >= 1
    pi, U, c, rho, dt, vc = np.pi, sim.Uinf, sim.chord, sim.rho, sim.dt, sim.v_core
    piv = getattr(sim, "piv", 0.25 * c)
    C, af = sim.circulation, sim.airfoil
    ramesh = sim.method == "Ramesh"
    itev, ilev, shed = counts(sim, i)
    a, ad, hd = sim.alpha[i], sim.alpha_dot[i], sim.h_dot[i]
    gp = sim.path["airfoil_gamma_points"]
    xp, zp = np.array(gp[i, 0]), np.array(gp[i, 1])
    th, thp = af["theta"], af["theta_panel"]
    detadx, eta_p, x_p = af["detadx_panel"], af["eta_panel"], af["x_panel"]
    nc = sim.fourier.shape[2]
    cm1 = np.cos(thp) - 1
    cosn = np.cos(np.arange(nc)[:, None] * thp[None, :])

    def frame(u1, w1):
        return u1 * np.cos(a) - w1 * np.sin(a), u1 * np.sin(a) + w1 * np.cos(a)         # :587-588

    def unit(xy):
        u1, w1 = iv(np.array([1.0]), np.array([xy[0]]), np.array([xy[1]]), xp, zp, vc)
        ut, un = frame(u1, w1)
        return detadx * ut - un, ut

    # T1, T2, T3
    g_old, xw, zw = old_wake(sim, i, row=i if fault == "row_i" else None)
    g1, x1, z1 = (g_old[:-1], xw[:-1], zw[:-1]) if fault == "drop_last" else (g_old, xw, zw)
    u1, w1 = iv(g1, x1, z1, xp, zp, vc)
    uo, wo = frame(u1, w1)
    T1 = detadx * (U * np.cos(a) + hd * np.sin(a) + uo - ad * eta_p) - U * np.sin(a) - ad * (x_p - piv) + hd * np.cos(a) - wo   # :590-595
    tev_xy, lev_xy = placements(sim, i, {"lev_le": "le", "lev_third": "third"}.get(fault))
    T2, ut = unit(tev_xy)
    T3, ul = unit(lev_xy)
    I1, I2, I3 = (_trapz(T * cm1, thp) for T in (T1, T2, T3))
    J1, J2, J3 = (-1 / pi * _trapz(T, thp) for T in (T1, T2, T3))
    s_old = np.sum(np.asarray(C["TEV"])[:itev]) + np.sum(np.asarray(C["LEV"])[:ilev]) + np.sum(C["FREE"])
    IC = C["IC"]
    cf = c if ramesh else 1.0       # Ramesh's bound circulation U c pi (A0 + A1 / 2) = c trapz(W (cos - 1)); Faure's has no c

    def coefficients(W, a0=None):
        A = 2 / pi * _trapz(W / U * cosn, thp, axis=1)          # row n: 2 / pi trapz(W / U cos(n theta)), :767-770
        A[0] = -1 / pi * _trapz(W / U, thp) if a0 is None else a0
        return A

    def bound_of(A, gt, gl, other=False):
        if ramesh != other:
            return U * c * pi * (A[0] + A[1] / 2)                                        # :703, :846
        return I1 + gt * I2 + gl * I3                                                   # :762, :956

    # before the leading-edge test: the exact root
    g0 = -(cf * I1 + s_old - IC) / (1 + cf * I2)                                         # :758-760 / root of :698-699
    jinv_pre = 1 / abs(1 + cf * I2)
    A_exact = coefficients(T1 + g0 * T2)
    shed_exp = bool(abs(A_exact[0]) >= abs(sim.LESPcrit))                                # :781
    margin = abs(abs(A_exact[0]) - abs(sim.LESPcrit))
    shed_run = bool(shed[i])
    sheds = shed_run if adopt else shed_exp
    gt_run = float(np.asarray(C["TEV"])[itev])
    gl_run = float(np.asarray(C["LEV"])[ilev]) if shed_run else 0.0
    # the pre-LEV solution of a step that does not shed is the step's solution: the run holds it
    g_pre = gt_run if (adopt and not sheds) else g0
    A_pre = coefficients(T1 + g_pre * T2)
    F1 = (A_pre - sim.fourier[i - 1, 0, :]) / dt                                         # :772-773, kept on a shedding step :963-966
    if fault == "deriv_post":
        F1 = None
    out = dict(LESP_prev=A_pre[0], fourier_dot=F1)

    jinv = jinv_pre
    lc = 0.0
    if sheds:
        lc = -abs(sim.LESPcrit) if (A_pre[0] < 0 and fault != "no_flip") else abs(sim.LESPcrit)     # :802-805
        if ramesh:
            M = np.array([[1 + c * I2, 1 + c * I3], [J2 / U, J3 / U]])
            b = np.array([-(c * I1 + s_old - IC), lc - J1 / U])
        else:
            M = np.array([[1 + I2, 1 + I3], [J2, J3]])                                   # :944-954
            b = np.array([-(I1 + s_old - IC), lc - J1])
        gt_x, gl_x = np.linalg.solve(M, b)
        jinv = np.abs(np.linalg.inv(M)).sum(axis=1).max()
    else:
        gt_x, gl_x = g0, 0.0
    gt, gl = (gt_run, gl_run) if adopt else (gt_x, gl_x)
    W = T1 + gt * T2 + gl * T3
    if sheds:
        F0 = coefficients(W, a0=None if ramesh else J1 + gt * J2 + gl * J3)              # :959 (Faure: no 1 / Uinf there)
    else:
        F0 = coefficients(W)
    if F1 is None:
        F1 = (F0 - sim.fourier[i - 1, 0, :]) / dt
        out["fourier_dot"] = F1
    bnd = bound_of(F0, gt, gl, other=fault == "bound_other")
    kel = bound_of(F0, gt, gl) + gt + gl + s_old - IC                                    # :698-699, :758-760, :946-948
    out.update(G_TEV=gt_x, G_LEV=gl_x, bound=bnd, kelvin=kel, lesp_cond=(lc - F0[0]) if sheds else 0.0, LESP=F0[0], fourier=F0)

    # bound vorticity (:987-1010) from the Fourier row (the run's own once it is compared)
    A = np.asarray(sim.fourier[i, 0, :], dtype=float) if adopt else F0
    Ad = np.asarray(sim.fourier[i, 1, :], dtype=float) if adopt else F1
    term2, abs2 = np.zeros(len(thp)), np.zeros(len(thp))
    for n in range(1, nc):
        term2 = A[n] * np.sin(n * thp) + term2
        abs2 = abs(A[n]) * np.abs(np.sin(n * thp)) + abs2
    cot = (1 + np.cos(thp)) / np.sin(thp)
    gamma = 2 * U * (A[0] * cot + term2)
    gamma_abs = 2 * U * (abs(A[0]) * cot + abs2)
    geo = c / 2 * np.sin(thp) * (th[1:] - th[:-1])
    dG = gamma * geo
    out.update(gamma_airfoil=gamma, airfoil=dG, Gamma_airfoil=np.cumsum(dG))      # (:1008-1010 sums dG[:j + 1] anew for every j: the same to rounding)

    # loads (:1035-1090): u from a direct pair sum over the wake with the step's new vortices in it
    new_g, new_x, new_z = [gt], [tev_xy[0]], [tev_xy[1]]
    if sheds:
        new_g.append(gl), new_x.append(lev_xy[0]), new_z.append(lev_xy[1])
    if fault == "loads_old_wake":
        gl_, xl_, zl_ = g_old, xw, zw
    else:
        gl_, xl_, zl_ = np.concatenate([g_old, new_g]), np.concatenate([xw, new_x]), np.concatenate([zw, new_z])
    uu, ww = iv(gl_, xl_, zl_, xp, zp, vc)
    u, _ = frame(uu, ww)
    Ueff = U * np.cos(a) + hd * np.sin(a)
    A0, A1, A2 = A[0], A[1], A[2]
    A0d, A1d, A2d, A3d = Ad[:4]
    Fn = rho * pi * c * U * (Ueff * (A0 + 0.5 * A1) + c * (3 / 4 * A0d + 1 / 4 * A1d + 1 / 8 * A2d)) + rho * _trapz(u * gamma, x_p)
    Fs = rho * pi * c * U**2 * A0**2
    L, D = Fn * np.cos(a) + Fs * np.sin(a), Fn * np.sin(a) - Fs * np.cos(a)
    Mo = piv * Fn - rho * pi * c**2 * U * (Ueff * (1 / 4 * A0 + 1 / 4 * A1 - 1 / 8 * A2)
                                           + c * (7 / 16 * A0d + 3 / 16 * A1d + 1 / 16 * A2d - 1 / 64 * A3d)) \
        - rho * _trapz(u * gamma * x_p, x_p)
    q = 0.5 * rho * U**2 * c
    out.update(Fn=Fn, Fs=Fs, L=L, D=D, M=Mo, Cl=L / q, Cd=D / q, Cm=Mo / (q * c))

    # ---- scales: the magnitudes of the terms each quantity is made of -----------------------------------------------------
    Wabs = np.abs(T1) + abs(gt) * np.abs(T2) + abs(gl) * np.abs(T3)
    Wabs_pre = np.abs(T1) + abs(g_pre) * np.abs(T2)
    s_g = cf * _trapz(Wabs * np.abs(cm1), thp) + np.abs(g_old).sum() + abs(gt) + abs(gl) + abs(IC)
    s_a0 = 1 / pi * _trapz(Wabs, thp) * (1.0 if (sheds and not ramesh) else 1 / U)
    s_an = 2 / pi * _trapz(Wabs, thp) / U
    s_pre = 2 / pi * _trapz(Wabs_pre, thp) / U
    u_abs = np.abs(uo) + abs(gt) * np.abs(ut) + abs(gl) * np.abs(ul)
    s_fn = rho * pi * c * U * (abs(Ueff) * (abs(A0) + 0.5 * abs(A1)) + c * (3 / 4 * abs(A0d) + 1 / 4 * abs(A1d) + 1 / 8 * abs(A2d))) \
        + rho * _trapz(u_abs * gamma_abs, x_p)
    s_fs = rho * pi * c * U**2 * A0**2
    s_m = piv * s_fn + rho * pi * c**2 * U * (abs(Ueff) * (1 / 4 * abs(A0) + 1 / 4 * abs(A1) + 1 / 8 * abs(A2))
                                              + c * (7 / 16 * abs(A0d) + 3 / 16 * abs(A1d) + 1 / 16 * abs(A2d) + 1 / 64 * abs(A3d))) \
        + rho * _trapz(u_abs * gamma_abs * np.abs(x_p), x_p)
    s_ld = s_fn + s_fs
    scale = dict(G_TEV=s_g, G_LEV=s_g, bound=s_g, kelvin=s_g, lesp_cond=s_a0 + abs(sim.LESPcrit), LESP_prev=s_pre / 2, LESP=s_a0,
                 fourier=s_an, fourier_dot=2 * s_pre / dt, gamma_airfoil=gamma_abs.max(), airfoil=(gamma_abs * geo).max(),
                 Gamma_airfoil=(gamma_abs * geo).sum(), Fn=s_fn, Fs=s_fs, L=s_ld, D=s_ld, M=s_m,
                 Cl=s_ld / q, Cd=s_ld / q, Cm=s_m / (q * c))
    if scale["Fs"] == 0.0:
        scale["Fs"] = np.finfo(float).tiny

    # ---- what Ramesh's Newton may leave (it stops at |residual| <= maxerror, :686, :812) -----------------------------------
    allow = {}
    if ramesh:
        me = getattr(sim, "maxerror", 1e-10)
        allow = dict(G_TEV=me * jinv, G_LEV=me * jinv if sheds else 0.0)
        if sheds:
            # the pre-LEV Gamma_TEV of a shedding step is not stored: |it - root| <= maxerror / |1 + c I2|
            proj = max(abs(J2), np.abs(2 / pi * _trapz(T2 * cosn[1:], thp, axis=1)).max()) / U
            allow["LESP_prev"] = me * jinv_pre * abs(J2) / U
            allow["fourier_dot"] = me * jinv_pre * proj / dt
    ev = set()
    if i == 1:
        ev.add("first step")
    if sheds:
        ev.add("first LEV" if ilev == 0 else ("consecutive LEV" if shed[i - 1] else "LEV after a gap"))
        ev.add("shed A0 < 0" if A_pre[0] < 0 else "shed A0 > 0")
    elif ilev > 0 and shed[i - 1]:
        ev.add("no LEV after shedding")
    out.update(_scale=scale, _allow=allow, _margin=margin, _shed=shed_exp, _shed_run=shed_run, _events=ev, _n_wake=len(g_old),
               _jinv=jinv, _sheds=sheds, _G_run=(gt_run, gl_run), _placements=(tev_xy, lev_xy))
    return out


def run_values(sim, i):
    """What the run stores for step i, under the names of QUANTITIES (Cl, Cd, Cm where the run has them)."""
    itev, ilev, shed = counts(sim, i)
    C = sim.circulation
    v = dict(G_TEV=C["TEV"][itev], G_LEV=C["LEV"][ilev] if shed[i] else 0.0, bound=C["bound"][itev],
             LESP_prev=sim.LESP_prev[itev], LESP=np.array([sim.LESP[itev], sim.fourier[i, 0, 0]]),
             fourier=sim.fourier[i, 0, :], fourier_dot=sim.fourier[i, 1, :], gamma_airfoil=C["gamma_airfoil"][itev],
             airfoil=C["airfoil"][itev], Gamma_airfoil=C["Gamma_airfoil"][itev],
             Fn=sim.Fn[i], Fs=sim.Fs[i], L=sim.L[i], D=sim.D[i], M=sim.M[i])
    for k in ("Cl", "Cd", "Cm"):
        if getattr(sim, k, None) is not None:
            v[k] = getattr(sim, k)[i]
    return v


def step_solve_residuals(sim, i, iv):
    """Residuals of step i >= 1 of `sim` (anything that holds, for step i, the wake after step i - 1, circulation, fourier,
    LESP, LESP_prev, LEV_shed, Fn, Fs, L, D, M, alpha, alpha_dot, h_dot, airfoil, path['airfoil' | 'airfoil_gamma_points']
    and the constants).  `iv(g, xs, zs, xp, zp, v_core) -> (u, w)`: a float64 pair sum."""
    m = model_step(sim, i, iv, adopt=True)
    run = run_values(sim, i)
    res = {}
    for k, got in run.items():
        res[k] = float(np.max(np.abs(np.asarray(got, dtype=float) - m[k])))
    # the two conditions at the run's circulations (for Faure residuals like any other; for Ramesh what Newton stopped at)
    res["kelvin"], res["lesp_cond"] = abs(m["kelvin"]), abs(m["lesp_cond"])
    newton = dict(kelvin=res["kelvin"], lesp_cond=res["lesp_cond"], jinv=m["_jinv"]) if sim.method == "Ramesh" else None
    if newton:
        del res["kelvin"], res["lesp_cond"]
    return Step(res, m["_scale"], m["_allow"], m["_margin"], m["_shed"], m["_shed_run"], m["_events"], m["_n_wake"], newton)


def over_bound(step, bound=None):
    """{quantity: residual / (bound * scale + allowance)} of the quantities of a step that exceed their bound."""
    bound = BOUND if bound is None else bound
    out = {}
    for k, r in step.res.items():
        lim = bound[k] * step.scale[k] + step.allow.get(k, 0.0)
        if not r <= lim:
            out[k] = r / lim
    return out


def worst(step, bound=None):
    """(residual / (bound * scale + allowance), quantity) of the worst quantity of a step."""
    bound = BOUND if bound is None else bound
    k = max(step.res, key=lambda q: step.res[q] / (bound[q] * step.scale[q] + step.allow.get(q, 0.0)))
    return step.res[k] / (bound[k] * step.scale[k] + step.allow.get(k, 0.0)), k


def reversed_iv(iv):
    """The same pair sum with the sources in reversed order: a second, equally exact float64 evaluation."""
    def f(g, xs, zs, xp, zp, v_core):
        return iv(np.asarray(g)[::-1].copy(), np.asarray(xs)[::-1].copy(), np.asarray(zs)[::-1].copy(), xp, zp, v_core)
    return f


ATTRS = ("Uinf", "chord", "rho", "dt", "piv", "v_core", "LESPcrit", "method", "maxerror", "nt", "alpha", "alpha_dot", "h_dot", "airfoil")


def history_copy(sim):
    """The attributes the checker reads, every result array a writable copy."""
    h = types.SimpleNamespace(**{k: getattr(sim, k) for k in ATTRS})
    h.path = {k: np.array(v) for k, v in sim.path.items()}
    h.circulation = copy.deepcopy(sim.circulation)
    for k in ("fourier", "LESP", "LESP_prev", "LEV_shed", "Fn", "Fs", "L", "D", "M", "Cl", "Cd", "Cm"):
        setattr(h, k, np.array(getattr(sim, k)))
    return h


def plant_row(h, i, m):
    """Write the row `m` (model_step's dict) into the arrays of `h` as step i's result."""
    itev, ilev, _ = counts(h, i)
    C = h.circulation
    C["TEV"][itev], C["bound"][itev] = m["G_TEV"], m["bound"]
    if m["_sheds"]:
        C["LEV"][ilev] = m["G_LEV"]
    h.LESP_prev[itev], h.LESP[itev] = m["LESP_prev"], m["LESP"]
    h.fourier[i, 0, :], h.fourier[i, 1, :] = m["fourier"], m["fourier_dot"]
    C["gamma_airfoil"][itev], C["airfoil"][itev], C["Gamma_airfoil"][itev] = m["gamma_airfoil"], m["airfoil"], m["Gamma_airfoil"]
    for k in ("Fn", "Fs", "L", "D", "M", "Cl", "Cd", "Cm"):
        getattr(h, k)[i] = m[k]


# ---- the cases of the CPU tier ---------------------------------------------------------------------------------------
# every event the case table as a whole must go through (asserted on the oracle's runs)
EVENTS = {"first step", "first LEV", "consecutive LEV", "LEV after a gap", "shed A0 > 0", "shed A0 < 0", "no LEV after shedding"}
MIN_MARGIN = 1e-6           # the smallest decision margin of every small case: the decision is checked with no exemption


def small_cases():
    """name -> constructor keywords without `method`: config 1, two cambered off-unit G10 cases (chord, Uinf, rho != 1; one
    with free vortices and 126 panels) and a free-vortex cloud of the roll-up cases."""
    from conftest import CONFIG1
    from oracle import g10_cases
    import rollup_common
    out = {"config1": dict(CONFIG1)}
    for name in ("c4412d", "c2412f"):
        kw = g10_cases.kwargs(g10_cases.BY_NAME[name])
        kw.pop("method")
        out[name] = kw
    kw = g10_cases.kwargs(g10_cases.BY_NAME["d23"])
    kw.pop("method")
    out["d23"] = kw
    out["c150"] = rollup_common.case_keywords("c150")
    return out
