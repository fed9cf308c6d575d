"""Shared by tests/test_tracer_gradient_host.py and tests/test_gpu_tracer_gradient.py: the tracers' deformation gradient through
its definition in NumPy.  A released tracer goes start -> start + dt (u, w)_i(start) in step i, and the step's sources do not
depend on it, so  F_i = (I + dt G_i(start)) F_{i-1}  with G_i = [[u_x, u_z], [w_x, -u_x]] the closed forms of
tests/gradient_common.py over the step's sources; F is the identity while a tracer is held and at its release step.  Rows are
[4, M] in the order F11, F12, F21, F22."""
import numpy as np

import gradient_common as G


def identity(M):
    F = np.zeros([4, M])
    F[0], F[3] = 1.0, 1.0
    return F


def step_gradient(sources, x, z, v_core):
    """(u_x, u_z, w_x) at the points over (g_wake, x, z, g_foil, x, z) of tracers_common.run_sources, float64 from long double"""
    gw, xs, zs, gf, xf, zf = sources
    return G.reference(np.concatenate([gw, gf]), np.concatenate([xs, xf]), np.concatenate([zs, zf]), x, z, v_core)[0]


def step_F(F_prev, start, rel, i, dt, v_core, sources):
    """-> (F after step i [4, M], the increments dt G F [4, M]) from F after step i - 1, the step's start positions [2, M] (used
    for the released tracers only), the release steps and the step's sources"""
    F, inc = F_prev.copy(), np.zeros_like(F_prev)
    free = rel <= i
    if free.any():
        f11, f12, f21, f22 = (np.where(rel[free] == i, one, F_prev[k][free]) for k, one in enumerate((1.0, 0.0, 0.0, 1.0)))
        ux, uz, wx = step_gradient(sources, start[0][free], start[1][free], v_core)
        wz = -ux
        inc[0][free] = dt * (ux * f11 + uz * f21)
        inc[1][free] = dt * (ux * f12 + uz * f22)
        inc[2][free] = dt * (wx * f11 + wz * f21)
        inc[3][free] = dt * (wx * f12 + wz * f22)
        for k, f in enumerate((f11, f12, f21, f22)):
            F[k][free] = f + inc[k][free]
    return F, inc


def rows_against_the_recursion(sim, rel, steps, sources_of):
    """Every row `tracer_F_path[i]`, i in steps, against step_F from the run's OWN row i - 1 at the run's own start positions
    (the seed of step i at a release, else tracer_path[i - 1]) over sources_of(i).
    -> (worst |difference|, max |F|, the largest single increment max |dt G F|)"""
    worst, fmax, inc_max = 0.0, 0.0, 0.0
    for i in steps:
        seeds = sim._tracer_seeds(i)
        start = np.where(rel == i, seeds, sim.tracer_path[i - 1])
        want, inc = step_F(sim.tracer_F_path[i - 1], start, rel, i, sim.dt, sim.v_core, sources_of(i))
        got = sim.tracer_F_path[i]
        worst = max(worst, float(np.abs(got - want).max()))
        fmax = max(fmax, float(np.abs(got).max()))
        inc_max = max(inc_max, float(np.abs(inc).max()))
    return worst, fmax, inc_max
