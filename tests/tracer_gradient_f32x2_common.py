"""Shared by tests/test_tracer_gradient_f32x2_host.py and tests/test_gpu_tracer_gradient_f32x2.py: a NumPy restatement of the
fused hi+lo fp32 walk of the tracers' deformation gradient (hilo_field_grad_f32 / march_f32x2_grad_tracer_partial,
ludvm_amd/csrc/march_kernels.hpp) and the derived tolerance of a row of F.

The walk: dx, dz, r2 = dx^2 + dz^2, y = 1 / sqrt(r2^2 + vc^4) and G y are formed ONCE per pair, as the plain hi+lo fp32 tracers
form them (tests/tracers_f32x2_common.py); u += dz (G y), w += dx (G y) as there, and from the same five values the gradient's
terms in the order of tests/gradient_f32x2_common.py: C += (G y)(y y), e = (G y)(y r2), A += e (y (dx dz)),
B += e (y (dx^2 - dz^2)).  Tiles of 256 sources, even and odd sources apart in float32, then even, odd into float64.

The two restatements this one is held against model the float32 roundings of the shared values differently --
tracers_f32x2_common rounds every product and sum (and takes sqrt, then the reciprocal, in float32), gradient_f32x2_common fuses
the multiply-adds as the kernel does (and rounds the float64 reciprocal square root once) -- so `rounding` picks the model:
'plain' or 'fused'.  Under either, the five sums come from one set of shared values; the fusion adds no operation to either
scheme and takes none away.

The tolerance of a row (derived, not tuned): gradient_f32x2_common.bound(ns, mag) bounds each component of the hi+lo gradient at
one target against the np.longdouble reference, (128 + 24) 2^-23 mag + (ns + 16) 2^-52 mag -- the per-pair products and the
two-level sums are that kernel's.  F_i = F_{i-1} + dt G F_{i-1}, so component by component

    tol(F11) = tol(F21) = dt b (|F11| + |F21|)_{i-1},    tol(F12) = tol(F22) = dt b (|F12| + |F22|)_{i-1}

(b bounds u_x, u_z, w_x and w_z = -u_x alike), plus 1e-9 of max|F| for the float64 roundings in another order."""
import numpy as np

import gradient_f32x2_common as GF
import tracer_gradient_common as TG

F32 = np.float32
TILE = 256
ROUNDING = 1e-9                 # of max|F|: float64 sums and products in another order (tests/test_gpu_tracer_gradient.py)


def fused_hilo_f32(g, xs, zs, px, pz, v_core, rounding="fused"):
    """-> (u, w, A, B, C) float64 per point: one pass over the sources (one split) by the fused walk"""
    assert rounding in ("fused", "plain")
    fused = rounding == "fused"
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    (xsh, xsl), (zsh, zsl), (xph, xpl), (zph, zpl) = (GF.split_hilo(np.asarray(a, float).reshape(-1)) for a in (xs, zs, px, pz))
    gf, vc4 = g.astype(F32), np.full(1, float(v_core) ** 4).astype(F32)
    fma = GF._fma32 if fused else (lambda a, b, c: ((a * b).astype(F32) + c).astype(F32))
    tot = [np.zeros(len(xph)) for _ in range(5)]
    for base in range(0, len(g), TILE):
        halves = []
        for par in (0, 1):
            idx = np.arange(base + par, min(base + TILE, len(g)), 2)
            if len(idx) == 0:
                halves.append([np.zeros(len(xph), F32)] * 5)
                continue
            # the shared values of a pair
            dx = ((xph[:, None] - xsh[idx][None]) + (xpl[:, None] - xsl[idx][None])).astype(F32)
            dz = ((zph[:, None] - zsh[idx][None]) + (zpl[:, None] - zsl[idx][None])).astype(F32)
            dxx = dx * dx
            r2 = fma(dz, dz, dxx)
            q = fma(r2, r2, vc4)
            with np.errstate(over="ignore", divide="ignore"):
                y = (1.0 / np.sqrt(q.astype(np.float64))).astype(F32) if fused else F32(1.0) / np.sqrt(q)
            gy = y * gf[idx][None]
            # the velocity's terms, then the gradient's
            e = gy * (y * r2)
            pairs = ((dz, gy), (dx, gy), (e, y * (dx * dz)), (e, y * fma(-dz, dz, dxx)), (gy, y * y))
            accs = []
            for m1, m2 in pairs:
                acc = np.zeros(len(xph), dtype=F32)
                for j in range(m1.shape[1]):
                    acc = fma(m1[:, j], m2[:, j], acc)
                accs.append(acc)
            halves.append(accs)
        for k in range(5):
            tot[k] = tot[k] + halves[0][k].astype(np.float64)
            tot[k] = tot[k] + halves[1][k].astype(np.float64)
    u, w, A, B, C = tot
    return u / (2 * np.pi), -w / (2 * np.pi), A, B, C


def _cat(sources):
    gw, xs, zs, gf, xf, zf = sources
    return np.concatenate([gw, gf]), np.concatenate([xs, xf]), np.concatenate([zs, zf])


def restated_step(F_prev, seeds_i, cur, rel, i, dt, v_core, sources):
    """One step of the route in NumPy: -> (positions [2, M], F [4, M]) after step i from the fused walk over the step's sources
    (wake, then bound vortices, in stored order) and the finisher's float64 update; held tracers keep seed and F"""
    g, xs, zs = _cat(sources)
    pos, F = seeds_i.copy(), F_prev.copy()
    free = rel <= i
    if free.any():
        first = (rel == i)[free]
        px = np.where(first, seeds_i[0][free], seeds_i[0][free] if cur is None else cur[0][free])
        pz = np.where(first, seeds_i[1][free], seeds_i[1][free] if cur is None else cur[1][free])
        u, w, A, B, C = fused_hilo_f32(g, xs, zs, px, pz, v_core)
        pos[0][free], pos[1][free] = px + dt * u, pz + dt * w
        vC = float(v_core) ** 4 * C
        ux, uz, wx = -A / np.pi, (B + vC) / (2 * np.pi), (B - vC) / (2 * np.pi)
        f11, f12, f21, f22 = (np.where(first, one, F_prev[k][free]) for k, one in enumerate((1.0, 0.0, 0.0, 1.0)))
        F[0][free] = f11 + dt * (ux * f11 + uz * f21)
        F[1][free] = f12 + dt * (ux * f12 + uz * f22)
        F[2][free] = f21 + dt * (wx * f11 - ux * f21)
        F[3][free] = f22 + dt * (wx * f12 - ux * f22)
    return pos, F


def step_tolerance(F_prev, start, rel, i, dt, v_core, sources):
    """-> (tol [4, M], b [M]): the tolerance above of row i (0 for a tracer still held: its F is untouched, exactly) and the bound of
    one gradient component at each start position (0 where held), from the np.longdouble reference's magnitude"""
    M = F_prev.shape[1]
    tol, b = np.zeros([4, M]), np.zeros(M)
    free = rel <= i
    if free.any():
        b[free] = GF.gradient_reference(*_cat(sources), start[0][free], start[1][free], v_core)[1]
        f = [np.where(rel == i, one, np.abs(F_prev[k])) for k, one in enumerate((1.0, 0.0, 0.0, 1.0))]
        col1, col2 = dt * b * (f[0] + f[2]), dt * b * (f[1] + f[3])
        for k, c in enumerate((col1, col2, col1, col2)):
            tol[k][free] = c[free]
    return tol, b


def rows_within_tolerance(sim, rel, steps, sources_of):
    """Every row `tracer_F_path[i]`, i in steps, against tracer_gradient_common.step_F from the run's OWN row i - 1 at the run's own
    start positions over sources_of(i), component by component within step_tolerance + ROUNDING max|F|.
    -> dict(ratio: worst |difference| / tolerance, of_F: worst |difference| / max|F|, tol: the largest tolerance, fmax: max|F|,
    inc: the largest single increment max|dt G F|, bad: (step, component, tracer) of the first row outside, or None)"""
    out = dict(ratio=0.0, of_F=0.0, tol=0.0, fmax=0.0, inc=0.0, bad=None)
    worst = 0.0
    for i in steps:
        seeds = sim._tracer_seeds(i)
        start = np.where(rel == i, seeds, sim.tracer_path[i - 1])
        F_prev, src = sim.tracer_F_path[i - 1], sources_of(i)
        want, inc = TG.step_F(F_prev, start, rel, i, sim.dt, sim.v_core, src)
        tol, _ = step_tolerance(F_prev, start, rel, i, sim.dt, sim.v_core, src)
        got = sim.tracer_F_path[i]
        free = rel <= i
        assert np.array_equal(got[:, ~free], F_prev[:, ~free]), ("a held tracer's F changed", i)
        if not free.any():
            continue
        fmax = float(np.abs(got).max())
        full = tol[:, free] + ROUNDING * fmax
        diff = np.abs(got - want)[:, free]
        if out["bad"] is None and (diff > full).any():
            k, m = np.argwhere(diff > full)[0]
            out["bad"] = (i, int(k), int(np.flatnonzero(free)[m]))
        out["ratio"] = max(out["ratio"], float((diff / full).max()))
        worst = max(worst, float(diff.max()))
        out["tol"] = max(out["tol"], float(full.max()))
        out["fmax"] = max(out["fmax"], fmax)
        out["inc"] = max(out["inc"], float(np.abs(inc).max()))
    out["of_F"] = worst / out["fmax"] if out["fmax"] else 0.0
    return out


def assert_rows(sim, rel, steps, sources_of, what):
    """rows_within_tolerance, printed, then asserted: every row inside; the checked steps deform (the largest single increment
    exceeds 1e-6) and the tolerance is below 1e-2 of it, so that a wake taken one step late cannot pass"""
    r = rows_within_tolerance(sim, rel, steps, sources_of)
    print(f"{what}: F rows vs (I + dt G_ref) F_prev over the run's own sources: worst {r['ratio']:.3f} of the tolerance, "
          f"{r['of_F']:.2e} of max|F| ({r['fmax']:.3f}); largest tolerance {r['tol']:.2e} = {r['tol'] / r['inc']:.2e} of the largest "
          f"single increment ({r['inc']:.3e})")
    assert r["inc"] > 1e-6
    assert r["tol"] < 1e-2 * r["inc"], r["tol"] / r["inc"]
    assert r["bad"] is None and r["ratio"] <= 1.0, (r["bad"], r["ratio"])
    return r
