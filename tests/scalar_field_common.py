"""Reference and bounds of the scalar pair sums (stream function, analytic vorticity): the two closed forms in np.longdouble
as plain numpy -- nothing from the product, nothing from the oracle (the reference code has neither sum).

For a target p and a source j: dx = xp - xj, dz = zp - zj, r2 = dx^2 + dz^2, s = sqrt(r2^2 + v_core^4), a = (r2 + s) / 2,

    psi(p)   = sum_j G_j / (4 pi) ln(a_pj)
    omega(p) = -sum_j G_j v_core^4 / (pi s_pj^3)

The bounds are derived, not tuned.  For every target, with eps = 2^-52:

    |psi - psi_ref|     <= (ns + 8) eps sum_j |G_j| / (4 pi) (1 + |ln a_pj|)
    |omega - omega_ref| <= (ns + 8) eps sum_j |G_j| v_core^4 / (pi s_pj^3)

ns eps is the worst case of any summation order; 8 ulp per term cover the square root, the logarithm and the products; the
`1 +` is there because a rounding of `a` is an ABSOLUTE error of ln a and does not vanish where ln a is near 0."""
import os
import re

import numpy as np

from conftest import ROOT

LD = np.longdouble
EPS = 2.0**-52
PI = LD("3.14159265358979323846264338327950288")
KINDS = ("psi", "omega")
V_CORE = 0.0195           # 1.3 dt of the README case


def header_constant(name):
    """an integer constant of csrc/plan_rule.hpp (the tiles the float64 launches walk their sources in)"""
    text = open(os.path.join(ROOT, "ludvm_amd", "csrc", "plan_rule.hpp")).read()
    return int(re.search(r"constexpr\s+(?:int|long long)\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


def _pairs(g, xs, zs, xt, zt, v_core):
    g, xs, zs = (np.asarray(a, LD).reshape(-1) for a in (g, xs, zs))
    xt, zt = (np.asarray(a, LD).reshape(-1) for a in (xt, zt))
    dx, dz = xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]
    r2 = dx * dx + dz * dz
    vc4 = LD(v_core) ** 4
    s = np.sqrt(r2 * r2 + vc4)
    return g[None, :], r2, s, vc4


def reference(kind, g, xs, zs, xt, zt, v_core, rows=2048):
    """(value, bound) per target, float64 arrays rounded from np.longdouble; `rows` targets at a time"""
    xt, zt = np.asarray(xt, float).reshape(-1), np.asarray(zt, float).reshape(-1)
    val, bnd = np.zeros(len(xt)), np.zeros(len(xt))
    ns = len(np.asarray(g).reshape(-1))
    for lo in range(0, len(xt), rows):
        sl = slice(lo, lo + rows)
        gg, r2, s, vc4 = _pairs(g, xs, zs, xt[sl], zt[sl], v_core)
        with np.errstate(divide="ignore", invalid="ignore"):
            if kind == "psi":
                ln = np.log((r2 + s) / 2)
                term, mag = gg / (4 * PI) * ln, np.abs(gg) / (4 * PI) * (1 + np.abs(ln))
            else:
                term = -gg * vc4 / (PI * s**3)
                mag = np.abs(term)
        val[sl] = term.sum(axis=1)
        bnd[sl] = (ns + 8) * EPS * mag.sum(axis=1)
    return val, bnd


def wake_strip(ns, seed=0):
    """a wake-like strip: x in [-60, 0], z ~ N(0, 0.5), G ~ N(0, 0.02)"""
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(0.0, 0.02, ns), rng.uniform(-60.0, 0.0, ns), rng.normal(0.0, 0.5, ns)


def targets(nt, seed=0):
    """points of [-61, 1] x [-3, 3]"""
    rng = np.random.default_rng(2000 + seed)
    return rng.uniform(-61.0, 1.0, nt), rng.uniform(-3.0, 3.0, nt)


def grid_points(xmin, zmin, dr, nx, nz, row_first=0, row_count=None):
    """the mesh the library generates: (xmin + i dr, zmin + j dr), x-major -- each coordinate with ONE rounding, as grid_point's
    fused multiply-add forms it (exact rational arithmetic, rounded once; on a dyadic mesh the unfused sum is the same)"""
    from fractions import Fraction
    rows = range(row_first, nx if row_count is None else row_first + row_count)
    xr = np.array([float(Fraction(xmin) + i * Fraction(dr)) for i in rows])
    zr = np.array([float(Fraction(zmin) + j * Fraction(dr)) for j in range(nz)])
    X, Z = np.meshgrid(xr, zr, indexing="ij")
    return X.reshape(-1), Z.reshape(-1)


_cache = {}


def cached_reference(key, kind, inputs):
    """the reference of one table entry, computed once per session and handed out read-only"""
    k = (kind,) + tuple(key)
    if k not in _cache:
        val, bnd = reference(kind, *inputs)
        val.setflags(write=False)
        bnd.setflags(write=False)
        _cache[k] = (val, bnd)
    return _cache[k]
