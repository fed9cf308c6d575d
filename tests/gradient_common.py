"""Reference and bound of the velocity-gradient pair sum: the three closed forms in np.longdouble as plain numpy -- nothing from
the product (tests/test_gradient_host.py checks them against centred differences of the ORACLE's induced velocity).

For a target p and a source j: dx = xp - xj, dz = zp - zj, r2 = dx^2 + dz^2, s = sqrt(r2^2 + v_core^4), y = 1 / s,

    A = sum_j G_j r2 dx dz y^3,    B = sum_j G_j r2 (dx^2 - dz^2) y^3,    C = sum_j G_j y^3
    ux = du/dx = -A / pi,    uz = du/dz = (B + v_core^4 C) / (2 pi),    wx = dw/dx = (B - v_core^4 C) / (2 pi)

(dw/dz = -ux; wx - uz = -v_core^4 C / pi is the analytic vorticity of tests/scalar_field_common.py).

The bound is derived, not tuned: per target and per component c, with eps = 2^-52,

    |c - c_ref| <= (ns + K) eps sum_j |G_j| / (2 pi s_pj),    K = 16.

Every term of A, B or C, scaled as it enters an output, is at most |G| / (2 pi s) in magnitude (|dx dz| <= r2 / 2,
|dx^2 - dz^2| <= r2, r2^2 <= s^2, and r2 |dx^2 - dz^2| + v_core^4 <= s^2 for the two terms of uz and wx together).  The rounding
of dx^2 - dz^2 is absolute in r2, not in the difference, which is why the magnitude is the one with s and not the term's own.
ns eps is the worst case of any summation order.  K counts the roundings of one term: dx and dz cost half an ulp each and enter
a term with logarithmic sensitivity at most 3 (3 ulp); then r2, q = r2^2 + v_core^4, the refined reciprocal square root cubed
(3 times its own rounding, plus the two products), the products with G, r2 and dx dz (or dx^2 - dz^2), and the fused add into the
accumulator: 13 more at the most, 16 in all."""
import numpy as np

from scalar_field_common import (EPS, LD, PI, V_CORE, _pairs, grid_points, header_constant, targets,  # noqa: F401  (shared helpers)
                                 wake_strip)

K = 16
NAMES = ("ux", "uz", "wx")


def reference_ld(g, xs, zs, xt, zt, v_core):
    """((ux, uz, wx), magnitude) in np.longdouble, unrounded: magnitude = sum_j |G_j| / (2 pi s_pj) per target"""
    xt, zt = np.asarray(xt, float).reshape(-1), np.asarray(zt, float).reshape(-1)
    xs, zs = np.asarray(xs, LD).reshape(-1), np.asarray(zs, LD).reshape(-1)
    gg, r2, s, vc4 = _pairs(g, xs, zs, xt, zt, v_core)
    dx, dz = np.asarray(xt, LD)[:, None] - xs[None, :], np.asarray(zt, LD)[:, None] - zs[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = gg / s**3
        A = (c * r2 * dx * dz).sum(axis=1)
        B = (c * r2 * (dx * dx - dz * dz)).sum(axis=1)
        C = c.sum(axis=1)
        mag = (np.abs(gg) / (2 * PI * s)).sum(axis=1)
    return (-A / PI, (B + vc4 * C) / (2 * PI), (B - vc4 * C) / (2 * PI)), mag


def reference(g, xs, zs, xt, zt, v_core, rows=2048):
    """((ux, uz, wx), bound) per target, float64 arrays rounded from np.longdouble; one bound for the three components; `rows`
    targets at a time"""
    xt, zt = np.asarray(xt, float).reshape(-1), np.asarray(zt, float).reshape(-1)
    vals, bnd = np.zeros((3, len(xt))), np.zeros(len(xt))
    ns = len(np.asarray(g).reshape(-1))
    for lo in range(0, len(xt), rows):
        sl = slice(lo, lo + rows)
        comp, mag = reference_ld(g, xs, zs, xt[sl], zt[sl], v_core)
        for k in range(3):
            vals[k, sl] = comp[k]
        bnd[sl] = (ns + K) * EPS * mag
    return (vals[0], vals[1], vals[2]), bnd


_cache = {}


def cached_reference(key, inputs):
    """the reference of one table entry, computed once per session and handed out read-only"""
    k = tuple(key)
    if k not in _cache:
        vals, bnd = reference(*inputs)
        for a in vals + (bnd,):
            a.setflags(write=False)
        _cache[k] = (vals, bnd)
    return _cache[k]
