"""Shared by tests/test_gradient_f32x2_host.py and tests/test_gpu_gradient_f32x2.py: a NumPy restatement of the hi+lo fp32 scheme
of the analytic vorticity and the velocity gradient (field_hilo_f32, ludvm_amd/csrc/field_kernels.hpp),
the bound, and the cases the two tiers use.

The scheme: every float64 coordinate v is split into hi = float32(v) and lo = float32(v - hi); a difference is
(hi_p - hi_s) + (lo_p - lo_s) in float32 and the pair is float32 from there: with r2 = dx^2 + dz^2 and y = 1 / sqrt(r2^2 + vc^4),

    C += (G y) (y y),    e = (G y) (y r2),    A += e (y (dx dz)),    B += e (y (dx^2 - dz^2))

with G and vc^4 rounded to float32.  The sources of a split go in tiles of 256 from the split's first one; within a tile the
even sources are summed, one after the other, in one float32 accumulator and the odd ones in another; at the end of a tile the
even sum, then the odd sum, is added to the target's float64 total; the splits' totals are added in the finishers' fixed order
and the outputs formed in float64 as the float64 route forms them.

The references are gradient_common.reference_ld and scalar_field_common.reference (np.longdouble).  The bound is derived, not
tuned: per target and per component c, with eps32 = 2^-23,

    |c - c_ref| <= (H + K32) eps32 mag + (ns + 16) 2^-52 mag

    mag = sum_j |G_j| / (2 pi s_pj)              for ux, uz, wx  (gradient_common's magnitude: every term of A, B or C, scaled
                                                  as it enters an output, is at most that)
    mag = sum_j |G_j| v_core^4 / (pi s_pj^3)     for omega       (scalar_field_common's)

H = 128: the terms ONE float32 accumulator adds per tile (a tile of 256 sources on two chains, as the kernel has them); each
addition rounds a partial sum that is at most the tile's share of mag.  The second term is the float64 part: the tile sums and
splits in any order, and the roundings of the float64 epilogue.
K32 = 24 counts the float32 roundings of one term.  gradient_common counts 16 for the float64 pair: dx and dz half an ulp each
at logarithmic sensitivity at most 3 (3), r2 and q (2), the reciprocal square root cubed (3 times its own rounding plus two
products: 5), the products with G, r2 and dx dz or dx^2 - dz^2 and the fused add (5), and one to spare.  Four changes:
  * a coordinate difference is two roundings here -- the hi and the lo differences are exact or rounded once each, their sum is
    rounded -- instead of one: twice the 3 ulp, +3
  * v_rsq_f32 is accurate to 1 ulp and is not refined, and y enters every term to the third power (C: G y, y y; A and B: G y,
    y r2, y dx dz): +3
  * G and v_core^4 are rounded to float32: half an ulp of G, and half an ulp of vc^4 in q at sensitivity 3 / 2 through s^3:
    +1.25
  * 16 + 3 + 3 + 1.25 = 23.25, rounded up: 24.
The products are as many as in the float64 pair -- there y y, y^2 y, G y^3, (G y^3) r2, dx dz and the fused add; here G y, y r2,
their product, dx dz, y (dx dz) and the fused add -- so the regrouping changes no count.

The restatement takes 1 / sqrt correctly rounded where the kernel has v_rsq_f32 (1 ulp): it shows that the bound can be met
and what the scheme's own error is (tests/test_gradient_f32x2_host.py), not the kernel's bits."""
import os
import sys

import numpy as np

import gradient_common as G
import scalar_field_common as S
from conftest import ROOT

F32 = np.float32
EPS32 = 2.0**-23
EPS64 = 2.0**-52
H = 128                         # terms per float32 accumulator and tile (kFieldHiloTile / 2)
K32 = 24
TILE = S.header_constant("kFieldHiloTile")
PER_LANE = S.header_constant("kFieldHiloPerLane")
WORKGROUP = S.header_constant("kPlanBlock") * PER_LANE          # targets of one workgroup
V_CORE = S.V_CORE
V_CORE_SMALL = 1.3e-3
assert TILE == 2 * H


def plan(plan_nt, ns):
    """(chunk, nsplit) of the library's rule, asked of its header (tools/plan_rule.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import plan_rule
    finally:
        sys.path.pop(0)
    p = plan_rule.field_hilo_plan(plan_nt, ns)
    assert p.tile == TILE and p.targets == WORKGROUP and p.chunk % TILE == 0
    return p.chunk, p.nsplit


def split_hilo(v):
    v = np.asarray(v, dtype=np.float64)
    hi = v.astype(F32)
    return hi, (v - hi.astype(np.float64)).astype(F32)


def _fma32(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 is exact in float64; the float64 sum rounds once more
    before the float32 rounding, which differs from the fused result only on a tie of the second rounding)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _sum_column(parts):
    """the finishers' association of the splits' float64 totals (sum_column, pair_kernels.hpp): four running sums over splits
    s mod 4, the rest of a ragged group of four on the first, then (a0 + a1) + (a2 + a3)"""
    a = [np.zeros_like(parts[0]) for _ in range(4)]
    full = len(parts) // 4 * 4
    for s in range(full):
        a[s % 4] = a[s % 4] + parts[s]
    for s in range(full, len(parts)):
        a[0] = a[0] + parts[s]
    return (a[0] + a[1]) + (a[2] + a[3])


def hilo_f32_sums(g, xs, zs, px, pz, v_core, chunk=None):
    """-> float64 (A, B, C) per point by the scheme above; chunk: sources per split (a multiple of TILE; None: one split)"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    ns = len(g)
    (xsh, xsl), (zsh, zsl), (xph, xpl), (zph, zpl) = (split_hilo(np.asarray(a, float).reshape(-1)) for a in (xs, zs, px, pz))
    gf = g.astype(F32)
    vc4 = np.full(1, float(v_core) ** 4).astype(F32)
    chunk = max(ns, 1) if chunk is None else int(chunk)
    assert chunk == max(ns, 1) or chunk % TILE == 0
    parts = []
    for s_begin in range(0, max(ns, 1), chunk):
        s_end = min(s_begin + chunk, ns)
        tot = [np.zeros(len(xph)) for _ in range(3)]
        for base in range(s_begin, s_end, TILE):
            tile = [[None, None] for _ in range(3)]
            for par in (0, 1):
                idx = np.arange(base + par, min(base + TILE, s_end), 2)
                if len(idx) == 0:
                    tile[0][par] = tile[1][par] = tile[2][par] = np.zeros(len(xph), F32)
                    continue
                dx = ((xph[:, None] - xsh[idx][None]) + (xpl[:, None] - xsl[idx][None])).astype(F32)
                dz = ((zph[:, None] - zsh[idx][None]) + (zpl[:, None] - zsl[idx][None])).astype(F32)
                dxx = dx * dx
                r2 = _fma32(dz, dz, dxx)
                q = _fma32(r2, r2, vc4)
                with np.errstate(over="ignore", divide="ignore"):
                    y = (1.0 / np.sqrt(q.astype(np.float64))).astype(F32)
                gy = gf[idx][None] * y
                e = gy * (y * r2)
                # (an accumulator takes a term by a fused multiply-add: the term's last product and the sum round once together)
                for k, (m1, m2) in enumerate(((e, y * (dx * dz)), (e, y * _fma32(-dz, dz, dxx)), (gy, y * y))):
                    acc = np.zeros(len(xph), dtype=F32)
                    for j in range(m1.shape[1]):
                        acc = _fma32(m1[:, j], m2[:, j], acc)
                    tile[k][par] = acc
            for k in range(3):
                tot[k] = tot[k] + tile[k][0].astype(np.float64)
                tot[k] = tot[k] + tile[k][1].astype(np.float64)
        parts.append(tot)
    return tuple(_sum_column([p[k] for p in parts]) for k in range(3))


def hilo_f32_gradient(g, xs, zs, px, pz, v_core, chunk=None):
    """-> (ux, uz, wx) float64 by the scheme (grad_outputs' float64 epilogue)"""
    A, B, C = hilo_f32_sums(g, xs, zs, px, pz, v_core, chunk)
    vC = float(v_core) ** 4 * C
    return -A / np.pi, (B + vC) / (2 * np.pi), (B - vC) / (2 * np.pi)


def hilo_f32_omega(g, xs, zs, px, pz, v_core, chunk=None):
    """-> omega float64 by the scheme (the scaled split totals are what the kernel hands the finisher; one split here scales the
    sum, which differs from scaling each split by float64 roundings the bound's second term covers)"""
    C = hilo_f32_sums(g, xs, zs, px, pz, v_core, chunk)[2]
    return C * (-(float(v_core) ** 4) / np.pi)


def bound(ns, mag):
    mag = np.asarray(mag, dtype=np.float64)
    return (H + K32) * EPS32 * mag + (ns + 16) * EPS64 * mag


def gradient_reference(g, xs, zs, xt, zt, v_core):
    """((ux, uz, wx), bound): float64 arrays from gradient_common's np.longdouble closed forms"""
    vals, b64 = G.reference(g, xs, zs, xt, zt, v_core)
    ns = len(np.asarray(g).reshape(-1))
    return vals, bound(ns, b64 / ((ns + G.K) * G.EPS))


def omega_reference(g, xs, zs, xt, zt, v_core):
    """(omega, bound): float64 arrays from scalar_field_common's np.longdouble closed form"""
    val, b64 = S.reference("omega", g, xs, zs, xt, zt, v_core)
    ns = len(np.asarray(g).reshape(-1))
    return val, bound(ns, b64 / ((ns + 8) * S.EPS))


_cache = {}


def cached(kind, key, inputs):
    """the reference of one case, computed once per session and handed out read-only; kind: 'grad' | 'omega'"""
    k = (kind,) + tuple(key)
    if k not in _cache:
        vals, bnd = (gradient_reference if kind == "grad" else omega_reference)(*inputs)
        for a in (vals if kind == "grad" else (vals,)) + (bnd,):
            a.setflags(write=False)
        _cache[k] = (vals, bnd)
    return _cache[k]


def case(ns, nt, v_core=V_CORE, shift=0.0, on_top=None, near=None):
    """(g, xs, zs, xt, zt, v_core): scalar_field_common's wake strip and targets, with the first `on_top` targets on top of
    sources and the next `near` ones 0.3 v_core away from one (as many as fit; default: a sixteenth of the targets each),
    everything moved by `shift` in x"""
    g, xs, zs = S.wake_strip(ns)
    xt, zt = S.targets(nt)
    xt, zt = xt.copy(), zt.copy()
    if ns > 0:
        on_top = nt // 16 if on_top is None else on_top
        near = nt // 16 if near is None else near
        rng = np.random.default_rng(3000 + ns + nt)
        pick = rng.integers(0, ns, on_top + near)
        xt[:on_top], zt[:on_top] = xs[pick[:on_top]], zs[pick[:on_top]]
        ang = rng.uniform(0, 2 * np.pi, near)
        xt[on_top:on_top + near] = xs[pick[on_top:]] + 0.3 * v_core * np.cos(ang)
        zt[on_top:on_top + near] = zs[pick[on_top:]] + 0.3 * v_core * np.sin(ang)
    return g, xs + shift, zs, xt + shift, zt, v_core


def wide_case(ns, nt, v_core=V_CORE):
    """sources spread over |x| <= 1e4 (z ~ N(0, 0.5)) and targets among them, a sixteenth on top of sources: the far pairs have
    r2 ~ 1e8 against near ones at r2 ~ v_core^2 -- the scaling the products' order is there for"""
    rng = np.random.default_rng(4000 + ns + nt)
    g, xs, zs = rng.normal(0.0, 0.02, ns), rng.uniform(-1.0e4, 1.0e4, ns), rng.normal(0.0, 0.5, ns)
    xt, zt = rng.uniform(-1.0e4, 1.0e4, nt), rng.uniform(-3.0, 3.0, nt)
    k = nt // 16
    pick = rng.integers(0, ns, 2 * k)
    xt[:k], zt[:k] = xs[pick[:k]], zs[pick[:k]]
    xt[k:2 * k], zt[k:2 * k] = xs[pick[k:]] + 0.3 * v_core, zs[pick[k:]]
    return g, xs, zs, xt, zt, v_core


def host_cases():
    """the CPU tier's cases -> {name: inputs}: wake_strip(3000) with 512 targets, 32 of them on top of sources and 32 at
    0.3 v_core from one; the small core; everything at x - 5000; and ns = 255 (one ragged tile)"""
    return {
        "strip": case(3000, 512, V_CORE),
        "small_core": case(3000, 512, V_CORE_SMALL),
        "at_-5000": case(3000, 512, V_CORE, shift=-5000.0),
        "ns255": case(255, 512, V_CORE),
    }
