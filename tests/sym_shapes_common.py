"""The symmetric pair kernels at small tile rings: the case table, its inputs and its float64 reference (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_sym_shapes_host.py (CPU: the partition the launch rule states -- enumerated from ludvm_amd/csrc/sym_rule.hpp by
tools/sym_rule.py's `cover` program --, what the table reaches, what the reference would notice) and tests/test_gpu_sym_shapes.py
(GPU: every case by value at ALL targets).

pair_sym_f32<T, HILO, R> and pair_sym_quad_f32<8> serve launches from 11 264 vortices up, where a ring has >= 33 tiles and every
work item one round.  Here the rings have 1 .. 17 tiles (quad: 16 .. 25) and the variants are FORCED: tile and waves per item by
set_sym_tuning, d-chunks by set_tuning(0, s), the mixed form, the quad variant and the XCD placement by the measurement build.
A ring of NT tiles of W = 64 T vortices whose last tile holds `last` members has (NT - 1) W + last vortices; the symmetric kernel
needs two (set_symmetric(2)), so the one-member last tile of a ONE-tile ring is taken as two members.

Inputs: clouds of direct_shapes_common (plain positions, v_core 0.065) and the sheet of tests/test_gpu_rollup_edges.py (|x| ~ 50,
neighbours 1e-3 apart, v_core 1.3e-3: local origins and hi+lo positions), both with strengths of |Gamma| in [0.5, 1.5) of their
scale and a random sign.  Reference: observer_sources_common.fast_iv(), float64 all pairs at all targets, once per input."""
import collections
import functools
import os
import sys

import numpy as np

import direct_shapes_common as D
from oracle import g8_cases as G8

ROOT = D.ROOT
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import sym_rule  # noqa: E402

VC, VC_SHEET, DT = D.VC, 1.3e-3, 1e-3
TILES = (1, 2, 3, 4, 5, 6, 9, 10, 16, 17)
TS = (4, 8)
RS = (1, 2, 4)
SPLITS = (0, 1, 2, 3)
N_FOIL = (0, 80)
QUAD_TILES = (16, 17, 18, 19, 20, 21, 24, 25)
QUAD_SPLITS = (0, 1, 2, 3, 5)              # 0: the tapered table; the others: uniform chunks
OWNER_WORLDS = (2, 3, 5, 7)                # (7: an owner without a tile on the quad rings too)
OWNER_TILES = {"plain": (4, 9, 17), "quad": (17, 20, 25)}
MIXED, QUAD = -1, -4                       # set_sym_tuning's codes of the measurement build
TAIL_ITEMS = 17                            # LUDVM_SYM_TAIL_ITEMS of the 'mixed' engines: ytail = ceil(17 / tiles), inside (0, ysplit)
# engines of the measurement build (libludvm_hip_exp.so): the environment their constructor reads
EXP = {
    "exp": {},
    "mixed": {"LUDVM_SYM_TAIL_ITEMS": str(TAIL_ITEMS)},
    "xcd1": {"LUDVM_XCD_RUN": "1"},
    "xcd3": {"LUDVM_XCD_RUN": "3"},
}
XCD_RUN = {"xcd1": 1, "xcd3": 3}

# family: what the GPU tier groups by; form: plain | local | hilo; build: 'product' or a key of EXP; code: waves per item (1, 2, 4),
# MIXED or QUAD; split: set_tuning(0, split)
Case = collections.namedtuple("Case", "family form build n T code split")


def lasts(T):
    W = 64 * T
    return (1, 63, 64, 65, W - 1, W)


def size(tiles, T, last):
    return max((tiles - 1) * 64 * T + last, 2)


def ring_sizes(T, tiles=TILES, last=None):
    return [size(nt, T, l) for nt in tiles for l in (last or lasts(T))]


@functools.lru_cache(maxsize=None)
def mixed_big_rings():
    """[(rbulk, tiles, split)]: the smallest rings at which code -1 works its bulk by 2 waves and by 1 wave per item (below, by 4),
    asked of the rule; split 1024 (one ring offset per chunk) is where they are smallest"""
    return [(rb, sym_rule.smallest_mixed_ring(rb, 1024), 1024) for rb in (2, 1)]


@functools.lru_cache(maxsize=None)
def table():
    rows = []
    for T in TS:
        for n in ring_sizes(T):
            for R in RS:
                for s in SPLITS:
                    rows.append(Case("plain", "plain", "product", n, T, R, s))
                    rows.append(Case("local", "local", "product", n, T, R, s))
                    if T == 4:
                        rows.append(Case("hilo", "hilo", "product", n, T, R, s))
    # the mixed form: a bulk of rbulk-wave items and a tail of four-wave items
    for T in TS:
        for n in ring_sizes(T, last=(1, 64 * T)):
            for s in SPLITS:
                rows.append(Case("mixed", "plain", "mixed", n, T, MIXED, s))
                rows.append(Case("mixed", "local", "mixed", n, T, MIXED, s))
    for _, tiles, s in mixed_big_rings():
        for form in ("plain", "local"):
            rows.append(Case("mixed_big", form, "mixed", size(tiles, 4, 65), 4, MIXED, s))
    for n in ring_sizes(8, QUAD_TILES, (1, 512)):
        for s in QUAD_SPLITS:
            rows.append(Case("quad", "plain", "exp", n, 8, QUAD, s))
            rows.append(Case("quad", "local", "exp", n, 8, QUAD, s))
    # the XCD placement: the same items in another order of the workgroups -- the same bits
    for build in ("xcd1", "xcd3"):
        for T in TS:
            for n in ring_sizes(T, last=(65,)):
                for R in RS + (MIXED,):
                    for s in (0, 3):
                        rows.append(Case("xcd", "plain", build, n, T, R, s))
        for n in ring_sizes(8, QUAD_TILES, (65,)):
            for s in (0, 3):
                rows.append(Case("xcd", "plain", build, n, 8, QUAD, s))
    return tuple(rows)


def owner_cases():
    """[(kind, n, world, split)]: sym_accumulate_dev over the blocks shard_block gives (512-vortex tile; quad: code -4)"""
    out = []
    for kind, tiles in OWNER_TILES.items():
        for nt in tiles:
            for last in (1, 65):
                for world in OWNER_WORLDS:
                    for s in (0, 3):
                        out.append((kind, size(nt, 8, last), world, s))
    return out


def geometry(c):
    """tools/sym_rule.py's Cover of a case: the launch's geometry and every XCD's items, from the header"""
    hilo = c.form == "hilo"
    code = c.code
    if hilo and code == 0:
        code = -2
    tail = TAIL_ITEMS if c.build == "mixed" else None
    return sym_rule.cover(c.n, 4 if hilo else c.T, c.split, code, tail, XCD_RUN.get(c.build, 0), 0, -1, c.code == QUAD)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(n):
    """(g, x, z, v_core): a cloud in direct_shapes_common's box, float32-representable"""
    x, z, g = D.cloud(9700 + n % 89, 0, n)
    return g, x, z, VC


@functools.lru_cache(maxsize=None)
def sheet(n):
    """(g, x, z, v_core): tests/test_gpu_rollup_edges.py's sheet -- n vortices in shedding order, index k at x = -50 - 1e-3 (n - 1 - k)
    -- with strengths +-[0.5, 1.5) 1e-3"""
    x = -50.0 - 1e-3 * (n - 1 - np.arange(n, dtype=float))
    z = 0.3 * np.sin(0.7 * x) + 1e-3 * (2.0 * G8.uniform24(9800 + n % 89, 7, n) - 1.0)
    return np.asarray(D.strengths(9800 + n % 89, 0, n, 1e-3), np.float64), x, z, VC_SHEET


@functools.lru_cache(maxsize=None)
def foil(nfoil):
    """bound vortices on x in [-50 + 1e-3, -49], strengths a hundredth of the wake's (tests/test_gpu_rollup_edges.py)"""
    x = np.linspace(-50.0 + 1e-3, -49.0, nfoil)
    return x, 0.3 * np.sin(0.7 * x), np.asarray(D.strengths(9900, 0, nfoil, 1e-5), np.float64) if nfoil else np.zeros(0)


def inputs(form, n):
    return cloud(n) if form == "plain" else sheet(n)


# ---- the reference -------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(iv, key, g, x, z, vc, nfoil=0):
    """(u, w) float64 of all pairs at all targets (plus the bound vortices'), once per key; read-only"""
    if key not in _REF:
        u, w = iv(np.asarray(g, np.float64), np.asarray(x, np.float64), np.asarray(z, np.float64), np.asarray(x, np.float64),
                  np.asarray(z, np.float64), vc)
        if nfoil:
            fx, fz, fg = foil(nfoil)
            uf, wf = iv(fg, fx, fz, np.asarray(x, np.float64), np.asarray(z, np.float64), vc)
            u, w = u + uf, w + wf
        u.setflags(write=False)
        w.setflags(write=False)
        _REF[key] = (u, w)
    return _REF[key]


def rel_err(u, w, ur, wr):
    return D.rel_err(u, w, ur, wr)


# ---- what a wrong partition would do to the sums (the sensitivity checks) --------------------------------------------------------
def tile_slice(I, W, n):
    return slice(I * W, min((I + 1) * W, n))


def pair_delta(g, x, z, vc, ti, sj, n):
    """(du, dw)[n]: what the sources sj (indices) induce at the targets ti (indices), zero elsewhere"""
    du, dw = np.zeros(n), np.zeros(n)
    u, w = D.contribution(np.asarray(g, float)[sj], np.asarray(x, float)[sj], np.asarray(z, float)[sj], np.asarray(x, float)[ti],
                          np.asarray(z, float)[ti], vc)
    du[ti], dw[ti] = u, w
    return du, dw


def rotation_quarter(I, J, W, n, k_lo, k_hi):
    """[(targets, sources)] index arrays of the pairs (lane l of tile I, home lane (l + k) % 64 of tile J), k in [k_lo, k_hi): what one
    wave of a four-wave item works of a tile pair.  Lane l holds vortices I W + l + 64 t."""
    out = []
    T = W // 64
    for k in range(k_lo, k_hi):
        lanes = np.arange(64)
        ti = (I * W + lanes[:, None] + 64 * np.arange(T)[None, :])
        sj = (J * W + ((lanes + k) % 64)[:, None] + 64 * np.arange(T)[None, :])
        out.append((ti, sj))
    return out
