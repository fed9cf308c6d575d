"""The direct pair kernels at ragged shapes: the case table, its inputs and its float64 reference (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_direct_shapes_host.py (CPU: the table reaches every instantiation launch_pair can launch, sits on the
right side of every routing precondition, and its reference would notice a lost, doubled or misplaced source) and
tests/test_gpu_direct_shapes.py (GPU: every case by value through the production entry points).

Sizes are the smallest at which an index can still go wrong: sources are counted in the kernel's LDS tile (256 | 1024 fp32,
128 | 512 fp64) and targets in its block of 256 x TPL lanes.  Inputs come from oracle/g8_cases.py's counter-based generators
(no library's random stream; every value float32-representable, so every entry point sees the numbers the reference saw).
The reference is the project's float64 oracle on the same numbers, at ALL targets; tolerances are the contract's (G8.TOL),
relative to max(|u_ref|, |w_ref|) of the call."""
import functools
import os
import sys

import numpy as np

from oracle import c_oracle
from oracle import g8_cases as G8
from oracle import ludvm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_rule  # noqa: E402

VC, VC_SHEET = G8.VC, G8.VC_SHEET          # 0.065 (O(1) clouds), 1.3e-3 (config 2's sheets)
# float64: what test_empty_and_ragged_shapes asserts for the same kernels at these sizes
TOL = {"plain": G8.TOL["plain"], "local": G8.TOL["local"], "hilo": G8.TOL["hilo"], "f64": 1e-12}
assert (TOL["plain"], TOL["local"], TOL["hilo"]) == (1e-5, 1e-5, 2e-6)
BOX = (-3.0, 0.0, -1.0, 1.0)               # the clouds' box
SIDE_CAP = 4097                            # no case has more points on a side (apart from F64_PRODUCT_PAIR)

# ---- plain fp32 (induce_dev, induce_f32) and hi+lo (induce(..., 'f32x2')) ---------------------------------------------------
NS_PLAIN = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 3073)
NT_PLAIN = (1, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
TPLS = (1, 2, 4)
SPLITS_PLAIN = (0, 1, 2, 3, 5)             # 0: the rule
# ---- local origins (induce(..., 'f32'), both sides >= kOrderMin) ---------------------------------------------------------------
N_LOCAL = (2048, 2049, 2050, 2303, 2304, 2305, 3073, 4097)
SPLITS_LOCAL = (0, 1, 2, 3)
LAYOUTS = ("kept", "cloud", "self", "mixed")
# ---- float64 (induce(..., 'f64'), wake_induce_on_points) -----------------------------------------------------------------------
NT_F64 = (1, 2, 42, 43, 63, 64, 65, 85, 86, 127, 128, 129, 257)
NS_F64 = (127, 128, 129, 257, 1023, 1025)
SPLITS_F64 = (0, 1, 2)                     # (the issue's cases are the rule's; 1 and 2 add a walk over several 128-source tiles)
NS_F64_512, NT_F64_512 = (511, 512, 513, 1025), (257, 513)      # measurement build, LUDVM_SMALL_TILE_MAX_F64=0
F64_PRODUCT_PAIR = ((12000, 257), (12001, 257))                 # both sides of small_tile_max_f64 in the product
WAKE_SRC_FIRST = 3                         # an odd first source of wake_induce_on_points
# ---- fused Euler step (advect_dev) ---------------------------------------------------------------------------------------------
NS_ADVECT = (1025, 3073)
SPLITS_ADVECT = (0, 1, 3)


def advect_ranges(ns):
    return ((0, 1), (1, 63), (63, 257), (ns - 1, 1), (ns - 257, 257), (0, ns))


# ---- flow-field grids ----------------------------------------------------------------------------------------------------------
NS_GRID = (1, 255, 257, 1025, 2049)
PATCH_NX, PATCH_NZ = (1, 2, 3, 5), (4, 8, 12)
GENERIC_NX, GENERIC_NZ, GENERIC_TPL = 7, (1, 3, 5, 37), (0, 1, 2, 4)     # (7 x 37 = 259 points: one more than a block of 256 x 1)
SPLITS_GRID = (0, 1)                       # (1: a walk over every source tile, the last one ragged)
# every grid point is a multiple of 2^-6 with |x| < 4: exact in float32, so the plain-fp32 entry sees the reference's points
GRID_XMIN, GRID_ZMIN, GRID_DR = -3.1875, -1.09375, 0.171875


def grid_points(nx, nz):
    x, z = GRID_XMIN + GRID_DR * np.arange(nx), GRID_ZMIN + GRID_DR * np.arange(nz)
    X, Z = np.meshgrid(x, z, indexing="ij")
    return X.ravel(), Z.ravel()


def grid_shapes():
    """(nx, nz, targets-per-lane settings) of the table's grids"""
    out = [(nx, nz, (0,) + TPLS) for nx in PATCH_NX for nz in PATCH_NZ]        # TPL 0: the patch kernels; forced: the generic path
    out += [(GENERIC_NX, nz, GENERIC_TPL) for nz in GENERIC_NZ]
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def strengths(seed, stream, n, scale):
    """Circulations of either sign with |Gamma| in [0.5, 1.5) scale: no source is so weak that losing it would go unseen (the
    generators' N(0, 1) strengths have members arbitrarily close to zero, and the sensitivity checks ask about single sources)"""
    mag = 0.5 + G8.uniform24(seed, 1000 + 2 * stream, n)
    sign = np.where(G8.uniform24(seed, 1001 + 2 * stream, n) < 0.5, -1.0, 1.0)
    return G8.f32(sign * mag * scale)


def cloud(seed, stream, n):
    x, z, _ = G8.cloud(seed, stream, n, *BOX)
    return x, z, strengths(seed, stream, n, 1.0 / n)


def kept_sheet(seed, stream, n, z0=0.0, x0=-50.0, spacing=1e-3):
    x, z, _ = G8.sheet(seed, stream, n, x0=x0, spacing=spacing, amp=0.02, jitter=1e-3, z0=z0)
    return x, z, strengths(seed, stream, n, 1e-3)


@functools.lru_cache(maxsize=None)
def plain_inputs(ns, nt):
    """(g, xs, zs, xt, zt, v_core): two clouds in the box"""
    xs, zs, g = cloud(9100 + ns % 89, 0, ns)
    xt, zt, _ = cloud(9100 + ns % 89, 1, nt)
    return g, xs, zs, xt, zt, VC


@functools.lru_cache(maxsize=None)
def hilo_sheet_inputs(ns, nt):
    """a sheet at x0 = -50, neighbours 1e-3 apart (what hi+lo positions exist for), seen from points 1.5 cores off it that run
    from its LAST vortex back to its first (so that even a single target is next to the last source)"""
    xs, zs, g = kept_sheet(9200 + ns % 89, 0, ns)
    xt, zt, _ = kept_sheet(9200 + ns % 89, 1, nt, z0=0.002, x0=0.0, spacing=1e-3 * max(ns, nt) / nt)
    xt = G8.f32(xs[-1] - xt)
    return g, xs, zs, xt, zt, VC_SHEET


@functools.lru_cache(maxsize=None)
def local_inputs(layout, ns, nt):
    """kept: a sheet kept as stored, targets a second one; cloud: both sides go through Morton gather / scatter; self: the
    same arrays on both sides (xt is xs); mixed: two sheets through the box, half a unit apart and stored ALTERNATING (the order
    of a wake that sheds a leading-edge vortex with every trailing-edge one: each family takes one index parity, i.e. one origin
    class of every block), as sources, a cloud as targets"""
    seed = 9300 + ns % 89
    if layout == "kept":
        xs, zs, g = kept_sheet(seed, 0, ns)
        xt, zt, _ = kept_sheet(seed, 1, nt, z0=0.05)
        return g, xs, zs, xt, zt, VC_SHEET
    if layout == "cloud":
        xs, zs, g = cloud(seed, 0, ns)
        xt, zt, _ = cloud(seed, 1, nt)
        return g, xs, zs, xt, zt, VC
    if layout == "self":
        assert ns == nt
        xs, zs, g = cloud(seed, 2, ns)
        return g, xs, zs, xs, zs, VC
    if layout == "mixed":
        xs, zs, g = (np.empty(ns) for _ in range(3))
        for parity, z0 in ((0, 0.0), (1, 0.5)):
            xs[parity::2], zs[parity::2], g[parity::2] = kept_sheet(seed, 3 + parity, len(xs[parity::2]), x0=-3.5, z0=z0, spacing=2e-3)
        xt, zt, _ = cloud(seed, 5, nt)
        return g, xs, zs, xt, zt, VC
    raise ValueError(layout)


def local_shapes(layout):
    return [(n, n) for n in N_LOCAL] if layout == "self" else [(ns, nt) for ns in N_LOCAL for nt in N_LOCAL]


@functools.lru_cache(maxsize=None)
def f64_inputs(ns, nt):
    xs, zs, g = cloud(9400 + ns % 89, 0, ns)
    xt, zt, _ = cloud(9400 + ns % 89, 1, nt)
    return g, xs, zs, xt, zt, VC


@functools.lru_cache(maxsize=None)
def advect_inputs(ns):
    xs, zs, g = cloud(9500 + ns % 89, 0, ns)
    return g, xs, zs, VC


@functools.lru_cache(maxsize=None)
def grid_inputs(ns):
    xs, zs, g = cloud(9600 + ns % 89, 0, ns)
    return g, xs, zs, VC


# ---- the reference -------------------------------------------------------------------------------------------------------------
def reference(g, xs, zs, xt, zt, vc):
    """(u, w) float64 at ALL targets: oracle/pair_oracle.c where it is built (same terms as the Python oracle, sequential row
    sums: 1e-13 apart), else oracle/ludvm_oracle.py"""
    if c_oracle.available():
        return c_oracle.induced_velocity(g, xs, zs, xt, zt, vc)
    return O.induced_velocity(g, xs, zs, xt, zt, vc, rows_per_chunk=max(1, (1 << 22) // max(len(xs), 1)))


_REF = {}


def cached_reference(key, inputs):
    """one reference per case, shared by every launch shape that evaluates it; read-only"""
    if key not in _REF:
        u, w = reference(*inputs)
        u.setflags(write=False)
        w.setflags(write=False)
        _REF[key] = (u, w)
    return _REF[key]


def rel_err(u, w, ur, wr):
    scale = max(np.abs(ur).max(), np.abs(wr).max(), 1e-300)
    return max(np.abs(np.asarray(u, np.float64) - ur).max(), np.abs(np.asarray(w, np.float64) - wr).max()) / scale


# ---- what the plan makes of the table (tools/plan_rule.py: the library's own header) ----------------------------------------------
# engines of the measurement build (libludvm_hip_exp.so) the table needs, as plan knobs and as the environment that sets them
EXP = {
    "tile1024": (dict(small_tile_max=0, small_tile_max_f64=0), {"LUDVM_SMALL_TILE_MAX": "0"}),
    "f64_tile512": (dict(small_tile_max_f64=0), {"LUDVM_SMALL_TILE_MAX_F64": "0"}),
    "few_unpacked": (dict(few_packed=0), {"LUDVM_FEW_PACKED": "0"}),
    "few_packed": (dict(few_packed=1), {"LUDVM_FEW_PACKED": "1"}),
    "grid_row": (dict(grid_kernel=1), {"LUDVM_GRID_KERNEL": "row"}),
    "grid_row_tile1024": (dict(grid_kernel=1, small_tile_max=0, small_tile_max_f64=0),
                          {"LUDVM_GRID_KERNEL": "row", "LUDVM_SMALL_TILE_MAX": "0"}),
    "grid_patch4_tile1024": (dict(grid_kernel=4, small_tile_max=0, small_tile_max_f64=0),
                             {"LUDVM_GRID_KERNEL": "patch4", "LUDVM_SMALL_TILE_MAX": "0"}),
}


def table():
    """Every launch of the table as (family, build, plan_rule case): family names the part of the table, build is 'product' or
    a key of EXP.  tests/test_gpu_direct_shapes.py runs exactly these."""
    rows = []

    def add(family, build, **case):
        if build != "product":
            case.update(EXP[build][0])
        rows.append((family, build, case))
    for build in ("product", "tile1024"):
        for ns in NS_PLAIN:
            for nt in NT_PLAIN:
                for tpl in TPLS:
                    for s in SPLITS_PLAIN:
                        add("plain", build, precision="f32", ns=ns, nt=nt, tune_tpl=tpl, tune_split=s)
                        add("hilo", build, precision="f32x2", ns=ns, nt=nt, tune_tpl=tpl, tune_split=s)
        for layout in LAYOUTS:
            for ns, nt in local_shapes(layout):
                for tpl in TPLS:
                    for s in SPLITS_LOCAL:
                        add("local_" + layout, build, precision="f32", local=True, ns=ns, nt=nt, tune_tpl=tpl, tune_split=s)
    for build in ("product", "few_unpacked", "few_packed"):
        for ns in NS_F64:
            for nt in NT_F64:
                for s in SPLITS_F64:
                    add("f64", build, precision="f64", ns=ns, nt=nt, tune_split=s)
    for ns in NS_F64_512:
        for nt in NT_F64_512:
            for s in SPLITS_F64:
                add("f64_512", "f64_tile512", precision="f64", ns=ns, nt=nt, tune_split=s)
    for ns, nt in F64_PRODUCT_PAIR:
        add("f64_product_pair", "product", precision="f64", ns=ns, nt=nt)
    for ns in NS_ADVECT:
        for t_first, nt in advect_ranges(ns):
            for tpl in TPLS:
                for s in SPLITS_ADVECT:
                    for build in ("product", "tile1024"):
                        add("advect", build, precision="f32", ns=ns, nt=nt, slab=True, tune_tpl=tpl, tune_split=s)
    for build in ("product", "tile1024", "grid_row", "grid_row_tile1024", "grid_patch4_tile1024"):
        for ns in NS_GRID:
            for nx, nz, tpls in grid_shapes():
                for tpl in tpls:
                    if build != "product" and tpl != 0:
                        continue          # (the measurement builds are here for the row / patch kernels)
                    for s in SPLITS_GRID:
                        for local in (True, False):      # host flowfield | flowfield_dev
                            add("grid_local" if local else "grid_plain", build, precision="f32", local=local, ns=ns, nt=nx * nz,
                                grid_nz=nz, tune_tpl=tpl, tune_split=s)
    return rows


@functools.lru_cache(maxsize=None)
def planned_table():
    """[(family, build, case, plan_rule.Plan)]"""
    rows = table()
    return [r + (p,) for r, p in zip(rows, plan_rule.plan([c for _, _, c in rows]))]


def split_sizes(ns, p):
    """sources of each split of a planned launch"""
    return [min(p.chunk, ns - k * p.chunk) for k in range(p.nsplit)]


# ---- single-source contributions (the sensitivity checks) ------------------------------------------------------------------------
def contribution(g, xs, zs, xt, zt, vc):
    """(u, w)[nt] of the sources (g, xs, zs) -- a few of them -- at the targets: the oracle's terms, summed by NumPy"""
    dx = xt[:, None] - np.atleast_1d(xs)[None, :]
    dz = zt[:, None] - np.atleast_1d(zs)[None, :]
    k = np.atleast_1d(g)[None, :] / (2 * np.pi * np.sqrt((dx * dx + dz * dz) ** 2 + vc**4))
    return (k * dz).sum(1), -(k * dx).sum(1)
