"""G8 case table: the fp32 pair-kernel routes at the library's routing thresholds (TEST INFRASTRUCTURE ONLY).

The one source of truth of fixture group G8.  oracle/gen_golden.py (g8) runs the reference on these cases and writes
tests/golden/g8_fp32_routes.npz; tests/test_g8_fixture.py (CPU) checks that the inputs regenerate, that the oracles agree
with the fixture and that every pair of cases still straddles the library's threshold; tests/test_gpu_g8.py runs each case
through the production entry points.  This module does not import the reference.

Inputs depend on no library's random stream: every value comes from splitmix64 of (seed, stream, index) and integer-exact
float64 arithmetic, then is rounded to float32 and stored as float64, so the host entry's fp32 conversion and the device
entry see exactly the numbers the reference saw, and the fixture regenerates bit for bit on any machine.
"""
import hashlib

import numpy as np

# ------------------------------------------------------------------------------------------------ counter-based inputs
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed, stream, n):
    """uint64[n]: splitmix64 outputs for counters (seed, stream, 0 .. n-1)."""
    base = (np.uint64(seed) << np.uint64(32)) ^ (np.uint64(stream) << np.uint64(48))
    z = (base + np.arange(n, dtype=np.uint64)) * _GOLDEN
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def uniform24(seed, stream, n):
    """float64[n] in [0, 1), multiples of 2^-24 (exact in float32)."""
    return (splitmix64(seed, stream, n) >> np.uint64(40)).astype(np.float64) * 2.0**-24


def normal12(seed, stream, n):
    """Irwin-Hall approximation of N(0, 1): twelve 24-bit uniforms minus 6 (exact in float64, no transcendental)."""
    s = np.zeros(n)
    for k in range(12):
        s += uniform24(seed, stream * 16 + k + 1, n)
    return s - 6.0


def f32(a):
    """Round to float32, keep as float64: the values every entry point sees unchanged."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def cloud(seed, stream, n, x0=-10.0, x1=0.0, z0=-2.0, z1=2.0):
    """Uniform cloud in [x0, x1] x [z0, z1] with Gamma ~ N(0, 1) / n (the box of test_symmetric_kernel_tile_edges)."""
    x = f32(x0 + (x1 - x0) * uniform24(seed, 3 * stream, n))
    z = f32(z0 + (z1 - z0) * uniform24(seed, 3 * stream + 1, n))
    g = f32(normal12(seed, 3 * stream + 2, n) / n)
    return x, z, g


def sheet(seed, stream, n, x0=-50.0, spacing=1e-3, amp=0.3, jitter=1e-3, gscale=1e-3, z0=0.0):
    """A shed sheet stored along itself (config 2's regime: |x| ~ 50, neighbours ~1e-3 apart): x increases with the index,
    z follows a parabola across the sheet plus a small jitter."""
    s = np.arange(n, dtype=np.float64)
    t = s / max(n - 1, 1)
    x = f32(x0 + spacing * (s + 0.5 * uniform24(seed, 3 * stream, n)))
    z = f32(z0 + amp * 4.0 * t * (1.0 - t) + jitter * (uniform24(seed, 3 * stream + 1, n) - 0.5))
    g = f32(normal12(seed, 3 * stream + 2, n) * gscale)
    return x, z, g


def foil(seed, n=80):
    """An 80-point bound-vortex row a chord upstream of sheet(): the airfoil of :1105-1106's second call."""
    k = np.arange(n, dtype=np.float64) / (n - 1)
    return f32(-51.0 + k), f32(0.01 * k), f32(normal12(seed, 9, n) * 1e-2)


# ------------------------------------------------------------------------------------------------ class extents
def class_extent_mean(x, z, order=None):
    """Mean over the 128-point origin classes (256-element block x index parity, ctx.hpp / order_kernels.hpp class_extents)
    of (xmax - xmin) + (zmax - zmin), points taken in `order` (None: as stored); divided by 2 ceil(n / 256) as order.hip does."""
    n = len(x)
    if order is not None:
        x, z = x[order], z[order]
    nblk = -(-n // 256)
    pad = nblk * 256 - n
    xp = np.concatenate([x, np.full(pad, np.nan)]).reshape(nblk, 128, 2)
    zp = np.concatenate([z, np.full(pad, np.nan)]).reshape(nblk, 128, 2)
    e = (np.nanmax(xp, 1) - np.nanmin(xp, 1)) + (np.nanmax(zp, 1) - np.nanmin(zp, 1))
    return float(np.nansum(e)) / (2.0 * nblk)


def _spread16(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(8))) & np.uint32(0x00FF00FF)
    v = (v | (v << np.uint32(4))) & np.uint32(0x0F0F0F0F)
    v = (v | (v << np.uint32(2))) & np.uint32(0x33333333)
    v = (v | (v << np.uint32(1))) & np.uint32(0x55555555)
    return v


def morton_order(x, z):
    """The library's Morton order (spatial_order.hip: 16-bit cells over the longer side of the box, stable sort)."""
    x0, z0 = x.min(), z.min()
    span = max(x.max() - x0, z.max() - z0)
    cx = np.minimum(np.maximum((x - x0) * (65535.0 / span), 0.0), 65535.0)
    cz = np.minimum(np.maximum((z - z0) * (65535.0 / span), 0.0), 65535.0)
    key = _spread16(cx) | (_spread16(cz) << np.uint32(1))
    return np.argsort(key, kind="stable")


def predicted_order(x, z):
    """(reordered, mean class extent) as order.hip's spatial_order_if_needed decides them (n >= kOrderMin), restated on the
    host; the sums run in another order than the device's, so use it with a margin."""
    n = len(x)
    nclass = 2.0 * np.ceil(n / 256)
    e_given = class_extent_mean(x, z) * nclass
    ex, ez = x.max() - x.min(), z.max() - z.min()
    side = np.sqrt(128.0 * ex * ez / n)
    if e_given <= 3.0 * nclass * 2.0 * side or e_given <= 3.0 * nclass * (ex + ez) * 256.0 / n:
        return False, e_given / nclass
    e_sorted = class_extent_mean(x, z, morton_order(x, z)) * nclass
    if e_given <= 1.5 * e_sorted:
        return False, e_given / nclass
    return True, e_sorted / nclass


# ------------------------------------------------------------------------------------------------ the cases
# Tolerances (x max(|u_ref|, |w_ref|) over the sampled targets): the contract of include/ludvm_hip.h and DESIGN section 2.
TOL = {"f64": 1e-11, "local": 1e-5, "plain": 1e-5, "hilo": 2e-6}

VC = 0.065           # the O(1) core of test_symmetric_kernel_tile_edges
VC_SHEET = 1.3e-3    # config 2's core
# Extent cases (their cores were set from the class extents the generator computes, class_extent_mean / predicted_order,
# rounded; tests/test_g8_fixture.py recomputes the ratio): a sheet kept as given at 0.9 x / 1.1 x of kMaxExtentOverCore and
# a cloud taken in Morton order at 0.85 x / 1.15 x of kMaxExtentOverCoreCloud.
VC_KEPT_LO, VC_KEPT_HI = 9.3e-4, 7.6e-4
VC_MORTON_LO, VC_MORTON_HI = 1.33e-2, 9.8e-3

PARAM_KEYS = ("seed", "ns", "nt", "v_core", "nx", "nz", "xmin", "zmin", "dr")


def _case(name, kind, seed, ns, nt, vc, entries, threshold, **kw):
    c = dict(name=name, kind=kind, seed=seed, ns=ns, nt=nt, v_core=vc, entries=dict(entries), threshold=threshold,
             nx=0, nz=0, xmin=0.0, zmin=0.0, dr=0.0, reordered=None, extent_side=None)
    c.update(kw)
    return c


def _build():
    cases = []
    # self-interaction of an O(1) cloud: the host entry (Morton order, local origins) and the plain-fp32 device entry
    for n, thr in ((14000, ("small_tile_max", 14000)), (14001, ("small_tile_max", 14000)),
                   (16383, ("kSymMinN", 16384)), (16384, ("kSymMinN", 16384)),
                   (36863, ("kSymT8MinN", 36864)), (36864, ("kSymT8MinN", 36864)),
                   (327168, ("sym_quad_min_tiles", 640)), (327169, ("sym_quad_min_tiles", 640))):
        cases.append(_case(f"self_cloud_{n}", "self_cloud", 8000 + n % 1000, n, n, VC,
                           {"induce_f32": "local", "induce_dev": "plain"}, thr))
    # a cloud too sparse for its core: hi+lo positions on the symmetric kernel (T = 4) from either precision
    cases.append(_case("self_sparse_40000", "self_cloud", 8101, 40000, 40000, VC_SHEET,
                       {"induce_f32": "hilo", "induce_f32x2": "hilo"}, ("kMaxExtentOverCoreCloud", 150.0),
                       reordered=True, extent_side="above"))
    # config-2-like sheets: symmetric T4 / T8 on local origins, the resident wake with an 80-point foil, hi+lo
    for n, thr in ((20000, ("kSymT8MinN", 36864)), (45000, ("kSymT8MinN", 36864))):
        cases.append(_case(f"sheet_{n}", "sheet", 8200 + n % 1000, n, n, VC_SHEET,
                           {"induce_f32": "local", "wake_f32": "local", "wake_f32x2": "hilo"}, thr,
                           reordered=False, extent_side="below"))
    # the extent bounds
    cases.append(_case("extent_kept_lo", "kept_sheet", 8301, 20000, 20000, VC_KEPT_LO, {"induce_f32": "local"},
                       ("kMaxExtentOverCore", 300.0), reordered=False, extent_side="below"))
    cases.append(_case("extent_kept_hi", "kept_sheet", 8301, 20000, 20000, VC_KEPT_HI, {"induce_f32": "hilo"},
                       ("kMaxExtentOverCore", 300.0), reordered=False, extent_side="above"))
    cases.append(_case("extent_morton_lo", "self_cloud", 8302, 40000, 40000, VC_MORTON_LO, {"induce_f32": "local"},
                       ("kMaxExtentOverCoreCloud", 150.0), reordered=True, extent_side="below"))
    cases.append(_case("extent_morton_hi", "self_cloud", 8302, 40000, 40000, VC_MORTON_HI, {"induce_f32": "hilo"},
                       ("kMaxExtentOverCoreCloud", 150.0), reordered=True, extent_side="above"))
    # separate sources and targets
    for ns, nt, route, thr in (
            (4096, 2047, "f64", ("kOrderMin", 2048)), (4096, 2048, "local", ("kOrderMin", 2048)),
            (2047, 4096, "f64", ("kOrderMin", 2048)), (2048, 4096, "local", ("kOrderMin", 2048))):
        side = f"t{nt}" if ns == 4096 else f"s{ns}"
        cases.append(_case(f"side_{side}", "pair_cloud", 8400 + ns % 97 + nt % 89, ns, nt, VC, {"induce_f32": route}, thr))
    for ns, route in ((524288, "f64"), (524289, "hilo")):
        cases.append(_case(f"pairs_{ns}", "pair_cloud", 8500 + ns % 7, ns, 512, VC, {"induce_f32": route},
                           ("kSmallSidePairsF64", 268435456.0)))
    for nt in (131071, 131072):
        cases.append(_case(f"tpl_{nt}", "pair_cloud", 8600 + nt % 7, 4096, nt, VC, {"induce_f32": "local"},
                           ("launch.hip nt >= 131072", 131072)))
    cases.append(_case("local_200k", "pair_cloud", 8701, 200000, 4096, VC, {"induce_f32": "local"}, None))
    cases.append(_case("sparse_pairs", "pair_cloud", 8702, 100000, 4096, VC_SHEET, {"induce_f32": "hilo"},
                       ("kMaxExtentOverCoreCloud", 150.0), reordered=True, extent_side="above"))
    # flow-field grids over a cloud plus a sheet (the reference's flowfield(), :1186-1217: np.arange grid, 'ij' meshgrid)
    for name, seed, ns, zmax, dr, thr in (
            ("ff_default", 8801, 30000, 4.0, 0.02, ("kPatch4MinTargets", 1 << 20)),
            ("ff_small", 8802, 12000, 4.0, 0.04, ("small_tile_max", 14000)),
            ("ff_fine", 8803, 30000, 4.0, 2.0**-7, ("kPatch4MinTargets", 1 << 20)),
            ("ff_ragged", 8804, 30000, 3.98, 0.02, None)):
        nx, nz = len(np.arange(-10.0, 0.0, dr)), len(np.arange(-4.0, zmax, dr))
        cases.append(_case(name, "grid", seed, ns, nx * nz, VC, {"flowfield": "local"}, thr, nx=nx, nz=nz, xmin=-10.0,
                           zmin=-4.0, dr=dr, zmax=zmax))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}

# (case below, case above, library constant): each pair is (t - 1, t) at the constant's current first size t on the far side
PAIRS = [("self_cloud_14000", "self_cloud_14001", "small_tile_max"),
         ("self_cloud_16383", "self_cloud_16384", "kSymMinN"),
         ("self_cloud_36863", "self_cloud_36864", "kSymT8MinN"),
         ("self_cloud_327168", "self_cloud_327169", "sym_quad_min_tiles"),
         ("side_t2047", "side_t2048", "kOrderMin"),
         ("side_s2047", "side_s2048", "kOrderMin"),
         ("pairs_524288", "pairs_524289", "kSmallSidePairsF64"),
         ("tpl_131071", "tpl_131072", "tpl2_min_targets")]


def params(c):
    """float64[len(PARAM_KEYS)]: the numbers a case is made of (stored in the fixture, compared with the table)."""
    return np.array([float(c[k]) for k in PARAM_KEYS])


def tolerance(c, entry):
    return TOL[c["entries"][entry]]


def inputs(c):
    """The case's full inputs, float64 arrays of float32 values: dict with g, xs, zs (sources); xt, zt (separate targets,
    else absent); foil_x, foil_z, foil_g (sheet cases)."""
    seed, ns, nt = c["seed"], c["ns"], c["nt"]
    kind = c["kind"]
    if kind == "self_cloud":
        x, z, g = cloud(seed, 0, ns)
        return dict(g=g, xs=x, zs=z)
    if kind == "sheet":
        x, z, g = sheet(seed, 0, ns)
        fx, fz, fg = foil(seed)
        return dict(g=g, xs=x, zs=z, foil_x=fx, foil_z=fz, foil_g=fg)
    if kind == "kept_sheet":
        # a thin sheet kept as given whose classes span ~0.26: spacing 1e-3 along x, a gentle parabola across
        x, z, g = sheet(seed, 0, ns, x0=-40.0, spacing=1e-3, amp=0.02, jitter=0.0)
        return dict(g=g, xs=x, zs=z)
    if kind == "pair_cloud":
        xs, zs, g = cloud(seed, 0, ns)
        xt, zt, _ = cloud(seed, 1, nt)
        return dict(g=g, xs=xs, zs=zs, xt=xt, zt=zt)
    if kind == "grid":
        m = ns // 3
        xc, zc, gc = cloud(seed, 0, ns - m)
        xs_, zs_, gs_ = sheet(seed, 1, m, x0=-9.0, spacing=8.0 / m, amp=0.5, jitter=1e-3, gscale=1.0 / ns, z0=-0.25)
        return dict(g=np.concatenate([gc, gs_]), xs=np.concatenate([xc, xs_]), zs=np.concatenate([zc, zs_]))
    raise ValueError(kind)


def grid_axes(c):
    """The reference's grid axes (np.arange, :1193) of a grid case."""
    return np.arange(c["xmin"], 0.0, c["dr"]), np.arange(c["zmin"], c["zmax"], c["dr"])


def sample(c):
    """int64 indices of the sampled targets: 0-63, the last 64 and 128 seeded others (256); all of 512 targets; on a grid
    (flat 'ij' index) the four corners, points of the first and last row and column, and seeded others (256)."""
    nt = c["nt"]
    if nt <= 512:
        return np.arange(nt, dtype=np.int64)
    if c["kind"] == "grid":
        nx, nz = c["nx"], c["nz"]
        ri = np.linspace(0, nx - 1, 16).astype(np.int64)
        cj = np.linspace(0, nz - 1, 16).astype(np.int64)
        edge = np.concatenate([0 * nz + cj, (nx - 1) * nz + cj, ri * nz + 0, ri * nz + (nz - 1)])
        edge = np.unique(edge)
        need = 256 - len(edge)
        key = splitmix64(c["seed"], 77, nt)
        key[edge] = np.iinfo(np.uint64).max
        return np.sort(np.concatenate([edge, np.argsort(key, kind="stable")[:need]]))
    first = np.arange(64, dtype=np.int64)
    last = np.arange(nt - 64, nt, dtype=np.int64)
    key = splitmix64(c["seed"], 78, nt - 128)
    mid = 64 + np.argsort(key, kind="stable")[:128]
    return np.sort(np.concatenate([first, mid, last]))


def targets(c, inp, idx):
    """(xp, zp) float64 of the sampled targets."""
    if c["kind"] == "grid":
        x1, z1 = grid_axes(c)
        return x1[idx // c["nz"]], z1[idx % c["nz"]]
    if "xt" in inp:
        return inp["xt"][idx], inp["zt"][idx]
    return inp["xs"][idx], inp["zs"][idx]


def digest(inp):
    """uint8[32]: sha256 of the case's inputs (float64, little-endian, fixed key order)."""
    h = hashlib.sha256()
    for k in ("g", "xs", "zs", "xt", "zt", "foil_x", "foil_z", "foil_g"):
        if k in inp:
            h.update(k.encode())
            h.update(np.ascontiguousarray(inp[k], dtype="<f8").tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()
