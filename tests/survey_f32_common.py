"""Shared by tests/test_survey_f32_host.py and tests/test_gpu_survey_f32.py: a NumPy restatement of the fp32 survey scheme
(march_f32_survey_partial), the bounds, and the source sets and points the two tiers use.

The scheme: sources in tiles of 256 slots counted from slot 0; a tile's two origin classes are its even and its odd slots; a
class's origin is the float64 position of its middle valid member; offsets and point differences are rounded to float32 after
a float64 subtraction; the pairs of a class are summed in float32, the class sums are added in float64 in class order; a class
whose largest |offset| exceeds `max_extent` v_core is evaluated in float64."""
import numpy as np

from conftest import load_golden

MEAN_VS_F64 = 1e-5              # of max|u|: the project's fp32 bound
MOMENT_VS_F64 = 3e-5            # of max|u|^2: |ab - a'b'| <= |a||b - b'| + |b'||a - a'| <= 2e-5 max|u|^2, and the 1e-10 term
GUARDED_VS_F64 = 1e-12          # of max|u|: every class in float64 -- the float64 arithmetic in another summation tree
MAX_EXTENT = 300.0              # kSurveyF32MaxExtent (ludvm_amd/csrc/march_kernels.hpp), in units of v_core
TILE = 256
FAR_X = -55.0


def _pairs(dx, dz, g, vc4, dtype):
    """(G dz / sqrt(r^4 + vc^4), G dx / sqrt(r^4 + vc^4)) in `dtype` for differences [points, members]."""
    dx, dz = dx.astype(dtype), dz.astype(dtype)
    r2 = dx * dx + dz * dz
    with np.errstate(over="ignore"):
        s = (dtype(1.0) / np.sqrt(r2 * r2 + dtype(vc4))) * g.astype(dtype)
    return dz * s, dx * s


def _sum_in_order(terms, dtype):
    """Sum [points, members] over the members one after the other in `dtype` (what one lane's accumulator does)."""
    acc = np.zeros(terms.shape[0], dtype=dtype)
    for j in range(terms.shape[1]):
        acc = (acc + terms[:, j]).astype(dtype)
    return acc


def local_f32_field(g, xs, zs, px, pz, v_core, max_extent=MAX_EXTENT, plain=False):
    """-> (u, w, guarded classes, classes): the field of the sources (g, xs, zs: float64, in stored order) at the points by the
    fp32 scheme.  plain=True: the same sums with every coordinate rounded to float32 as it stands (no origins, no guard)."""
    g, xs, zs, px, pz = (np.asarray(a, dtype=np.float64) for a in (g, xs, zs, px, pz))
    vc4 = float(v_core) ** 4
    u, w = np.zeros(len(px)), np.zeros(len(px))
    guarded = classes = 0
    for base in range(0, len(g), TILE):
        for par in (0, 1):
            idx = np.arange(base + par, min(base + TILE, len(g)), 2)
            if len(idx) == 0:
                continue
            classes += 1
            if plain:
                cu, cw = _pairs(px.astype(np.float32)[:, None] - xs[idx].astype(np.float32)[None],
                                pz.astype(np.float32)[:, None] - zs[idx].astype(np.float32)[None], g[idx], vc4, np.float32)
                u += _sum_in_order(cu, np.float32)
                w += _sum_in_order(cw, np.float32)
                continue
            mid = idx[len(idx) // 2]
            ox, oz = xs[mid], zs[mid]
            fx, fz = (xs[idx] - ox).astype(np.float32), (zs[idx] - oz).astype(np.float32)
            if max(np.abs(fx).max(), np.abs(fz).max()) > np.float32(max_extent * v_core):
                guarded += 1
                cu, cw = _pairs(px[:, None] - xs[idx][None], pz[:, None] - zs[idx][None], g[idx], vc4, np.float64)
                u += _sum_in_order(cu, np.float64)
                w += _sum_in_order(cw, np.float64)
            else:
                cu, cw = _pairs((px - ox).astype(np.float32)[:, None] - fx[None], (pz - oz).astype(np.float32)[:, None] - fz[None],
                                g[idx], vc4, np.float32)
                u += _sum_in_order(cu, np.float32)
                w += _sum_in_order(cw, np.float32)
    return u / (2 * np.pi), -w / (2 * np.pi), guarded, classes


def f64_field(g, xs, zs, px, pz, v_core):
    from oracle import ludvm_oracle as O
    return O.induced_velocity(np.asarray(g), np.asarray(xs), np.asarray(zs), np.asarray(px), np.asarray(pz), v_core)


def field_error(a, b):
    """max |a - b| over (u, w) and points, of max|u| of b."""
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) / max(np.abs(b[0]).max(), np.abs(b[1]).max())


def far_cloud(x0=FAR_X, fill=0):
    """G5's 61 free vortices, their box moved so that it is centred on x = x0 -> (gamma, x, z).  fill > 61: followed by more
    vortices drawn in the same box with circulations of the same size, `fill` in all -- fill = 256 is one whole source tile, so
    that in a run the cloud's two origin classes hold nothing but the cloud (a smaller cloud shares its tile with the shed and
    the bound vortices 55 chords away, and both classes of that tile take the guard)."""
    g5 = load_golden("g5_freevort.npz")
    xy = g5["xy_freevort"]
    g, x, z = g5["gamma_freevort"].copy(), xy[0] - xy[0].mean() + x0, xy[1].copy()
    if fill > len(g):
        rng = np.random.default_rng(61)
        m = fill - len(g)
        x = np.concatenate([x, rng.uniform(x.min(), x.max(), m)])
        z = np.concatenate([z, rng.uniform(z.min(), z.max(), m)])
        g = np.concatenate([g, rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m) * np.abs(g).max()])
    return g, x, z


def far_cloud_keywords(x0=FAR_X, fill=0):
    g, x, z = far_cloud(x0, fill)
    return dict(circulation_freevort=g, xy_freevort=np.stack([x, z]))


def far_sheet(n=600, x0=FAR_X, spacing=1e-3):
    """A rolled-up piece of vortex sheet of n vortices `spacing` apart, beginning at x = x0 -> (gamma, x, z)."""
    k = np.arange(n)
    x = x0 + spacing * k
    z = 0.02 * np.sin(2 * np.pi * k / 157.0) + 1e-4 * np.cos(0.7 * k)
    g = 1e-3 * (1.0 + 0.3 * np.sin(0.05 * k))
    return g, x, z


def points_around(xs, zs, v_core, chord=1.0, seed=3):
    """Survey points ON the sources, within one core of them, and several chords away -> [2, 3 n]."""
    rng = np.random.default_rng(seed)
    n = len(xs)
    ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.05, 1.0, n) * v_core
    far_ang, far_rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(3.0, 8.0, n) * chord
    x = np.concatenate([xs, xs + rad * np.cos(ang), xs + far_rad * np.cos(far_ang)])
    z = np.concatenate([zs, zs + rad * np.sin(ang), zs + far_rad * np.sin(far_ang)])
    return np.stack([x, z])


def sparse_cloud_keywords(n=300, v_core=0.065, seed=11):
    """n free vortices of +-(0.5 .. 1) 1e-2 on a jittered lattice whose spacing is 1000 v_core: every origin class is far wider
    than MAX_EXTENT v_core."""
    rng = np.random.default_rng(seed)
    h = 1000.0 * v_core
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    x = -h * (k % side) + rng.uniform(-0.1, 0.1, n) * h - 5.0
    z = h * (k // side - side / 2) + rng.uniform(-0.1, 0.1, n) * h
    g = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 1e-2
    return dict(circulation_freevort=g, xy_freevort=np.stack([x, z]))
