"""Shared by tests/test_tracers_f32x2_host.py and tests/test_gpu_tracers_f32x2.py: a NumPy restatement of the hi+lo fp32 tracer
scheme (march_f32x2_tracer_partial), the bounds, and the cases the two tiers use.

The scheme: every float64 position v is split into hi = float32(v) and lo = float32(v - hi); a difference is
(hi_p - hi_s) + (lo_p - lo_s) in float32 and the pair is float32 from there; the sources go in tiles of 256 from the first one;
within a tile the even sources are summed, one after the other, in one float32 accumulator and the odd ones in another; at the
end of a tile the even sum, then the odd sum, is added to the point's float64 total; 1 / 2 pi and the sign in float64."""
import numpy as np

from survey_f32_common import far_cloud, far_sheet, sparse_cloud_keywords

# of max|u|: the project's hi+lo tier ("<= 2e-6 with hi+lo positions")
VELOCITY_VS_F64 = 2e-6
# a row against a float64 Euler step from the same start: dt |du| <= VELOCITY_VS_F64 x the largest single step, and the float64
# rounding of start + dt u in another summation order, 1e-9 of the largest displacement
STEP_VS_F64 = 2e-6
STEP_ROUNDING = 1e-9
TILE = 256                      # kHiloTile (ludvm_amd/csrc/march_kernels.hpp): sources per staged tile
F32 = np.float32


def split_hilo(v):
    v = np.asarray(v, dtype=np.float64)
    hi = v.astype(F32)
    return hi, (v - hi.astype(np.float64)).astype(F32)


def _sum_in_order(terms):
    """Sum float32 [points, members] over the members one after the other in float32 (what one half of a lane's packed
    accumulator does)."""
    acc = np.zeros(terms.shape[0], dtype=F32)
    for j in range(terms.shape[1]):
        acc = (acc + terms[:, j]).astype(F32)
    return acc


def hilo_f32_field(g, xs, zs, px, pz, v_core):
    """-> (u, w): the field of the sources (g, xs, zs: float64, in stored order) at the points by the hi+lo fp32 scheme."""
    g = np.asarray(g, dtype=np.float64)
    (xsh, xsl), (zsh, zsl), (xph, xpl), (zph, zpl) = (split_hilo(a) for a in (xs, zs, px, pz))
    gf, vc4 = g.astype(F32), F32(float(v_core) ** 4)
    u, w = np.zeros(len(xph)), np.zeros(len(xph))
    for base in range(0, len(g), TILE):
        for par in (0, 1):
            idx = np.arange(base + par, min(base + TILE, len(g)), 2)
            if len(idx) == 0:
                continue
            dx = ((xph[:, None] - xsh[idx][None]) + (xpl[:, None] - xsl[idx][None])).astype(F32)
            dz = ((zph[:, None] - zsh[idx][None]) + (zpl[:, None] - zsl[idx][None])).astype(F32)
            r2 = dx * dx + dz * dz
            with np.errstate(over="ignore"):
                s = (F32(1.0) / np.sqrt(r2 * r2 + vc4)) * gf[idx][None]
            u += _sum_in_order(dz * s).astype(np.float64)
            w += _sum_in_order(dx * s).astype(np.float64)
    return u / (2 * np.pi), -w / (2 * np.pi)


def table_cases():
    """The five cases of DESIGN.md section 4.9's accuracy table -> {name: (gamma, x, z, v_core)}."""
    from conftest import load_golden
    vc5 = float(load_golden("g5_freevort.npz")["v_core"])
    sparse = sparse_cloud_keywords()
    return {
        "cloud256_at_-55": (*far_cloud(fill=256), vc5),
        "cloud256_at_-5000": (*far_cloud(x0=-5000.0, fill=256), vc5),
        "sheet600_1e-3_at_-55": (*far_sheet(), 1.3e-3),
        "sheet2000_5e-3": (*far_sheet(n=2000, spacing=5e-3), 1.3e-3),
        "sparse_cloud": (sparse["circulation_freevort"], sparse["xy_freevort"][0], sparse["xy_freevort"][1], 0.065),
    }
