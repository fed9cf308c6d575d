// Kernels of the flow field (flowfield.hip): source staging conversions, the vorticity stencil of LUDVM.flowfield
// (LUDVM.py:1224-1292), the scalar pair sums (stream function, analytic vorticity) and the velocity gradient in float64, and the
// latter two in hi+lo fp32 (field_hilo_f32).  Non-template kernels: this header
// belongs to ONE translation unit (flowfield.hip).
#pragma once
#include "pair_kernels.hpp"
#include "pair_sym_kernels.hpp"
#include "scalar_term.hpp"

namespace ludvm {

// float64 -> float32 staging conversion for the stateless host API.
__global__ void __launch_bounds__(kBlock)
cvt_f64_to_f32(const double* in, float* hi, float* lo, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float h, l;
  split_hilo(in[i], h, l);
  hi[i] = h;
  if (lo) lo[i] = l;
}

__global__ void __launch_bounds__(kBlock)
cvt_f32_to_f64(const float* in, double* out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// float64 -> local-origin fp32 for the stateless host API: off[i] = (float)(in[i] - org[origin_slot(i)]) with
// org[2 b + p] = (float)in[origin_index(b, p, n)].  n is rounded up to whole blocks by the grid: the threads of a
// class without a member still write its record (a number: the kernels read both records of every block they stage).
__global__ void __launch_bounds__(kBlock)
cvt_f64_to_local(const double* in, float* off, float* org, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long b = i >> kOriginShift;
  if ((b << kOriginShift) >= n) return;
  const int p = (int)(i & 1);
  const float o = (float)in[origin_index(b, p, n)];
  if ((i & (kOriginBlock - 1)) < 2) org[2 * b + p] = o;
  if (i < n) off[i] = (float)(in[i] - (double)o);
}

// ---------------------------------------------------------------------------------------------
// Vorticity stencil of LUDVM.flowfield (LUDVM.py:1224-1292): ome = dw/dx - du/dz on the uniform
// grid, centred in the interior, one-sided on edges and corners.  u, w, ome are [nx][nz], z fastest.
// HBM-bound (reads ~4 neighbours from L2, writes one float).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
vorticity_f32(const float* u, const float* w, long long nx, long long nz, float dr, float* ome) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nx * nz) return;
  const long long i = p / nz, j = p - i * nz;
  const long long ip = i + 1 < nx ? i + 1 : i, im = i > 0 ? i - 1 : i;
  const long long jp = j + 1 < nz ? j + 1 : j, jm = j > 0 ? j - 1 : j;
  // the reference takes dx, dz from the mesh itself: (ip - im) * dr, (jp - jm) * dr
  const float dxm = (float)(ip - im) * dr;
  const float dzm = (float)(jp - jm) * dr;
  const float dw = w[ip * nz + j] - w[im * nz + j];
  const float du = u[i * nz + jp] - u[i * nz + jm];
  ome[p] = dw / dxm - du / dzm;
}

// The same stencil in float64 on rows [row0, row0 + nx) of the grid, with the mesh differences taken from the mesh
// values themselves as the reference does (x[i+1, j] - x[i-1, j] with x = xmin + i dr, LUDVM.py:1193, :1228-1229): the
// float64 flow field then equals the reference's to rounding.
__global__ void __launch_bounds__(kBlock)
vorticity_f64(const double* u, const double* w, long long nx, long long nz, long long row0, double xmin, double zmin, double dr,
              double* ome) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nx * nz) return;
  const long long i = p / nz, j = p - i * nz;
  const long long ip = i + 1 < nx ? i + 1 : i, im = i > 0 ? i - 1 : i;
  const long long jp = j + 1 < nz ? j + 1 : j, jm = j > 0 ? j - 1 : j;
  const double dxm = (xmin + (double)(row0 + ip) * dr) - (xmin + (double)(row0 + im) * dr);
  const double dzm = (zmin + (double)jp * dr) - (zmin + (double)jm * dr);
  const double dw = w[ip * nz + j] - w[im * nz + j];
  const double du = u[i * nz + jp] - u[i * nz + jm];
  ome[p] = dw / dxm - du / dzm;
}

// ---------------------------------------------------------------------------------------------
// Scalar pair sums over the sources of the velocity sum (LUDVM.py:565-566), float64 throughout: with r2 = dx^2 + dz^2,
// q = r2^2 + vc^4 (pair_f64's q), s = sqrt(q) and a = (r2 + s) / 2,
//     PSI:    psi(p)   = sum_j G_j / (4 pi) ln(a_pj)        (d psi / dz = u, -d psi / dx = w of pair_f64)
//     OMEGA:  omega(p) = -sum_j G_j vc^4 / (pi s_pj^3)      (dw/dx - du/dz of that field in closed form: a positive circulation
//                                                            turns clockwise, LUDVM.py:565-566)
// The shape of pair_f64: sources in LDS tiles, one target per lane (arrays, or grid points generated in registers), source
// splits over blockIdx.y into a ONE-column slab [split][nt_pad] that finish_scalar sums in split order.
// Ragged tiles are NOT padded: pair_f64's far-away source of zero circulation would give 0 * ln(inf) = NaN here, and no pad
// position is safe for every target when vc = 0 (a target on the pad has a = 0).  The inner loop is bounded by the tile's
// source count instead (uniform over the workgroup): a slot past the end is neither staged nor read.
// Per pair: PSI 2 sub, mul, 2 fma, rsq + 2 Newton steps (rsqrt_f64), mul, add, mul, the logarithm (log_f64 below: an fp32
// logarithm misses the test bound by 4e4), fma; OMEGA the same up to rsqrt_f64, then 2 mul, fma.
// ---------------------------------------------------------------------------------------------
// (ScalarKind, log_f64 and scalar_term, the pair term itself: scalar_term.hpp, which the march's energy kernel shares)

template <int KIND, int TILE>
__global__ void __launch_bounds__(kBlock)
pair_scalar_f64(PairArgs a) {
  __shared__ __attribute__((aligned(16))) double lx[TILE];
  __shared__ __attribute__((aligned(16))) double lz[TILE];
  __shared__ __attribute__((aligned(16))) double lg[TILE];

  const double* __restrict__ xs = static_cast<const double*>(a.xs);
  const double* __restrict__ zs = static_cast<const double*>(a.zs);
  const double* __restrict__ gs = static_cast<const double*>(a.gs);

  const int tid = threadIdx.x;
  const long long ti = (long long)blockIdx.x * kBlock + tid;
  const long long s_begin = (long long)blockIdx.y * a.chunk;
  long long s_end = s_begin + a.chunk;
  if (s_end > a.ns) s_end = a.ns;

  double xp = 0.0, zp = 0.0;
  if (ti < a.nt) {
    if (a.grid_nz > 0) {
      grid_point(a, ti, xp, zp);
    } else {
      xp = static_cast<const double*>(a.xt)[ti];
      zp = static_cast<const double*>(a.zt)[ti];
    }
  }
  double acc = 0.0;
  const double vc4 = a.vc4;

  for (long long base = s_begin; base < s_end; base += TILE) {
    const int cnt = s_end - base < TILE ? (int)(s_end - base) : TILE;      // sources of this tile (uniform)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (TILE + kBlock - 1) / kBlock; ++k) {
      const int l = tid + k * kBlock;
      if (l < cnt) {
        lx[l] = xs[base + l];
        lz[l] = zs[base + l];
        lg[l] = gs[base + l];
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) acc = __builtin_fma(lg[j], scalar_term<KIND>(xp - lx[j], zp - lz[j], vc4), acc);
  }

  if (ti < a.nt) {
    const double v = acc * (KIND == kScalarOmega ? -vc4 * kInvPiD : kInv4PiD);
    if (gridDim.y == 1) static_cast<double*>(a.u)[ti] = v;
    else static_cast<double*>(a.part)[(long long)blockIdx.y * a.nt_pad + ti] = v;
  }
}

// the splits of one target, added in split order in sum_column's fixed association
__global__ void __launch_bounds__(kBlock)
finish_scalar(const double* part, long long nt, long long nt_pad, int nsplit, double* out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < nt) out[i] = sum_column(part + i, nt_pad, nsplit);
}

// ---------------------------------------------------------------------------------------------
// Velocity gradient of the same field, float64 throughout: with y = 1 / s, three raw sums per target
//     A = sum G r2 dx dz y^3,   B = sum G r2 (dx^2 - dz^2) y^3,   C = sum G y^3
// give  du/dx = -A / pi (= -dw/dz: the field is divergence free),  du/dz = (B + vc^4 C) / (2 pi),
//       dw/dx = (B - vc^4 C) / (2 pi),  so that dw/dx - du/dz = -vc^4 C / pi is OMEGA above exactly.
// pair_scalar_f64's shape: one walk over the sources with three accumulators per target (one reciprocal square root per
// pair serves all three), the ragged tile bounded by its count (with vc = 0 no pad position is safe for every target), source
// splits into a THREE-column slab [split][3][nt_pad] of the raw sums that finish_grad adds in split order.  The outputs are
// formed once per target, by grad_outputs in both routes; `out` is [3][nt]: du/dx, du/dz, dw/dx.
// Per pair: 2 sub, mul, 2 fma, rsqrt_f64, 2 mul (y^3), mul (G y^3), add, mul (r2), mul (dx dz), fma (dx^2 - dz^2), 2 fma.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void grad_outputs(double A, double B, double C, double vc4, long long stride, double* out) {
  const double vC = vc4 * C;
  out[0] = -A * kInvPiD;
  out[stride] = (B + vC) * kInv2PiD;
  out[2 * stride] = (B - vC) * kInv2PiD;
}

template <int TILE>
__global__ void __launch_bounds__(kBlock)
pair_grad_f64(PairArgs a) {
  __shared__ __attribute__((aligned(16))) double lx[TILE];
  __shared__ __attribute__((aligned(16))) double lz[TILE];
  __shared__ __attribute__((aligned(16))) double lg[TILE];

  const double* __restrict__ xs = static_cast<const double*>(a.xs);
  const double* __restrict__ zs = static_cast<const double*>(a.zs);
  const double* __restrict__ gs = static_cast<const double*>(a.gs);

  const int tid = threadIdx.x;
  const long long ti = (long long)blockIdx.x * kBlock + tid;
  const long long s_begin = (long long)blockIdx.y * a.chunk;
  long long s_end = s_begin + a.chunk;
  if (s_end > a.ns) s_end = a.ns;

  double xp = 0.0, zp = 0.0;
  if (ti < a.nt) {
    if (a.grid_nz > 0) {
      grid_point(a, ti, xp, zp);
    } else {
      xp = static_cast<const double*>(a.xt)[ti];
      zp = static_cast<const double*>(a.zt)[ti];
    }
  }
  double sa = 0.0, sb = 0.0, sc = 0.0;
  const double vc4 = a.vc4;

  for (long long base = s_begin; base < s_end; base += TILE) {
    const int cnt = s_end - base < TILE ? (int)(s_end - base) : TILE;      // sources of this tile (uniform)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (TILE + kBlock - 1) / kBlock; ++k) {
      const int l = tid + k * kBlock;
      if (l < cnt) {
        lx[l] = xs[base + l];
        lz[l] = zs[base + l];
        lg[l] = gs[base + l];
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const double dx = xp - lx[j];
      const double dz = zp - lz[j];
      const double dxx = dx * dx;
      const double r2 = __builtin_fma(dz, dz, dxx);
      const double q = __builtin_fma(r2, r2, vc4);
      const double y = rsqrt_f64(q);
      const double c = lg[j] * (y * y * y);                 // G / s^3
      const double e = c * r2;
      sc += c;
      sa = __builtin_fma(e, dx * dz, sa);
      sb = __builtin_fma(e, __builtin_fma(-dz, dz, dxx), sb);
    }
  }

  if (ti < a.nt) {
    if (gridDim.y == 1) {
      grad_outputs(sa, sb, sc, vc4, a.nt, static_cast<double*>(a.u) + ti);
    } else {
      double* row = static_cast<double*>(a.part) + (long long)blockIdx.y * 3 * a.nt_pad + ti;
      row[0] = sa;
      row[a.nt_pad] = sb;
      row[2 * a.nt_pad] = sc;
    }
  }
}

// the three raw sums of one target, each added in split order in sum_column's fixed association, then the outputs
__global__ void __launch_bounds__(kBlock)
finish_grad(const double* part, long long nt, long long nt_pad, int nsplit, double vc4, double* out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nt) return;
  const double* col = part + i;
  grad_outputs(sum_column(col, 3 * nt_pad, nsplit), sum_column(col + nt_pad, 3 * nt_pad, nsplit),
               sum_column(col + 2 * nt_pad, 3 * nt_pad, nsplit), vc4, nt, out + i);
}

// ---------------------------------------------------------------------------------------------
// The analytic vorticity (GRAD = false: C alone) and the velocity gradient (GRAD = true: A, B, C) in hi+lo fp32: the scheme of
// hilo_field_f32 (march_kernels.hpp) on the float64 device arrays of the float64 route -- no origins, no fall-back.
//   points   a lane owns kFieldHiloPerLane targets (target b * 1024 + k * 256 + lane in register set k; arrays, or grid_point in
//            float64), each coordinate split once by split_hilo before the source loop; a lane without a point sits at
//            -kPadPosF, away from the sources' padding, and stores nothing
//   tiles    256 consecutive sources from the split's first one (`chunk` is a multiple of 256); each lane splits one source and
//            stages xh, xl, zh, zl, (float)G: five float planes.  Slots past the end are pair_f32's padding (hi = kPadPosF,
//            lo = 0, G = 0)
//   pairs    dx = (xh_p - xh_s) + (xl_p - xl_s), dz likewise, then packed fp32, two sources per v_pk_*_f32, one v_rsq_f32 per
//            pair, the sources by broadcast ds_read_b128.  With y = rsq(r2^2 + vc^4):
//                C += (G y) (y y),   e = (G y) (y r2),   A += e (y (dx dz)),   B += e (y (dx^2 - dz^2))
//            Every factor of e's products is at most about 1 whatever the distance (y r2 <= 1, y |dx dz| <= 1 / 2,
//            y |dx^2 - dz^2| <= 1) and G y is a velocity-sized number: over |coordinates| <= 1e4 with v_core >= 1e-4 no
//            intermediate leaves fp32's normal range (y in [1e-9, 1e8], y^2 in [1e-18, 1e16], r2 and |dx dz| <= 8e8); G y^3
//            formed first would flush for a far source of small circulation while its A and B terms still count.  Only the
//            C term may flush, and it enters the outputs times vc^4.
//            A pad pair adds exact zeros: r2 <= 7.2e37 and |dx dz| <= 3.6e37 stay finite (also between a lane and a slot that are
//            both padding), r2^2 overflows to +inf, y = 0, G y = 0, and every product of y meets a finite partner.
//            20 (GRAD) or 12 v_pk_*_f32 + 2 v_rsq_f32 per two pairs and point.
//   sums     two levels: a tile's terms in fp32 packed registers (even sources in the low halves, odd ones in the high halves:
//            128 terms per accumulator), then low half and high half, in that order, added to the lane's float64 sums
// Every target sees the same operations on the same operands in the same order, whichever lane, register set, row block or
// target form it arrives in.  Source splits over blockIdx.y write pair_scalar_f64's / pair_grad_f64's slab ([split][nt_pad]
// of scaled values, [split][3][nt_pad] of raw sums) for finish_scalar / finish_grad.
// ---------------------------------------------------------------------------------------------
template <bool GRAD, int PPL>
__global__ void __launch_bounds__(kBlock)
field_hilo_f32(PairArgs a) {
  static_assert(kFieldHiloTile == kBlock, "one source slot per lane");
  __shared__ __attribute__((aligned(16))) float lxh[kFieldHiloTile];
  __shared__ __attribute__((aligned(16))) float lxl[kFieldHiloTile];
  __shared__ __attribute__((aligned(16))) float lzh[kFieldHiloTile];
  __shared__ __attribute__((aligned(16))) float lzl[kFieldHiloTile];
  __shared__ __attribute__((aligned(16))) float lg[kFieldHiloTile];

  const double* __restrict__ xs = static_cast<const double*>(a.xs);
  const double* __restrict__ zs = static_cast<const double*>(a.zs);
  const double* __restrict__ gs = static_cast<const double*>(a.gs);

  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * (kBlock * PPL) + tid;
  const long long s_begin = (long long)blockIdx.y * a.chunk;
  long long s_end = s_begin + a.chunk;
  if (s_end > a.ns) s_end = a.ns;

  const float vc4s = (float)a.vc4;
  const f32x2 vc4p = {vc4s, vc4s};
  f32x2 xph[PPL], xpl[PPL], zph[PPL], zpl[PPL];
  double sa[PPL], sb[PPL], sc[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long ti = t0 + (long long)k * kBlock;
    double xd = -(double)kPadPosF, zd = -(double)kPadPosF;
    if (ti < a.nt) {
      if (a.grid_nz > 0) {
        grid_point(a, ti, xd, zd);
      } else {
        xd = static_cast<const double*>(a.xt)[ti];
        zd = static_cast<const double*>(a.zt)[ti];
      }
    }
    float h, l;
    split_hilo(xd, h, l);
    xph[k] = (f32x2){h, h}; xpl[k] = (f32x2){l, l};
    split_hilo(zd, h, l);
    zph[k] = (f32x2){h, h}; zpl[k] = (f32x2){l, l};
    sa[k] = 0.0; sb[k] = 0.0; sc[k] = 0.0;
  }

  for (long long base = s_begin; base < s_end; base += kFieldHiloTile) {
    __syncthreads();                                // previous tile fully consumed
    {
      const long long si = base + tid;
      float xh = kPadPosF, xl = 0.0f, zh = kPadPosF, zl = 0.0f, g = 0.0f;
      if (si < s_end) {
        split_hilo(xs[si], xh, xl);
        split_hilo(zs[si], zh, zl);
        g = (float)gs[si];
      }
      lxh[tid] = xh; lxl[tid] = xl; lzh[tid] = zh; lzl[tid] = zl; lg[tid] = g;
    }
    __syncthreads();
    f32x2 ta[PPL], tb[PPL], tc[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) { ta[k] = (f32x2){0.0f, 0.0f}; tb[k] = (f32x2){0.0f, 0.0f}; tc[k] = (f32x2){0.0f, 0.0f}; }
#pragma unroll 2
    for (int j = 0; j < kFieldHiloTile; j += 4) {
      const f32x4 X = *reinterpret_cast<const f32x4*>(&lxh[j]);
      const f32x4 XL = *reinterpret_cast<const f32x4*>(&lxl[j]);
      const f32x4 Z = *reinterpret_cast<const f32x4*>(&lzh[j]);
      const f32x4 ZL = *reinterpret_cast<const f32x4*>(&lzl[j]);
      const f32x4 G = *reinterpret_cast<const f32x4*>(&lg[j]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x2 xs2 = h ? (f32x2){X.z, X.w} : (f32x2){X.x, X.y};
        const f32x2 xl2 = h ? (f32x2){XL.z, XL.w} : (f32x2){XL.x, XL.y};
        const f32x2 zs2 = h ? (f32x2){Z.z, Z.w} : (f32x2){Z.x, Z.y};
        const f32x2 zl2 = h ? (f32x2){ZL.z, ZL.w} : (f32x2){ZL.x, ZL.y};
        const f32x2 gs2 = h ? (f32x2){G.z, G.w} : (f32x2){G.x, G.y};
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
          const f32x2 dx = (xph[k] - xs2) + (xpl[k] - xl2);
          const f32x2 dz = (zph[k] - zs2) + (zpl[k] - zl2);
          const f32x2 dxx = dx * dx;
          const f32x2 r2 = __builtin_elementwise_fma(dz, dz, dxx);
          const f32x2 q = __builtin_elementwise_fma(r2, r2, vc4p);
          const f32x2 y = {__builtin_amdgcn_rsqf(q.x), __builtin_amdgcn_rsqf(q.y)};
          const f32x2 gy = gs2 * y;
          tc[k] = __builtin_elementwise_fma(gy, y * y, tc[k]);
          if (GRAD) {
            const f32x2 e = gy * (y * r2);
            ta[k] = __builtin_elementwise_fma(e, y * (dx * dz), ta[k]);
            tb[k] = __builtin_elementwise_fma(e, y * __builtin_elementwise_fma(-dz, dz, dxx), tb[k]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      sc[k] += (double)tc[k].x; sc[k] += (double)tc[k].y;
      if (GRAD) {
        sa[k] += (double)ta[k].x; sa[k] += (double)ta[k].y;
        sb[k] += (double)tb[k].x; sb[k] += (double)tb[k].y;
      }
    }
  }

#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long ti = t0 + (long long)k * kBlock;
    if (ti >= a.nt) continue;
    if (GRAD) {
      if (gridDim.y == 1) {
        grad_outputs(sa[k], sb[k], sc[k], a.vc4, a.nt, static_cast<double*>(a.u) + ti);
      } else {
        double* row = static_cast<double*>(a.part) + (long long)blockIdx.y * 3 * a.nt_pad + ti;
        row[0] = sa[k];
        row[a.nt_pad] = sb[k];
        row[2 * a.nt_pad] = sc[k];
      }
    } else {
      const double v = sc[k] * (-a.vc4 * kInvPiD);
      if (gridDim.y == 1) static_cast<double*>(a.u)[ti] = v;
      else static_cast<double*>(a.part)[(long long)blockIdx.y * a.nt_pad + ti] = v;
    }
  }
}

}  // namespace ludvm
