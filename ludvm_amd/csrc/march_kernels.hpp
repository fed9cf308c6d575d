// Device-resident time march (LUDVM.time_loop, reference LUDVM.py:597-1171, 'Faure' method): the per-step
// solve that the per-step path does on the host runs here, so consecutive time steps can be enqueued without
// a host round trip.  All of it is float64 and small (Npanels = 80 chord points, Ncoeffs = 30): one
// workgroup per step.
//
// Per time step i the device runs, in this order,
//   pair_f64_few        fp64 partial sums of the wake at Npanels + 3 targets: the chord points of step i
//                       (:746, :921), the two points where step i will shed its TEV and candidate LEV, and the
//                       origin (where the reference keeps a zero-strength LEV slot that it convects, :1112-1118)
//   march_chord_finish  sums the partials; unit influences of those two vortices at the chord points
//                       (:751, :926-931)                                              -> MarchState
//   march_solve         T1/T2/T3 downwash rows, Gamma_TEV (and Gamma_LEV when |A0| reaches LESPcrit), Fourier
//                       coefficients, bound vorticity, loads; appends the shed vortices and stages the bound
//                       vortices behind the wake                                     (:743-1090)
//   roll-up             (:1095-1127) the pair kernels of pair_kernels.hpp / pair_sym_kernels.hpp with the wake
//                       size taken from MarchState; their Euler finisher also places the TEV / LEV of step i + 1
//                       (:680-681, :797-800) and stages its chord points (TailDuty)
// Round 6 (profiles/r06_march_chain_ab.txt): the waves of the first three raise their issue priority (they run beside a roll-up
// kernel that keeps every SIMD busy) and march_solve's ~14 dependent workgroup reductions are done in 2 rounds (3 with
// 'Ramesh'), each value by the same tree: the same bits, config 2 -0.07 s.  Measured and dropped: summing the slabs inside
// march_solve with 12 helper wavefronts (a 1024-thread workgroup has to find a whole CU free: config 2 +1.2 s) and
// 64-source tiles for the chord sums (more slabs than the shorter walks save).
// Once the wake is large enough for the symmetric kernel the first three run on a second stream BESIDE the bulk of
// the roll-up: old wake on old wake depends only on the positions after the previous roll-up, not on this step's
// solve.  The shed vortices are then handled apart: what the old wake induces on them comes from the two extra
// targets of the chord launch, what they induce on the old wake is added by march_finish_sym.
#pragma once
#include <hip/hip_runtime.h>
#include "pair_kernels.hpp"
#include "pair_sym_kernels.hpp"
#include "march_types.hpp"
#include "scalar_term.hpp"

namespace ludvm {

// Sum v over the workgroup (fixed tree: wavefront shuffles, then the 4 wave partials in order); every thread
// gets the result.  `scratch` holds kBlock / 64 doubles.
__device__ __forceinline__ double block_sum(double v, double* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// K sums at once, each by block_sum's tree (the same bits per value): one pair of barriers for all of them instead of one
// pair each -- march_solve is a chain of reductions, and two barriers + six dependent shuffles per value were most of its
// time.  `scratch` holds 4 K doubles.
template <int K>
__device__ __forceinline__ void block_sum_n(double (&v)[K], double* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_down(v[k], off, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) scratch[4 * k + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (scratch[4 * k] + scratch[4 * k + 1]) + (scratch[4 * k + 2] + scratch[4 * k + 3]);
}

// 2x2 solve as LAPACK's dgesv does it (partial pivoting), so that the result has the rounding of
// np.linalg.solve in the reference (:944-954).
__device__ __forceinline__ void solve2(double a00, double a01, double a10, double a11, double b0, double b1, double& x0,
                                       double& x1) {
  if (fabs(a10) > fabs(a00)) {
    double t;
    t = a00; a00 = a10; a10 = t;
    t = a01; a01 = a11; a11 = t;
    t = b0; b0 = b1; b1 = t;
  }
  const double l = a10 / a00;
  const double u11 = a11 - l * a01;
  const double y1 = b1 - l * b0;
  x1 = y1 / u11;
  x0 = (b0 - a01 * x1) / a00;
}

// Vatistas pair: velocity at (xp, zp) per unit circulation of a vortex at (xs, zs)
__device__ __forceinline__ void unit_pair_f64(double xp, double zp, double xs, double zs, double vc4, double& u, double& w) {
  const double dx = xp - xs, dz = zp - zs;
  const double r2 = __builtin_fma(dz, dz, dx * dx);
  const double s = kInv2PiD * rsqrt_f64(__builtin_fma(r2, r2, vc4));
  u = dz * s;
  w = -dx * s;
}

// 'Ramesh' residuals.  The downwash is linear in the circulations being solved for, W = T1 + gt T2 + gl T3, so the
// reference's residual  U c pi (A0 + A1 / 2) + kelvin + (gt + gl)  with A0, A1 projected from W (:692-700, :820-835)
// needs only the six projections p0[k] = cproj[0] . T_k / U, p1[k] = cproj[1] . T_k / U.
struct RameshProj { double p0[3], p1[3], ucpi, kelvin; };
__device__ __forceinline__ double ramesh_res(const RameshProj& r, double gt, double gl, double& A0) {
  A0 = r.p0[0] + gt * r.p0[1] + gl * r.p0[2];
  const double A1 = r.p1[0] + gt * r.p1[1] + gl * r.p1[2];
  return r.ucpi * (A0 + A1 / 2) + r.kelvin + (gt + gl);
}
// Newton with a forward-difference slope, start -1, as the reference iterates it (:683-739)
__device__ __forceinline__ double ramesh_tev(const RameshProj& r, double maxerror, int maxiter, double eps) {
  double f = 1.0, g = -1.0, A0;
  int niter = 1;
  while (fabs(f) > maxerror && niter < maxiter) {
    f = ramesh_res(r, g, 0.0, A0);
    const double fd = ramesh_res(r, g + eps, 0.0, A0);
    g = g - f / ((fd - f) / eps);
    niter += 1;
  }
  return g;
}
// 2x2 Newton for (Gamma_LEV, Gamma_TEV) with the LESP condition as second equation (:807-914)
__device__ __forceinline__ void ramesh_tev_lev(const RameshProj& r, double lesp_crit, double guess, double maxerror, int maxiter,
                                               double eps, double& g_tev, double& g_lev) {
  g_tev = guess; g_lev = guess;
  double f1 = 0.1, f2 = 0.1;
  int niter = 1;
  while ((fabs(f1) > maxerror || fabs(f2) > maxerror) && niter < maxiter) {
    double A0;
    f1 = ramesh_res(r, g_tev, g_lev, A0);
    f2 = lesp_crit - A0;
    const double f1t = ramesh_res(r, g_tev + eps, g_lev, A0);
    const double f2t = lesp_crit - A0;
    const double f1l = ramesh_res(r, g_tev, g_lev + eps, A0);
    const double f2l = lesp_crit - A0;
    double dl, dt_;
    solve2((f1l - f1) / eps, (f1t - f1) / eps, (f2l - f2) / eps, (f2t - f2) / eps, f1, f2, dl, dt_);
    g_lev -= dl;
    g_tev -= dt_;
    niter += 1;
  }
}

// Start of a march call: the caller supplied the placements of the first step; stage its targets, and sum |Gamma|
// over the wake as it stands (fixed order) for the symmetric kernel's fixed-point scale.
__global__ void __launch_bounds__(kBlock)
march_begin(MarchState* S, const double* kin, int npan, int slot, const double* g64, double vc4) {
  __shared__ double part[kBlock / 64];
  const int t = threadIdx.x;
  const int ntt = npan + 3;
  const long long n = S->n;
  double a = 0.0;
  for (long long i = t; i < n; i += kBlock) a += fabs(g64[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((t & 63) == 0) part[t >> 6] = a;
  __syncthreads();
  if (t < npan) { S->tgt[t] = kin[7 + t]; S->tgt[ntt + t] = kin[7 + npan + t]; }
  if (t == 0) {
    S->tgt[npan] = S->place[0]; S->tgt[npan + 1] = S->place[1]; S->tgt[npan + 2] = 0.0;
    S->tgt[ntt + npan] = S->place[2]; S->tgt[ntt + npan + 1] = S->place[3]; S->tgt[ntt + npan + 2] = 0.0;
    S->n_old[slot] = n;
    const double tot = (part[0] + part[1]) + (part[2] + part[3]);
    S->sum_abs_g = tot;
    S->sym_bad = 0;
    sym_scale_from_sum(tot, vc4, &S->sc[slot], &S->sym_bad);
    S->sc[slot ^ 1] = S->sc[slot];
  }
}

// Sums the fp64 partial slabs of the chord launch (one WAVEFRONT per output column, fixed shuffle tree) and
// evaluates the unit influences of the coming TEV / candidate LEV at the chord points.  Columns: component k
// (0: u, 1: w) x target p; p < npan is a chord point, p = npan, npan + 1 the two placements, npan + 2 the origin.
__global__ void __launch_bounds__(kBlock)
march_chord_finish(const double* part, long long nt_pad, int nsplit, const double* direct_u, int npan, MarchState* S,
                   double vc4) {
  __builtin_amdgcn_s_setprio(3);                 // (see march_solve)
  const long long gtid = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long col = gtid >> 6;
  const int lane = threadIdx.x & 63;
  const int ntt = npan + 3;
  if (col >= 2 * ntt) return;   // whole wavefronts leave together
  const int k = (int)(col / ntt), p = (int)(col - (long long)k * ntt);
  double acc = 0.0;
  if (part != nullptr) {
    const double* c0 = part + k * nt_pad + p;
    for (int sidx = lane; sidx < nsplit; sidx += 64) acc += c0[(long long)sidx * 2 * nt_pad];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  } else if (nsplit == 1) {
    acc = direct_u[k * nt_pad + p];
  }
  if (lane != 0) return;
  if (p >= npan) {
    S->pvel[k * 3 + (p - npan)] = acc;
    return;
  }
  double* out = S->chord;
  out[k * npan + p] = acc;
  // unit vortex k (0: TEV, 1: LEV candidate) at chord point p
  double uu, ww;
  unit_pair_f64(S->tgt[p], S->tgt[ntt + p], S->place[k], S->place[2 + k], vc4, uu, ww);
  out[2 * npan + (k * 2 + 0) * npan + p] = uu;
  out[2 * npan + (k * 2 + 1) * npan + p] = ww;
}

// One workgroup.  kin = this step's kinematics row [alpha, alpha_dot, h_dot, te_x, te_z, le_x, le_z,
// xg[npan], zg[npan]]; row = this step's output row (kMarchRowHead + 2 ncoef + 2 npan doubles);
// progress (host-mapped, may be null) receives (step << 32 | n) so the host can bound the wake size of the
// steps it enqueues next without synchronizing.
__global__ void __launch_bounds__(kBlock)
march_solve(MarchSetup m, MarchState* S, const double* kin, double* row, long long step, double* x64, double* z64,
            double* g64, Mirrors mir, float* g32, unsigned long long* progress) {
  __shared__ double Wn[kMarchMaxPan];
  __shared__ double A[kMarchMaxCoef], Ad[kMarchMaxCoef];
  __shared__ double scratch[4 * 8];
  // the chain runs beside a roll-up kernel that keeps every SIMD's issue slots busy: its few waves go first
  __builtin_amdgcn_s_setprio(3);
  const int j = threadIdx.x;
  const int npan = m.npan, ncoef = m.ncoef;
  const bool on = j < npan;
  const double pi = 3.14159265358979323846;
  const double al = kin[0], ald = kin[1], hd = kin[2];
  const double ca = cos(al), sa = sin(al);
  const double* xg = kin + 7;
  const double* zg = kin + 7 + npan;

  // what the solve reads of the state, before anything is rewritten
  const long long n0 = S->n;
  const double tev_x = S->place[0], lev_x = S->place[1], tev_z = S->place[2], lev_z = S->place[3];
  const double pu0 = S->pvel[0], pu1 = S->pvel[1], pw0 = S->pvel[3], pw1 = S->pvel[4];
  const double puo = S->pvel[2], pwo = S->pvel[5];

  double u1 = 0, w1 = 0, ut1 = 0, wt1 = 0, ul1 = 0, wl1 = 0, dedx = 0, cm1 = 0, wq = 0;
  if (on) {
    u1 = S->chord[j]; w1 = S->chord[npan + j];
    ut1 = S->chord[2 * npan + j]; wt1 = S->chord[3 * npan + j];
    ul1 = S->chord[4 * npan + j]; wl1 = S->chord[5 * npan + j];
    dedx = m.detadx[j]; cm1 = m.cm1[j]; wq = m.wq[j];
  }
  // chord frame (:586-587) and the downwash rows: T1 from the existing wake + kinematics (:588-593), T2 / T3
  // from the unit TEV / LEV (only the induced part enters)
  double t1 = 0, t2 = 0, t3 = 0;
  if (on) {
    const double u = u1 * ca - w1 * sa, w = u1 * sa + w1 * ca;
    t1 = dedx * (m.U * ca + hd * sa + u - ald * m.eta[j]) - m.U * sa - ald * (m.xpan[j] - m.piv) + hd * ca - w;
    const double ut = ut1 * ca - wt1 * sa, un = ut1 * sa + wt1 * ca;
    t2 = dedx * ut - un;
    const double ult = ul1 * ca - wl1 * sa, uln = ul1 * sa + wl1 * ca;
    t3 = dedx * ult - uln;
  }
  // the six chord integrals at once (I3 and the J's are needed on shedding steps only: summed anyway, one pair of barriers)
  double ij[6] = {t1 * cm1, t2 * cm1, t3 * cm1, t1 * wq, t2 * wq, t3 * wq};
  block_sum_n<6>(ij, scratch);
  const double I1 = ij[0], I2 = ij[1];
  const double kelvin = S->sum_tev + S->sum_lev + m.kelvin0;
  const bool ramesh = m.method == 1;
  RameshProj rp{};
  double g_tev;
  if (ramesh) {
    const double c0 = on ? m.cproj[j] / m.U : 0.0, c1 = on ? m.cproj[npan + j] / m.U : 0.0;
    double pr[6] = {t1 * c0, t2 * c0, t3 * c0, t1 * c1, t2 * c1, t3 * c1};
    block_sum_n<6>(pr, scratch);
    rp.p0[0] = pr[0]; rp.p0[1] = pr[1]; rp.p0[2] = pr[2];
    rp.p1[0] = pr[3]; rp.p1[1] = pr[4]; rp.p1[2] = pr[5];
    rp.ucpi = m.U * m.chord * pi;
    rp.kelvin = kelvin;
    g_tev = ramesh_tev(rp, m.maxerror, m.maxiter, m.epsilon);
  } else {
    g_tev = -(I1 + kelvin) / (1 + I2);               // :758-760
  }
  double g_lev = 0.0;
  if (on) Wn[j] = (t1 + g_tev * t2) / m.U;
  __syncthreads();
  if (j < ncoef) {
    double acc = 0.0;
    const double* cp = m.cproj + (long long)j * npan;
    for (int q = 0; q < npan; ++q) acc = __builtin_fma(cp[q], Wn[q], acc);
    A[j] = acc;
    Ad[j] = (acc - S->prevA[j]) / m.dt;              // :772-773
  }
  __syncthreads();
  const double ucpi = m.U * m.chord * pi;
  double bound = ramesh ? ucpi * (A[0] + A[1] / 2) : I1 + g_tev * I2;     // :761 / :738
  const double lesp_prev = A[0];
  double lesp_crit = S->lesp_crit;
  const bool shed = fabs(A[0]) >= fabs(lesp_crit);   // :781
  __syncthreads();                                   // everyone has read A[0] before it is rewritten
  if (shed) {
    lesp_crit = A[0] < 0 ? -fabs(lesp_crit) : fabs(lesp_crit);     // :802-805
    const double I3 = ij[2];
    const double J1 = -1 / pi * ij[3];
    const double J2 = -1 / pi * ij[4];
    const double J3 = -1 / pi * ij[5];
    if (ramesh) ramesh_tev_lev(rp, lesp_crit, g_tev, m.maxerror, m.maxiter, m.epsilon, g_tev, g_lev);
    else solve2(1 + I2, 1 + I3, J2, J3, -(I1 + kelvin), lesp_crit - J1, g_tev, g_lev);   // :944-954
    if (on) Wn[j] = (t1 + g_tev * t2 + g_lev * t3) / m.U;
    __syncthreads();
    if (j < ncoef) {
      double acc = 0.0;
      const double* cp = m.cproj + (long long)j * npan;
      for (int q = 0; q < npan; ++q) acc = __builtin_fma(cp[q], Wn[q], acc);
      // 'Faure' takes A0 from the LESP form (:959); derivatives keep their values in both methods (:963-966)
      A[j] = (j == 0 && !ramesh) ? J1 + g_tev * J2 + g_lev * J3 : acc;
    }
    __syncthreads();
    bound = ramesh ? ucpi * (A[0] + A[1] / 2) : I1 + g_tev * I2 + g_lev * I3;
  }

  // bound vorticity per panel (:987-1010)
  double gamma = 0.0, dgamma = 0.0;
  if (on) {
    double ssum = 0.0;
    for (int q = 1; q < ncoef; ++q) ssum = __builtin_fma(A[q], m.ssin[(long long)(q - 1) * npan + j], ssum);
    gamma = 2 * m.U * (A[0] * m.opcs[j] + ssum);
    dgamma = gamma * m.hcsd[j];
  }
  const int k = shed ? 2 : 1;
  // One more round of sums: the loads (:1035-1090; tangential velocity on the chord from the whole wake by linearity), and
  // the velocity of the vortices shed now, for the roll-up that treats them apart (:1105-1124 restricted to them): the
  // wake's part came with the chord sums; the bound vortices' part is summed here; plus each other.
  // The reference convects LEV slot `ilev` -- zero strength, at the origin -- on a step that sheds no LEV and stores
  // where it lands in path['LEV'][i] (:1112-1118); its velocity: wake (chord launch), the new TEV, the bound vortices.
  double r8[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // fn, m, fu0, fw0, fu1, fw1, fuo, fwo
  if (on) {
    const double uc1 = u1 + g_tev * ut1 + (shed ? g_lev * ul1 : 0.0);
    const double wc1 = w1 + g_tev * wt1 + (shed ? g_lev * wl1 : 0.0);
    const double u = uc1 * ca - wc1 * sa;
    r8[0] = u * gamma * m.wx[j];
    r8[1] = u * gamma * m.xpan[j] * m.wx[j];
    double uu, ww;
    unit_pair_f64(tev_x, tev_z, xg[j], zg[j], m.vc4, uu, ww);
    r8[2] = dgamma * uu; r8[3] = dgamma * ww;
    if (shed) {
      unit_pair_f64(lev_x, lev_z, xg[j], zg[j], m.vc4, uu, ww);
      r8[4] = dgamma * uu; r8[5] = dgamma * ww;
    } else {
      unit_pair_f64(0.0, 0.0, xg[j], zg[j], m.vc4, uu, ww);
      r8[6] = dgamma * uu; r8[7] = dgamma * ww;
    }
  }
  block_sum_n<8>(r8, scratch);
  const double fn_sum = r8[0], m_sum = r8[1];
  const double su0 = r8[2], sw0 = r8[3], su1 = r8[4], sw1 = r8[5], suo = r8[6], swo = r8[7];
  __syncthreads();                                   // all reads of S are done; it is rewritten below

  // Local-origin mirrors of the entries written now -- wake index n0 (TEV), n0 + 1 (LEV when shed), then the npan
  // bound vortices: an origin class (256-vortex block x index parity) whose first member is among them takes its origin
  // from the entry written there, the others keep the origin the last Euler finisher gave them.
  auto origin_of = [&](long long i, float& ox, float& oz) {
    const long long b = i >> kOriginShift, cs = (b << kOriginShift) + (i & 1), slot = origin_slot(i);
    if (cs >= n0) {
      double bx, bz;
      if (cs == n0) { bx = tev_x; bz = tev_z; }
      else if (shed && cs == n0 + 1) { bx = lev_x; bz = lev_z; }
      else { bx = xg[cs - n0 - k]; bz = zg[cs - n0 - k]; }
      ox = (float)bx; oz = (float)bz;
      if (i == cs) { mir.cx[slot] = ox; mir.cz[slot] = oz; }
      // a block opened by the very last entry written now: its still empty odd class gets a number too
      if (i == cs && (i & 1) == 0 && i == n0 + k + npan - 1) { mir.cx[slot + 1] = ox; mir.cz[slot + 1] = oz; }
    } else {
      ox = mir.cx[slot]; oz = mir.cz[slot];
    }
  };

  if (j == 0) {
    const double c = m.chord, U = m.U, rho = m.rho;
    const double A0 = A[0], A1 = A[1], A2 = A[2];
    const double A0d = Ad[0], A1d = Ad[1], A2d = Ad[2], A3d = Ad[3];
    const double Ueff = U * ca + hd * sa;
    const double Fn = rho * pi * c * U * (Ueff * (A0 + 0.5 * A1) + c * (3.0 / 4 * A0d + 1.0 / 4 * A1d + 1.0 / 8 * A2d))
        + rho * fn_sum;
    const double Fs = rho * pi * c * U * U * A0 * A0;
    const double M = m.piv * Fn - rho * pi * c * c * U * (Ueff * (1.0 / 4 * A0 + 1.0 / 4 * A1 - 1.0 / 8 * A2)
        + c * (7.0 / 16 * A0d + 3.0 / 16 * A1d + 1.0 / 16 * A2d - 1.0 / 64 * A3d)) - rho * m_sum;
    row[0] = g_tev; row[1] = g_lev; row[2] = shed ? 1.0 : 0.0; row[3] = bound; row[4] = lesp_prev; row[5] = A0;
    row[6] = Fn; row[7] = Fs; row[8] = M; row[9] = (double)n0;
    row[10] = 0.0; row[11] = 0.0;
    if (!shed) {
      double uu, ww;
      unit_pair_f64(0.0, 0.0, tev_x, tev_z, m.vc4, uu, ww);
      row[10] = puo + suo + g_tev * uu;
      row[11] = pwo + swo + g_tev * ww;
    }
    // the shed vortices join the wake (:1095-1098)
    float ox, oz;
    origin_of(n0, ox, oz);
    x64[n0] = tev_x; z64[n0] = tev_z; g64[n0] = g_tev;
    store_mirrors(mir, n0, tev_x, tev_z, ox, oz); g32[n0] = (float)g_tev;
    double m01u = 0, m01w = 0, m10u = 0, m10w = 0;   // TEV <- LEV, LEV <- TEV
    if (shed) {
      const long long n1 = n0 + 1;
      origin_of(n1, ox, oz);
      x64[n1] = lev_x; z64[n1] = lev_z; g64[n1] = g_lev;
      store_mirrors(mir, n1, lev_x, lev_z, ox, oz); g32[n1] = (float)g_lev;
      double uu, ww;
      unit_pair_f64(tev_x, tev_z, lev_x, lev_z, m.vc4, uu, ww);
      m01u = g_lev * uu; m01w = g_lev * ww;
      unit_pair_f64(lev_x, lev_z, tev_x, tev_z, m.vc4, uu, ww);
      m10u = g_tev * uu; m10w = g_tev * ww;
    }
    S->newv[0] = tev_x; S->newv[1] = lev_x; S->newv[2] = tev_z; S->newv[3] = lev_z;
    S->newv[4] = g_tev; S->newv[5] = shed ? g_lev : 0.0;
    S->newvel[0] = pu0 + su0 + m01u; S->newvel[2] = pw0 + sw0 + m01w;
    S->newvel[1] = pu1 + su1 + m10u; S->newvel[3] = pw1 + sw1 + m10w;
    S->n = n0 + k;
    S->itev += 1;
    S->ilev += shed ? 1 : 0;
    S->shed = shed ? 1 : 0;
    S->tail = k;
    S->lesp_crit = lesp_crit;
    S->sum_tev += g_tev;
    S->sum_lev += g_lev;
    const double sabs = S->sum_abs_g + fabs(g_tev) + fabs(g_lev);
    S->sum_abs_g = sabs;
    sym_scale_from_sum(sabs, m.vc4, &S->sc[(step + 1) & 1], &S->sym_bad);
    if (progress) {
      __atomic_store_n(progress + (step % kProgressRing), ((unsigned long long)step << 32) | (unsigned long long)(n0 + k),
                       __ATOMIC_RELAXED);
    }
  }
  if (j < ncoef) {
    S->prevA[j] = A[j];
    row[kMarchRowHead + j] = A[j];
    row[kMarchRowHead + ncoef + j] = Ad[j];
  }
  if (on) {
    row[kMarchRowHead + 2 * ncoef + j] = gamma;
    row[kMarchRowHead + 2 * ncoef + npan + j] = dgamma;
    // bound vortices ride behind the wake as sources of the roll-up (:1106, :1115, :1124)
    const long long i = n0 + k + j;
    const double x = xg[j], z = zg[j];
    float ox, oz;
    origin_of(i, ox, oz);
    x64[i] = x; z64[i] = z; g64[i] = dgamma;
    store_mirrors(mir, i, x, z, ox, oz); g32[i] = (float)dgamma;
  }
}

// Euler finisher of the overlapped roll-up.  The symmetric kernel ran on the wake as it was BEFORE this step's
// solve ([0, n_old), raw fixed-point sums in acc_u / acc_w, scale sc); here every old vortex also feels the vortices
// shed this step (S->newv) and the bound vortices (staged at [n, n + nfoil)), and the shed vortices move with the
// velocities march_solve left in S->newvel.  The raw sums are zeroed after use, so the accumulators need no memset
// between steps.  One workgroup = one origin block (see finish_wake_advect).
__global__ void __launch_bounds__(kFinBlock)
march_finish_sym(long long* acc_u, long long* acc_w, const SymScale* sc, MarchState* S, const long long* n_old_p,
                 int nfoil, float vc4, double dt, double* x64, double* z64, Mirrors m, const float* g32, TailDuty td,
                 long long* bad_step = nullptr, long long* bad_next = nullptr) {
  // bad_step / bad_next (sharded roll-up): this step's count of non-finite partial sums, summed over all owners by
  // the all-reduce that also summed acc_u / acc_w, and the next step's counter, cleared here; S->sym_bad keeps it
  __shared__ float org[4];
  const bool bad = S->sym_bad != 0 || (bad_step && *bad_step != 0);
  const long long n = S->n, n_old = *n_old_p;
  const int k = (int)(n - n_old);
  tail_duty_block0(td, n);
  const long long i = (long long)blockIdx.x * kFinBlock + threadIdx.x;
  const bool on = i < n, old = i < n_old;
  const double xo = on ? x64[i] : 0.0, zo = on ? z64[i] : 0.0;
  float fu, fw;
  staged_sources_on(old, xo, zo, x64, z64, g32, n, nfoil, vc4, fu, fw, k, S->newv);
  double xn = 0.0, zn = 0.0;
  if (on) {
    double su, sw;
    if (old) {
      const float s = (float)kInv2PiD;
      su = (double)((fx_read(acc_u, i, sc, bad) + fu) * s);
      sw = (double)(-(fx_read(acc_w, i, sc, bad) + fw) * s);
      acc_u[i] = 0;
      acc_w[i] = 0;
    } else {
      const int q = (int)(i - n_old);
      su = S->newvel[q];
      sw = S->newvel[2 + q];
    }
    xn = xo + dt * su;
    zn = zo + dt * sw;
    publish_origins(m, i, n, xn, zn, org);
  }
  __syncthreads();
  if (bad_step && blockIdx.x == 0 && threadIdx.x == 0) {
    if (bad) S->sym_bad = 1;       // (every block has read S->sym_bad OR *bad_step: both say the same from here on)
    *bad_next = 0;
  }
  if (!on) return;
  x64[i] = xn;
  z64[i] = zn;
  store_mirrors(m, i, xn, zn, org[i & 1], org[2 + (i & 1)]);
  tail_duty(td, i, n, xn, zn);
}

// ---- velocity probes (ludvm_march_set_probes) ---------------------------------------------------------------------------------
// For time step i >= 1 and probe point p, (u, w)_i(p) is the field that convects the wake in step i, evaluated at p: the
// reference's  induced_velocity(circulation_wake, xw, zw, p) + induced_velocity(circulation_foil, xa, za, p)  of
// LUDVM.py:1095-1106 with xp, zp = p -- the wake BEFORE the Euler update of step i, the vortices shed in step i at their
// placement, the bound vortices of step i at airfoil_gamma_points[i]; Vatistas core, no freestream term; a probe that
// coincides with a vortex gets 0 from it (dx = dz = 0 against a finite core).  Right after march_solve of step i those
// sources are ONE contiguous range [0, S->n + nfoil) of x64 / z64 / g64, and nothing moves them before the roll-up's
// finisher, which the probe kernels precede in stream order (ludvm_march_run).  Always float64, like the chord sums.
//
// march_probe_partial  grid = probe tiles (64 probes: one per lane of a one-wavefront workgroup) x source splits; every lane
//                      walks its split's sources in order from LDS tiles (all lanes read the same address: a broadcast),
//                      its probe's position -- with the step's x offset added -- in registers; the source count is read on
//                      the device; (split, probe) partial sums go to a slab [split][2][p_pad]
// march_probe_finish   one wavefront per output column (component x probe): splits lane, lane + 64, ... then the fixed
//                      shuffle tree of march_chord_finish; writes the step's row of the call's probe buffer
// The splits are a function of the probe count and of the step's anchor-derived bound alone (observer_plan, plan_rule.hpp),
// and every partial sum is formed by one lane in source order: the bits do not depend on how a run is cut into calls.
//
// ---- what every marched observer is made of ------------------------------------------------------------------------------------
// A partial kernel (probes, tracers, survey; float64, fp32 on local origins, hi+lo fp32) is a point loader, one field body
// and observer_store; grid = point tiles x source splits, the slab [split][2][pad] is the observer's own.  A workgroup of
// LANES lanes owns LANES x PPL points: point  blockIdx.x * LANES * PPL + k * LANES + lane  in register set k of the lane.
// A body (field_f64, local_field_f32, hilo_field_f32) takes the lane's PPL points (xp, zp: float64) against the sources
// [s_begin, s_end) -> au += sum G dz / sqrt(r^4 + vc^4), aw += sum G dx / sqrt(..) (no 1 / 2 pi, no sign); every lane of the
// workgroup calls it (barriers inside).  One lane forms a partial sum in source order, then tile order.
constexpr int kProbeLanes = 64;
constexpr int kFieldTile = 256;                    // sources per LDS tile of field_f64

template <int PPL, int LANES>
__device__ __forceinline__ long long observer_point(int k) {
  return ((long long)blockIdx.x * (LANES * PPL) + threadIdx.x) + (long long)k * LANES;
}

// the sources of split blockIdx.y: [s_begin, s_end) of the step's [0, S->n + nfoil), the count read on the device
struct SplitRange { long long begin, end; };
__device__ __forceinline__ SplitRange split_range(const MarchState* S, int nfoil, long long chunk) {
  const long long ns = S->n + nfoil;               // old wake + shed vortices + staged bound vortices
  const long long s_begin = (long long)blockIdx.y * chunk;
  long long s_end = s_begin + chunk;
  if (s_end > ns) s_end = ns;
  return {s_begin, s_end};
}

// points that stay where they are: (px[m] + the step's shift, pz[m]) and zero sums; a lane without a point walks along at
// `absent`
template <int PPL, int LANES>
__device__ __forceinline__ void load_fixed_points(const double* __restrict__ px, const double* __restrict__ pz, const double* shift,
                                                  long long count, double absent, double (&xp)[PPL], double (&zp)[PPL],
                                                  double (&au)[PPL], double (&aw)[PPL]) {
  const double sh = shift ? *shift : 0.0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long m = observer_point<PPL, LANES>(k);
    const bool on = m < count;
    xp[k] = on ? px[m] + sh : absent;
    zp[k] = on ? pz[m] : absent;
    au[k] = 0.0; aw[k] = 0.0;
  }
}

// the lane's rows of split blockIdx.y's slab, for the points that on(k, m) says it has (a split past the end of the sources
// leaves exact zeros: the finisher sums every split of the launch)
template <int PPL, int LANES, class On>
__device__ __forceinline__ void observer_store(double* slab, long long pad, On on, const double (&au)[PPL], const double (&aw)[PPL]) {
  double* row = slab + (long long)blockIdx.y * 2 * pad;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long m = observer_point<PPL, LANES>(k);
    if (on(k, m)) {
      row[m] = au[k] * kInv2PiD;
      row[pad + m] = -aw[k] * kInv2PiD;
    }
  }
}

// the float64 pair update (pair_f64's arithmetic)
__device__ __forceinline__ void pair_acc_f64(double xp, double zp, double sx, double sz, double sg, double vc4, double& au,
                                             double& aw) {
  const double dx = xp - sx;
  const double dz = zp - sz;
  const double r2 = __builtin_fma(dz, dz, dx * dx);
  const double q = __builtin_fma(r2, r2, vc4);
  const double s = sg * rsqrt_f64(q);
  au = __builtin_fma(dz, s, au);
  aw = __builtin_fma(dx, s, aw);
}

// The float64 body: kFieldTile-source tiles staged in three LDS planes (kFieldTile / LANES slots per lane; slots past the
// end are pair_f64's padding: kPadPosD, G = 0), every lane walks a tile in source order and every broadcast read of a
// source serves its PPL pairs.  UNROLL: sources per trip of the walk.
template <int PPL, int LANES, int UNROLL>
__device__ __forceinline__ void field_f64(const double (&xp)[PPL], const double (&zp)[PPL], const double* __restrict__ xs,
                                          const double* __restrict__ zs, const double* __restrict__ gs, long long s_begin,
                                          long long s_end, double vc4, double (&au)[PPL], double (&aw)[PPL]) {
  static_assert(kFieldTile % LANES == 0, "whole source slots per lane");
  __shared__ __attribute__((aligned(16))) double lx[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lz[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lg[kFieldTile];
  const int tid = threadIdx.x;
  for (long long base = s_begin; base < s_end; base += kFieldTile) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFieldTile / LANES; ++k) {
      const int l = tid + k * LANES;
      const long long si = base + l;
      const bool ok = si < s_end;
      lx[l] = ok ? xs[si] : kPadPosD;
      lz[l] = ok ? zs[si] : kPadPosD;
      lg[l] = ok ? gs[si] : 0.0;
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int j = 0; j < kFieldTile; ++j) {
      const double sx = lx[j], sz = lz[j], sg = lg[j];
#pragma unroll
      for (int k = 0; k < PPL; ++k) pair_acc_f64(xp[k], zp[k], sx, sz, sg, vc4, au[k], aw[k]);
    }
  }
}

__global__ void __launch_bounds__(kProbeLanes)
march_probe_partial(const double* __restrict__ px, const double* __restrict__ pz, const double* shift, int count, long long p_pad,
                    const double* __restrict__ xs, const double* __restrict__ zs, const double* __restrict__ gs,
                    const MarchState* S, int nfoil, long long chunk, double vc4, double* slab) {
  // like the solve chain, these waves run beside a roll-up kernel that keeps every SIMD's issue slots busy
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[1], zp[1], au[1], aw[1];
  load_fixed_points<1, kProbeLanes>(px, pz, shift, count, 0.0, xp, zp, au, aw);
  field_f64<1, kProbeLanes, 4>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw);
  observer_store<1, kProbeLanes>(slab, p_pad, [=](int, long long m) { return m < count; }, au, aw);
}

__global__ void __launch_bounds__(kBlock)
march_probe_finish(const double* slab, long long p_pad, int nsplit, int count, double* out_u, double* out_w) {
  __builtin_amdgcn_s_setprio(3);
  const long long gtid = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long col = gtid >> 6;
  const int lane = threadIdx.x & 63;
  if (col >= 2LL * count) return;   // whole wavefronts leave together
  const int k = (int)(col / count);
  const long long p = col - (long long)k * count;
  const double* c0 = slab + k * p_pad + p;
  double acc = 0.0;
  for (int sidx = lane; sidx < nsplit; sidx += 64) acc += c0[(long long)sidx * 2 * p_pad];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) (k == 0 ? out_u : out_w)[p] = acc;
}

// ---- passive tracers (ludvm_march_set_tracers) -----------------------------------------------------------------------------------
// A tracer is a probe that moves with what it measures.  Tracer m has a seed (xs, zs) and a release step r_m >= 1; with
// shift[i] the frame offset of step i (0 in the lab frame):
//   step i <  r_m   held: its position of step i is (xs + shift[i], zs); it takes part in no pair sum
//   step i >= r_m   start = (xs + shift[i], zs) if i == r_m, else its position after step i - 1;
//                   position after step i = start + dt (u, w)_i(start)
// (u, w)_i is the probes' field (above): the sources [0, S->n + nfoil) right behind march_solve of step i, Vatistas core, no
// freestream term, float64 -- the forward-Euler step the roll-up gives a wake vortex of zero circulation (LUDVM.py:1120-1127).
//
// march_tracer_partial  grid = tracer tiles (kTracerTile = 256 lanes x kTracerPerLane tracers: tracer t0 + k * 256 + lane in
//                       register set k of the lane) x source splits; 256-source tiles staged in LDS, every broadcast read of a
//                       source serves kTracerPerLane pairs (field_f64); the source count is read on the device;
//                       (split, tracer) partial sums to a slab [split][2][m_pad] of the tracers' own.  A tile whose earliest
//                       release (tile_min, precomputed by the host) is after step i leaves at once; a held lane of a mixed
//                       tile walks along at the pad position and stores nothing
// march_tracer_finish   one lane per tracer: splits 0, 1, 2, ... in that order, `start` by the rule above, the new position
//                       into the resident cur_x / cur_z (held: seed + shift[i]) and -- rec_x given -- into the call's row
// The splits are a function of the tracer count and of the step's anchor-derived bound alone (observer_plan, plan_rule.hpp),
// every partial sum is formed by one lane in source order and the splits are combined in split order: a trajectory repeats
// bit for bit however a run is cut into calls.  Both kernels write the tracers' buffers only.
constexpr int kTracerPerLane = 2;
constexpr int kTracerTile = kBlock * kTracerPerLane;

__device__ __forceinline__ void tracer_start(const double* __restrict__ seed_x, const double* __restrict__ seed_z,
                                             const double* cur_x, const double* cur_z, long long m, long long rel, long long step,
                                             double sh, double& x, double& z) {
  if (rel == step) {
    x = seed_x[m] + sh;
    z = seed_z[m];
  } else {
    x = cur_x[m];
    z = cur_z[m];
  }
}

// is every tracer of the workgroup's SUB tiles of kTracerTile still held?  (`tile_min`: one entry per kTracerTile tracers)
template <int SUB>
__device__ __forceinline__ bool tiles_held(const long long* __restrict__ tile_min, long long step, long long count) {
  const long long nsub = (count + kTracerTile - 1) / kTracerTile;
  bool held = true;
#pragma unroll
  for (int q = 0; q < SUB; ++q) {
    const long long e = (long long)blockIdx.x * SUB + q;
    if (e < nsub && tile_min[e] <= step) held = false;
  }
  return held;
}

// the lane's tracers of step `step`: free_[k], the start of a released one and zero sums; a held lane (or one without a tracer) of a
// mixed tile walks along at `absent` and stores nothing
template <int PPL>
__device__ __forceinline__ void load_tracers(const double* __restrict__ seed_x, const double* __restrict__ seed_z,
                                             const long long* __restrict__ release, const double* cur_x, const double* cur_z,
                                             const double* shift, long long step, long long count, double absent,
                                             double (&xp)[PPL], double (&zp)[PPL], double (&au)[PPL], double (&aw)[PPL],
                                             bool (&free_)[PPL]) {
  const double sh = shift ? *shift : 0.0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long m = observer_point<PPL, kBlock>(k);
    xp[k] = absent; zp[k] = absent; au[k] = 0.0; aw[k] = 0.0;
    bool free = false;
    if (m < count) {
      const long long rel = release[m];
      free = rel <= step;
      if (free) tracer_start(seed_x, seed_z, cur_x, cur_z, m, rel, step, sh, xp[k], zp[k]);
    }
    free_[k] = free;
  }
}

// (u, w) of point m: its column of the slab, splits 0, 1, 2, ... in that order
__device__ __forceinline__ void split_sums(const double* slab, long long pad, int nsplit, long long m, double& u, double& w) {
  u = 0.0; w = 0.0;
  const double* c0 = slab + m;
  for (int sidx = 0; sidx < nsplit; ++sidx) {
    u += c0[(long long)sidx * 2 * pad];
    w += c0[(long long)sidx * 2 * pad + pad];
  }
}

__global__ void __launch_bounds__(kBlock)
march_tracer_partial(const double* __restrict__ seed_x, const double* __restrict__ seed_z, const long long* __restrict__ release,
                     const long long* __restrict__ tile_min, const double* cur_x, const double* cur_z, const double* shift,
                     long long step, long long count, long long m_pad, const double* __restrict__ xs, const double* __restrict__ zs,
                     const double* __restrict__ gs, const MarchState* S, int nfoil, long long chunk, double vc4, double* slab) {
  if (tiles_held<1>(tile_min, step, count)) return;         // (uniform: before any barrier)
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kTracerPerLane], zp[kTracerPerLane], au[kTracerPerLane], aw[kTracerPerLane];
  bool free_[kTracerPerLane];
  load_tracers<kTracerPerLane>(seed_x, seed_z, release, cur_x, cur_z, shift, step, count, kPadPosD, xp, zp, au, aw, free_);
  field_f64<kTracerPerLane, kBlock, 2>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw);
  observer_store<kTracerPerLane, kBlock>(slab, m_pad, [&](int k, long long) { return free_[k]; }, au, aw);
}

__global__ void __launch_bounds__(kBlock)
march_tracer_finish(const double* slab, long long m_pad, int nsplit, const double* __restrict__ seed_x,
                    const double* __restrict__ seed_z, const long long* __restrict__ release, const double* shift, long long step,
                    long long count, double dt, double* cur_x, double* cur_z, double* rec_x, double* rec_z) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  const double sh = shift ? *shift : 0.0;
  const long long rel = release[m];
  double x, z;
  if (rel > step) {
    x = seed_x[m] + sh;
    z = seed_z[m];
  } else {
    tracer_start(seed_x, seed_z, cur_x, cur_z, m, rel, step, sh, x, z);
    double u, w;
    split_sums(slab, m_pad, nsplit, m, u, w);
    x = __builtin_fma(dt, u, x);
    z = __builtin_fma(dt, w, z);
  }
  cur_x[m] = x;
  cur_z[m] = z;
  if (rec_x) {
    rec_x[m] = x;
    rec_z[m] = z;
  }
}

// ---- deformation gradient of the tracers (ludvm_march_set_tracer_gradient) -----------------------------------------------------
// The sources of a step do not depend on a tracer, so the exact derivative of the discrete map start -> start + dt (u, w)_i(start)
// with respect to the seed is one 2 x 2 product per step: F <- (I + dt G_i(start)) F, G_i = grad (u, w)_i in closed form
// (field_kernels.hpp: du/dx = -A / pi, du/dz = (B + vc^4 C) / (2 pi), dw/dx = (B - vc^4 C) / (2 pi), dw/dz = -du/dx, from the raw
// sums A = sum G r2 dx dz y^3, B = sum G r2 (dx^2 - dz^2) y^3, C = sum G y^3, y = 1 / sqrt(r2^2 + vc^4)).  F = [[dx/dX, dx/dZ],
// [dz/dX, dz/dZ]] lives in four resident arrays F11 | F12 | F21 | F22 [M]: the identity while a tracer is held and at its release.
//
// field_grad_f64              field_f64 with three more accumulators per point: per pair pair_acc_f64's arithmetic for au, aw,
//                             operation for operation (the positions keep their bits), then the A, B, C updates from that pair's
//                             dx, dz, r2 and reciprocal square root.  A pad slot (G = 0 at kPadPosD) adds exact zeros: y = 0
//                             there and G y^3 is multiplied in BEFORE r2 and dx dz (both finite at the pad)
// march_grad_tracer_partial   march_tracer_partial's loader and launch geometry (kObsTracers: the same tiles, splits and chunk, so
//                             the same summation order for u and w), the body above, five columns u | w | A | B | C to a slab
//                             [split][5][m_pad] of its own
// march_grad_tracer_finish    march_tracer_finish's position update with the same operations, then the product above (held: F
//                             untouched; the release step starts from the identity) and -- recorded -- the step's F row
template <int PPL, int LANES, int UNROLL>
__device__ __forceinline__ void field_grad_f64(const double (&xp)[PPL], const double (&zp)[PPL], const double* __restrict__ xs,
                                               const double* __restrict__ zs, const double* __restrict__ gs, long long s_begin,
                                               long long s_end, double vc4, double (&au)[PPL], double (&aw)[PPL], double (&ga)[PPL],
                                               double (&gb)[PPL], double (&gc)[PPL]) {
  static_assert(kFieldTile % LANES == 0, "whole source slots per lane");
  __shared__ __attribute__((aligned(16))) double lx[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lz[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lg[kFieldTile];
  const int tid = threadIdx.x;
  for (long long base = s_begin; base < s_end; base += kFieldTile) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFieldTile / LANES; ++k) {
      const int l = tid + k * LANES;
      const long long si = base + l;
      const bool ok = si < s_end;
      lx[l] = ok ? xs[si] : kPadPosD;
      lz[l] = ok ? zs[si] : kPadPosD;
      lg[l] = ok ? gs[si] : 0.0;
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int j = 0; j < kFieldTile; ++j) {
      const double sx = lx[j], sz = lz[j], sg = lg[j];
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        // (pair_acc_f64, operation for operation)
        const double dx = xp[k] - sx;
        const double dz = zp[k] - sz;
        const double dxx = dx * dx;
        const double r2 = __builtin_fma(dz, dz, dxx);
        const double q = __builtin_fma(r2, r2, vc4);
        const double y = rsqrt_f64(q);
        const double s = sg * y;
        au[k] = __builtin_fma(dz, s, au[k]);
        aw[k] = __builtin_fma(dx, s, aw[k]);
        // the gradient's raw sums
        const double c = s * (y * y);                       // G y^3
        const double e = c * r2;
        gc[k] += c;
        ga[k] = __builtin_fma(e, dx * dz, ga[k]);
        gb[k] = __builtin_fma(e, __builtin_fma(-dz, dz, dxx), gb[k]);
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock)
march_grad_tracer_partial(const double* __restrict__ seed_x, const double* __restrict__ seed_z, const long long* __restrict__ release,
                          const long long* __restrict__ tile_min, const double* cur_x, const double* cur_z, const double* shift,
                          long long step, long long count, long long m_pad, const double* __restrict__ xs,
                          const double* __restrict__ zs, const double* __restrict__ gs, const MarchState* S, int nfoil,
                          long long chunk, double vc4, double* slab) {
  if (tiles_held<1>(tile_min, step, count)) return;         // (uniform: before any barrier)
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kTracerPerLane], zp[kTracerPerLane], au[kTracerPerLane], aw[kTracerPerLane];
  double ga[kTracerPerLane], gb[kTracerPerLane], gc[kTracerPerLane];
  bool free_[kTracerPerLane];
  load_tracers<kTracerPerLane>(seed_x, seed_z, release, cur_x, cur_z, shift, step, count, kPadPosD, xp, zp, au, aw, free_);
#pragma unroll
  for (int k = 0; k < kTracerPerLane; ++k) { ga[k] = 0.0; gb[k] = 0.0; gc[k] = 0.0; }
  field_grad_f64<kTracerPerLane, kBlock, 2>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw, ga, gb, gc);
  double* row = slab + (long long)blockIdx.y * 5 * m_pad;
#pragma unroll
  for (int k = 0; k < kTracerPerLane; ++k) {
    const long long m = observer_point<kTracerPerLane, kBlock>(k);
    if (free_[k]) {
      row[m] = au[k] * kInv2PiD;
      row[m_pad + m] = -aw[k] * kInv2PiD;
      row[2 * m_pad + m] = ga[k];
      row[3 * m_pad + m] = gb[k];
      row[4 * m_pad + m] = gc[k];
    }
  }
}

__global__ void __launch_bounds__(kBlock)
march_grad_tracer_finish(const double* slab, long long m_pad, int nsplit, const double* __restrict__ seed_x,
                         const double* __restrict__ seed_z, const long long* __restrict__ release, const double* shift,
                         long long step, long long count, double dt, double vc4, double* cur_x, double* cur_z, double* F,
                         double* rec_x, double* rec_z, double* rec_F) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  const double sh = shift ? *shift : 0.0;
  const long long rel = release[m];
  double x, z;
  double f11 = F[m], f12 = F[count + m], f21 = F[2 * count + m], f22 = F[3 * count + m];
  if (rel > step) {
    x = seed_x[m] + sh;
    z = seed_z[m];
  } else {
    tracer_start(seed_x, seed_z, cur_x, cur_z, m, rel, step, sh, x, z);
    // (march_tracer_finish's sums and update: splits 0, 1, 2, ... in that order)
    double u = 0.0, w = 0.0, A = 0.0, B = 0.0, C = 0.0;
    const double* c0 = slab + m;
    for (int sidx = 0; sidx < nsplit; ++sidx) {
      const double* cs = c0 + (long long)sidx * 5 * m_pad;
      u += cs[0];
      w += cs[m_pad];
      A += cs[2 * m_pad];
      B += cs[3 * m_pad];
      C += cs[4 * m_pad];
    }
    x = __builtin_fma(dt, u, x);
    z = __builtin_fma(dt, w, z);
    const double vC = vc4 * C;
    const double ux = -A * kInvPiD, uz = (B + vC) * kInv2PiD, wx = (B - vC) * kInv2PiD, wz = -ux;
    if (rel == step) { f11 = 1.0; f12 = 0.0; f21 = 0.0; f22 = 1.0; }
    const double n11 = __builtin_fma(dt, __builtin_fma(ux, f11, uz * f21), f11);
    const double n12 = __builtin_fma(dt, __builtin_fma(ux, f12, uz * f22), f12);
    const double n21 = __builtin_fma(dt, __builtin_fma(wx, f11, wz * f21), f21);
    const double n22 = __builtin_fma(dt, __builtin_fma(wx, f12, wz * f22), f22);
    f11 = n11; f12 = n12; f21 = n21; f22 = n22;
    F[m] = f11; F[count + m] = f12; F[2 * count + m] = f21; F[3 * count + m] = f22;
  }
  cur_x[m] = x;
  cur_z[m] = z;
  if (rec_x) {
    rec_x[m] = x;
    rec_z[m] = z;
    rec_F[m] = f11; rec_F[count + m] = f12; rec_F[2 * count + m] = f21; rec_F[3 * count + m] = f22;
  }
}

// ---- wake survey: running field moments (ludvm_march_set_survey) ------------------------------------------------------------------
// Survey point k sits at (x[k] + shift[i], z[k]) in step i (shift[i] = 0 in the lab frame).  In every SAMPLED step i -- the
// host knows the window first <= i < stop, (i - first) % every == 0 and launches nothing outside it -- the probes' field
// (u, w)_i (above: LUDVM.py:1095-1106, the sources [0, S->n + nfoil) right behind march_solve of step i, Vatistas core, no
// freestream term, float64) is evaluated there and added to five raw sums per point, sums[0..4][k] = sum u, sum w, sum u^2,
// sum w^2, sum u w: the time-averaged wake and its Reynolds stresses without a time series ever leaving the device.
//
// march_survey_partial  grid = point tiles (kSurveyTile = 256 lanes x kSurveyPerLane points: point t0 + k * 256 + lane in
//                       register set k of the lane) x source splits; 256-source tiles staged in LDS, every broadcast read of a
//                       source serves kSurveyPerLane pairs (field_f64); the source count is read on the device;
//                       (split, point) partial sums to a slab [split][2][k_pad] of the survey's own
// march_survey_finish   one lane per point: splits 0, 1, 2, ... in that order give (u, w), then sums[0..4][k] += with plain
//                       loads and stores (the lane is the only writer of its point; steps follow each other in stream order)
// march_binned_survey_finish  march_survey_finish for a sampled step that has a bin (ludvm_march_set_survey_bins), launched in its
//                       place: the same (u, w) and the same update of sums, then the same five terms into the bin's own block
// The splits are a function of the point count and of the step's anchor-derived bound alone (observer_plan, plan_rule.hpp),
// every partial sum is formed by one lane in source order, the splits are combined in split order and the steps in step
// order: the sums repeat bit for bit however a run is cut into calls.  Both kernels write the survey's buffers only.
constexpr int kSurveyPerLane = 2;
constexpr int kSurveyTile = kBlock * kSurveyPerLane;
constexpr int kSurveySums = 5;

__global__ void __launch_bounds__(kBlock)
march_survey_partial(const double* __restrict__ px, const double* __restrict__ pz, const double* shift, long long count,
                     long long k_pad, const double* __restrict__ xs, const double* __restrict__ zs, const double* __restrict__ gs,
                     const MarchState* S, int nfoil, long long chunk, double vc4, double* slab) {
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kSurveyPerLane], zp[kSurveyPerLane], au[kSurveyPerLane], aw[kSurveyPerLane];
  load_fixed_points<kSurveyPerLane, kBlock>(px, pz, shift, count, kPadPosD, xp, zp, au, aw);
  field_f64<kSurveyPerLane, kBlock, 2>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw);
  observer_store<kSurveyPerLane, kBlock>(slab, k_pad, [=](int, long long m) { return m < count; }, au, aw);
}

// ---- the survey's field in fp32 on local origins (ludvm_march_set_survey_precision) ------------------------------------------------
// The same quantity as march_survey_partial into the same slab, with the pair arithmetic in fp32 (pair2_f32: pair_f32's, packed
// over sources) and everything around it in float64.  It reads the float64 master arrays and makes its own offsets, so it
// depends neither on the resident wake's fp32 mirrors nor on the finishers' origin tables:
//   tiles    256 consecutive source slots at 256-aligned indices counted from slot 0 (`chunk` is a multiple of 256); a tile holds
//            two origin CLASSES of 128 by index parity (TEV and LEV each sit on one parity)
//   origin   of a class: the float64 position of its middle valid member (member cnt / 2 of cnt; a class without a member
//            borrows the tile's slot 0).  LDS holds (float)(xs - ox), (float)(zs - oz), (float)G; slots past the end are
//            pair_f32's padding (kPadPosF, G = 0: exactly 0)
//   points   each lane forms (float)(xp - ox), (float)(zp - oz) once per class and point, the subtraction in float64: the low
//            half of the packed operand is referred to the even class's origin, the high half to the odd one's
//   sums     two levels: a class's 128 pairs in fp32 registers (the halves of the packed accumulators ARE the two class sums),
//            then class 0 and class 1, in that order, added to the lane's float64 (u, w)
//   guard    while staging, the workgroup reduces each class's extent, max over its members of max(|x offset|, |z offset|); a
//            class whose extent exceeds kSurveyF32MaxExtent x v_core is struck from the fp32 tile (padding) and evaluated by
//            pair_acc_f64 on the float64 values instead -- a sparse set has no neighbours within a few
//            cores whose differences need the precision, but an fp32 offset of that size no longer resolves the core
//            (DESIGN section 3's calibration).  The branch is uniform over the workgroup
// One lane forms every partial sum in tile order, the class sums in class order: with the plan (observer_plan) a function of
// K and the step's bound alone, the sums repeat bit for bit however a run is cut into calls.
// local_field_f32 is the body: PPL points of the lane (xd, zd: float64; a lane without a point passes -kPadPosF, away
// from the sources' padding) against the
// sources [s_begin, s_end), s_begin a multiple of 256 -> au += sum G dz / sqrt(r^4 + vc^4), aw += sum G dx / sqrt(..) (no
// 1 / 2 pi, no sign).  Every lane of the workgroup calls it (barriers inside).
constexpr int kSurveyF32PerLane = 4;
constexpr int kSurveyF32Tile = kBlock * kSurveyF32PerLane;
constexpr int kLocalTile = 256;                    // = kOriginBlock: two classes of 128
constexpr double kSurveyF32MaxExtent = 300.0;      // in units of v_core

template <int PPL>
__device__ __forceinline__ void local_field_f32(const double (&xd)[PPL], const double (&zd)[PPL], const double* __restrict__ xs,
                                                const double* __restrict__ zs, const double* __restrict__ gs, long long s_begin,
                                                long long s_end, double vc4, float max_extent, double (&au)[PPL],
                                                double (&aw)[PPL]) {
  static_assert(kLocalTile == kBlock, "one source slot per lane");
  __shared__ __attribute__((aligned(16))) double mx[kLocalTile];     // the tile's float64 values: origins, and the guard's loop
  __shared__ __attribute__((aligned(16))) double mz[kLocalTile];
  __shared__ __attribute__((aligned(16))) double mg[kLocalTile];
  __shared__ __attribute__((aligned(16))) float lx[kLocalTile];      // offsets from the class origins
  __shared__ __attribute__((aligned(16))) float lz[kLocalTile];
  __shared__ __attribute__((aligned(16))) float lg[kLocalTile];
  __shared__ float lext[kBlock / 64][2];
  const int tid = threadIdx.x, par = tid & 1;
  const float vc4s = (float)vc4;
  const f32x2 vc4p = {vc4s, vc4s};
  for (long long base = s_begin; base < s_end; base += kLocalTile) {
    __syncthreads();                                // previous tile fully consumed
    const long long si = base + tid;
    const bool ok = si < s_end;
    const double x = ok ? xs[si] : kPadPosD, z = ok ? zs[si] : kPadPosD, g = ok ? gs[si] : 0.0;
    mx[tid] = x; mz[tid] = z; mg[tid] = g;
    __syncthreads();
    // the classes' middle valid members (uniform)
    const int nv = (int)(s_end - base < kLocalTile ? s_end - base : kLocalTile);       // >= 1
    const int cnt0 = (nv + 1) >> 1, cnt1 = nv >> 1;
    const int oi0 = 2 * (cnt0 >> 1), oi1 = cnt1 ? 1 + 2 * (cnt1 >> 1) : 0;
    const double ox0 = mx[oi0], oz0 = mz[oi0], ox1 = mx[oi1], oz1 = mz[oi1];
    {
      const float fx = ok ? (float)(x - (par ? ox1 : ox0)) : kPadPosF;
      const float fz = ok ? (float)(z - (par ? oz1 : oz0)) : kPadPosF;
      lx[tid] = fx; lz[tid] = fz; lg[tid] = (float)g;
      // strides 2 .. 32 keep the lane parity: lanes 0 / 1 of each wavefront end up with the even / odd class's extent
      float e = ok ? fmaxf(fabsf(fx), fabsf(fz)) : 0.0f;
      for (int s = 2; s < 64; s <<= 1) e = fmaxf(e, __shfl_xor(e, s));
      if ((tid & 63) < 2) lext[tid >> 6][tid & 63] = e;
    }
    __syncthreads();
    float e0 = 0.0f, e1 = 0.0f;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) { e0 = fmaxf(e0, lext[w][0]); e1 = fmaxf(e1, lext[w][1]); }
    // bit p: class p takes the float64 loop (the same value in every lane: say so, the branches below hold barriers)
    const int guard = __builtin_amdgcn_readfirstlane((e0 > max_extent ? 1 : 0) | (e1 > max_extent ? 2 : 0));
    if (guard != 0) {
      if ((guard >> par) & 1) { lx[tid] = kPadPosF; lz[tid] = kPadPosF; lg[tid] = 0.0f; }
      __syncthreads();
    }
    f32x2 tu[PPL], tw[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) { tu[k] = (f32x2){0.0f, 0.0f}; tw[k] = (f32x2){0.0f, 0.0f}; }
    if (guard != 3) {
      f32x2 xp[PPL], zp[PPL];
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        xp[k] = (f32x2){(float)(xd[k] - ox0), (float)(xd[k] - ox1)};
        zp[k] = (f32x2){(float)(zd[k] - oz0), (float)(zd[k] - oz1)};
      }
#pragma unroll 2
      for (int j = 0; j < kLocalTile; j += 4) {
        const f32x4 X = *reinterpret_cast<const f32x4*>(&lx[j]);
        const f32x4 Z = *reinterpret_cast<const f32x4*>(&lz[j]);
        const f32x4 G = *reinterpret_cast<const f32x4*>(&lg[j]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x2 xs2 = h ? (f32x2){X.z, X.w} : (f32x2){X.x, X.y};
          const f32x2 zs2 = h ? (f32x2){Z.z, Z.w} : (f32x2){Z.x, Z.y};
          const f32x2 gs2 = h ? (f32x2){G.z, G.w} : (f32x2){G.x, G.y};
#pragma unroll
          for (int k = 0; k < PPL; ++k) pair2_f32(xp[k] - xs2, zp[k] - zs2, gs2, vc4p, tu[k], tw[k]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if ((guard >> p) & 1) {
        double cu[PPL], cw[PPL];
#pragma unroll
        for (int k = 0; k < PPL; ++k) { cu[k] = 0.0; cw[k] = 0.0; }
        for (int j = p; j < kLocalTile; j += 2) {
          const double sx = mx[j], sz = mz[j], sg = mg[j];
#pragma unroll
          for (int k = 0; k < PPL; ++k) pair_acc_f64(xd[k], zd[k], sx, sz, sg, vc4, cu[k], cw[k]);
        }
#pragma unroll
        for (int k = 0; k < PPL; ++k) { au[k] += cu[k]; aw[k] += cw[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < PPL; ++k) { au[k] += (double)(p ? tu[k].y : tu[k].x); aw[k] += (double)(p ? tw[k].y : tw[k].x); }
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock)
march_f32_survey_partial(const double* __restrict__ px, const double* __restrict__ pz, const double* shift, long long count,
                         long long k_pad, const double* __restrict__ xs, const double* __restrict__ zs,
                         const double* __restrict__ gs, const MarchState* S, int nfoil, long long chunk, double vc4, double v_core,
                         double* slab) {
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kSurveyF32PerLane], zp[kSurveyF32PerLane], au[kSurveyF32PerLane], aw[kSurveyF32PerLane];
  load_fixed_points<kSurveyF32PerLane, kBlock>(px, pz, shift, count, -(double)kPadPosF, xp, zp, au, aw);
  local_field_f32<kSurveyF32PerLane>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, (float)(kSurveyF32MaxExtent * v_core), au, aw);
  observer_store<kSurveyF32PerLane, kBlock>(slab, k_pad, [=](int, long long m) { return m < count; }, au, aw);
}

// one sample (u, w) of a point into its five raw sums s[0..4][count] (s: at the point's column), with plain loads and stores
__device__ __forceinline__ void survey_add(double* s, long long count, double u, double w) {
  s[0] += u;
  s[count] += w;
  s[2 * count] = __builtin_fma(u, u, s[2 * count]);
  s[3 * count] = __builtin_fma(w, w, s[3 * count]);
  s[4 * count] = __builtin_fma(u, w, s[4 * count]);
}

__global__ void __launch_bounds__(kBlock)
march_survey_finish(const double* slab, long long k_pad, int nsplit, long long count, double* sums) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  double u, w;
  split_sums(slab, k_pad, nsplit, m, u, w);
  survey_add(sums + m, count, u, w);
}

// The finisher of a sampled step that has a bin (ludvm_march_set_survey_bins), launched INSTEAD of march_survey_finish: the
// slab is read once, `sums` is updated as march_survey_finish does (the plain sums cannot change a bit), then the bin's own
// block bin_sums[5][count] -- the host knows the step's bin and passes the block -- with the same five terms in the same
// way: a bin's block is, bit for bit, the plain sums of a survey that samples that bin's steps alone.
// One lane per point, loads and stores at stride `count` (coalesced), no LDS; serves both survey precisions, which differ
// only in the partial kernel.  Writes the survey's buffers only.
__global__ void __launch_bounds__(kBlock)
march_binned_survey_finish(const double* slab, long long k_pad, int nsplit, long long count, double* sums, double* bin_sums) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  double u, w;
  split_sums(slab, k_pad, nsplit, m, u, w);
  survey_add(sums + m, count, u, w);
  survey_add(bin_sums + m, count, u, w);
}

// ---- gradient sums of the survey (ludvm_march_set_survey_gradient) ----------------------------------------------------------------
// In every sampled step the closed-form gradient of the same field at the same points (field_kernels.hpp; the raw sums A, B, C
// of the tracers' deformation gradient above) gives
//   ux = -A / pi     e = B / (2 pi) = (du/dz + dw/dx) / 2     om = -vc^4 C / pi     Q = om^2 / 4 - ux^2 - e^2 (= -ux^2 - uz wx)
// and five more raw sums per point, gsums[0..4][k] = sum ux, sum e, sum om, sum om^2, sum Q: the mean vorticity, the mean strain,
// the enstrophy and the vortex cores (Q > 0) of a run without a stored wake.  om is never formed as wx - uz: outside the cores
// |B| >> vc^4 |C| and the difference would lose its digits.
//
// march_grad_survey_partial   march_survey_partial's loader and launch geometry (kObsSurvey: the same tiles, splits and chunk, so
//                             the same summation order for u and w), field_grad_f64 as the body, five columns u | w | A | B | C
//                             to a slab [split][5][k_pad] of its own.  A pad source (G = 0 at kPadPosD) adds exact zeros to all
//                             five (field_grad_f64); a lane without a point walks along at kPadPosD and stores nothing
// march_grad_survey_finish    one lane per point: splits 0, 1, 2, ... in that order for all five columns, survey_add on `sums` with
//                             the (u, w) that march_survey_finish forms (the velocity sums keep their bits), then the five terms
//                             above into gsums with plain loads and stores
// march_binned_grad_survey_finish  the same for a sampled step that has a bin, launched in its place: `sums` and `gsums`, then the
//                             same terms into the bin's two blocks: a bin's gradient block is, bit for bit, the plain gradient
//                             sums of a survey that samples that bin's steps alone
// Still one partial kernel and ONE finisher per sampled step; the sample count and the bin counts are the velocity sums' own.
__global__ void __launch_bounds__(kBlock)
march_grad_survey_partial(const double* __restrict__ px, const double* __restrict__ pz, const double* shift, long long count,
                          long long k_pad, const double* __restrict__ xs, const double* __restrict__ zs,
                          const double* __restrict__ gs, const MarchState* S, int nfoil, long long chunk, double vc4, double* slab) {
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kSurveyPerLane], zp[kSurveyPerLane], au[kSurveyPerLane], aw[kSurveyPerLane];
  double ga[kSurveyPerLane], gb[kSurveyPerLane], gc[kSurveyPerLane];
  load_fixed_points<kSurveyPerLane, kBlock>(px, pz, shift, count, kPadPosD, xp, zp, au, aw);
#pragma unroll
  for (int k = 0; k < kSurveyPerLane; ++k) { ga[k] = 0.0; gb[k] = 0.0; gc[k] = 0.0; }
  field_grad_f64<kSurveyPerLane, kBlock, 2>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw, ga, gb, gc);
  double* row = slab + (long long)blockIdx.y * 5 * k_pad;
#pragma unroll
  for (int k = 0; k < kSurveyPerLane; ++k) {
    const long long m = observer_point<kSurveyPerLane, kBlock>(k);
    if (m < count) {
      row[m] = au[k] * kInv2PiD;
      row[k_pad + m] = -aw[k] * kInv2PiD;
      row[2 * k_pad + m] = ga[k];
      row[3 * k_pad + m] = gb[k];
      row[4 * k_pad + m] = gc[k];
    }
  }
}

// point m's sample of a five-column slab: (u, w) as split_sums forms them and the gradient's terms, splits 0, 1, 2, ... in order
struct GradSample { double u, w, ux, e, om; };
__device__ __forceinline__ GradSample grad_split_sums(const double* slab, long long pad, int nsplit, long long m, double vc4) {
  double u = 0.0, w = 0.0, A = 0.0, B = 0.0, C = 0.0;
  const double* c0 = slab + m;
  for (int sidx = 0; sidx < nsplit; ++sidx) {
    const double* cs = c0 + (long long)sidx * 5 * pad;
    u += cs[0];
    w += cs[pad];
    A += cs[2 * pad];
    B += cs[3 * pad];
    C += cs[4 * pad];
  }
  return {u, w, -A * kInvPiD, B * kInv2PiD, -(vc4 * C) * kInvPiD};
}

// one sample (ux, e, om) of a point into its five gradient sums g[0..4][count] (g: at the point's column), in survey_add's style
__device__ __forceinline__ void survey_grad_add(double* g, long long count, double ux, double e, double om) {
  const double q = __builtin_fma(-e, e, __builtin_fma(-ux, ux, 0.25 * (om * om)));
  g[0] += ux;
  g[count] += e;
  g[2 * count] += om;
  g[3 * count] = __builtin_fma(om, om, g[3 * count]);
  g[4 * count] += q;
}

__global__ void __launch_bounds__(kBlock)
march_grad_survey_finish(const double* slab, long long k_pad, int nsplit, long long count, double vc4, double* sums, double* gsums) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  const GradSample s = grad_split_sums(slab, k_pad, nsplit, m, vc4);
  survey_add(sums + m, count, s.u, s.w);
  survey_grad_add(gsums + m, count, s.ux, s.e, s.om);
}

__global__ void __launch_bounds__(kBlock)
march_binned_grad_survey_finish(const double* slab, long long k_pad, int nsplit, long long count, double vc4, double* sums,
                                double* gsums, double* bin_sums, double* bin_gsums) {
  __builtin_amdgcn_s_setprio(3);
  const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (m >= count) return;
  const GradSample s = grad_split_sums(slab, k_pad, nsplit, m, vc4);
  survey_add(sums + m, count, s.u, s.w);
  survey_grad_add(gsums + m, count, s.ux, s.e, s.om);
  survey_add(bin_sums + m, count, s.u, s.w);
  survey_grad_add(bin_gsums + m, count, s.ux, s.e, s.om);
}

// ---- the tracers' field in hi+lo fp32 (ludvm_march_set_tracer_precision) ---------------------------------------------------------
// The same quantity as march_tracer_partial into the same slab, with the pair arithmetic in fp32 on hi+lo positions (pair_f32<...,
// HILO = true>'s inner loop) and everything around it in float64.  It reads the float64 master arrays and splits them itself
// (split_hilo), so it depends neither on the resident wake's fp32 mirrors nor on any origin table: no classes, no guard, and
// an error that does not grow with the distance from the coordinate origin or with how far the roll-up has stretched the wake:
//   tiles    256 consecutive sources from the split's first one (`chunk` is a multiple of 256); each lane splits one source's
//            x and z into (hi, lo) and stages xh, xl, zh, zl, (float)G: five float planes, 5 KiB.  Slots past the end are
//            pair_f32's padding (hi = kPadPosF, lo = 0, G = 0: exactly 0)
//   points   each lane splits its PPL points once, before the source loop
//   pairs    dx = (xh_p - xh_s) + (xl_p - xl_s), dz likewise, then pair2_f32: two sources per packed instruction, 12 v_pk_*_f32
//            + 2 v_rsq_f32 per two pairs and point; the sources come by broadcast ds_read_b128
//   sums     two levels: a tile's contributions in fp32 packed registers (even sources in the low halves, odd ones in the high
//            halves), then low half and high half, in that order, added to the lane's float64 (u, w)
// One lane forms every partial sum in source order and the tiles in tile order: with the plan (observer_plan) a function of
// M and the step's bound alone, a trajectory repeats bit for bit however a run is cut into calls.
// hilo_field_f32 is the body: PPL points of the lane (xd, zd: float64; a lane without a point passes -kPadPosF, away from the
// sources' padding) against the sources [s_begin, s_end) -> au += sum G dz / sqrt(r^4 + vc^4), aw += sum G dx / sqrt(..) (no
// 1 / 2 pi, no sign).  Every lane of the workgroup calls it (barriers inside).
constexpr int kTracerF32PerLane = 4;
constexpr int kTracerF32Tile = kBlock * kTracerF32PerLane;
constexpr int kHiloTile = 256;

template <int PPL>
__device__ __forceinline__ void hilo_field_f32(const double (&xd)[PPL], const double (&zd)[PPL], const double* __restrict__ xs,
                                               const double* __restrict__ zs, const double* __restrict__ gs, long long s_begin,
                                               long long s_end, double vc4, double (&au)[PPL], double (&aw)[PPL]) {
  static_assert(kHiloTile == kBlock, "one source slot per lane");
  __shared__ __attribute__((aligned(16))) float lxh[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lxl[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lzh[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lzl[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lg[kHiloTile];
  const int tid = threadIdx.x;
  const float vc4s = (float)vc4;
  const f32x2 vc4p = {vc4s, vc4s};
  f32x2 xph[PPL], xpl[PPL], zph[PPL], zpl[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    float h, l;
    split_hilo(xd[k], h, l);
    xph[k] = (f32x2){h, h}; xpl[k] = (f32x2){l, l};
    split_hilo(zd[k], h, l);
    zph[k] = (f32x2){h, h}; zpl[k] = (f32x2){l, l};
  }
  for (long long base = s_begin; base < s_end; base += kHiloTile) {
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
    f32x2 tu[PPL], tw[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) { tu[k] = (f32x2){0.0f, 0.0f}; tw[k] = (f32x2){0.0f, 0.0f}; }
#pragma unroll 2
    for (int j = 0; j < kHiloTile; j += 4) {
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
        for (int k = 0; k < PPL; ++k)
          pair2_f32((xph[k] - xs2) + (xpl[k] - xl2), (zph[k] - zs2) + (zpl[k] - zl2), gs2, vc4p, tu[k], tw[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      au[k] += (double)tu[k].x; au[k] += (double)tu[k].y;
      aw[k] += (double)tw[k].x; aw[k] += (double)tw[k].y;
    }
  }
}

// march_tracer_partial's contract (the same arguments, the same slab [split][2][m_pad], march_tracer_finish behind it) with
// hilo_field_f32 as the body.  A workgroup owns kTracerF32Tile tracers: tracer t0 + k * 256 + lane in register set k of the lane.
// `tile_min` holds one entry per kTracerTile tracers, so a workgroup takes the earliest of its kTracerF32Tile / kTracerTile entries.
__global__ void __launch_bounds__(kBlock)
march_f32x2_tracer_partial(const double* __restrict__ seed_x, const double* __restrict__ seed_z, const long long* __restrict__ release,
                           const long long* __restrict__ tile_min, const double* cur_x, const double* cur_z, const double* shift,
                           long long step, long long count, long long m_pad, const double* __restrict__ xs,
                           const double* __restrict__ zs, const double* __restrict__ gs, const MarchState* S, int nfoil,
                           long long chunk, double vc4, double* slab) {
  static_assert(kTracerF32Tile % kTracerTile == 0, "whole tile_min entries per workgroup");
  if (tiles_held<kTracerF32Tile / kTracerTile>(tile_min, step, count)) return;      // (uniform: before any barrier)
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[kTracerF32PerLane], zp[kTracerF32PerLane], au[kTracerF32PerLane], aw[kTracerF32PerLane];
  bool free_[kTracerF32PerLane];
  load_tracers<kTracerF32PerLane>(seed_x, seed_z, release, cur_x, cur_z, shift, step, count, -(double)kPadPosF, xp, zp, au, aw, free_);
  hilo_field_f32<kTracerF32PerLane>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw);
  observer_store<kTracerF32PerLane, kBlock>(slab, m_pad, [&](int k, long long) { return free_[k]; }, au, aw);
}

// ---- the tracers' deformation gradient in hi+lo fp32 (ludvm_march_set_tracer_gradient_f32x2) ----------------------------------------
// The five columns of march_grad_tracer_partial -- u | w | A | B | C -- from ONE walk in packed fp32 on hi+lo positions, for
// march_grad_tracer_finish unchanged behind it (the float64 Euler step and F <- (I + dt G) F).
// hilo_field_grad_f32 is the body: hilo_field_f32's staging, padding and splits, and per packed pair of sources
//   first   pair2_f32's operations for tu, tw, operation for operation: dx dx, fma(dz, dz, .), fma(r2, r2, vc4), v_rsq_f32, the
//           product with G, two fmas -- a tracer's (u, w), so its path, has the plain f32x2 tracers' bits
//   then    from the same dx, dz, r2, y and G y, field_hilo_f32<true>'s terms in that kernel's product order (field_kernels.hpp:
//           every factor of e's products is at most about 1, so no intermediate leaves fp32's range over |x| <= 1e4):
//               C += (G y) (y y),   e = (G y) (y r2),   A += e (y (dx dz)),   B += e (y (dx^2 - dz^2))
// One reciprocal square root per pair, five packed tile accumulators per point; 22 v_pk_*_f32 + 2 v_rsq_f32 per two pairs and
// point (6 for the differences, 6 of pair2_f32, 10 of the gradient terms).  A pad pair adds exact zeros to all five (y = 0 there and every
// product of y meets a finite partner).  At the end of a 256-source tile the low half, then the high half, of each accumulator
// is added to the lane's float64 sum.
template <int PPL>
__device__ __forceinline__ void hilo_field_grad_f32(const double (&xd)[PPL], const double (&zd)[PPL], const double* __restrict__ xs,
                                                    const double* __restrict__ zs, const double* __restrict__ gs, long long s_begin,
                                                    long long s_end, double vc4, double (&au)[PPL], double (&aw)[PPL],
                                                    double (&ga)[PPL], double (&gb)[PPL], double (&gc)[PPL]) {
  static_assert(kHiloTile == kBlock, "one source slot per lane");
  __shared__ __attribute__((aligned(16))) float lxh[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lxl[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lzh[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lzl[kHiloTile];
  __shared__ __attribute__((aligned(16))) float lg[kHiloTile];
  const int tid = threadIdx.x;
  const float vc4s = (float)vc4;
  const f32x2 vc4p = {vc4s, vc4s};
  f32x2 xph[PPL], xpl[PPL], zph[PPL], zpl[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    float h, l;
    split_hilo(xd[k], h, l);
    xph[k] = (f32x2){h, h}; xpl[k] = (f32x2){l, l};
    split_hilo(zd[k], h, l);
    zph[k] = (f32x2){h, h}; zpl[k] = (f32x2){l, l};
  }
  for (long long base = s_begin; base < s_end; base += kHiloTile) {
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
    f32x2 tu[PPL], tw[PPL], ta[PPL], tb[PPL], tc[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      tu[k] = (f32x2){0.0f, 0.0f}; tw[k] = (f32x2){0.0f, 0.0f};
      ta[k] = (f32x2){0.0f, 0.0f}; tb[k] = (f32x2){0.0f, 0.0f}; tc[k] = (f32x2){0.0f, 0.0f};
    }
#pragma unroll 2
    for (int j = 0; j < kHiloTile; j += 4) {
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
          // (pair2_f32, operation for operation)
          const f32x2 dxx = dx * dx;
          const f32x2 r2 = __builtin_elementwise_fma(dz, dz, dxx);
          const f32x2 q = __builtin_elementwise_fma(r2, r2, vc4p);
          const f32x2 y = {__builtin_amdgcn_rsqf(q.x), __builtin_amdgcn_rsqf(q.y)};
          const f32x2 gy = y * gs2;
          tu[k] = __builtin_elementwise_fma(dz, gy, tu[k]);
          tw[k] = __builtin_elementwise_fma(dx, gy, tw[k]);
          // (field_hilo_f32<true>'s terms, in its product order)
          tc[k] = __builtin_elementwise_fma(gy, y * y, tc[k]);
          const f32x2 e = gy * (y * r2);
          ta[k] = __builtin_elementwise_fma(e, y * (dx * dz), ta[k]);
          tb[k] = __builtin_elementwise_fma(e, y * __builtin_elementwise_fma(-dz, dz, dxx), tb[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      au[k] += (double)tu[k].x; au[k] += (double)tu[k].y;
      aw[k] += (double)tw[k].x; aw[k] += (double)tw[k].y;
      ga[k] += (double)ta[k].x; ga[k] += (double)ta[k].y;
      gb[k] += (double)tb[k].x; gb[k] += (double)tb[k].y;
      gc[k] += (double)tc[k].x; gc[k] += (double)tc[k].y;
    }
  }
}

// march_f32x2_tracer_partial's loader, tiles_held test and pad position under the kObsTracersF32x2 plan (the same chunk, nsplit
// and m_pad: the summation order of u and w is the plain f32x2 tracers'), hilo_field_grad_f32 as the body, and
// march_grad_tracer_partial's slab [split][5][m_pad].  A workgroup owns kTracerGradF32Tile tracers (tracer t0 + k * 256 + lane in
// register set k of the lane): kTracerF32Tile / kTracerGradF32Tile workgroups per tile of the plan.  Nothing of a tracer's sums
// depends on that spread: every tracer sees the same operations on the same operands in the same order in whichever lane.
constexpr int kTracerGradF32PerLane = 2;
constexpr int kTracerGradF32Tile = kBlock * kTracerGradF32PerLane;

__global__ void __launch_bounds__(kBlock)
march_f32x2_grad_tracer_partial(const double* __restrict__ seed_x, const double* __restrict__ seed_z,
                                const long long* __restrict__ release, const long long* __restrict__ tile_min, const double* cur_x,
                                const double* cur_z, const double* shift, long long step, long long count, long long m_pad,
                                const double* __restrict__ xs, const double* __restrict__ zs, const double* __restrict__ gs,
                                const MarchState* S, int nfoil, long long chunk, double vc4, double* slab) {
  constexpr int PPL = kTracerGradF32PerLane;
  static_assert(kTracerGradF32Tile % kTracerTile == 0 && kTracerF32Tile % kTracerGradF32Tile == 0,
                "whole tile_min entries per workgroup, whole workgroups per tile of the plan");
  if (tiles_held<kTracerGradF32Tile / kTracerTile>(tile_min, step, count)) return;      // (uniform: before any barrier)
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[PPL], zp[PPL], au[PPL], aw[PPL], ga[PPL], gb[PPL], gc[PPL];
  bool free_[PPL];
  load_tracers<PPL>(seed_x, seed_z, release, cur_x, cur_z, shift, step, count, -(double)kPadPosF, xp, zp, au, aw, free_);
#pragma unroll
  for (int k = 0; k < PPL; ++k) { ga[k] = 0.0; gb[k] = 0.0; gc[k] = 0.0; }
  hilo_field_grad_f32<PPL>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw, ga, gb, gc);
  double* row = slab + (long long)blockIdx.y * 5 * m_pad;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long m = observer_point<PPL, kBlock>(k);
    if (free_[k]) {
      row[m] = au[k] * kInv2PiD;
      row[m_pad + m] = -aw[k] * kInv2PiD;
      row[2 * m_pad + m] = ga[k];
      row[3 * m_pad + m] = gb[k];
      row[4 * m_pad + m] = gc[k];
    }
  }
}

// ---- the survey's gradient sums in hi+lo fp32 (ludvm_march_set_survey_gradient_f32x2) --------------------------------------------
// The five columns of march_grad_survey_partial -- u | w | A | B | C -- from ONE walk in packed fp32 on hi+lo positions, for
// march_grad_survey_finish / march_binned_grad_survey_finish unchanged behind it.  Made of existing pieces:
//   loader  load_fixed_points, the survey's (the per-step shift included); a lane without a point walks along at -kPadPosF, as in
//           the hi+lo tracer kernels (kPadPosD does not fit fp32), away from the sources' padding, and stores nothing
//   body    hilo_field_grad_f32<2>, the tracers' instantiation: no classes, no guard, an error that does not grow with the distance
//           from the coordinate origin.  A pad pair (G = 0 at hi = kPadPosF) adds exact zeros to all five accumulators: y = 0
//           there and every product of y meets a finite partner (section 4.17's argument)
//   plan    kObsSurveyF32's (chunk, nsplit and k_pad; its source tile is kHiloTile).  A workgroup owns kSurveyGradF32Tile points
//           (point t0 + k * 256 + lane in register set k of the lane): kSurveyF32Tile / kSurveyGradF32Tile workgroups per tile of
//           the plan.  A workgroup whose points all lie past `count` leaves before the first barrier
//   store   march_grad_survey_partial's slab [split][5][k_pad], u and w scaled as there, A, B, C raw, where m < count
// Nothing of a point's sums depends on the spread: every point sees the same operations on the same operands in the same order in
// whichever lane or workgroup it lands.  The velocity columns are this walk's (hi+lo tier), not march_survey_partial's bits.
constexpr int kSurveyGradF32PerLane = 2;
constexpr int kSurveyGradF32Tile = kBlock * kSurveyGradF32PerLane;

__global__ void __launch_bounds__(kBlock)
march_f32x2_grad_survey_partial(const double* __restrict__ px, const double* __restrict__ pz, const double* shift, long long count,
                                long long k_pad, const double* __restrict__ xs, const double* __restrict__ zs,
                                const double* __restrict__ gs, const MarchState* S, int nfoil, long long chunk, double vc4,
                                double* slab) {
  constexpr int PPL = kSurveyGradF32PerLane;
  static_assert(kSurveyF32Tile % kSurveyGradF32Tile == 0, "whole workgroups per tile of the plan");
  if ((long long)blockIdx.x * kSurveyGradF32Tile >= count) return;      // (uniform: before any barrier)
  __builtin_amdgcn_s_setprio(3);
  const SplitRange src = split_range(S, nfoil, chunk);
  double xp[PPL], zp[PPL], au[PPL], aw[PPL], ga[PPL], gb[PPL], gc[PPL];
  load_fixed_points<PPL, kBlock>(px, pz, shift, count, -(double)kPadPosF, xp, zp, au, aw);
#pragma unroll
  for (int k = 0; k < PPL; ++k) { ga[k] = 0.0; gb[k] = 0.0; gc[k] = 0.0; }
  hilo_field_grad_f32<PPL>(xp, zp, xs, zs, gs, src.begin, src.end, vc4, au, aw, ga, gb, gc);
  double* row = slab + (long long)blockIdx.y * 5 * k_pad;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const long long m = observer_point<PPL, kBlock>(k);
    if (m < count) {
      row[m] = au[k] * kInv2PiD;
      row[k_pad + m] = -aw[k] * kInv2PiD;
      row[2 * k_pad + m] = ga[k];
      row[3 * k_pad + m] = gb[k];
      row[4 * k_pad + m] = gc[k];
    }
  }
}

// ---- wake integrals: class moments and kinetic energy of the vortex system (ludvm_march_set_integrals) ------------------------------
// The SYSTEM of time step i is what the probes see: the sources [0, S->n + nfoil) right behind march_solve of step i -- the wake
// before the Euler update of step i, the vortices shed in step i at their placement, the bound vortices of step i -- in the lab
// frame.  Everything is float64.
//
// Moments.  Classes FREE, TEV, LEV, BOUND (0 .. 3), signs slot 0: G >= 0, slot 1: G < 0; for every (class, sign) six sums over
// its vortices: the count, G, G x, G z, G (x^2 + z^2), G^2 -- kIntegralSums = 48 doubles per step.  The wake is stored in shedding
// order, so the class of a wake index is kept in one byte per vortex (`tags`): the host gives the tags of the wake that exists
// when the observer is set; the S->tail vortices appended by the step just solved are the TEV and -- S->shed -- the LEV, and the
// kernel stores their tags for the later steps (hence it runs at EVERY step of a run that has the observer on); the nfoil
// entries behind S->n are BOUND.
// march_integral_partial  one workgroup per chunk of kIntegralChunk source indices (a compile-time constant: which lane adds
//                         which vortex, and in what order, depends on the index alone): lane t takes begin + t + 256 k,
//                         k = 0 .. 7, in that order; the workgroup's 48 sums by block_sum_n's fixed tree; -> part[chunk][48].
//                         The source count is read on the device: a workgroup past the end leaves at once
// march_integral_finish   one lane per sum: the chunk partials in chunk order -> the step's row of the call's buffer
// A run of config 2's size (67 000 vortices: 1.6 MB of x, z, G) is 33 workgroups, not one.
constexpr int kIntegralClasses = 4;
constexpr int kIntegralMoments = 6;
constexpr int kIntegralSums = kIntegralClasses * 2 * kIntegralMoments;
constexpr int kIntegralPerLane = 8;
constexpr int kIntegralChunk = kBlock * kIntegralPerLane;
enum IntegralClass { kClassFree = 0, kClassTev = 1, kClassLev = 2, kClassBound = 3 };

__global__ void __launch_bounds__(kBlock)
march_integral_partial(const double* __restrict__ xs, const double* __restrict__ zs, const double* __restrict__ gs,
                       const MarchState* S, int nfoil, unsigned char* tags, double* part) {
  __shared__ double scratch[4 * kIntegralMoments];
  __builtin_amdgcn_s_setprio(3);
  const long long n = S->n, ns = n + nfoil, n_old = n - S->tail;
  const long long begin = (long long)blockIdx.x * kIntegralChunk;
  if (begin >= ns) return;                           // (uniform: before any barrier)
  double x[kIntegralPerLane], z[kIntegralPerLane], g[kIntegralPerLane];
  int key[kIntegralPerLane];                         // 2 class + sign; -1: no vortex
#pragma unroll
  for (int k = 0; k < kIntegralPerLane; ++k) {
    const long long i = begin + threadIdx.x + (long long)k * kBlock;
    const bool on = i < ns;
    x[k] = on ? xs[i] : 0.0;
    z[k] = on ? zs[i] : 0.0;
    g[k] = on ? gs[i] : 0.0;
    int cls = kClassBound;
    if (i < n_old) {
      cls = tags[i];
    } else if (i < n) {
      cls = i == n_old ? kClassTev : kClassLev;      // the step's own: the TEV first, then -- if shed -- the LEV
      tags[i] = (unsigned char)cls;
    }
    key[k] = on ? 2 * cls + (g[k] < 0.0 ? 1 : 0) : -1;
  }
  double* out = part + (long long)blockIdx.x * kIntegralSums;
#pragma unroll
  for (int q = 0; q < 2 * kIntegralClasses; ++q) {
    double v[kIntegralMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kIntegralPerLane; ++k) {
      const bool m = key[k] == q;
      const double gk = m ? g[k] : 0.0;
      v[0] += m ? 1.0 : 0.0;
      v[1] += gk;
      v[2] += gk * x[k];
      v[3] += gk * z[k];
      v[4] += gk * __builtin_fma(z[k], z[k], x[k] * x[k]);
      v[5] += gk * gk;
    }
    block_sum_n<kIntegralMoments>(v, scratch);
    if (threadIdx.x < kIntegralMoments) {
      double r = v[0];
#pragma unroll
      for (int k = 1; k < kIntegralMoments; ++k) r = (int)threadIdx.x == k ? v[k] : r;
      out[q * kIntegralMoments + threadIdx.x] = r;
    }
  }
}

__global__ void __launch_bounds__(64)
march_integral_finish(const double* part, const MarchState* S, int nfoil, double* row) {
  __builtin_amdgcn_s_setprio(3);
  const long long ns = S->n + nfoil;
  const long long chunks = (ns + kIntegralChunk - 1) / kIntegralChunk;
  const int t = threadIdx.x;
  if (t >= kIntegralSums) return;
  double acc = 0.0;
  for (long long c = 0; c < chunks; ++c) acc += part[c * kIntegralSums + t];
  row[t] = acc;
}

// Energy.  W_i = 1/2 sum_a sum_b G_a G_b / (4 pi) ln((r_ab^2 + s_ab) / 2), s = sqrt(r^4 + vc^4), over ALL sources of step i,
// the bound vortices and a = b included: 1/2 sum_a G_a psi(x_a) with psi exactly LUDVM.stream_function's pair term
// (scalar_term<kScalarPsi>, scalar_term.hpp).  The self part, ln(vc^2 / 2) / (8 pi) sum G^2, follows from moment 6 on the host.
// march_energy_partial  the points are the step's own sources: point tiles of kEnergyTile (256 lanes x 2 points: point
//                       t0 + 256 k + lane in register set k) x source splits; kFieldTile-source tiles in LDS, walked in
//                       source order and bounded by the tile's count (a padded slot would give 0 ln(inf): pair_scalar_f64's
//                       rule); both counts are read on the device; psi partials to a slab [split][pad] of the observer's own
// march_energy_tiles    one workgroup per point tile: every lane adds its points' splits in split order, multiplies by G_a / 2,
//                       adds its two points; the workgroup's block_sum tree -> tile_sums[tile]
// march_energy_finish   one lane: the tiles in tile order -> the step's entry of the call's buffer
// Points and sources both grow with the run: tiles, chunk and nsplit are functions of the step's anchor-derived bound ns_ub
// alone (observer_plan(kEnergyRule, ns_ub, ns_ub), plan_rule.hpp), so a run's bits do not depend on how it is cut into calls.
constexpr int kEnergyPerLane = 2;
constexpr int kEnergyTile = kBlock * kEnergyPerLane;

__global__ void __launch_bounds__(kBlock)
march_energy_partial(const double* __restrict__ xs, const double* __restrict__ zs, const double* __restrict__ gs,
                     const MarchState* S, int nfoil, long long chunk, long long pad, double vc4, double* slab) {
  __shared__ __attribute__((aligned(16))) double lx[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lz[kFieldTile];
  __shared__ __attribute__((aligned(16))) double lg[kFieldTile];
  static_assert(kFieldTile == kBlock, "one source slot per lane");
  __builtin_amdgcn_s_setprio(3);
  const long long ns = S->n + nfoil;
  if ((long long)blockIdx.x * kEnergyTile >= ns) return;       // (uniform: before any barrier)
  const SplitRange src = split_range(S, nfoil, chunk);
  const int tid = threadIdx.x;
  double xp[kEnergyPerLane], zp[kEnergyPerLane], acc[kEnergyPerLane];
#pragma unroll
  for (int k = 0; k < kEnergyPerLane; ++k) {
    const long long m = observer_point<kEnergyPerLane, kBlock>(k);
    const bool on = m < ns;
    xp[k] = on ? xs[m] : 0.0;                        // (a lane without a point walks along at the origin: every a > 0)
    zp[k] = on ? zs[m] : 0.0;
    acc[k] = 0.0;
  }
  for (long long base = src.begin; base < src.end; base += kFieldTile) {
    const int cnt = src.end - base < kFieldTile ? (int)(src.end - base) : kFieldTile;      // sources of this tile (uniform)
    __syncthreads();
    if (tid < cnt) {
      lx[tid] = xs[base + tid];
      lz[tid] = zs[base + tid];
      lg[tid] = gs[base + tid];
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < cnt; ++j) {
      const double sx = lx[j], sz = lz[j], sg = lg[j];
#pragma unroll
      for (int k = 0; k < kEnergyPerLane; ++k)
        acc[k] = __builtin_fma(sg, scalar_term<kScalarPsi>(xp[k] - sx, zp[k] - sz, vc4), acc[k]);
    }
  }
  double* row = slab + (long long)blockIdx.y * pad;
#pragma unroll
  for (int k = 0; k < kEnergyPerLane; ++k) {
    const long long m = observer_point<kEnergyPerLane, kBlock>(k);
    if (m < ns) row[m] = acc[k] * kInv4PiD;
  }
}

__global__ void __launch_bounds__(kBlock)
march_energy_tiles(const double* slab, long long pad, int nsplit, const double* __restrict__ gs, const MarchState* S, int nfoil,
                   double* tile_sums) {
  __shared__ double scratch[kBlock / 64];
  __builtin_amdgcn_s_setprio(3);
  const long long ns = S->n + nfoil;
  if ((long long)blockIdx.x * kEnergyTile >= ns) return;       // (uniform: before any barrier)
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < kEnergyPerLane; ++k) {
    const long long m = observer_point<kEnergyPerLane, kBlock>(k);
    double term = 0.0;
    if (m < ns) {
      double psi = 0.0;
      for (int sidx = 0; sidx < nsplit; ++sidx) psi += slab[(long long)sidx * pad + m];
      term = 0.5 * gs[m] * psi;
    }
    v += term;
  }
  v = block_sum(v, scratch);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = v;
}

__global__ void __launch_bounds__(64)
march_energy_finish(const double* tile_sums, const MarchState* S, int nfoil, double* out) {
  if (threadIdx.x != 0) return;
  const long long ns = S->n + nfoil;
  const long long tiles = (ns + kEnergyTile - 1) / kEnergyTile;
  double acc = 0.0;
  for (long long t = 0; t < tiles; ++t) acc += tile_sums[t];
  *out = acc;
}

}  // namespace ludvm
