// Ensemble of small simulations (LUDVM.time_loop, reference LUDVM.py:597-1171, run many times at once): ONE workgroup owns
// one member and runs all of its time steps inside the kernel, __syncthreads() between the phases of a step.  A member of
// the README size (400 steps, wake <= ~800 vortices) is a chain of tiny dependent launches when it runs alone
// (march_kernels.hpp); here it is one CU's worth of fp64 work and up to a few hundred members run side by side.
//
// Per time step s = 1 .. nt - 1 of a member, all float64, the mathematics of march_chord_finish / march_solve / the fp64
// roll-up (march_kernels.hpp has the map to the reference's lines):
//   1. chord sums      wake -> the npan + 1 targets (chord points of the step and the origin; the two placements, which the
//                      solo march adds for its overlapped steps, are not needed: the roll-up below treats the shed
//                      vortices like every other), the source tile staged through LDS; few targets: lane = (target,
//                      slice of the tile), slices summed in order
//   2. solve           T1 / T2 / T3, Gamma_TEV, LESP test, Gamma_LEV, Fourier coefficients, bound vorticity, loads; the
//                      shed vortices join the member's wake slab, the bound vortices are staged behind them
//   3. roll-up         every wake vortex <- wake + bound vortices, explicit Euler.  Positions are double-buffered: every
//                      velocity is computed from the pre-step buffer and the new positions go to the other one, so no
//                      position a pair still has to read is ever overwritten
//   4. placement       of the next step's TEV / candidate LEV by the threads that have just moved the newest vortices;
//                      snapshot of the wake on the listed steps and after the last one
// With velocity probes (ensemble_march<true>; the definition of march_probe_partial, reference LUDVM.py:1095-1106 with xp, zp
// = the probe), between 2 and 3:
//   2p. probes         wake (this step's shed vortices included, before the Euler update) + bound vortices -> the P probe
//                      points of the sweep, shifted by the member's own offset of the step; row `step` of the member's probe
//                      rows.  Row 0 -- the field of the free vortices -- is written before the first step.  The phase reads
//                      the slab and writes nothing but the probe rows: ensemble_march<false> does not contain it.
// With passive tracers (ensemble_traced<PROBES>; the definition of march_tracer_partial / march_tracer_finish), between 2p and 3:
//   2t. tracers        the same sources -> the start positions of the M tracers of the sweep that are released (seed + the
//                      member's offset of the step on the release step, the member's own current position after it), then
//                      start + dt (u, w) to the member's current positions; a copy of all M positions to the member's tracer
//                      record on the listed steps and on the last one (held tracers: seed + offset).  The phase reads the
//                      slab and writes nothing but the member's tracer buffers: ensemble_march<...> does not contain it.
// With a wake survey (ensemble_surveyed<PROBES, TRACERS>; the definition of march_survey_partial / march_survey_finish), between
// 2t and 3:
//   2s. survey         on the sampled steps (first <= step < stop, (step - first) % every == 0) the same sources -> (u, w) at
//                      the K survey points of the sweep, shifted by the member's own offset of the step, then the member's five
//                      raw sums [5][K] += u, w, u^2, w^2, u w by the lane that owns the point.  The phase reads the slab and
//                      writes nothing but the member's sums: ensemble_march / ensemble_traced do not contain it.
// With bins of the survey (ensemble_binned<PROBES, TRACERS>; the definition of march_binned_survey_finish), inside 2s:
//   2s. bins           on a sampled step whose entry b of the member's table is >= 0 the lane that has just added a point's
//                      five terms to the plain sums adds the same five terms to block b of the member's bin sums [B][5][K].
//                      Nothing else changes: ensemble_surveyed does not contain it.
// With gradient sums of the survey (ensemble_graded<PROBES, TRACERS>; the definition of march_grad_survey_partial /
// march_grad_survey_finish and, with a bin, march_binned_grad_survey_finish), inside 2s:
//   2s. gradient       the pair walk of a sampled step also carries the raw sums A, B, C of the closed-form velocity gradient
//                      at the survey points; the lane that adds a point's velocity terms then adds ux, e, om, om^2, Q to the
//                      member's gradient sums [5][K] and, on a step with a bin, to block b of its [B][5][K].  (u, w) keep their
//                      bits: the velocity sums and bins are those of the sweep without gradient sums.  The bins' table is a
//                      run-time value here (null: no bins).  Nothing else changes: no other kernel contains it.
// With wake integrals (ensemble_integrals<PROBES, TRACERS, SURVEY>; the definitions of march_integral_partial /
// march_energy_partial, march_kernels.hpp), between 2 and 2p:
//   2i. moments        every step: the sources [0, n + npan) of 2p -> for each class (FREE, TEV, LEV, BOUND) and sign the count,
//                      sum G, sum G x, sum G z, sum G (x^2 + z^2), sum G^2; row `step` of the member's integral rows [nt][48].
//                      The class of a wake vortex is a byte of the member's tag buffer [cap]: FREE for the free vortices
//                      (step 0), TEV / LEV written by the lane that appends the shed vortices; an index >= n is BOUND.
//   2e. energy         on the sampled steps W = 1/2 sum_a G_a psi(x_a) over the same sources, a = b included (scalar_term<
//                      kScalarPsi>): O((n + npan)^2) float64 pairs with a logarithm each, inside the one workgroup.
//                      Both phases read the slab and write nothing but the member's integral buffers: no other kernel contains
//                      them.
//

// Determinism: every sum is formed in an order that depends on the member's own wake size, npan and ncoef only (lane p
// walks the sources in index order; the fixed trees of block_sum_n; slices combined in slice order).  No atomics, nothing
// is shared between workgroups, no workgroup waits for another: a member's bits do not depend on the batch, on its index
// in it, or on the CU it ran on.  Pair arithmetic is pair_f64's, so a member differs from a solo precision='f64' run by
// summation order only.
#pragma once
#include "march_kernels.hpp"

namespace ludvm {

constexpr int kEnsTile = kBlock;        // sources staged per pass: 3 x 2 KiB of LDS
constexpr int kEnsSlicesMax = 4;        // few targets: up to this many lanes share a target, each walking a slice of the tile
constexpr int kEnsInitHead = 8;         // init row: tev_x, lev_x, tev_z, lev_z, LESPcrit, 3 reserved, then A[ncoef] of step 0

// Everything a member's workgroup needs, one record per member in a device array indexed by blockIdx.x.
struct EnsembleMember {
  MarchSetup m;                 // scalars and (device) table pointers of this member
  const double* kin;            // nt kinematics rows [alpha, alpha_dot, h_dot, te_x, te_z, le_x, le_z, xg[npan], zg[npan]]
  const double* init;           // kEnsInitHead + ncoef doubles
  const double* free_x; const double* free_z; const double* free_g;
  long long nt;                 // time levels: steps 1 .. nt - 1 are run
  long long nfree;
  long long cap;                // nfree + 2 (nt - 1): the most vortices the wake can hold
  double* xa; double* za;       // wake slab, positions double-buffered (cap + npan each) ...
  double* xb; double* zb;
  double* g;                    // ... and circulations (cap + npan)
  double* rows;                 // nt - 1 rows of kMarchRowHead + 2 ncoef + 2 npan doubles
  double* rec;                  // nsnap + 1 wake records of x[cap] | z[cap] | g[cap]: the snapshot steps, then the last step
  long long* rec_n;             // ... and their sizes (-1: the member has no such step)
  // velocity probes (ensemble_march<true> only)
  const double* px; const double* pz;   // the P probe points, common to the batch
  long long P;
  const double* shift;          // nt x offsets of the probes, one per time level of this member, or null
  double* pu_rows; double* pw_rows;     // nt rows of P doubles each
};

// One Vatistas pair, pair_f64's arithmetic
__device__ __forceinline__ void ens_pair(double xp, double zp, double xs, double zs, double gs, double vc4, double& au, double& aw) {
  const double dx = xp - xs;
  const double dz = zp - zs;
  const double r2 = __builtin_fma(dz, dz, dx * dx);
  const double q = __builtin_fma(r2, r2, vc4);
  const double s = gs * rsqrt_f64(q);
  au = __builtin_fma(dz, s, au);
  aw = __builtin_fma(dx, s, aw);
}

// fp64 Vatistas sums of sources [0, ns) at this lane's target, sources staged through LDS in tiles (lx, lz, lg hold
// kEnsTile + kEnsGroup doubles each); every lane with `mine` adds the sources in index order.  Raw sums: the caller scales
// by kInv2PiD.
//   SLICED = false (the roll-up: a target per lane)  the lane walks the whole tile, four sources at a time with the next
//                  four already on their way from LDS -- a workgroup has ONE wave per SIMD, nothing else hides that latency.
//                  The tile is padded to a multiple of four with far-away zero-strength sources, which add exactly 0.
//   SLICED = true  (few targets: `slices` lanes per target)  the lane walks slice `slice` of every tile.
constexpr int kEnsGroup = 4;
template <bool SLICED>
__device__ __forceinline__ void ens_pair_sums(const double* __restrict__ xs, const double* __restrict__ zs,
                                              const double* __restrict__ gs, long long ns, double xp, double zp, double vc4,
                                              bool mine, int slice, int slices, double* lx, double* lz, double* lg, double& au,
                                              double& aw) {
  const int tid = threadIdx.x;
  const int sub = (kEnsTile + slices - 1) / slices;
  au = 0.0; aw = 0.0;
  for (long long base = 0; base < ns; base += kEnsTile) {
    const int cnt = (int)(ns - base < kEnsTile ? ns - base : kEnsTile);
    const int cnt_pad = (cnt + kEnsGroup - 1) / kEnsGroup * kEnsGroup;
    __syncthreads();
    if (tid < cnt_pad) {
      const bool ok = tid < cnt;
      lx[tid] = ok ? xs[base + tid] : kPadPosD; lz[tid] = ok ? zs[base + tid] : kPadPosD; lg[tid] = ok ? gs[base + tid] : 0.0;
    }
    __syncthreads();
    if (!mine) continue;
    if (SLICED) {
      const int j0 = slice * sub;
      int j1 = j0 + sub;
      if (j1 > cnt) j1 = cnt;
#pragma unroll 4
      for (int j = j0; j < j1; ++j) ens_pair(xp, zp, lx[j], lz[j], lg[j], vc4, au, aw);
    } else {
      double cx[kEnsGroup], cz[kEnsGroup], cg[kEnsGroup];
#pragma unroll
      for (int k = 0; k < kEnsGroup; ++k) { cx[k] = lx[k]; cz[k] = lz[k]; cg[k] = lg[k]; }
      for (int j = 0; j < cnt_pad; j += kEnsGroup) {
        double nx[kEnsGroup], nz[kEnsGroup], ng[kEnsGroup];
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) { nx[k] = lx[j + kEnsGroup + k]; nz[k] = lz[j + kEnsGroup + k]; ng[k] = lg[j + kEnsGroup + k]; }
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) ens_pair(xp, zp, cx[k], cz[k], cg[k], vc4, au, aw);
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) { cx[k] = nx[k]; cz[k] = nz[k]; cg[k] = ng[k]; }
      }
    }
  }
}

// One Vatistas pair with the three raw sums of the closed-form gradient (ensemble_graded only): ens_pair's statements first,
// operation for operation -- au and aw keep their bits -- then field_grad_f64's updates of A, B, C (march_kernels.hpp) in its
// order.  A pad source (G = 0 at kPadPosD) adds exact zeros by the argument written there: y = 0 at the pad, and G y^3 is
// multiplied in before r2 and dx dz, both finite.
__device__ __forceinline__ void ens_grad_pair(double xp, double zp, double xs, double zs, double gs, double vc4, double& au, double& aw,
                                              double& ga, double& gb, double& gc) {
  const double dx = xp - xs;
  const double dz = zp - zs;
  const double dxx = dx * dx;
  const double r2 = __builtin_fma(dz, dz, dxx);
  const double q = __builtin_fma(r2, r2, vc4);
  const double y = rsqrt_f64(q);
  const double s = gs * y;
  au = __builtin_fma(dz, s, au);
  aw = __builtin_fma(dx, s, aw);
  const double c = s * (y * y);                       // G y^3
  const double e = c * r2;
  gc += c;
  ga = __builtin_fma(e, dx * dz, ga);
  gb = __builtin_fma(e, __builtin_fma(-dz, dz, dxx), gb);
}

// ens_pair_sums with ens_grad_pair as the body: the same staging, the same four-ahead prefetching walk of the point-per-lane
// path and the same slice ranges, so au and aw are ens_pair_sums' bits.  Raw sums: the caller scales.
template <bool SLICED>
__device__ __forceinline__ void ens_grad_pair_sums(const double* __restrict__ xs, const double* __restrict__ zs,
                                                   const double* __restrict__ gs, long long ns, double xp, double zp, double vc4,
                                                   bool mine, int slice, int slices, double* lx, double* lz, double* lg, double& au,
                                                   double& aw, double& ga, double& gb, double& gc) {
  const int tid = threadIdx.x;
  const int sub = (kEnsTile + slices - 1) / slices;
  au = 0.0; aw = 0.0; ga = 0.0; gb = 0.0; gc = 0.0;
  for (long long base = 0; base < ns; base += kEnsTile) {
    const int cnt = (int)(ns - base < kEnsTile ? ns - base : kEnsTile);
    const int cnt_pad = (cnt + kEnsGroup - 1) / kEnsGroup * kEnsGroup;
    __syncthreads();
    if (tid < cnt_pad) {
      const bool ok = tid < cnt;
      lx[tid] = ok ? xs[base + tid] : kPadPosD; lz[tid] = ok ? zs[base + tid] : kPadPosD; lg[tid] = ok ? gs[base + tid] : 0.0;
    }
    __syncthreads();
    if (!mine) continue;
    if (SLICED) {
      const int j0 = slice * sub;
      int j1 = j0 + sub;
      if (j1 > cnt) j1 = cnt;
#pragma unroll 4
      for (int j = j0; j < j1; ++j) ens_grad_pair(xp, zp, lx[j], lz[j], lg[j], vc4, au, aw, ga, gb, gc);
    } else {
      double cx[kEnsGroup], cz[kEnsGroup], cg[kEnsGroup];
#pragma unroll
      for (int k = 0; k < kEnsGroup; ++k) { cx[k] = lx[k]; cz[k] = lz[k]; cg[k] = lg[k]; }
      for (int j = 0; j < cnt_pad; j += kEnsGroup) {
        double nx[kEnsGroup], nz[kEnsGroup], ng[kEnsGroup];
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) { nx[k] = lx[j + kEnsGroup + k]; nz[k] = lz[j + kEnsGroup + k]; ng[k] = lg[j + kEnsGroup + k]; }
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) ens_grad_pair(xp, zp, cx[k], cz[k], cg[k], vc4, au, aw, ga, gb, gc);
#pragma unroll
        for (int k = 0; k < kEnsGroup; ++k) { cx[k] = nx[k]; cz[k] = nz[k]; cg[k] = ng[k]; }
      }
    }
  }
}

// Probe rows of one time level: sources [0, ns) of the member's slab -> (u, w) at the P probes, each shifted by `shift` in
// x.  Probes in tiles of kBlock.  A tile of more than kBlock / 2 probes: a probe per lane, the roll-up's prefetching walk.
// A smaller one: up to kEnsSlicesMax lanes share a probe like the chord sums, every lane sums its slice of each source
// tile in index order, and the slices are added in slice order through pu / pw.  All threads of the workgroup call this;
// it ends in a barrier (the caller restages lx / lz / lg, and pu / pw are free again).
__device__ __forceinline__ void ens_probe_row(const EnsembleMember& E, const double* __restrict__ xs, const double* __restrict__ zs,
                                              const double* __restrict__ gs, long long ns, double shift, double vc4,
                                              double* __restrict__ urow, double* __restrict__ wrow, double* lx, double* lz,
                                              double* lg, double (*pu)[kBlock / 2], double (*pw)[kBlock / 2]) {
  const int j = threadIdx.x;
  const int P = (int)E.P;
  for (int t0 = 0; t0 < P; t0 += kBlock) {
    const int cnt = P - t0 < kBlock ? P - t0 : kBlock;
    if (cnt > kBlock / 2) {
      const bool mine = j < cnt;
      const double xp = mine ? E.px[t0 + j] + shift : 0.0, zp = mine ? E.pz[t0 + j] : 0.0;
      double au, aw;
      ens_pair_sums<false>(xs, zs, gs, ns, xp, zp, vc4, mine, 0, 1, lx, lz, lg, au, aw);
      if (mine) { urow[t0 + j] = au * kInv2PiD; wrow[t0 + j] = -aw * kInv2PiD; }
    } else {
      int slices = kBlock / cnt;
      if (slices > kEnsSlicesMax) slices = kEnsSlicesMax;
      const int slice = j / cnt, q = j - slice * cnt;
      const bool mine = slice < slices;
      const double xp = mine ? E.px[t0 + q] + shift : 0.0, zp = mine ? E.pz[t0 + q] : 0.0;
      double au, aw;
      ens_pair_sums<true>(xs, zs, gs, ns, xp, zp, vc4, mine, slice, slices, lx, lz, lg, au, aw);
      double su = au * kInv2PiD, sw = -aw * kInv2PiD;
      if (mine && slice > 0) { pu[slice - 1][q] = su; pw[slice - 1][q] = sw; }
      __syncthreads();
      if (slice == 0) {
        for (int r = 1; r < slices; ++r) { su += pu[r - 1][q]; sw += pw[r - 1][q]; }
        urow[t0 + q] = su; wrow[t0 + q] = sw;
      }
    }
  }
  __syncthreads();
}

// The tracers of a member (ensemble_traced only), one record per member in a device array of its own indexed by blockIdx.x:
// EnsembleMember stays what ensemble_march reads.
struct EnsembleTracers {
  const double* seed_x; const double* seed_z;   // the M seeds, common to the batch
  const long long* release;     // M release steps >= 1, common to the batch
  const long long* tile_min;    // the earliest release step of each tile of kBlock tracers (host-computed: uniform over a workgroup)
  long long M;
  const double* shift;          // nt x offsets of the seeds, one per time level of this member, or null
  double* cur_x; double* cur_z; // M current positions of this member (defined from a tracer's release step on)
  double* rec;                  // ntrec + 1 records of x[M] | z[M]: the recorded steps, then the last step
};

// One Euler step of the released tracers: sources [0, ns) of the member's slab -> (u, w) at every released tracer's start
// position (seed + shift on its release step, its current position after it), start + dt (u, w) to cur_x / cur_z.  Tiles as
// ens_probe_row's; a held tracer takes part in no pair, a tile whose earliest release lies after `step` is skipped before
// its first barrier (tile_min: the same for every lane).  A tracer's current position is read before the tile's first
// barrier and written after its last by the lane that owns it.  All threads of the workgroup call this; it ends in a barrier.
__device__ __forceinline__ void ens_tracer_step(const EnsembleTracers& T, const double* __restrict__ xs, const double* __restrict__ zs,
                                                const double* __restrict__ gs, long long ns, long long step, double shift, double dt,
                                                double vc4, double* lx, double* lz, double* lg, double (*pu)[kBlock / 2],
                                                double (*pw)[kBlock / 2]) {
  const int j = threadIdx.x;
  const int M = (int)T.M;
  for (int t0 = 0; t0 < M; t0 += kBlock) {
    if (T.tile_min[t0 / kBlock] > step) continue;
    const int cnt = M - t0 < kBlock ? M - t0 : kBlock;
    if (cnt > kBlock / 2) {
      const long long rel = j < cnt ? T.release[t0 + j] : step + 1;
      const bool mine = rel <= step;
      double xp = 0.0, zp = 0.0;
      if (mine) {
        if (rel == step) { xp = T.seed_x[t0 + j] + shift; zp = T.seed_z[t0 + j]; }
        else { xp = T.cur_x[t0 + j]; zp = T.cur_z[t0 + j]; }
      }
      double au, aw;
      ens_pair_sums<false>(xs, zs, gs, ns, xp, zp, vc4, mine, 0, 1, lx, lz, lg, au, aw);
      if (mine) { T.cur_x[t0 + j] = xp + dt * (au * kInv2PiD); T.cur_z[t0 + j] = zp + dt * (-aw * kInv2PiD); }
    } else {
      int slices = kBlock / cnt;
      if (slices > kEnsSlicesMax) slices = kEnsSlicesMax;
      const int slice = j / cnt, q = j - slice * cnt;
      const long long rel = slice < slices ? T.release[t0 + q] : step + 1;
      const bool mine = rel <= step;
      double xp = 0.0, zp = 0.0;
      if (mine) {
        if (rel == step) { xp = T.seed_x[t0 + q] + shift; zp = T.seed_z[t0 + q]; }
        else { xp = T.cur_x[t0 + q]; zp = T.cur_z[t0 + q]; }
      }
      double au, aw;
      ens_pair_sums<true>(xs, zs, gs, ns, xp, zp, vc4, mine, slice, slices, lx, lz, lg, au, aw);
      double su = au * kInv2PiD, sw = -aw * kInv2PiD;
      if (mine && slice > 0) { pu[slice - 1][q] = su; pw[slice - 1][q] = sw; }
      __syncthreads();
      if (mine && slice == 0) {
        for (int r = 1; r < slices; ++r) { su += pu[r - 1][q]; sw += pw[r - 1][q]; }
        T.cur_x[t0 + q] = xp + dt * su; T.cur_z[t0 + q] = zp + dt * sw;
      }
    }
  }
  __syncthreads();
}

// The wake survey of a member (ensemble_surveyed only), one record per member in a device array of its own indexed by
// blockIdx.x: EnsembleMember and EnsembleTracers stay what ensemble_march and ensemble_traced read.
struct EnsembleSurvey {
  const double* x; const double* z;     // the K survey points, common to the batch
  long long K;
  const double* shift;          // nt x offsets of the points, one per time level of this member, or null
  long long first, stop, every; // sampled steps: first <= step < stop, (step - first) % every == 0 (common to the batch)
  double* sums;                 // [5][K] raw sums of this member: u, w, u^2, w^2, u w (zero before the launch)
};

// The bins of a member's survey (ensemble_binned only), one record per member in a device array of its own indexed by
// blockIdx.x: EnsembleMember, EnsembleTracers and EnsembleSurvey stay what the other kernels read.
struct EnsembleSurveyBins {
  const int* bin_of_step;       // nt entries of this member: the bin of a sampled step, -1 for none
  double* sums;                 // [nbins][5][K] raw sums of this member, a block per bin (zero before the launch)
};

// One sampled step of the survey: sources [0, ns) of the member's slab -> (u, w) at the K points, each shifted by `shift` in
// x, then sums[c][k] += for c = 0 .. 4, the terms formed as march_survey_finish forms them.  Tiles as ens_probe_row's, and
// its order of summation: (u, w) are the bits of a probe row at the same points.  The lane that owns a point (the slice-0
// lane of the sliced path) is the only writer of its five sums: plain loads and stores.  BINS: the same lane then adds the
// same five terms to `bin` [5][K], the block of the step's bin (null: the step has none; the same for every lane).  All
// threads of the workgroup call this; it ends in a barrier.
template <bool BINS>
__device__ __forceinline__ void ens_survey_step(const EnsembleSurvey& V, const double* __restrict__ xs, const double* __restrict__ zs,
                                                const double* __restrict__ gs, long long ns, double shift, double vc4, double* lx,
                                                double* lz, double* lg, double (*pu)[kBlock / 2], double (*pw)[kBlock / 2],
                                                [[maybe_unused]] double* bin) {
  const int j = threadIdx.x;
  const int K = (int)V.K;
  for (int t0 = 0; t0 < K; t0 += kBlock) {
    const int cnt = K - t0 < kBlock ? K - t0 : kBlock;
    double u = 0.0, w = 0.0;
    int k = -1;                 // the point this lane adds to the sums, if any
    if (cnt > kBlock / 2) {
      const bool mine = j < cnt;
      const double xp = mine ? V.x[t0 + j] + shift : 0.0, zp = mine ? V.z[t0 + j] : 0.0;
      double au, aw;
      ens_pair_sums<false>(xs, zs, gs, ns, xp, zp, vc4, mine, 0, 1, lx, lz, lg, au, aw);
      u = au * kInv2PiD; w = -aw * kInv2PiD;
      if (mine) k = t0 + j;
    } else {
      int slices = kBlock / cnt;
      if (slices > kEnsSlicesMax) slices = kEnsSlicesMax;
      const int slice = j / cnt, q = j - slice * cnt;
      const bool mine = slice < slices;
      const double xp = mine ? V.x[t0 + q] + shift : 0.0, zp = mine ? V.z[t0 + q] : 0.0;
      double au, aw;
      ens_pair_sums<true>(xs, zs, gs, ns, xp, zp, vc4, mine, slice, slices, lx, lz, lg, au, aw);
      u = au * kInv2PiD; w = -aw * kInv2PiD;
      if (mine && slice > 0) { pu[slice - 1][q] = u; pw[slice - 1][q] = w; }
      __syncthreads();
      if (slice == 0) {
        for (int r = 1; r < slices; ++r) { u += pu[r - 1][q]; w += pw[r - 1][q]; }
        k = t0 + q;
      }
    }
    if (k >= 0) {
      double* s = V.sums + k;
      s[0] += u;
      s[K] += w;
      s[2 * (size_t)K] = __builtin_fma(u, u, s[2 * (size_t)K]);
      s[3 * (size_t)K] = __builtin_fma(w, w, s[3 * (size_t)K]);
      s[4 * (size_t)K] = __builtin_fma(u, w, s[4 * (size_t)K]);
      if constexpr (BINS) {
        if (bin) {
          double* b = bin + k;
          b[0] += u;
          b[K] += w;
          b[2 * (size_t)K] = __builtin_fma(u, u, b[2 * (size_t)K]);
          b[3 * (size_t)K] = __builtin_fma(w, w, b[3 * (size_t)K]);
          b[4 * (size_t)K] = __builtin_fma(u, w, b[4 * (size_t)K]);
        }
      }
    }
  }
  __syncthreads();
}

// The gradient sums of a member's survey (ensemble_graded only), one record per member in a device array of its own indexed by
// blockIdx.x: EnsembleMember, EnsembleTracers, EnsembleSurvey and EnsembleSurveyBins stay what the other kernels read.
struct EnsembleSurveyGrad {
  double* sums;                 // [5][K] raw sums of this member: ux, e, om, om^2, Q (zero before the launch)
  double* bin_sums;             // [nbins][5][K], a block per bin (zero before the launch), or null without bins
};

// ens_survey_step<true> with the gradient sums (the definition of march_grad_survey_partial / march_grad_survey_finish): the
// walk is ens_grad_pair_sums, (u, w) and the ten velocity terms are formed and added exactly as ens_survey_step forms and adds
// them -- the velocity sums keep the bits of the sweep without gradient sums.  On the sliced path the raw partials of A, B, C
// are added in slice order like u and w; pu / pw carry (u, w), (A, B) and C in turn, a barrier between the rounds.  Then ux,
// e, om as grad_split_sums forms them and survey_grad_add with stride K into `gsums`, and -- the step has a bin -- into `gbin`
// [5][K], the bin's gradient block (`bin` and `gbin` are null together; the same for every lane).  The lane that owns a point
// is the only writer of its ten sums and of its bin's ten: plain loads and stores.  All threads of the workgroup call this; it
// ends in a barrier.
__device__ __forceinline__ void ens_grad_survey_step(const EnsembleSurvey& V, const double* __restrict__ xs,
                                                     const double* __restrict__ zs, const double* __restrict__ gs, long long ns,
                                                     double shift, double vc4, double* lx, double* lz, double* lg,
                                                     double (*pu)[kBlock / 2], double (*pw)[kBlock / 2], double* bin, double* gsums,
                                                     double* gbin) {
  const int j = threadIdx.x;
  const int K = (int)V.K;
  for (int t0 = 0; t0 < K; t0 += kBlock) {
    const int cnt = K - t0 < kBlock ? K - t0 : kBlock;
    double u = 0.0, w = 0.0, ga = 0.0, gb = 0.0, gc = 0.0;
    int k = -1;                 // the point this lane adds to the sums, if any
    if (cnt > kBlock / 2) {
      const bool mine = j < cnt;
      const double xp = mine ? V.x[t0 + j] + shift : 0.0, zp = mine ? V.z[t0 + j] : 0.0;
      double au, aw;
      ens_grad_pair_sums<false>(xs, zs, gs, ns, xp, zp, vc4, mine, 0, 1, lx, lz, lg, au, aw, ga, gb, gc);
      u = au * kInv2PiD; w = -aw * kInv2PiD;
      if (mine) k = t0 + j;
    } else {
      int slices = kBlock / cnt;
      if (slices > kEnsSlicesMax) slices = kEnsSlicesMax;
      const int slice = j / cnt, q = j - slice * cnt;
      const bool mine = slice < slices;
      const double xp = mine ? V.x[t0 + q] + shift : 0.0, zp = mine ? V.z[t0 + q] : 0.0;
      double au, aw;
      ens_grad_pair_sums<true>(xs, zs, gs, ns, xp, zp, vc4, mine, slice, slices, lx, lz, lg, au, aw, ga, gb, gc);
      u = au * kInv2PiD; w = -aw * kInv2PiD;
      if (mine && slice > 0) { pu[slice - 1][q] = u; pw[slice - 1][q] = w; }
      __syncthreads();
      if (slice == 0) {
        for (int r = 1; r < slices; ++r) { u += pu[r - 1][q]; w += pw[r - 1][q]; }
        k = t0 + q;
      }
      __syncthreads();
      if (mine && slice > 0) { pu[slice - 1][q] = ga; pw[slice - 1][q] = gb; }
      __syncthreads();
      if (slice == 0)
        for (int r = 1; r < slices; ++r) { ga += pu[r - 1][q]; gb += pw[r - 1][q]; }
      __syncthreads();
      if (mine && slice > 0) pu[slice - 1][q] = gc;
      __syncthreads();
      if (slice == 0)
        for (int r = 1; r < slices; ++r) gc += pu[r - 1][q];
    }
    if (k >= 0) {
      double* s = V.sums + k;
      s[0] += u;
      s[K] += w;
      s[2 * (size_t)K] = __builtin_fma(u, u, s[2 * (size_t)K]);
      s[3 * (size_t)K] = __builtin_fma(w, w, s[3 * (size_t)K]);
      s[4 * (size_t)K] = __builtin_fma(u, w, s[4 * (size_t)K]);
      // (grad_split_sums' three terms.  They are rounded HERE, for both blocks below: contraction is on and works one basic
      // block at a time, so without the fences the `+=` of the plain sums -- in this block -- would fuse with these products
      // while the bin's -- behind the branch -- would add the rounded values, and a bin would lose the bits of the plain sums
      // of its steps)
      double ux = -ga * kInvPiD, e = gb * kInv2PiD, om = -(vc4 * gc) * kInvPiD;
      asm volatile("" : "+v"(ux), "+v"(e), "+v"(om));
      survey_grad_add(gsums + k, K, ux, e, om);
      if (bin) {
        double* b = bin + k;
        b[0] += u;
        b[K] += w;
        b[2 * (size_t)K] = __builtin_fma(u, u, b[2 * (size_t)K]);
        b[3 * (size_t)K] = __builtin_fma(w, w, b[3 * (size_t)K]);
        b[4 * (size_t)K] = __builtin_fma(u, w, b[4 * (size_t)K]);
        survey_grad_add(gbin + k, K, ux, e, om);
      }
    }
  }
  __syncthreads();
}

// The wake integrals of a member (ensemble_integrals only), one record per member in a device array of its own indexed by
// blockIdx.x: the records above stay what the other kernels read.
struct EnsembleIntegrals {
  unsigned char* tags;          // [cap]: the class (IntegralClass) of every wake vortex of this member
  double* sums;                 // nt rows of kIntegralSums doubles (row 0 is the host's)
  double* energy;               // nt doubles (NaN before the launch), or null without samples
  long long first, stop, every; // sampled steps of the energy: first <= step < stop, (step - first) % every == 0
};

// Phase 2i: the 48 moment sums of sources [0, ns) -- wake [0, n), bound vortices behind it -- into `row`.  For each of the eight
// (class, sign) keys lane j walks i = j, j + kBlock, ... in that order and adds the six terms by select (march_integral_partial's
// statements), then block_sum_n's fixed tree: the order of every add depends on n and ns alone.  All threads of the workgroup
// call this.
__device__ __forceinline__ void ens_moment_row(const double* __restrict__ xs, const double* __restrict__ zs,
                                               const double* __restrict__ gs, const unsigned char* __restrict__ tags, long long n,
                                               long long ns, double* __restrict__ row, double* scratch) {
  const int j = threadIdx.x;
  for (int q = 0; q < 2 * kIntegralClasses; ++q) {
    double v[kIntegralMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = j; i < ns; i += kBlock) {
      const double x = xs[i], z = zs[i], g = gs[i];
      const int cls = i < n ? (int)tags[i] : (int)kClassBound;
      const bool m = 2 * cls + (g < 0.0 ? 1 : 0) == q;
      const double gk = m ? g : 0.0;
      v[0] += m ? 1.0 : 0.0;
      v[1] += gk;
      v[2] += gk * x;
      v[3] += gk * z;
      v[4] += gk * __builtin_fma(z, z, x * x);
      v[5] += gk * gk;
    }
    block_sum_n<kIntegralMoments>(v, scratch);
    if (j < kIntegralMoments) {
      double r = v[0];
#pragma unroll
      for (int k = 1; k < kIntegralMoments; ++k) r = j == k ? v[k] : r;
      row[q * kIntegralMoments + j] = r;
    }
  }
}

// Phase 2e: W = 1/2 sum_a G_a psi(x_a) over sources [0, ns), the points being the sources themselves in tiles of kBlock points.
// Every source tile is staged through lx / lz / lg and walked in index order, bounded by the tile's count: a padded slot is
// never evaluated (0 ln(inf), pair_scalar_f64's rule).  A lane multiplies each of its points' sums by G_a and accumulates in
// tile order; block_sum's tree; times 1/2 1/(4 pi).  A lane without a point walks along at the origin and its sum is dropped by
// select.  All threads of the workgroup call this; every thread gets W.
__device__ __forceinline__ double ens_energy(const double* __restrict__ xs, const double* __restrict__ zs,
                                             const double* __restrict__ gs, long long ns, double vc4, double* lx, double* lz,
                                             double* lg, double* scratch) {
  const int j = threadIdx.x;
  double acc = 0.0;
  for (long long t0 = 0; t0 < ns; t0 += kBlock) {
    const long long a = t0 + j;
    const bool mine = a < ns;
    const double xp = mine ? xs[a] : 0.0, zp = mine ? zs[a] : 0.0, ga = mine ? gs[a] : 0.0;
    double psi = 0.0;
    for (long long base = 0; base < ns; base += kEnsTile) {
      const int cnt = (int)(ns - base < kEnsTile ? ns - base : kEnsTile);
      __syncthreads();
      if (j < cnt) { lx[j] = xs[base + j]; lz[j] = zs[base + j]; lg[j] = gs[base + j]; }
      __syncthreads();
#pragma unroll 2
      for (int s = 0; s < cnt; ++s) psi = __builtin_fma(lg[s], scalar_term<kScalarPsi>(xp - lx[s], zp - lz[s], vc4), psi);
    }
    acc += mine ? ga * psi : 0.0;
  }
  return block_sum(acc, scratch) * (0.5 * kInv4PiD);
}

// The time loop of one member.  ensemble_march<PROBES> is <PROBES, false, false>: what it compiled to before there were tracers;
// ensemble_traced<PROBES> is <PROBES, true, false>: what it compiled to before there was a survey; ensemble_surveyed<PROBES,
// TRACERS> is <PROBES, TRACERS, true>: what it compiled to before there were bins; ensemble_binned<PROBES, TRACERS> is <PROBES,
// TRACERS, true, true>: what it compiled to before there were gradient sums.  GRAD (ensemble_graded) takes the bins' table as
// a run-time value: a null table is a gradient survey without bins.  INTEG (ensemble_integrals) adds phases 2i and 2e to any of
// them.
template <bool PROBES, bool TRACERS, bool SURVEY, bool BINS = false, bool GRAD = false, bool INTEG = false>
__device__ __forceinline__ void ens_member_run(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps,
                                               int nsnap, const EnsembleTracers* __restrict__ tracers,
                                               const long long* __restrict__ trec_steps, int ntrec,
                                               const EnsembleSurvey* __restrict__ surveys,
                                               [[maybe_unused]] const EnsembleSurveyBins* __restrict__ bins = nullptr,
                                               [[maybe_unused]] const EnsembleSurveyGrad* __restrict__ grads = nullptr,
                                               [[maybe_unused]] const EnsembleIntegrals* __restrict__ integrals = nullptr) {
  static_assert(SURVEY || !BINS, "bins belong to a survey");
  static_assert(BINS || !GRAD, "the gradient sums take the bins' table at run time");
  __shared__ __attribute__((aligned(16))) double lx[kEnsTile + kEnsGroup];
  __shared__ __attribute__((aligned(16))) double lz[kEnsTile + kEnsGroup];
  __shared__ __attribute__((aligned(16))) double lg[kEnsTile + kEnsGroup];
  __shared__ double pu[kEnsSlicesMax - 1][kBlock / 2], pw[kEnsSlicesMax - 1][kBlock / 2];
  __shared__ double Wn[kMarchMaxPan];
  __shared__ double A[kMarchMaxCoef], Ad[kMarchMaxCoef], prevA[kMarchMaxCoef];
  __shared__ double scratch[4 * 8];
  __shared__ double place[4];           // coming step: tev_x, lev_x, tev_z, lev_z
  __shared__ double pvel[2];            // what the wake induces at the origin: u, w

  const EnsembleMember& E = members[blockIdx.x];
  const MarchSetup m = E.m;
  const int j = threadIdx.x;
  const int npan = m.npan, ncoef = m.ncoef, ntt = npan + 1;
  const bool on = j < npan;
  const double pi = 3.14159265358979323846;
  const long long nt = E.nt, cap = E.cap;
  const size_t krow = 7 + 2 * (size_t)npan;
  const size_t row_doubles = kMarchRowHead + 2 * (size_t)ncoef + 2 * (size_t)npan;
  double* xc = E.xa; double* zc = E.za;      // positions before the step
  double* xn_ = E.xb; double* zn_ = E.zb;    // ... and after it
  double* g = E.g;
  const bool ramesh = m.method == 1;
  const double ucpi = m.U * m.chord * pi;

  // step 0: the free vortices are the wake; state of the march as ludvm_march_run takes it from its caller
  for (long long i = j; i < E.nfree; i += kBlock) { xc[i] = E.free_x[i]; zc[i] = E.free_z[i]; g[i] = E.free_g[i]; }
  if constexpr (INTEG)
    for (long long i = j; i < E.nfree; i += kBlock) integrals[blockIdx.x].tags[i] = (unsigned char)kClassFree;
  if (j < ncoef) prevA[j] = E.init[kEnsInitHead + j];
  if (j < 4) place[j] = E.init[j];
  if (j <= nsnap) E.rec_n[j] = -1;
  for (int r = kBlock + j; r <= nsnap; r += kBlock) E.rec_n[r] = -1;
  long long n = E.nfree;
  double lesp_crit = E.init[4], sum_tev = 0.0, sum_lev = 0.0;
  int snap_i = 0;
  [[maybe_unused]] int trec_i = 0;
  __syncthreads();
  if constexpr (PROBES)        // row 0: the field of the free vortices
    ens_probe_row(E, xc, zc, g, E.nfree, E.shift ? E.shift[0] : 0.0, m.vc4, E.pu_rows, E.pw_rows, lx, lz, lg, pu, pw);

  for (long long step = 1; step < nt; ++step) {
    const double* kin = E.kin + (size_t)step * krow;
    const double* xg = kin + 7;
    const double* zg = kin + 7 + npan;
    const double tev_x = place[0], lev_x = place[1], tev_z = place[2], lev_z = place[3];

    // ---- 1. chord sums: wake -> chord points and the origin (:746, :751, :921-931, :1112-1118) ----------------------------
    double u1 = 0, w1 = 0;
    for (int t0 = 0; t0 < ntt; t0 += kBlock) {
      const int cnt = ntt - t0 < kBlock ? ntt - t0 : kBlock;
      int slices = kBlock / cnt;
      if (slices > kEnsSlicesMax) slices = kEnsSlicesMax;
      const int slice = j / cnt, p = t0 + (j - slice * cnt);
      const bool mine = slice < slices;
      double xp = 0.0, zp = 0.0;
      if (p < npan) { xp = xg[p]; zp = zg[p]; }          // (p = npan: the origin)
      double au, aw;
      ens_pair_sums<true>(xc, zc, g, n, xp, zp, m.vc4, mine, slice, slices, lx, lz, lg, au, aw);
      double su = au * kInv2PiD, sw = -aw * kInv2PiD;
      __syncthreads();                               // (pu / pw of the previous pass have been read)
      if (mine && slice > 0) { pu[slice - 1][p - t0] = su; pw[slice - 1][p - t0] = sw; }
      __syncthreads();
      if (slice == 0) {
        for (int q = 1; q < slices; ++q) { su += pu[q - 1][p - t0]; sw += pw[q - 1][p - t0]; }
        if (p < npan) { u1 = su; w1 = sw; }          // (t0 = 0: thread p keeps chord point p)
        else { pvel[0] = su; pvel[1] = sw; }
      }
    }
    __syncthreads();
    const double puo = pvel[0], pwo = pvel[1];

    // ---- 2. solve (march_solve's arithmetic; the state lives in registers and LDS) --------------------------------------------
    const double al = kin[0], ald = kin[1], hd = kin[2];
    const double ca = cos(al), sa = sin(al);
    double ut1 = 0, wt1 = 0, ul1 = 0, wl1 = 0, dedx = 0, cm1 = 0, wq = 0;
    if (on) {
      unit_pair_f64(xg[j], zg[j], tev_x, tev_z, m.vc4, ut1, wt1);     // unit TEV / candidate LEV at the chord points
      unit_pair_f64(xg[j], zg[j], lev_x, lev_z, m.vc4, ul1, wl1);
      dedx = m.detadx[j]; cm1 = m.cm1[j]; wq = m.wq[j];
    }
    double t1 = 0, t2 = 0, t3 = 0;
    if (on) {
      const double u = u1 * ca - w1 * sa, w = u1 * sa + w1 * ca;
      t1 = dedx * (m.U * ca + hd * sa + u - ald * m.eta[j]) - m.U * sa - ald * (m.xpan[j] - m.piv) + hd * ca - w;
      const double ut = ut1 * ca - wt1 * sa, un = ut1 * sa + wt1 * ca;
      t2 = dedx * ut - un;
      const double ult = ul1 * ca - wl1 * sa, uln = ul1 * sa + wl1 * ca;
      t3 = dedx * ult - uln;
    }
    double ij[6] = {t1 * cm1, t2 * cm1, t3 * cm1, t1 * wq, t2 * wq, t3 * wq};
    block_sum_n<6>(ij, scratch);
    const double I1 = ij[0], I2 = ij[1];
    const double kelvin = sum_tev + sum_lev + m.kelvin0;
    RameshProj rp{};
    double g_tev;
    if (ramesh) {
      const double c0 = on ? m.cproj[j] / m.U : 0.0, c1 = on ? m.cproj[npan + j] / m.U : 0.0;
      double pr[6] = {t1 * c0, t2 * c0, t3 * c0, t1 * c1, t2 * c1, t3 * c1};
      block_sum_n<6>(pr, scratch);
      rp.p0[0] = pr[0]; rp.p0[1] = pr[1]; rp.p0[2] = pr[2];
      rp.p1[0] = pr[3]; rp.p1[1] = pr[4]; rp.p1[2] = pr[5];
      rp.ucpi = ucpi;
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
      Ad[j] = (acc - prevA[j]) / m.dt;                 // :772-773
    }
    __syncthreads();
    double bound = ramesh ? ucpi * (A[0] + A[1] / 2) : I1 + g_tev * I2;     // :761 / :738
    const double lesp_prev = A[0];
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
    // loads (:1035-1090; tangential velocity on the chord from the whole wake by linearity) and, on a step that sheds no
    // LEV, what the bound vortices induce at the origin (the reference's zero-strength LEV slot, :1112-1118)
    double r4[4] = {0, 0, 0, 0};     // fn, m, fuo, fwo
    if (on) {
      const double uc1 = u1 + g_tev * ut1 + (shed ? g_lev * ul1 : 0.0);
      const double wc1 = w1 + g_tev * wt1 + (shed ? g_lev * wl1 : 0.0);
      const double u = uc1 * ca - wc1 * sa;
      r4[0] = u * gamma * m.wx[j];
      r4[1] = u * gamma * m.xpan[j] * m.wx[j];
      if (!shed) {
        double uu, ww;
        unit_pair_f64(0.0, 0.0, xg[j], zg[j], m.vc4, uu, ww);
        r4[2] = dgamma * uu; r4[3] = dgamma * ww;
      }
    }
    block_sum_n<4>(r4, scratch);
    const double fn_sum = r4[0], m_sum = r4[1], suo = r4[2], swo = r4[3];

    const long long n0 = n;
    double* row = E.rows + (size_t)(step - 1) * row_doubles;
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
      xc[n0] = tev_x; zc[n0] = tev_z; g[n0] = g_tev;
      if (shed) { xc[n0 + 1] = lev_x; zc[n0 + 1] = lev_z; g[n0 + 1] = g_lev; }
      if constexpr (INTEG) {
        unsigned char* tags = integrals[blockIdx.x].tags;
        tags[n0] = (unsigned char)kClassTev;
        if (shed) tags[n0 + 1] = (unsigned char)kClassLev;
      }
    }
    if (j < ncoef) {
      prevA[j] = A[j];
      row[kMarchRowHead + j] = A[j];
      row[kMarchRowHead + ncoef + j] = Ad[j];
    }
    if (on) {
      row[kMarchRowHead + 2 * ncoef + j] = gamma;
      row[kMarchRowHead + 2 * ncoef + npan + j] = dgamma;
      // bound vortices ride behind the wake as sources of the roll-up (:1106, :1115, :1124)
      const long long i = n0 + k + j;
      xc[i] = xg[j]; zc[i] = zg[j]; g[i] = dgamma;
    }
    n = n0 + k;
    sum_tev += g_tev;
    sum_lev += g_lev;
    __syncthreads();

    // ---- 2i. moments of every step, 2e. energy of a sampled one: the sources of 2p, into the member's integral buffers ----------
    if constexpr (INTEG) {
      const EnsembleIntegrals& I = integrals[blockIdx.x];
      ens_moment_row(xc, zc, g, I.tags, n, n + npan, I.sums + (size_t)step * kIntegralSums, scratch);
      // (the same for every lane of the workgroup: an unsampled step skips the phase before its first barrier)
      if (I.energy && step >= I.first && step < I.stop && (step - I.first) % I.every == 0) {
        const double W = ens_energy(xc, zc, g, n + npan, m.vc4, lx, lz, lg, scratch);
        if (j == 0) I.energy[step] = W;
      }
    }

    // ---- 2p. probes: the sources of the roll-up below, at the probe points (:1095-1106) -----------------------------------
    if constexpr (PROBES)
      ens_probe_row(E, xc, zc, g, n + npan, E.shift ? E.shift[step] : 0.0, m.vc4, E.pu_rows + (size_t)step * (size_t)E.P,
                    E.pw_rows + (size_t)step * (size_t)E.P, lx, lz, lg, pu, pw);

    // ---- 2t. tracers: the same sources at the released tracers, their Euler step, the records ----------------------------
    if constexpr (TRACERS) {
      const EnsembleTracers& T = tracers[blockIdx.x];
      const double tshift = T.shift ? T.shift[step] : 0.0;
      ens_tracer_step(T, xc, zc, g, n + npan, step, tshift, m.dt, m.vc4, lx, lz, lg, pu, pw);
      while (trec_i < ntrec && trec_steps[trec_i] < step) ++trec_i;
      for (int pass = 0; pass < 2; ++pass) {
        const int r = pass == 0 ? (trec_i < ntrec && trec_steps[trec_i] == step ? trec_i : -1) : (step == nt - 1 ? ntrec : -1);
        if (r < 0) continue;
        double* o = T.rec + (size_t)r * 2 * (size_t)T.M;
        for (long long i = j; i < T.M; i += kBlock) {
          const bool free_ = T.release[i] <= step;
          o[i] = free_ ? T.cur_x[i] : T.seed_x[i] + tshift;
          o[T.M + i] = free_ ? T.cur_z[i] : T.seed_z[i];
        }
      }
    }

    // ---- 2s. survey: on a sampled step the same sources at the survey points, added to the member's five raw sums --------
    if constexpr (SURVEY) {
      const EnsembleSurvey& V = surveys[blockIdx.x];
      // (the same for every lane of the workgroup: an unsampled step skips the phase before its first barrier)
      if (step >= V.first && step < V.stop && (step - V.first) % V.every == 0) {
        double* bin = nullptr;
        if constexpr (GRAD) {
          // (read once per sampled step; the same for every lane of the workgroup)
          const EnsembleSurveyBins& Q = bins[blockIdx.x];
          const EnsembleSurveyGrad& G = grads[blockIdx.x];
          const int b = Q.bin_of_step ? Q.bin_of_step[step] : -1;
          double* gbin = nullptr;
          if (b >= 0) { bin = Q.sums + (size_t)b * 5 * (size_t)V.K; gbin = G.bin_sums + (size_t)b * 5 * (size_t)V.K; }
          ens_grad_survey_step(V, xc, zc, g, n + npan, V.shift ? V.shift[step] : 0.0, m.vc4, lx, lz, lg, pu, pw, bin, G.sums, gbin);
        } else if constexpr (BINS) {
          // (read once per sampled step; the same for every lane of the workgroup)
          const EnsembleSurveyBins& Q = bins[blockIdx.x];
          const int b = Q.bin_of_step[step];
          if (b >= 0) bin = Q.sums + (size_t)b * 5 * (size_t)V.K;
        }
        if constexpr (!GRAD)
          ens_survey_step<BINS>(V, xc, zc, g, n + npan, V.shift ? V.shift[step] : 0.0, m.vc4, lx, lz, lg, pu, pw, bin);
      }
    }

    // ---- 3. roll-up (:1095-1127) and 4. placement of the coming step (:672-681, :788-800) -------------------------------
    const double* kin_next = step + 1 < nt ? kin + krow : nullptr;
    for (long long t0 = 0; t0 < n; t0 += kBlock) {
      const long long i = t0 + j;
      const bool mine = i < n;
      const double xp = mine ? xc[i] : 0.0, zp = mine ? zc[i] : 0.0;
      double au, aw;
      ens_pair_sums<false>(xc, zc, g, n + npan, xp, zp, m.vc4, mine, 0, 1, lx, lz, lg, au, aw);
      if (mine) {
        const double xn = xp + m.dt * (au * kInv2PiD);
        const double zn = zp + m.dt * (-aw * kInv2PiD);
        xn_[i] = xn; zn_[i] = zn;
        if (kin_next) {
          if (i == n - k) {
            const double tex = kin_next[3], tez = kin_next[4];
            place[0] = tex + (xn - tex) / 3; place[2] = tez + (zn - tez) / 3;
          }
          if (i == n - 1) {
            const double lex = kin_next[5], lez = kin_next[6];
            double px = lex, pz = lez;
            if (shed) { px = lex + (xn - lex) / 3; pz = lez + (zn - lez) / 3; }
            place[1] = px; place[3] = pz;
          }
        }
      }
    }
    { double* t = xc; xc = xn_; xn_ = t; t = zc; zc = zn_; zn_ = t; }
    __syncthreads();

    // wake records: the listed steps, and the last one
    while (snap_i < nsnap && snap_steps[snap_i] < step) ++snap_i;
    int rec = -1;
    if (snap_i < nsnap && snap_steps[snap_i] == step) rec = snap_i;
    for (int pass = 0; pass < 2; ++pass) {
      const int r = pass == 0 ? rec : (step == nt - 1 ? nsnap : -1);
      if (r < 0) continue;
      double* o = E.rec + (size_t)r * 3 * (size_t)cap;
      for (long long i = j; i < n; i += kBlock) { o[i] = xc[i]; o[cap + i] = zc[i]; o[2 * cap + i] = g[i]; }
      if (j == 0) E.rec_n[r] = n;
    }
  }
}

template <bool PROBES>
__global__ void __launch_bounds__(kBlock)
ensemble_march(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap) {
  ens_member_run<PROBES, false, false>(members, snap_steps, nsnap, nullptr, nullptr, 0, nullptr);
}

// ensemble_march<PROBES> with phase 2t: the launch of ludvm_ensemble_run_traced
template <bool PROBES>
__global__ void __launch_bounds__(kBlock)
ensemble_traced(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap,
                const EnsembleTracers* __restrict__ tracers, const long long* __restrict__ trec_steps, int ntrec) {
  ens_member_run<PROBES, true, false>(members, snap_steps, nsnap, tracers, trec_steps, ntrec, nullptr);
}

// ensemble_march<PROBES> / ensemble_traced<PROBES> with phase 2s: the launches of ludvm_ensemble_run_surveyed
template <bool PROBES, bool TRACERS>
__global__ void __launch_bounds__(kBlock)
ensemble_surveyed(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap,
                  const EnsembleTracers* __restrict__ tracers, const long long* __restrict__ trec_steps, int ntrec,
                  const EnsembleSurvey* __restrict__ surveys) {
  ens_member_run<PROBES, TRACERS, true>(members, snap_steps, nsnap, tracers, trec_steps, ntrec, surveys);
}

// ensemble_surveyed<PROBES, TRACERS> with the bins of phase 2s: the launches of ludvm_ensemble_run_surveyed_binned
template <bool PROBES, bool TRACERS>
__global__ void __launch_bounds__(kBlock)
ensemble_binned(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap,
                const EnsembleTracers* __restrict__ tracers, const long long* __restrict__ trec_steps, int ntrec,
                const EnsembleSurvey* __restrict__ surveys, const EnsembleSurveyBins* __restrict__ bins) {
  ens_member_run<PROBES, TRACERS, true, true>(members, snap_steps, nsnap, tracers, trec_steps, ntrec, surveys, bins);
}

// ensemble_binned<PROBES, TRACERS> with the gradient sums of phase 2s: the launches of ludvm_ensemble_run_surveyed_graded (a null
// table in a member's bin record: a gradient survey without bins)
template <bool PROBES, bool TRACERS>
__global__ void __launch_bounds__(kBlock)
ensemble_graded(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap,
                const EnsembleTracers* __restrict__ tracers, const long long* __restrict__ trec_steps, int ntrec,
                const EnsembleSurvey* __restrict__ surveys, const EnsembleSurveyBins* __restrict__ bins,
                const EnsembleSurveyGrad* __restrict__ grads) {
  ens_member_run<PROBES, TRACERS, true, true, true>(members, snap_steps, nsnap, tracers, trec_steps, ntrec, surveys, bins, grads);
}

// Any of the kernels above with phases 2i and 2e: the launches of ludvm_ensemble_run_integrals.  SURVEY: 0 none (ensemble_march /
// ensemble_traced), 1 plain (ensemble_surveyed), 2 binned (ensemble_binned), 3 graded (ensemble_graded).
template <bool PROBES, bool TRACERS, int SURVEY>
__global__ void __launch_bounds__(kBlock)
ensemble_integrals(const EnsembleMember* __restrict__ members, const long long* __restrict__ snap_steps, int nsnap,
                   const EnsembleTracers* __restrict__ tracers, const long long* __restrict__ trec_steps, int ntrec,
                   const EnsembleSurvey* __restrict__ surveys, const EnsembleSurveyBins* __restrict__ bins,
                   const EnsembleSurveyGrad* __restrict__ grads, const EnsembleIntegrals* __restrict__ integrals) {
  static_assert(SURVEY >= 0 && SURVEY <= 3, "0 none, 1 plain, 2 binned, 3 graded");
  ens_member_run<PROBES, TRACERS, SURVEY >= 1, SURVEY >= 2, SURVEY == 3, true>(members, snap_steps, nsnap, tracers, trec_steps, ntrec,
                                                                               surveys, bins, grads, integrals);
}

}  // namespace ludvm
