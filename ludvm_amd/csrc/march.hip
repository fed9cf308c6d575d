// libludvm_hip.so -- C-ABI implementation (see include/ludvm_hip.h for the contract and the reference file:line each entry point
// replaces; ctx.hpp for how the library is divided into translation units).  gfx950 only; no CPU path: every entry point either
// runs the HIP kernels or returns an error code.
// This unit: the device-resident time march (LUDVM.time_loop, LUDVM.py:597-1171, with the solve on the device), and the
// ensemble of small simulations (many such time loops in one launch).
#include "ctx.hpp"
#include "march_kernels.hpp"
#include "ensemble_kernels.hpp"

#include <limits>

extern "C" {

/* ---- device-resident time march ------------------------------------------------------------- */

int ludvm_march_setup(ludvm_ctx* c, int npan, int ncoef, const double* scalars, const double* tables, const double* kin,
                      size_t kin_rows) {
  if (!c) return LUDVM_E_ARG;
  c->march_ready = false;
  c->probe_count = 0;       // a new run: its probes are set after this call (ludvm_march_set_probes)
  c->probe_rows = 0;
  c->tracer_count = 0;      // ... and its tracers (ludvm_march_set_tracers)
  c->tracer_ran = false;
  c->tracer_record.clear();
  c->tracer_rows.clear();
  c->tracer_precision = 0;
  c->tracer_gradient = false;
  c->tracer_grad_ran = false;
  c->survey_count = 0;      // ... and its survey (ludvm_march_set_survey)
  c->survey_samples = 0;
  c->survey_precision = 0;
  c->survey_nbins = 0;      // ... and its bins (ludvm_march_set_survey_bins)
  c->survey_gradient = c->survey_gradient_f32x2 = false;
  c->integrals_on = false;  // ... and its wake integrals (ludvm_march_set_integrals)
  c->integral_rows = 0;
  if (!scalars || !tables || !kin) return fail(c, LUDVM_E_ARG, "null array");
  if (npan < 1 || npan > kMarchMaxPan || ncoef < 4 || ncoef > kMarchMaxCoef)
    return fail(c, LUDVM_E_ARG, "march: 1 <= Npanels <= 256 and 4 <= Ncoeffs <= 64");
  if (kin_rows < 2) return fail(c, LUDVM_E_ARG, "march: kinematics table too short");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t P = (size_t)npan;
  const size_t tab_doubles = 8 * P + (size_t)ncoef * P + (size_t)(ncoef - 1) * P;
  const size_t kin_doubles = kin_rows * (7 + 2 * P);
  CHK(ensure(c, c->march_tab, tab_doubles * 8));
  CHK(ensure(c, c->march_kin, kin_doubles * 8));
  CHK(ensure(c, c->march_state, sizeof(MarchState)));
  HIPCHK(c, hipMemcpyAsync(c->march_tab.p, tables, tab_doubles * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->march_kin.p, kin, kin_doubles * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  MarchSetup& m = c->msetup;
  m.npan = npan; m.ncoef = ncoef;
  m.U = scalars[0]; m.chord = scalars[1]; m.rho = scalars[2]; m.dt = scalars[3]; m.piv = scalars[4];
  c->march_vcore = scalars[5];
  m.kelvin0 = scalars[7] - scalars[6];          // sum(Gamma_free) - IC
  m.vc4 = (scalars[5] * scalars[5]) * (scalars[5] * scalars[5]);
  m.method = scalars[8] != 0.0 ? 1 : 0;
  m.maxerror = scalars[9]; m.maxiter = (int)scalars[10]; m.epsilon = scalars[11];
  if (m.method == 1 && !(m.maxerror > 0.0 && m.maxiter >= 1 && m.epsilon > 0.0))
    return fail(c, LUDVM_E_ARG, "march: 'Ramesh' needs maxerror > 0, maxiter >= 1, epsilon > 0");
  const double* t = static_cast<const double*>(c->march_tab.p);
  m.detadx = t; m.eta = t + P; m.xpan = t + 2 * P; m.cm1 = t + 3 * P; m.wq = t + 4 * P; m.opcs = t + 5 * P;
  m.hcsd = t + 6 * P; m.wx = t + 7 * P; m.cproj = t + 8 * P; m.ssin = t + 8 * P + (size_t)ncoef * P;
  c->march_kin_rows = kin_rows;
  if (!c->progress) {
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->progress), kProgressRing * sizeof(unsigned long long), hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->progress_dev), c->progress, 0));
  }
  for (auto& e : c->march_ev)
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  if (!c->stream_b) {
    int least = 0, greatest = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    // the solve chain is short and latency-critical: let it cut in front of the roll-up's workgroups
    HIPCHK(c, hipStreamCreateWithPriority(&c->stream_b, hipStreamNonBlocking, greatest));
  }
  c->march_ready = true;
  return LUDVM_OK;
}

}  // extern "C"

namespace {

// fp64 partial sums of the wake at the npan + 3 targets staged in MarchState (chord points of the coming solve, its
// two placements, the origin), then the finisher that leaves sums and unit influences in the device state.  Launches on
// c->stream (the caller points it at the second stream for overlapped steps).
int march_chord_launch(ludvm_ctx* c, long long n_ub) {
  const MarchSetup& m = c->msetup;
  const size_t P = (size_t)m.npan, NT = P + 3;
  MarchState* S = static_cast<MarchState*>(c->march_state.p);
  PairArgs a{};
  a.xs = c->x64; a.zs = c->z64; a.gs = c->g64;
  a.ns = 0; a.n_dev = &S->n; a.ns_dev = 1; a.nt_dev = 0;
  a.xt = S->tgt; a.zt = S->tgt + NT; a.nt = (long long)NT;
  a.vc4 = m.vc4;
  Plan p = make_plan(c, (long long)NT, std::max<long long>(n_ub, 1), LUDVM_PREC_F64);
  const bool was = c->timing;
  c->timing = false;   // the chord sums are not the dominant kernel
  int rc = launch_pair(c, a, p, LUDVM_PREC_F64, nullptr, nullptr);
  c->timing = was;
  CHK(rc);
  const double* slab = static_cast<const double*>(c->part.p);
  hipLaunchKernelGGL(march_chord_finish, dim3(blocks_for((long long)(2 * NT * 64))), dim3(kBlock), 0, c->stream,
                     p.nsplit > 1 ? slab : (const double*)nullptr, p.nt_pad, p.nsplit, slab, (int)P, S, m.vc4);
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// workspace a march step may need when the wake holds at most n_ub vortices
void march_workspace(const ludvm_ctx* c, long long n_ub, int precision, size_t nfoil, size_t& part_bytes, size_t& acc_bytes) {
  const long long nt = std::max<long long>(n_ub, 1);
  // (both kernels' workspaces where either may run: the overlapped march switches to the symmetric kernel earlier
  // than the serial one)
  if (precision != LUDVM_PREC_F64 && use_symmetric(c, nt, c->msetup.vc4, true))
    acc_bytes = std::max(acc_bytes, (size_t)2 * (size_t)((nt + 63) / 64 * 64) * sizeof(long long));
  if (precision == LUDVM_PREC_F64 || !use_symmetric(c, nt, c->msetup.vc4, false)) {
    Plan p = make_plan(c, nt, nt + (long long)nfoil, precision);
    const size_t elt = precision == LUDVM_PREC_F64 ? 8 : 4;
    part_bytes = std::max(part_bytes, (size_t)p.nsplit * 2 * (size_t)p.nt_pad * elt);
  }
  Plan q = make_plan(c, (long long)nfoil + 3, nt, LUDVM_PREC_F64);
  part_bytes = std::max(part_bytes, (size_t)q.nsplit * 2 * (size_t)q.nt_pad * 8);
}

// The launch rule of the observer kernels is observer_plan (plan_rule.hpp); its tiles are the kernels'.
constexpr bool rule_is(ObserverKind kind, int point_tile, int src_tile) {
  return kObserverRules[kind].point_tile == point_tile && kObserverRules[kind].src_tile == src_tile;
}
static_assert(rule_is(kObsProbes, kProbeLanes, kFieldTile) && rule_is(kObsTracers, kTracerTile, kFieldTile) &&
                  rule_is(kObsTracersF32x2, kTracerF32Tile, kHiloTile) && rule_is(kObsSurvey, kSurveyTile, kFieldTile) &&
                  rule_is(kObsSurveyF32, kSurveyF32Tile, kLocalTile),
              "the observer rules' point and source tiles are the kernels'");
// the survey's hi+lo fp32 gradient walk runs under kObsSurveyF32: its source tile, and whole workgroups per tile of that plan
static_assert(rule_is(kObsSurveyF32, kSurveyF32Tile, kHiloTile) && kSurveyF32Tile % kSurveyGradF32Tile == 0 &&
                  kSurveyGradF32Tile == kBlock * kSurveyGradF32PerLane,
              "march_f32x2_grad_survey_partial: kObsSurveyF32's tiles, spread over kSurveyF32Tile / kSurveyGradF32Tile workgroups");

// the x offset of time step s (NULL: the lab frame)
const double* step_shift(const Buf& shift, bool shifted, long long s) {
  return shifted ? static_cast<const double*>(shift.p) + s : nullptr;
}

// Probe row `rel` of the call: the field of [0, S->n + nfoil) -- the wake before step s's roll-up, its shed vortices, the
// staged bound vortices -- at the probes.  Enqueued right behind march_solve of step s on the stream that ran it, so before
// the roll-up's finisher moves anything.  The slab is the probes' own buffer, written and read only by these two kernels in
// stream order (the next step's pair follows this step's finisher, which follows this pair).  Reads the wake, writes
// nothing of it: rows, state, hist and the resident wake keep their bits.
int march_probe_launch(ludvm_ctx* c, hipStream_t st, long long n_ub, long long s, long long rel, long long rows) {
  const MarchSetup& m = c->msetup;
  const size_t P = c->probe_count;
  const ObserverPlan p = observer_plan(kObserverRules[kObsProbes], (long long)P, n_ub + (long long)m.npan);
  const double* pxz = static_cast<const double*>(c->probe_xz.p);
  const double* shift = step_shift(c->probe_shift, c->probe_shifted, s);
  double* slab = static_cast<double*>(c->probe_part.p);
  double* out = static_cast<double*>(c->probe_out.p);
  hipLaunchKernelGGL(march_probe_partial, dim3((unsigned)p.tiles, (unsigned)p.nsplit), dim3(kProbeLanes), 0, st, pxz, pxz + P, shift,
                     (int)P, p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                     static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, slab);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(march_probe_finish, dim3(blocks_for((long long)(2 * P * 64))), dim3(kBlock), 0, st, (const double*)slab, p.pad,
                     p.nsplit, (int)P, out + (size_t)rel * P, out + ((size_t)rows + (size_t)rel) * P);
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// The tracers' Euler step of time step s (rec_row >= 0: also row rec_row of the call's record): enqueued where the probes
// are, behind march_solve of step s on the stream that ran it and behind the probe kernels when both are set, so before the
// roll-up's finisher moves anything.  The slab, the positions and the record are the tracers' own buffers, touched only by
// these two kernels in stream order.  Reads the wake, writes nothing of it: rows, state, hist, the resident wake and the
// probe rows keep their bits.  With the deformation gradient on (ludvm_march_set_tracer_gradient) the gradient pair of kernels
// takes the place of the plain pair under the same plan: the positions keep their bits, F and its record are further buffers
// of the tracers' own.
int march_tracer_launch(ludvm_ctx* c, hipStream_t st, long long n_ub, long long s, long long rec_row, size_t rec_rows) {
  const MarchSetup& m = c->msetup;
  const size_t M = c->tracer_count;
  const bool f32x2 = c->tracer_precision == 2;
  const ObserverPlan p = observer_plan(kObserverRules[f32x2 ? kObsTracersF32x2 : kObsTracers], (long long)M, n_ub + (long long)m.npan);
  const double* seed = static_cast<const double*>(c->tracer_seed.p);
  const long long* release = static_cast<const long long*>(c->tracer_release.p);
  const double* shift = step_shift(c->tracer_shift, c->tracer_shifted, s);
  double* cur = static_cast<double*>(c->tracer_cur.p);
  double* out = static_cast<double*>(c->tracer_out.p);
  if (c->tracer_gradient) {
    double* gslab = static_cast<double*>(c->tracer_grad_part.p);
    // (hi+lo fp32: the plan's tiles, each spread over kTracerF32Tile / kTracerGradF32Tile workgroups; chunk, nsplit and pad are the plan's)
    const unsigned gx = (unsigned)(f32x2 ? p.tiles * (kTracerF32Tile / kTracerGradF32Tile) : p.tiles);
    hipLaunchKernelGGL(f32x2 ? march_f32x2_grad_tracer_partial : march_grad_tracer_partial, dim3(gx, (unsigned)p.nsplit), dim3(kBlock), 0,
                       st, seed, seed + M, release, release + M, (const double*)cur, (const double*)(cur + M), shift, s, (long long)M,
                       p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                       static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, gslab);
    HIPCHK(c, hipGetLastError());
    const bool rec = rec_row >= 0;
    hipLaunchKernelGGL(march_grad_tracer_finish, dim3(blocks_for((long long)M)), dim3(kBlock), 0, st, (const double*)gslab, p.pad,
                       p.nsplit, seed, seed + M, release, shift, s, (long long)M, m.dt, m.vc4, cur, cur + M,
                       static_cast<double*>(c->tracer_F.p), rec ? out + (size_t)rec_row * M : nullptr,
                       rec ? out + (rec_rows + (size_t)rec_row) * M : nullptr,
                       rec ? static_cast<double*>(c->tracer_F_out.p) + (size_t)rec_row * 4 * M : nullptr);
    HIPCHK(c, hipGetLastError());
    return LUDVM_OK;
  }
  double* slab = static_cast<double*>(c->tracer_part.p);
  hipLaunchKernelGGL(f32x2 ? march_f32x2_tracer_partial : march_tracer_partial, dim3((unsigned)p.tiles, (unsigned)p.nsplit), dim3(kBlock),
                     0, st, seed, seed + M, release, release + M, (const double*)cur, (const double*)(cur + M), shift, s, (long long)M,
                     p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                     static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, slab);
  HIPCHK(c, hipGetLastError());
  double* rec_x = rec_row >= 0 ? out + (size_t)rec_row * M : nullptr;
  double* rec_z = rec_row >= 0 ? out + (rec_rows + (size_t)rec_row) * M : nullptr;
  hipLaunchKernelGGL(march_tracer_finish, dim3(blocks_for((long long)M)), dim3(kBlock), 0, st, (const double*)slab, p.pad, p.nsplit,
                     seed, seed + M, release, shift, s, (long long)M, m.dt, cur, cur + M, rec_x, rec_z);
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// is time step s one of the survey's sampled steps?
bool survey_samples_step(const ludvm_ctx* c, long long s) {
  return c->survey_count != 0 && s >= c->survey_first && s < c->survey_stop && (s - c->survey_first) % c->survey_every == 0;
}

// The survey's sample of time step s: enqueued where the probes and the tracers are, behind march_solve of step s on the
// stream that ran it (and behind their kernels when they are set), so before the roll-up's finisher moves anything.  The
// slab and the sums are the survey's own buffers, touched only by these two kernels in stream order.  Reads the wake, writes
// nothing of it: rows, state, hist, the resident wake, the probe rows and the tracer paths keep their bits.
int march_survey_launch(ludvm_ctx* c, hipStream_t st, long long n_ub, long long s) {
  const MarchSetup& m = c->msetup;
  const size_t K = c->survey_count;
  const bool f32 = c->survey_precision == 1, gf32 = c->survey_gradient && c->survey_gradient_f32x2;
  const ObserverPlan p = observer_plan(kObserverRules[f32 || gf32 ? kObsSurveyF32 : kObsSurvey], (long long)K, n_ub + (long long)m.npan);
  const double* pxz = static_cast<const double*>(c->survey_xz.p);
  const double* shift = step_shift(c->survey_shift, c->survey_shifted, s);
  const int bin = c->survey_nbins ? c->survey_bin_of_row[(size_t)s] : -1;
  if (c->survey_gradient) {
    // the gradient pair takes the place of the plain pair.  float64: under the same plan (the setters see to it), the velocity
    // sums keep their bits.  hi+lo fp32: kObsSurveyF32's plan, its tiles each spread over kSurveyF32Tile / kSurveyGradF32Tile
    // workgroups (chunk, nsplit and pad are the plan's); the velocity sums are that walk's.  The gradient sums and the
    // five-column slab are further buffers of the survey's own
    double* gslab = static_cast<double*>(c->survey_grad_part.p);
    double* sums = static_cast<double*>(c->survey_sums.p);
    double* gsums = static_cast<double*>(c->survey_gsums.p);
    const unsigned gx = (unsigned)(gf32 ? p.tiles * (kSurveyF32Tile / kSurveyGradF32Tile) : p.tiles);
    hipLaunchKernelGGL(gf32 ? march_f32x2_grad_survey_partial : march_grad_survey_partial, dim3(gx, (unsigned)p.nsplit), dim3(kBlock), 0,
                       st, pxz, pxz + K, shift, (long long)K, p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                       static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, gslab);
    HIPCHK(c, hipGetLastError());
    if (bin >= 0)
      hipLaunchKernelGGL(march_binned_grad_survey_finish, dim3(blocks_for((long long)K)), dim3(kBlock), 0, st, (const double*)gslab,
                         p.pad, p.nsplit, (long long)K, m.vc4, sums, gsums,
                         static_cast<double*>(c->survey_bin_sums.p) + (size_t)bin * kSurveySums * K,
                         static_cast<double*>(c->survey_bin_gsums.p) + (size_t)bin * kSurveySums * K);
    else
      hipLaunchKernelGGL(march_grad_survey_finish, dim3(blocks_for((long long)K)), dim3(kBlock), 0, st, (const double*)gslab, p.pad,
                         p.nsplit, (long long)K, m.vc4, sums, gsums);
    HIPCHK(c, hipGetLastError());
    return LUDVM_OK;
  }
  double* slab = static_cast<double*>(c->survey_part.p);
  // (the two precisions' argument lists differ: the fp32 kernel's guard is in units of v_core)
  if (f32)
    hipLaunchKernelGGL(march_f32_survey_partial, dim3((unsigned)p.tiles, (unsigned)p.nsplit), dim3(kBlock), 0, st, pxz, pxz + K, shift,
                       (long long)K, p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                       static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, c->march_vcore, slab);
  else
    hipLaunchKernelGGL(march_survey_partial, dim3((unsigned)p.tiles, (unsigned)p.nsplit), dim3(kBlock), 0, st, pxz, pxz + K, shift,
                       (long long)K, p.pad, (const double*)c->x64, (const double*)c->z64, (const double*)c->g64,
                       static_cast<const MarchState*>(c->march_state.p), m.npan, p.chunk, m.vc4, slab);
  HIPCHK(c, hipGetLastError());
  // a step with a bin: one finisher, as without bins, that also updates the bin's block (the host knows the step's bin)
  if (bin >= 0)
    hipLaunchKernelGGL(march_binned_survey_finish, dim3(blocks_for((long long)K)), dim3(kBlock), 0, st, (const double*)slab, p.pad,
                       p.nsplit, (long long)K, static_cast<double*>(c->survey_sums.p),
                       static_cast<double*>(c->survey_bin_sums.p) + (size_t)bin * kSurveySums * K);
  else
    hipLaunchKernelGGL(march_survey_finish, dim3(blocks_for((long long)K)), dim3(kBlock), 0, st, (const double*)slab, p.pad, p.nsplit,
                       (long long)K, static_cast<double*>(c->survey_sums.p));
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// is time step s one of the energy's sampled steps?
bool energy_samples_step(const ludvm_ctx* c, long long s) {
  return c->integrals_on && c->energy_every > 0 && s >= c->energy_first && s < c->energy_stop &&
         (s - c->energy_first) % c->energy_every == 0;
}

// The wake integrals of time step s, row `rel` of the call: enqueued where the probes are, behind march_solve of step s on
// the stream that ran it, so before the roll-up's finisher moves anything.  The moments run at EVERY step (they also tag the
// vortices the step shed); the energy at its sampled steps, under the plan of the step's bound alone.  The tags, the partials,
// the slab and the rows are the observer's own buffers, touched only by these kernels in stream order.  Reads the wake,
// writes nothing of it: rows, state, hist, the resident wake and every other observer's results keep their bits.
int march_integral_launch(ludvm_ctx* c, hipStream_t st, long long n_ub, long long s, long long rel) {
  const MarchSetup& m = c->msetup;
  const long long ns_ub = n_ub + (long long)m.npan;
  if (n_ub > (long long)c->integral_cap) return fail(c, LUDVM_E_STATE, "march: the wake outgrew what ludvm_march_set_integrals sized");
  const MarchState* S = static_cast<const MarchState*>(c->march_state.p);
  double* part = static_cast<double*>(c->integral_part.p);
  const unsigned chunks = (unsigned)((ns_ub + kIntegralChunk - 1) / kIntegralChunk);
  hipLaunchKernelGGL(march_integral_partial, dim3(chunks), dim3(kBlock), 0, st, (const double*)c->x64, (const double*)c->z64,
                     (const double*)c->g64, S, m.npan, static_cast<unsigned char*>(c->integral_tags.p), part);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(march_integral_finish, dim3(1), dim3(64), 0, st, (const double*)part, S, m.npan,
                     static_cast<double*>(c->integral_out.p) + (size_t)rel * kIntegralSums);
  HIPCHK(c, hipGetLastError());
  if (!energy_samples_step(c, s)) return LUDVM_OK;
  const ObserverPlan p = energy_plan(ns_ub);
  if ((size_t)p.nsplit * (size_t)p.pad * 8 > c->energy_part.cap || (size_t)p.tiles * 8 > c->energy_tiles.cap)
    return fail(c, LUDVM_E_STATE, "march: the energy's slab is smaller than this step's plan");
  double* slab = static_cast<double*>(c->energy_part.p);
  double* tiles = static_cast<double*>(c->energy_tiles.p);
  hipLaunchKernelGGL(march_energy_partial, dim3((unsigned)p.tiles, (unsigned)p.nsplit), dim3(kBlock), 0, st, (const double*)c->x64,
                     (const double*)c->z64, (const double*)c->g64, S, m.npan, p.chunk, p.pad, m.vc4, slab);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(march_energy_tiles, dim3((unsigned)p.tiles), dim3(kBlock), 0, st, (const double*)slab, p.pad, p.nsplit,
                     (const double*)c->g64, S, m.npan, tiles);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(march_energy_finish, dim3(1), dim3(64), 0, st, (const double*)tiles, S, m.npan,
                     static_cast<double*>(c->energy_out.p) + (size_t)rel);
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// What the observers' setters share: `count` points (x, z) and, optionally, one x offset per kinematics row.  check_points
// validates them (`points` / `offsets`: the observer's nouns for the messages) and changes nothing; upload_points stores
// x | z in `xz` and the offsets in `shift`, enqueued on c->stream: the caller waits for the copies.
int check_points(ludvm_ctx* c, const double* x, const double* z, size_t count, const double* shift_x, size_t shift_rows,
                 const std::string& points, const std::string& offsets) {
  if (count && (!x || !z)) return fail(c, LUDVM_E_ARG, "null array");
  if (count && shift_x && shift_rows != c->march_kin_rows)
    return fail(c, LUDVM_E_ARG, "march: " + offsets + " must be one per kinematics row");
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(x[k]) || !std::isfinite(z[k])) return fail(c, LUDVM_E_ARG, "march: " + points + " must be finite");
  for (size_t k = 0; count && shift_x && k < shift_rows; ++k)
    if (!std::isfinite(shift_x[k])) return fail(c, LUDVM_E_ARG, "march: " + offsets + " must be finite");
  return LUDVM_OK;
}

int upload_points(ludvm_ctx* c, Buf& xz, Buf& shift, bool& shifted, const double* x, const double* z, size_t count,
                  const double* shift_x, size_t shift_rows) {
  CHK(ensure(c, xz, 2 * count * 8));
  if (shift_x) CHK(ensure(c, shift, shift_rows * 8));
  double* pxz = static_cast<double*>(xz.p);
  HIPCHK(c, hipMemcpyAsync(pxz, x, count * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(pxz + count, z, count * 8, hipMemcpyHostToDevice, c->stream));
  if (shift_x) HIPCHK(c, hipMemcpyAsync(shift.p, shift_x, shift_rows * 8, hipMemcpyHostToDevice, c->stream));
  shifted = shift_x != nullptr;
  return LUDVM_OK;
}

// the largest slab either precision's kernel of an observer may write
size_t slab_bytes(ObserverKind f64, ObserverKind f32, size_t count) {
  return std::max(observer_slab_bytes(kObserverRules[f64], (long long)count), observer_slab_bytes(kObserverRules[f32], (long long)count));
}

}  // namespace

extern "C" {

int ludvm_march_set_survey(ludvm_ctx* c, const double* x, const double* z, size_t count, const double* shift_x, size_t shift_rows,
                           long long first, long long stop, long long every, const double* sums, long long samples) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready) return fail(c, LUDVM_E_STATE, "ludvm_march_setup has not been called");
  if (c->shard_world > 1 || (c->comm && c->comm_world > 1))
    return fail(c, LUDVM_E_STATE, "march: the context is sharded; a survey runs on one device");
  if (count > LUDVM_MARCH_MAX_SURVEY) return fail(c, LUDVM_E_ARG, "march: at most " + std::to_string(LUDVM_MARCH_MAX_SURVEY) + " survey points");
  CHK(check_points(c, x, z, count, shift_x, shift_rows, "survey points", "survey offsets"));
  if (count && (first < 1 || every < 1)) return fail(c, LUDVM_E_ARG, "march: the survey window needs first >= 1 and every >= 1");
  if (count && sums && samples < 0) return fail(c, LUDVM_E_ARG, "march: survey samples must be >= 0");
  for (size_t k = 0; count && sums && k < kSurveySums * count; ++k)
    if (!std::isfinite(sums[k])) return fail(c, LUDVM_E_ARG, "march: survey sums must be finite");
  c->survey_count = 0;
  c->survey_samples = 0;
  c->survey_precision = 0;         // float64 until ludvm_march_set_survey_precision says otherwise
  c->survey_nbins = 0;             // (and no bins until ludvm_march_set_survey_bins)
  c->survey_gradient = c->survey_gradient_f32x2 = false;      // (and no gradient sums until ludvm_march_set_survey_gradient)
  if (count == 0) return LUDVM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->survey_sums, kSurveySums * count * 8));
  CHK(ensure(c, c->survey_part, slab_bytes(kObsSurvey, kObsSurveyF32, count)));
  CHK(upload_points(c, c->survey_xz, c->survey_shift, c->survey_shifted, x, z, count, shift_x, shift_rows));
  if (sums) HIPCHK(c, hipMemcpyAsync(c->survey_sums.p, sums, kSurveySums * count * 8, hipMemcpyHostToDevice, c->stream));
  else HIPCHK(c, hipMemsetAsync(c->survey_sums.p, 0, kSurveySums * count * 8, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->survey_first = first;
  c->survey_stop = std::min<long long>(stop, (long long)c->march_kin_rows);
  c->survey_every = every;
  c->survey_samples = sums ? samples : 0;
  c->survey_count = count;
  return LUDVM_OK;
}

int ludvm_march_set_survey_precision(ludvm_ctx* c, int precision) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  if (precision != 0 && precision != 1) return fail(c, LUDVM_E_ARG, "march: survey precision is 0 (float64) or 1 (fp32)");
  if (precision == 1 && c->survey_gradient) return fail(c, LUDVM_E_STATE, "march: the survey's gradient sums need a float64 survey");
  c->survey_precision = precision;
  return LUDVM_OK;
}

// gsums / bin_gsums (NULL: zeros) into the resident gradient sums, and the five-column slab [split][5][k_pad] of `kind`'s plan
// (5 / 2 of the plain one); the gradient sums are on, by the float64 pair (kObsSurvey) or by the hi+lo fp32 walk (kObsSurveyF32),
// when this returns LUDVM_OK.  A refusal leaves the context as it was; a failure behind it, without gradient sums.
static int survey_gradient_on(ludvm_ctx* c, const double* gsums, const double* bin_gsums, ObserverKind kind) {
  if (c->survey_precision != 0) return fail(c, LUDVM_E_STATE, "march: the survey's gradient sums need a float64 survey");
  const size_t K = c->survey_count, B = (size_t)c->survey_nbins;
  if (bin_gsums && B == 0) return fail(c, LUDVM_E_ARG, "march: survey bin gradient sums without survey bins");
  if (bin_gsums && !gsums) return fail(c, LUDVM_E_ARG, "march: survey bin gradient sums come with the gradient sums");
  if (!gsums) {
    // one count serves the velocity and the gradient sums: sums that start from zero start with the survey
    bool sampled = c->survey_samples != 0;
    for (size_t b = 0; b < B; ++b) sampled = sampled || c->survey_bin_samples[b] != 0;
    if (sampled) return fail(c, LUDVM_E_STATE, "march: the survey already has samples; its gradient sums must be given");
  }
  for (size_t k = 0; gsums && k < kSurveySums * K; ++k)
    if (!std::isfinite(gsums[k])) return fail(c, LUDVM_E_ARG, "march: survey gradient sums must be finite");
  for (size_t k = 0; bin_gsums && k < B * kSurveySums * K; ++k)
    if (!std::isfinite(bin_gsums[k])) return fail(c, LUDVM_E_ARG, "march: survey bin gradient sums must be finite");
  c->survey_gradient = c->survey_gradient_f32x2 = false;      // (a failure from here on leaves the context without gradient sums)
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->survey_gsums, kSurveySums * K * 8));
  if (B) CHK(ensure(c, c->survey_bin_gsums, B * kSurveySums * K * 8));
  CHK(ensure(c, c->survey_grad_part, observer_slab_bytes(kObserverRules[kind], (long long)K) / 2 * 5));
  if (gsums) HIPCHK(c, hipMemcpyAsync(c->survey_gsums.p, gsums, kSurveySums * K * 8, hipMemcpyHostToDevice, c->stream));
  else HIPCHK(c, hipMemsetAsync(c->survey_gsums.p, 0, kSurveySums * K * 8, c->stream));
  if (B && bin_gsums)
    HIPCHK(c, hipMemcpyAsync(c->survey_bin_gsums.p, bin_gsums, B * kSurveySums * K * 8, hipMemcpyHostToDevice, c->stream));
  else if (B) HIPCHK(c, hipMemsetAsync(c->survey_bin_gsums.p, 0, B * kSurveySums * K * 8, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->survey_gradient = true;
  c->survey_gradient_f32x2 = kind == kObsSurveyF32;
  return LUDVM_OK;
}

int ludvm_march_set_survey_gradient(ludvm_ctx* c, int on, const double* gsums, const double* bin_gsums) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  if (on != 0 && on != 1) return fail(c, LUDVM_E_ARG, "march: the survey gradient flag is 0 or 1");
  if (!on) {
    c->survey_gradient = c->survey_gradient_f32x2 = false;      // (the sums and, where it was on, the hi+lo fp32 route)
    return LUDVM_OK;
  }
  return survey_gradient_on(c, gsums, bin_gsums, kObsSurvey);
}

int ludvm_march_set_survey_gradient_f32x2(ludvm_ctx* c, const double* gsums, const double* bin_gsums) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  return survey_gradient_on(c, gsums, bin_gsums, kObsSurveyF32);
}

int ludvm_march_read_survey_gradient(ludvm_ctx* c, double* gsums, double* bin_gsums) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  if (!c->survey_gradient) return fail(c, LUDVM_E_STATE, "march: the survey's gradient sums are not on");
  if (!gsums) return fail(c, LUDVM_E_ARG, "null array");
  if (bin_gsums && c->survey_nbins == 0) return fail(c, LUDVM_E_ARG, "march: survey bin gradient sums without survey bins");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(gsums, c->survey_gsums.p, kSurveySums * c->survey_count * 8, hipMemcpyDeviceToHost, c->stream));
  if (bin_gsums)
    HIPCHK(c, hipMemcpyAsync(bin_gsums, c->survey_bin_gsums.p, (size_t)c->survey_nbins * kSurveySums * c->survey_count * 8,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LUDVM_OK;
}

int ludvm_march_read_survey(ludvm_ctx* c, double* sums, long long* samples) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  if (!sums || !samples) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(sums, c->survey_sums.p, kSurveySums * c->survey_count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *samples = c->survey_samples;
  return LUDVM_OK;
}

int ludvm_march_set_survey_bins(ludvm_ctx* c, const int* bin_of_row, size_t rows, int nbins, const double* sums,
                                const long long* counts) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0) return fail(c, LUDVM_E_STATE, "march: no survey is set");
  const size_t K = c->survey_count;
  if (nbins < 0 || nbins > LUDVM_MARCH_MAX_SURVEY_BINS)
    return fail(c, LUDVM_E_ARG, "march: at most " + std::to_string(LUDVM_MARCH_MAX_SURVEY_BINS) + " survey bins");
  if (nbins == 0) {
    c->survey_nbins = 0;
    c->survey_gradient = c->survey_gradient_f32x2 = false;    // (the gradient sums are set after the bins)
    return LUDVM_OK;
  }
  if ((size_t)nbins * K > (size_t)LUDVM_MARCH_MAX_SURVEY_BIN_POINTS)
    return fail(c, LUDVM_E_ARG, "march: survey bins x points over " + std::to_string(LUDVM_MARCH_MAX_SURVEY_BIN_POINTS) +
                                    " (40 bytes of sums per bin and point)");
  if (!bin_of_row) return fail(c, LUDVM_E_ARG, "null array");
  if (rows != c->march_kin_rows) return fail(c, LUDVM_E_ARG, "march: survey bins must be one per kinematics row");
  if ((sums == nullptr) != (counts == nullptr))
    return fail(c, LUDVM_E_ARG, "march: survey bin sums and counts are given together or not at all");
  for (size_t k = 0; k < rows; ++k)
    if (bin_of_row[k] < -1 || bin_of_row[k] >= nbins) return fail(c, LUDVM_E_ARG, "march: a survey bin lies in [-1, nbins)");
  const size_t doubles = (size_t)nbins * kSurveySums * K;
  for (size_t k = 0; sums && k < doubles; ++k)
    if (!std::isfinite(sums[k])) return fail(c, LUDVM_E_ARG, "march: survey bin sums must be finite");
  for (int b = 0; counts && b < nbins; ++b)
    if (counts[b] < 0) return fail(c, LUDVM_E_ARG, "march: survey bin counts must be >= 0");
  c->survey_nbins = 0;             // (a failure from here on leaves the context without bins)
  c->survey_gradient = c->survey_gradient_f32x2 = false;      // (the gradient sums are set after the bins)
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->survey_bin_sums, doubles * 8));
  if (sums) HIPCHK(c, hipMemcpyAsync(c->survey_bin_sums.p, sums, doubles * 8, hipMemcpyHostToDevice, c->stream));
  else HIPCHK(c, hipMemsetAsync(c->survey_bin_sums.p, 0, doubles * 8, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->survey_bin_of_row.assign(bin_of_row, bin_of_row + rows);
  if (counts) c->survey_bin_samples.assign(counts, counts + nbins);
  else c->survey_bin_samples.assign((size_t)nbins, 0);
  c->survey_nbins = nbins;
  return LUDVM_OK;
}

int ludvm_march_read_survey_bins(ludvm_ctx* c, double* sums, long long* counts) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->survey_count == 0 || c->survey_nbins == 0) return fail(c, LUDVM_E_STATE, "march: no survey bins are set");
  if (!sums || !counts) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(sums, c->survey_bin_sums.p, (size_t)c->survey_nbins * kSurveySums * c->survey_count * 8,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < c->survey_nbins; ++b) counts[b] = c->survey_bin_samples[(size_t)b];
  return LUDVM_OK;
}

int ludvm_march_set_tracers(ludvm_ctx* c, const double* seed_x, const double* seed_z, const long long* release, size_t count,
                            const double* shift_x, size_t shift_rows, const double* cur_x, const double* cur_z,
                            const long long* record_steps, size_t nrecord) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready) return fail(c, LUDVM_E_STATE, "ludvm_march_setup has not been called");
  if (count > LUDVM_MARCH_MAX_TRACERS) return fail(c, LUDVM_E_ARG, "march: at most " + std::to_string(LUDVM_MARCH_MAX_TRACERS) + " tracers");
  CHK(check_points(c, seed_x, seed_z, count, shift_x, shift_rows, "tracer seeds", "tracer offsets"));
  if (count && ((cur_x == nullptr) != (cur_z == nullptr))) return fail(c, LUDVM_E_ARG, "march: tracer positions need both cur_x and cur_z");
  if (count && nrecord && !record_steps) return fail(c, LUDVM_E_ARG, "null array");
  for (size_t k = 0; k < count; ++k) {
    if (cur_x && (!std::isfinite(cur_x[k]) || !std::isfinite(cur_z[k]))) return fail(c, LUDVM_E_ARG, "march: tracer positions must be finite");
    if (release && release[k] < 1) return fail(c, LUDVM_E_ARG, "march: tracer release steps must be >= 1");
  }
  for (size_t k = 0; count && k < nrecord; ++k)
    if (record_steps[k] < 1 || (size_t)record_steps[k] >= c->march_kin_rows || (k && record_steps[k] <= record_steps[k - 1]))
      return fail(c, LUDVM_E_ARG, "march: tracer record steps must be ascending and inside the kinematics table");
  c->tracer_count = 0;
  c->tracer_ran = false;
  c->tracer_record.clear();
  c->tracer_rows.clear();
  c->tracer_precision = 0;         // float64 until ludvm_march_set_tracer_precision says otherwise
  c->tracer_gradient = false;      // no deformation gradient until ludvm_march_set_tracer_gradient says otherwise
  c->tracer_grad_ran = false;
  if (count == 0) return LUDVM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const long long ttiles = observer_tiles(kObserverRules[kObsTracers], (long long)count);
  // host images: release steps (NULL: all 1) with the earliest release of every tile behind them; the first positions
  std::vector<long long> rel(count + (size_t)ttiles);
  for (size_t k = 0; k < count; ++k) rel[k] = release ? release[k] : 1;
  for (long long t = 0; t < ttiles; ++t) {
    const size_t lo = (size_t)t * kTracerTile, hi = std::min(count, lo + (size_t)kTracerTile);
    rel[count + (size_t)t] = *std::min_element(rel.begin() + lo, rel.begin() + hi);
  }
  std::vector<double> cur(2 * count);
  for (size_t k = 0; k < count; ++k) {
    cur[k] = cur_x ? cur_x[k] : seed_x[k] + (shift_x ? shift_x[0] : 0.0);
    cur[count + k] = cur_z ? cur_z[k] : seed_z[k];
  }
  CHK(ensure(c, c->tracer_release, rel.size() * 8));
  CHK(ensure(c, c->tracer_cur, 2 * count * 8));
  CHK(ensure(c, c->tracer_part, slab_bytes(kObsTracers, kObsTracersF32x2, count)));
  CHK(upload_points(c, c->tracer_seed, c->tracer_shift, c->tracer_shifted, seed_x, seed_z, count, shift_x, shift_rows));
  HIPCHK(c, hipMemcpyAsync(c->tracer_release.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->tracer_cur.p, cur.data(), 2 * count * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // (rel and cur live on this frame)
  c->tracer_record.assign(record_steps, record_steps + nrecord);
  c->tracer_count = count;
  return LUDVM_OK;
}

int ludvm_march_set_tracer_precision(ludvm_ctx* c, int precision) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (precision != 0 && precision != 2) return fail(c, LUDVM_E_ARG, "march: tracer precision is 0 (float64) or 2 (hi+lo fp32)");
  if (c->tracer_gradient && c->tracer_precision == 2)
    return fail(c, LUDVM_E_STATE, "march: the tracers carry their deformation gradient in hi+lo fp32 (ludvm_march_set_tracer_gradient_f32x2); "
                                  "switch it off first");
  if (precision == 2 && c->tracer_gradient) return fail(c, LUDVM_E_STATE, "march: the tracers' deformation gradient needs float64 tracers");
  c->tracer_precision = precision;
  return LUDVM_OK;
}

// F (NULL: the identity) into the resident F11 | F12 | F21 | F22 [M], and the five-column slab [split][5][m_pad] of `kind`'s plan
// (5 / 2 of the plain one); the deformation gradient is on when this returns LUDVM_OK
static int tracer_gradient_on(ludvm_ctx* c, const double* F, ObserverKind kind) {
  const size_t M = c->tracer_count;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> f(4 * M, 0.0);
  if (F) std::copy(F, F + 4 * M, f.begin());
  else std::fill(f.begin(), f.begin() + M, 1.0), std::fill(f.begin() + 3 * M, f.end(), 1.0);
  CHK(ensure(c, c->tracer_F, 4 * M * 8));
  CHK(ensure(c, c->tracer_grad_part, observer_slab_bytes(kObserverRules[kind], (long long)M) / 2 * 5));
  HIPCHK(c, hipMemcpyAsync(c->tracer_F.p, f.data(), 4 * M * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // (f lives on this frame)
  c->tracer_gradient = true;
  c->tracer_grad_ran = false;
  return LUDVM_OK;
}

int ludvm_march_set_tracer_gradient(ludvm_ctx* c, int on, const double* F) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (on != 0 && on != 1) return fail(c, LUDVM_E_ARG, "march: the tracer gradient flag is 0 or 1");
  const size_t M = c->tracer_count;
  if (on && c->tracer_precision != 0) return fail(c, LUDVM_E_STATE, "march: the tracers' deformation gradient needs float64 tracers");
  if (on && F)
    for (size_t k = 0; k < 4 * M; ++k)
      if (!std::isfinite(F[k])) return fail(c, LUDVM_E_ARG, "march: the tracers' deformation gradient must be finite");
  if (!on) {
    c->tracer_gradient = false;      // (the tracers keep their precision: plain hi+lo fp32 tracers after the fp32 route)
    c->tracer_grad_ran = false;
    return LUDVM_OK;
  }
  return tracer_gradient_on(c, F, kObsTracers);
}

int ludvm_march_set_tracer_gradient_f32x2(ludvm_ctx* c, const double* F) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (F)
    for (size_t k = 0; k < 4 * c->tracer_count; ++k)
      if (!std::isfinite(F[k])) return fail(c, LUDVM_E_ARG, "march: the tracers' deformation gradient must be finite");
  CHK(tracer_gradient_on(c, F, kObsTracersF32x2));
  c->tracer_precision = 2;
  return LUDVM_OK;
}

int ludvm_march_read_tracer_gradient(ludvm_ctx* c, double* F, size_t rows_cap, long long* steps_out, size_t* nrows_out) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (!c->tracer_gradient) return fail(c, LUDVM_E_STATE, "march: the tracers' deformation gradient is not on");
  if (!c->tracer_ran || !c->tracer_grad_ran)
    return fail(c, LUDVM_E_STATE, "march: no ludvm_march_run call has succeeded since the tracers' deformation gradient was set");
  if (!nrows_out) return fail(c, LUDVM_E_ARG, "null array");
  const size_t rows = c->tracer_rows.size();
  *nrows_out = rows;
  if (rows_cap < rows) return fail(c, LUDVM_E_ARG, "march: the last ludvm_march_run call recorded " + std::to_string(rows) + " tracer rows");
  if (rows == 0) return LUDVM_OK;
  if (!F || !steps_out) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(F, c->tracer_F_out.p, rows * 4 * c->tracer_count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < rows; ++k) steps_out[k] = c->tracer_rows[k];
  return LUDVM_OK;
}

int ludvm_march_tracer_gradient_state(ludvm_ctx* c, double* F) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (!c->tracer_gradient) return fail(c, LUDVM_E_STATE, "march: the tracers' deformation gradient is not on");
  if (!F) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(F, c->tracer_F.p, 4 * c->tracer_count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LUDVM_OK;
}

int ludvm_march_read_tracers(ludvm_ctx* c, double* x, double* z, size_t rows_cap, long long* steps_out, size_t* nrows_out) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (!c->tracer_ran) return fail(c, LUDVM_E_STATE, "march: no ludvm_march_run call has succeeded since the tracers were set");
  if (!nrows_out) return fail(c, LUDVM_E_ARG, "null array");
  const size_t rows = c->tracer_rows.size();
  *nrows_out = rows;
  if (rows_cap < rows) return fail(c, LUDVM_E_ARG, "march: the last ludvm_march_run call recorded " + std::to_string(rows) + " tracer rows");
  if (rows == 0) return LUDVM_OK;
  if (!x || !z || !steps_out) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = rows * c->tracer_count;
  const double* out = static_cast<const double*>(c->tracer_out.p);
  HIPCHK(c, hipMemcpyAsync(x, out, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(z, out + n, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < rows; ++k) steps_out[k] = c->tracer_rows[k];
  return LUDVM_OK;
}

int ludvm_march_tracer_state(ludvm_ctx* c, double* x, double* z) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->tracer_count == 0) return fail(c, LUDVM_E_STATE, "march: no tracers are set");
  if (!x || !z) return fail(c, LUDVM_E_ARG, "null array");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t M = c->tracer_count;
  const double* cur = static_cast<const double*>(c->tracer_cur.p);
  HIPCHK(c, hipMemcpyAsync(x, cur, M * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(z, cur + M, M * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LUDVM_OK;
}

int ludvm_march_set_probes(ludvm_ctx* c, const double* x, const double* z, size_t count, const double* shift_x, size_t shift_rows) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready) return fail(c, LUDVM_E_STATE, "ludvm_march_setup has not been called");
  if (count > LUDVM_MARCH_MAX_PROBES) return fail(c, LUDVM_E_ARG, "march: at most " + std::to_string(LUDVM_MARCH_MAX_PROBES) + " probes");
  CHK(check_points(c, x, z, count, shift_x, shift_rows, "probe positions", "probe offsets"));
  c->probe_count = 0;
  c->probe_rows = 0;
  if (count == 0) return LUDVM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->probe_part, observer_slab_bytes(kObserverRules[kObsProbes], (long long)count)));
  CHK(upload_points(c, c->probe_xz, c->probe_shift, c->probe_shifted, x, z, count, shift_x, shift_rows));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->probe_count = count;
  return LUDVM_OK;
}

int ludvm_march_read_probes(ludvm_ctx* c, double* u, double* w, size_t rows) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || c->probe_count == 0) return fail(c, LUDVM_E_STATE, "march: no probes are set");
  if (c->probe_rows == 0) return fail(c, LUDVM_E_STATE, "march: no ludvm_march_run call has left probe rows");
  if (!u || !w) return fail(c, LUDVM_E_ARG, "null array");
  if (rows != c->probe_rows) return fail(c, LUDVM_E_ARG, "march: rows must equal the count of the last ludvm_march_run call");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = rows * c->probe_count;
  const double* out = static_cast<const double*>(c->probe_out.p);
  HIPCHK(c, hipMemcpyAsync(u, out, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(w, out + n, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LUDVM_OK;
}

int ludvm_march_set_integrals(ludvm_ctx* c, int on, const unsigned char* tags, size_t ntags, long long energy_first,
                              long long energy_stop, long long energy_every) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready) return fail(c, LUDVM_E_STATE, "ludvm_march_setup has not been called");
  if (!on) {
    c->integrals_on = false;
    c->integral_rows = 0;
    return LUDVM_OK;
  }
  if (c->shard_world > 1 || c->comm_world > 1)
    return fail(c, LUDVM_E_STATE, "march: the wake integrals run on one GPU: not on a sharded or multi-device context");
  // everything is validated before anything is changed
  if (ntags != c->wake_n) return fail(c, LUDVM_E_ARG, "march: one tag per vortex of the resident wake (" + std::to_string(c->wake_n) + ")");
  if (ntags && !tags) return fail(c, LUDVM_E_ARG, "null array");
  for (size_t k = 0; k < ntags; ++k)
    if (tags[k] > kClassLev) return fail(c, LUDVM_E_ARG, "march: a tag is 0 (FREE), 1 (TEV) or 2 (LEV)");
  if (energy_every < 0 || (energy_every > 0 && (energy_first < 1 || energy_stop <= energy_first)))
    return fail(c, LUDVM_E_ARG, "march: the energy window needs first >= 1, stop > first and every >= 1 (every = 0: no samples)");
  HIPCHK(c, hipSetDevice(c->device));
  c->integrals_on = false;
  c->integral_rows = 0;
  // the run's cap: at most two vortices per remaining kinematics row on top of the wake as it stands
  const size_t cap = c->wake_n + 2 * c->march_kin_rows;
  const size_t ns_cap = cap + (size_t)c->msetup.npan;
  CHK(ensure(c, c->integral_tags, cap + 64));
  CHK(ensure(c, c->integral_part, (ns_cap + kIntegralChunk - 1) / kIntegralChunk * kIntegralSums * 8));
  if (energy_every > 0) {
    CHK(ensure(c, c->energy_part, energy_slab_bytes((long long)ns_cap)));
    CHK(ensure(c, c->energy_tiles, (size_t)observer_tiles(kEnergyRule, (long long)ns_cap) * 8));
  }
  if (ntags) {
    HIPCHK(c, hipMemcpyAsync(c->integral_tags.p, tags, ntags, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->integral_tagged = ntags;
  c->integral_cap = cap;
  c->energy_first = energy_first; c->energy_stop = energy_stop; c->energy_every = energy_every;
  c->integrals_on = true;
  return LUDVM_OK;
}

int ludvm_march_read_integrals(ludvm_ctx* c, double* sums, double* energy, size_t rows) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready || !c->integrals_on) return fail(c, LUDVM_E_STATE, "march: the wake integrals are not set");
  if (c->integral_rows == 0) return fail(c, LUDVM_E_STATE, "march: no ludvm_march_run call has left integral rows");
  if (!sums || !energy) return fail(c, LUDVM_E_ARG, "null array");
  if (rows != c->integral_rows) return fail(c, LUDVM_E_ARG, "march: rows must equal the count of the last ludvm_march_run call");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(sums, c->integral_out.p, rows * kIntegralSums * 8, hipMemcpyDeviceToHost, c->stream));
  bool sampled = false;
  for (size_t r = 0; r < rows; ++r) sampled = sampled || energy_samples_step(c, c->integral_first_step + (long long)r);
  if (sampled) HIPCHK(c, hipMemcpyAsync(energy, c->energy_out.p, rows * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t r = 0; r < rows; ++r)
    if (!energy_samples_step(c, c->integral_first_step + (long long)r)) energy[r] = std::numeric_limits<double>::quiet_NaN();
  return LUDVM_OK;
}

int ludvm_march_run(ludvm_ctx* c, long long first_step, long long count, int precision, double* state, double* rows,
                    double* hist, size_t hist_nmax, const long long* anchors) {
  if (!c) return LUDVM_E_ARG;
  if (!c->march_ready) return fail(c, LUDVM_E_STATE, "ludvm_march_setup has not been called");
  c->probe_rows = 0;
  c->integral_rows = 0;
  c->tracer_ran = false;
  c->tracer_grad_ran = false;
  c->tracer_rows.clear();
  if (!valid_precision(precision)) return fail(c, LUDVM_E_ARG, "unknown precision");
  if (!state || !rows) return fail(c, LUDVM_E_ARG, "null array");
  if (count < 1 || first_step < 1 || (size_t)(first_step + count) > c->march_kin_rows)
    return fail(c, LUDVM_E_ARG, "march: steps outside the kinematics table");
  const MarchSetup& m = c->msetup;
  const size_t P = (size_t)m.npan, nfoil = P;
  const size_t row_doubles = kMarchRowHead + 2 * (size_t)m.ncoef + 2 * P;
  const long long n0 = (long long)c->wake_n;
  if ((long long)state[0] != n0) return fail(c, LUDVM_E_ARG, "march: state[0] must be the current wake size");
  if (n0 + 2 * count + (long long)nfoil >= (1LL << 32)) return fail(c, LUDVM_E_ARG, "march: wake too large");
  if (hist && (long long)hist_nmax < n0 + 2 * count) return fail(c, LUDVM_E_ARG, "march: history rows shorter than the wake can get");
  HIPCHK(c, hipSetDevice(c->device));
  // everything that could reallocate happens before the first launch: the steps then run without a host sync
  CHK(wake_grow(c, (size_t)(n0 + 2 * count) + nfoil));
  size_t part_bytes = 0, acc_bytes = 0;
  for (long long k = 0; k <= count; k += std::max<long long>(1, count / 256))
    march_workspace(c, n0 + 2 * k, precision, nfoil, part_bytes, acc_bytes);
  march_workspace(c, n0 + 2 * count, precision, nfoil, part_bytes, acc_bytes);
  CHK(ensure(c, c->part, part_bytes + (1 << 20)));
  if (acc_bytes && !c->ext_acc) CHK(ensure(c, c->acc, acc_bytes + (1 << 20)));
  if (acc_bytes && c->ext_acc && acc_bytes + 16 > c->ext_acc_bytes)
    return fail(c, LUDVM_E_NOMEM, "march: the accumulator buffer given to ludvm_set_shard is too small for this stretch");
  CHK(ensure(c, c->symsc, 128));
  CHK(ensure(c, c->march_rows, (size_t)count * row_doubles * 8));
  if (hist) CHK(ensure(c, c->march_hist, (size_t)count * 2 * hist_nmax * 8));
  const bool probes = c->probe_count != 0;
  if (probes) CHK(ensure(c, c->probe_out, (size_t)count * 2 * c->probe_count * 8));      // (the slab: ludvm_march_set_probes)
  const bool integrals = c->integrals_on;
  if (integrals) {
    // (the tags, the partials and the energy's slab: ludvm_march_set_integrals, for the run's cap)
    if (c->integral_tagged != (size_t)n0)
      return fail(c, LUDVM_E_STATE, "march: the resident wake changed since ludvm_march_set_integrals tagged it");
    if ((size_t)(n0 + 2 * count) > c->integral_cap)
      return fail(c, LUDVM_E_STATE, "march: the wake can outgrow what ludvm_march_set_integrals sized");
    CHK(ensure(c, c->integral_out, (size_t)count * kIntegralSums * 8));
    if (c->energy_every > 0) CHK(ensure(c, c->energy_out, (size_t)count * 8));
  }
  const bool tracers = c->tracer_count != 0;
  std::vector<long long> trec;      // the call's recorded tracer steps, ascending: row k of the record is step trec[k]
  if (tracers) {
    for (long long r : c->tracer_record)
      if (r >= first_step && r < first_step + count) trec.push_back(r);
    if (!trec.empty()) CHK(ensure(c, c->tracer_out, trec.size() * 2 * c->tracer_count * 8));
    if (!trec.empty() && c->tracer_gradient) CHK(ensure(c, c->tracer_F_out, trec.size() * 4 * c->tracer_count * 8));
  }
  size_t trec_at = 0;               // the next recorded step
  const bool survey = c->survey_count != 0;
  long long surveyed = 0;           // sampled steps of this call
  std::vector<long long> binned(survey ? (size_t)c->survey_nbins : 0, 0);     // ... and those of every bin
  auto count_bin = [&](long long sstep) {
    if (binned.empty()) return;
    const int b = c->survey_bin_of_row[(size_t)sstep];
    if (b >= 0) ++binned[(size_t)b];
  };

  MarchState hs{};
  hs.n = n0;
  hs.itev = (long long)state[1];
  hs.ilev = (long long)state[2];
  hs.shed = state[3] != 0.0;
  hs.tail = 0;
  hs.lesp_crit = state[4]; hs.sum_tev = state[5]; hs.sum_lev = state[6];
  for (int k = 0; k < 4; ++k) hs.place[k] = state[7 + k];
  for (int k = 0; k < m.ncoef; ++k) hs.prevA[k] = state[16 + k];
  MarchState* S = static_cast<MarchState*>(c->march_state.p);
  HIPCHK(c, hipMemcpyAsync(S, &hs, sizeof(MarchState), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // hs lives on this stack frame
  for (int k = 0; k < kProgressRing; ++k) c->progress[k] = 0;

  double* drows = static_cast<double*>(c->march_rows.p);
  const double* kin = static_cast<const double*>(c->march_kin.p);
  const size_t krow = 7 + 2 * P;
  hipLaunchKernelGGL(march_begin, dim3(1), dim3(kBlock), 0, c->stream, S, kin + (size_t)first_step * krow, (int)P,
                     (int)(first_step & 1), c->g64, m.vc4);
  HIPCHK(c, hipGetLastError());

  // The wake size is decided on the device (LEV shedding); the host needs an upper bound of it to size each step's
  // launches, and -- for the direct kernels -- that bound also fixes how the sources are split, i.e. the summation
  // order.  Every kSyncEvery steps the host waits for the event it recorded 2 * kSyncEvery steps earlier and reads,
  // from the progress ring, the wake size after the last step enqueued BEFORE that event: a step that is certainly
  // finished, and always the same one.  All bounds are therefore functions of the call's arguments and of the
  // simulation itself, never of how far the host happens to run ahead: two runs repeat bit for bit, direct or
  // symmetric kernel (whose fixed-point sums do not depend on the order of their atomics).
  //
  // Round 3: the bounds no longer restart at the call.  Step s is sized from the ANCHOR step A(s) = 64 (floor(s / 64) - 2) - 1
  // (the last step of the sync period two periods back; step 0 for the first 128 steps of a run): an anchor inside this
  // call is read from the ring as above, an anchor before it is given by the caller in `anchors` (the class knows the wake
  // size after every step it has run).  Tile size, waves per item, serial or overlapped step and the direct kernels'
  // source splits are then functions of the step number and of the simulation alone: the same bits whatever the chunking
  // (march_chunk, checkpoint_every, dense or sparse history) -- and a resumed run continues bit for bit.
  // Round 4 (ABI 4): FOUR anchors, periods floor(first_step / 64) - 3 + q, in an argument of their own.  The bound after
  // step first_step - 1 -- the first step's `n_before` -- belongs to the period before first_step's when first_step is a
  // multiple of 64, one period further back than the three that state[12..14] used to carry: every call that began at
  // 192, 256, 320, ... failed with "anchor step not among the caller's" (default chunks never start there,
  // snapshot_steps, checkpoint_every and resume do).  -1 = not given (0 is a wake size: a run without free vortices has
  // an empty wake after step 0); anchors = NULL or all four -1: the bounds restart at this call's exact wake size.
  constexpr long long kSyncEvery = 64;
  auto anchor_of = [](long long s) { return std::max<long long>(kSyncEvery * (s / kSyncEvery - 2) - 1, 0); };
  long long ev_anchor[2] = {-1, -1};      // the last step enqueued before the slot's event was recorded
  const long long k0 = first_step / kSyncEvery - 3;
  long long given_step[4], given_n[4];
  bool anchors_given = false;
  for (int q = 0; q < 4; ++q) {
    given_step[q] = std::max<long long>(kSyncEvery * (k0 + q) - 1, 0);
    given_n[q] = anchors ? anchors[q] : -1;
    if (given_n[q] < 0) continue;
    anchors_given = true;
    // a given size must be one the wake can have had: one or two vortices per step between the anchor and now
    const long long gap = first_step - 1 - given_step[q];
    if (gap < 0 || given_n[q] + gap > n0 || given_n[q] + 2 * gap < n0)
      return fail(c, LUDVM_E_ARG, "march: anchors[] (wake sizes after the anchor steps) contradict state[0]");
  }
  long long cur_a = -1, cur_n = 0;        // the anchor in force and the wake size after it
  // wake size after step s's solve is at most n_after(anchor) + 2 (s - anchor)
  auto set_anchor = [&](long long sstep) -> int {
    const long long a = anchor_of(sstep);
    if (!anchors_given && a < first_step) {
      // (no history from the caller: anchors before the call are replaced by the call's own start)
      cur_a = first_step - 1; cur_n = n0;
      return LUDVM_OK;
    }
    if (a == cur_a) return LUDVM_OK;
    if (a < first_step) {
      for (int q = 0; q < 4; ++q)
        if (given_step[q] == a && given_n[q] >= 0) { cur_a = a; cur_n = given_n[q]; return LUDVM_OK; }
      return fail(c, LUDVM_E_ARG, "march: the wake size after anchor step " + std::to_string(a) + " is not among anchors[]");
    }
    const int slot = (int)(((a + 1) / kSyncEvery) & 1);
    if (ev_anchor[slot] != a) return fail(c, LUDVM_E_STATE, "march: no event for the anchor step");
    HIPCHK(c, hipEventSynchronize(c->march_ev[slot]));
    const unsigned long long w = __atomic_load_n(c->progress + (a % kProgressRing), __ATOMIC_RELAXED);
    if ((long long)(w >> 32) != a) return fail(c, LUDVM_E_STATE, "march: progress ring out of step");
    cur_a = a;
    cur_n = (long long)(w & 0xffffffffULL);
    return LUDVM_OK;
  };
  CHK(set_anchor(first_step - 1 > 0 ? first_step - 1 : 0));
  long long prev_ub = cur_n + 2 * (std::max<long long>(first_step - 1, 0) - cur_a);   // bound after step first_step - 1
  if (prev_ub < n0) return fail(c, LUDVM_E_ARG, "march: anchors[] contradict state[0]");
  bool overlapped = false;          // the accumulators have been zeroed for the overlapped steps
  bool fork_signalled = false;      // the previous step's finisher already signals ev_fork
  static const bool ext_fork = [] { const char* e = LUDVM_EXP_ENV("LUDVM_MARCH_EXT_EVENTS"); return !(e && e[0] == '0'); }();
  // LUDVM_MARCH_OVERLAP=0 keeps every step serial (A/B measurements; results agree to fp32 rounding)
  const char* ov_env = LUDVM_EXP_ENV("LUDVM_MARCH_OVERLAP");
  const bool overlap_ok = !(ov_env && ov_env[0] == '0');
  hipStream_t const main_stream = c->stream;
  const double vc4 = m.vc4;
  const long long thr = sym_threshold(c, overlap_ok);      // serial symmetric steps pay from the usual size only
  for (long long s = first_step; s < first_step + count; ++s) {
    const long long rel = s - first_step;
    CHK(set_anchor(s));       // (may wait for, and read, the event slot that is re-used just below)
    if (s % kSyncEvery == 0 && s - 1 >= first_step) {
      // everything up to step s - 1 is enqueued: this event's completion makes s - 1 an anchor that can be read
      const int slot = (int)((s / kSyncEvery) & 1);
      HIPCHK(c, hipEventRecord(c->march_ev[slot], c->stream));
      ev_anchor[slot] = s - 1;
    }
    // wake size after this step's solve: at most two vortices per step since the anchor
    const long long n_ub = cur_n + 2 * (s - cur_a);
    const long long n_lo = cur_n + (s - 1 - cur_a);      // ... and before it: at least one per step
    long long n_before = std::min<long long>(prev_ub, n_ub);     // upper bound of the wake size before this step's solve
    prev_ub = n_ub;
    const bool symreg = precision != LUDVM_PREC_F64 && use_symmetric(c, n_ub, vc4, overlap_ok);
    // overlapped steps need an old wake that already fills the symmetric kernel
    const bool fork = symreg && overlap_ok && n_lo >= thr;
    const double* krow_s = kin + (size_t)s * krow;
    const double* krow_next = (size_t)(s + 1) < c->march_kin_rows ? kin + (size_t)(s + 1) * krow : nullptr;
    TailDuty td = make_tail_duty(S, s, krow_next, (int)P);
    if (hist) {
      td.hist_row = static_cast<double*>(c->march_hist.p) + (size_t)rel * 2 * hist_nmax;
      td.hist_nmax = (long long)hist_nmax;
    }
    double* row = drows + (size_t)rel * row_doubles;
    if (!fork) {
      // serial step: chord sums -> solve -> roll-up (direct, or symmetric with its memset) and Euler finisher
      CHK(march_chord_launch(c, n_before));
      hipLaunchKernelGGL(march_solve, dim3(1), dim3(kBlock), 0, c->stream, m, S, krow_s, row, s, c->x64, c->z64, c->g64,
                         c->mir(), c->g32, c->progress_dev);
      HIPCHK(c, hipGetLastError());
      if (probes) CHK(march_probe_launch(c, c->stream, n_ub, s, rel, count));
      if (tracers) {
        const bool rec = trec_at < trec.size() && trec[trec_at] == s;
        CHK(march_tracer_launch(c, c->stream, n_ub, s, rec ? (long long)trec_at : -1, trec.size()));
        trec_at += rec;
      }
      if (survey && survey_samples_step(c, s)) {
        CHK(march_survey_launch(c, c->stream, n_ub, s));
        ++surveyed;
        count_bin(s);
      }
      if (integrals) CHK(march_integral_launch(c, c->stream, n_ub, s, rel));
      MarchSym ms;
      ms.scale = &S->sc[(s + 1) & 1]; ms.bad = &S->sym_bad; ms.n_lo = n_lo + 1; ms.march = overlap_ok;
      CHK(advect_launch(c, (size_t)n_ub, &S->n, m.dt, nfoil, c->march_vcore, precision, nullptr, nullptr, td, ms));
      overlapped = false;    // the serial symmetric step leaves its sums in the accumulators
    } else {
      // overlapped step: the symmetric kernel on the wake as the last roll-up left it runs on the main stream
      // while chord sums and solve run on the second one; they meet at the Euler finisher
      const bool hilo = precision == LUDVM_PREC_F32X2;
      const long long nt_pad = (n_ub + 63) / 64 * 64;
      long long* acc = nullptr;
      CHK(acc_buffer(c, nt_pad, &acc));
      const bool sharded = sharded_at(c, n_ub);
      if (!overlapped) {
        // (march_finish_sym re-zeroes what it reads, so once is enough)
        const size_t all = c->ext_acc ? c->ext_acc_bytes : c->acc.cap;
        HIPCHK(c, hipMemsetAsync(acc - 2, 0, all, c->stream));
        overlapped = true;
      }
      // (an overlapped step's finisher carries the fork event as its completion signal: no packet of its own)
      if (!fork_signalled) HIPCHK(c, hipEventRecord(c->ev_fork, main_stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream_b, c->ev_fork, 0));
      c->stream = c->stream_b;
      int rc = march_chord_launch(c, n_before);
      if (rc == LUDVM_OK) {
        hipLaunchKernelGGL(march_solve, dim3(1), dim3(kBlock), 0, c->stream, m, S, krow_s, row, s, c->x64, c->z64, c->g64,
                           c->mir(), c->g32, c->progress_dev);
        if (hipGetLastError() != hipSuccess) rc = fail(c, LUDVM_E_HIP, "march_solve launch failed");
      }
      // (probes: behind the solve on the second stream, before ev_join lets the finisher move the wake)
      if (rc == LUDVM_OK && probes) rc = march_probe_launch(c, c->stream_b, n_ub, s, rel, count);
      if (rc == LUDVM_OK && tracers) {
        const bool rec = trec_at < trec.size() && trec[trec_at] == s;
        rc = march_tracer_launch(c, c->stream_b, n_ub, s, rec ? (long long)trec_at : -1, trec.size());
        trec_at += rec;
      }
      if (rc == LUDVM_OK && survey && survey_samples_step(c, s)) {
        rc = march_survey_launch(c, c->stream_b, n_ub, s);
        ++surveyed;
        count_bin(s);
      }
      if (rc == LUDVM_OK && integrals) rc = march_integral_launch(c, c->stream_b, n_ub, s, rel);
      c->stream = main_stream;
      CHK(rc);
      HIPCHK(c, hipEventRecord(c->ev_join, c->stream_b));
      const long long nb = std::max<long long>(n_before, 1);
      const int T = sym_tile_t(c, nb, hilo);
      const long long ntiles = (nb + 64LL * T - 1) / (64LL * T);
      SymOperands o{};
      o.g = c->g32;
      if (hilo) { o.x = c->xh; o.z = c->zh; o.xl = c->xl; o.zl = c->zl; }
      else { o.x = c->xr; o.z = c->zr; o.cx = c->cx; o.cz = c->cz; }
      o.acc_u = acc; o.acc_w = acc + nt_pad;
      o.scale = &S->sc[s & 1];
      // sharded: this step's NaN counter travels with the sums through the all-reduce (two slots by step parity: the
      // finisher clears the next step's while blocks of its own launch may still read this step's)
      long long* bad_step = sharded ? acc - 2 + (s & 1) : nullptr;
      long long* bad_next = sharded ? acc - 2 + ((s + 1) & 1) : nullptr;
      o.bad = sharded ? bad_step : &S->sym_bad;
      long long first = 0, cnt = ntiles;
      if (sharded) shard_tiles(c, ntiles, &first, &cnt);
      CHK(launch_sym_tiles(c, T, o, nb, first, cnt, vc4, &S->n_old[s & 1], n_lo, sharded));
      if (sharded) CHK(reduce_accumulators(c, acc, nt_pad));
      HIPCHK(c, hipStreamWaitEvent(main_stream, c->ev_join, 0));
      if (ext_fork) {
        hipExtLaunchKernelGGL(march_finish_sym, dim3(fin_blocks(n_ub)), dim3(kFinBlock), 0, c->stream, nullptr, c->ev_fork, 0,
                              acc, acc + nt_pad, (const SymScale*)&S->sc[s & 1], S,
                              (const long long*)&S->n_old[s & 1], (int)nfoil, (float)vc4, m.dt, c->x64, c->z64, c->mir(), c->g32, td,
                              bad_step, bad_next);
        fork_signalled = true;
      } else {
        hipLaunchKernelGGL(march_finish_sym, dim3(fin_blocks(n_ub)), dim3(kFinBlock), 0, c->stream, acc, acc + nt_pad,
                           &S->sc[s & 1], S, &S->n_old[s & 1], (int)nfoil, (float)vc4, m.dt, c->x64, c->z64, c->mir(), c->g32, td,
                           bad_step, bad_next);
      }
      HIPCHK(c, hipGetLastError());
    }
    if (!fork) fork_signalled = false;
  }
  // results: per-step rows, final state, the two newest wake vortices
  HIPCHK(c, hipMemcpyAsync(rows, drows, (size_t)count * row_doubles * 8, hipMemcpyDeviceToHost, c->stream));
  if (hist) HIPCHK(c, hipMemcpyAsync(hist, c->march_hist.p, (size_t)count * 2 * hist_nmax * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&hs, S, sizeof(MarchState), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hs.n < n0 + count || hs.n > n0 + 2 * count) return fail(c, LUDVM_E_STATE, "march: inconsistent wake size on the device");
  c->wake_n = (size_t)hs.n;
  state[0] = (double)hs.n; state[1] = (double)hs.itev; state[2] = (double)hs.ilev; state[3] = (double)hs.shed;
  state[4] = hs.lesp_crit; state[5] = hs.sum_tev; state[6] = hs.sum_lev;
  for (int k = 0; k < 4; ++k) state[7 + k] = hs.place[k];
  state[11] = (double)hs.tail;
  double tailbuf[4] = {0, 0, 0, 0};
  const size_t nn = (size_t)hs.n;
  if (nn >= 2) {
    HIPCHK(c, hipMemcpy(tailbuf, c->x64 + nn - 2, 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tailbuf + 2, c->z64 + nn - 2, 16, hipMemcpyDeviceToHost));
  }
  for (int k = 0; k < 4; ++k) state[12 + k] = tailbuf[k];
  for (int k = 0; k < m.ncoef; ++k) state[16 + k] = hs.prevA[k];
  if (c->timing) CHK(drain_timing(c));
  if (probes) c->probe_rows = (size_t)count;
  if (integrals) { c->integral_rows = (size_t)count; c->integral_first_step = first_step; c->integral_tagged = (size_t)hs.n; }
  if (tracers) { c->tracer_rows = trec; c->tracer_ran = true; c->tracer_grad_ran = c->tracer_gradient; }
  c->survey_samples += surveyed;
  for (size_t b = 0; b < binned.size(); ++b) c->survey_bin_samples[b] += binned[b];
  return LUDVM_OK;
}

}  // extern "C"

/* ---- ensemble of small simulations ------------------------------------------------------------ */

extern "C" {

int ludvm_ensemble_limits(ludvm_ctx* c, long long* limits3) {
  if (!c) return LUDVM_E_ARG;
  if (!limits3) return fail(c, LUDVM_E_ARG, "null array");
  limits3[0] = LUDVM_ENSEMBLE_MAX_STEPS; limits3[1] = LUDVM_ENSEMBLE_MAX_WAKE; limits3[2] = LUDVM_ENSEMBLE_MAX_SNAPSHOTS;
  return LUDVM_OK;
}

}  // extern "C"

namespace {

// The tracer arguments of ludvm_ensemble_run_traced (count = 0: none, nothing else is looked at)
struct EnsembleTracerArgs {
  const double* seed_x = nullptr; const double* seed_z = nullptr; const long long* release = nullptr;
  size_t count = 0;
  const double* shift_x = nullptr; size_t shift_rows = 0;
  const long long* rec_steps = nullptr; size_t nrec = 0;
  double* rows = nullptr; size_t doubles = 0;
};

// The survey arguments of ludvm_ensemble_run_surveyed (count = 0: none, nothing else is looked at)
struct EnsembleSurveyArgs {
  const double* x = nullptr; const double* z = nullptr; size_t count = 0;
  const double* shift_x = nullptr; size_t shift_rows = 0;
  long long first = 1, stop = 0, every = 1;
  double* sums = nullptr; size_t doubles = 0;
  // the bins of ludvm_ensemble_run_surveyed_binned (nbins = 0: none, nothing else is looked at)
  const int* bin_of_step = nullptr; size_t bin_rows = 0;
  int nbins = 0;
  double* bin_sums = nullptr; size_t bin_doubles = 0;
  // the gradient sums of ludvm_ensemble_run_surveyed_graded (grad_doubles = 0 and both arrays null: none)
  double* grad_sums = nullptr; size_t grad_doubles = 0;
  double* bin_grad_sums = nullptr; size_t bin_grad_doubles = 0;
};

// The integral arguments of ludvm_ensemble_run_integrals (all zero / null: none)
struct EnsembleIntegralArgs {
  double* sums = nullptr; size_t doubles = 0;
  double* energy = nullptr; size_t energy_doubles = 0;
  long long first = 0, stop = 0, every = 0;
};

// ludvm_ensemble_run (nprobe = 0: the probe arguments are not looked at), ludvm_ensemble_run_probed, with tracers
// ludvm_ensemble_run_traced, with a survey ludvm_ensemble_run_surveyed, with bins ludvm_ensemble_run_surveyed_binned and, with
// gradient sums, ludvm_ensemble_run_surveyed_graded; any of them with wake integrals, ludvm_ensemble_run_integrals
int ensemble_run_body(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                      const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                      size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                      size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n, const double* probe_x,
                      const double* probe_z, size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u,
                      double* probe_w, const EnsembleTracerArgs& tr = EnsembleTracerArgs(),
                      const EnsembleSurveyArgs& sv = EnsembleSurveyArgs(),
                      const EnsembleIntegralArgs& ig = EnsembleIntegralArgs()) {
  if (!c) return LUDVM_E_ARG;
  if (c->shard_world > 1 || (c->comm && c->comm_world > 1))
    return fail(c, LUDVM_E_STATE, "ensemble: the context is sharded; members are independent -- split the list per device");
  if (members == 0) return LUDVM_OK;
  if (nprobe) {
    if (nprobe > LUDVM_ENSEMBLE_MAX_PROBES)
      return fail(c, LUDVM_E_ARG, "ensemble: at most " + std::to_string(LUDVM_ENSEMBLE_MAX_PROBES) + " probes");
    if (!probe_x || !probe_z || !probe_u || !probe_w) return fail(c, LUDVM_E_ARG, "null array");
    if (shift_x && shift_rows != kin_rows) return fail(c, LUDVM_E_ARG, "ensemble: probe offsets must be one per kinematics row");
    if (kin_rows > (((size_t)1 << 30) / 16) / nprobe)
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(16.0 * (double)kin_rows * (double)nprobe / (1 << 20)) + " MiB of probe rows (2 x 8 x " +
                                      std::to_string(kin_rows) + " kinematics rows x " + std::to_string(nprobe) +
                                      " probes) are over 1 GiB; split the batch");
    for (size_t k = 0; k < nprobe; ++k)
      if (!std::isfinite(probe_x[k]) || !std::isfinite(probe_z[k])) return fail(c, LUDVM_E_ARG, "ensemble: probe positions must be finite");
    for (size_t k = 0; shift_x && k < shift_rows; ++k)
      if (!std::isfinite(shift_x[k])) return fail(c, LUDVM_E_ARG, "ensemble: probe offsets must be finite");
  }
  const size_t M = tr.count, ntrec = tr.nrec;
  if (M) {
    if (M > LUDVM_ENSEMBLE_MAX_TRACERS)
      return fail(c, LUDVM_E_ARG, "ensemble: at most " + std::to_string(LUDVM_ENSEMBLE_MAX_TRACERS) + " tracers");
    if (!tr.seed_x || !tr.seed_z || !tr.release || !tr.rows || (ntrec && !tr.rec_steps)) return fail(c, LUDVM_E_ARG, "null array");
    if (tr.shift_x && tr.shift_rows != kin_rows) return fail(c, LUDVM_E_ARG, "ensemble: tracer offsets must be one per kinematics row");
    for (size_t k = 0; k < M; ++k) {
      if (!std::isfinite(tr.seed_x[k]) || !std::isfinite(tr.seed_z[k])) return fail(c, LUDVM_E_ARG, "ensemble: tracer seeds must be finite");
      if (tr.release[k] < 1) return fail(c, LUDVM_E_ARG, "ensemble: tracer release steps must be >= 1");
    }
    for (size_t k = 0; tr.shift_x && k < tr.shift_rows; ++k)
      if (!std::isfinite(tr.shift_x[k])) return fail(c, LUDVM_E_ARG, "ensemble: tracer offsets must be finite");
    for (size_t k = 0; k < ntrec; ++k)
      if (tr.rec_steps[k] < 1 || (k && tr.rec_steps[k] <= tr.rec_steps[k - 1]))
        return fail(c, LUDVM_E_ARG, "ensemble: tracer record steps must be >= 1 and strictly increasing");
    // members x (ntrec + 1) records of 2 x 8 x M bytes: at most 1 GiB (each factor is checked before it is multiplied in)
    const size_t most = (((size_t)1 << 30) / 16) / M;           // records of all members
    if (ntrec + 1 > most || members > most / (ntrec + 1))
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(16.0 * (double)members * (double)(ntrec + 1) * (double)M / (1 << 20)) +
                                      " MiB of tracer records (2 x 8 x " + std::to_string(members) + " members x " +
                                      std::to_string(ntrec + 1) + " records x " + std::to_string(M) + " tracers) are over 1 GiB; split the batch");
    if (tr.doubles < members * (ntrec + 1) * 2 * M) return fail(c, LUDVM_E_ARG, "ensemble: tracer records outside the array");
  }
  const size_t K = sv.count;
  if (K) {
    if (K > LUDVM_ENSEMBLE_MAX_SURVEY)
      return fail(c, LUDVM_E_ARG, "ensemble: at most " + std::to_string(LUDVM_ENSEMBLE_MAX_SURVEY) + " survey points");
    if (!sv.x || !sv.z || !sv.sums) return fail(c, LUDVM_E_ARG, "null array");
    if (sv.shift_rows != 0 && sv.shift_rows != kin_rows)
      return fail(c, LUDVM_E_ARG, "ensemble: survey offsets must be one per kinematics row");
    if (sv.shift_rows && !sv.shift_x) return fail(c, LUDVM_E_ARG, "null array");
    if (sv.first < 1 || sv.every < 1) return fail(c, LUDVM_E_ARG, "ensemble: survey steps: first >= 1 and every >= 1");
    for (size_t k = 0; k < K; ++k)
      if (!std::isfinite(sv.x[k]) || !std::isfinite(sv.z[k])) return fail(c, LUDVM_E_ARG, "ensemble: survey points must be finite");
    for (size_t k = 0; k < sv.shift_rows; ++k)
      if (!std::isfinite(sv.shift_x[k])) return fail(c, LUDVM_E_ARG, "ensemble: survey offsets must be finite");
    // members x 5 x 8 x K bytes of sums: at most 1 GiB
    if (members > (((size_t)1 << 30) / 40) / K)
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(40.0 * (double)members * (double)K / (1 << 20)) +
                                      " MiB of survey sums (5 x 8 x " + std::to_string(members) + " members x " + std::to_string(K) +
                                      " points) are over 1 GiB; split the batch");
    if (sv.doubles != members * 5 * K) return fail(c, LUDVM_E_ARG, "ensemble: survey sums must hold members x 5 x points doubles");
  }
  if (sv.nbins < 0 || sv.nbins > LUDVM_ENSEMBLE_MAX_SURVEY_BINS)
    return fail(c, LUDVM_E_ARG, "ensemble: 0 <= survey bins <= " + std::to_string(LUDVM_ENSEMBLE_MAX_SURVEY_BINS));
  const size_t B = (size_t)sv.nbins;
  if (B) {
    if (!K) return fail(c, LUDVM_E_ARG, "ensemble: survey bins need survey points");
    if (!sv.bin_of_step || !sv.bin_sums) return fail(c, LUDVM_E_ARG, "null array");
    if (sv.bin_rows != kin_rows) return fail(c, LUDVM_E_ARG, "ensemble: survey bins must be one per kinematics row");
    for (size_t k = 0; k < sv.bin_rows; ++k)
      if (sv.bin_of_step[k] < -1 || sv.bin_of_step[k] >= sv.nbins)
        return fail(c, LUDVM_E_ARG, "ensemble: a survey bin is -1 (none) or 0 .. bins - 1");
    // members x (bins + 1) x 5 x 8 x K bytes of plain and bin sums: at most 1 GiB
    if (members > ((((size_t)1 << 30) / 40) / K) / (B + 1))
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(40.0 * (double)members * (double)(B + 1) * (double)K / (1 << 20)) +
                                      " MiB of survey sums (5 x 8 x " + std::to_string(members) + " members x (" + std::to_string(B) +
                                      " bins + 1) x " + std::to_string(K) + " points) are over 1 GiB; split the batch");
    if (sv.bin_doubles != members * B * 5 * K)
      return fail(c, LUDVM_E_ARG, "ensemble: survey bin sums must hold members x bins x 5 x points doubles");
  }
  const bool G = sv.grad_doubles || sv.grad_sums || sv.bin_grad_sums || sv.bin_grad_doubles;
  if (G) {
    if (!K) return fail(c, LUDVM_E_ARG, "ensemble: survey gradient sums need survey points");
    if (!sv.grad_sums || (B && !sv.bin_grad_sums)) return fail(c, LUDVM_E_ARG, "null array");
    if (!B && (sv.bin_grad_sums || sv.bin_grad_doubles))
      return fail(c, LUDVM_E_ARG, "ensemble: survey bin gradient sums need survey bins");
    // members x (bins + 1) x 10 x 8 x K bytes of plain, bin and gradient sums: at most 1 GiB
    if (members > ((((size_t)1 << 30) / 80) / K) / (B + 1))
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(80.0 * (double)members * (double)(B + 1) * (double)K / (1 << 20)) +
                                      " MiB of survey and gradient sums (10 x 8 x " + std::to_string(members) + " members x (" +
                                      std::to_string(B) + " bins + 1) x " + std::to_string(K) + " points) are over 1 GiB; split the batch");
    if (sv.grad_doubles != members * 5 * K)
      return fail(c, LUDVM_E_ARG, "ensemble: survey gradient sums must hold members x 5 x points doubles");
    if (sv.bin_grad_doubles != members * B * 5 * K)
      return fail(c, LUDVM_E_ARG, "ensemble: survey bin gradient sums must hold members x bins x 5 x points doubles");
  }
  const bool I = ig.sums || ig.doubles;
  const bool E = ig.energy || ig.energy_doubles || ig.every != 0;
  if (E && !I) return fail(c, LUDVM_E_ARG, "ensemble: the wake energy needs the integral sums");
  if (I) {
    if (!ig.sums) return fail(c, LUDVM_E_ARG, "null array");
    // kin_rows x (48 + 1) x 8 bytes of integral rows and energy: at most 1 GiB
    if (kin_rows > ((size_t)1 << 30) / (8 * (kIntegralSums + 1)))
      return fail(c, LUDVM_E_ARG, "ensemble: " + std::to_string(8.0 * (kIntegralSums + 1) * (double)kin_rows / (1 << 20)) +
                                      " MiB of integral rows (8 x 49 x " + std::to_string(kin_rows) +
                                      " kinematics rows) are over 1 GiB; split the batch");
    if (ig.doubles != kin_rows * kIntegralSums)
      return fail(c, LUDVM_E_ARG, "ensemble: integral sums must hold kinematics rows x 48 doubles");
  }
  if (E) {
    if (!ig.energy) return fail(c, LUDVM_E_ARG, "null array");
    if (ig.energy_doubles != kin_rows) return fail(c, LUDVM_E_ARG, "ensemble: the wake energy must hold one double per kinematics row");
    if (ig.first < 1 || ig.every < 1) return fail(c, LUDVM_E_ARG, "ensemble: energy steps: first >= 1 and every >= 1");
    if (ig.stop <= ig.first) return fail(c, LUDVM_E_ARG, "ensemble: energy steps: the window holds no time step");
  }
  if (!scalars || !tables || !kin || !init || !desc || !rows || !wakes || !wake_n || (free_count && !free_xzg) || (nsnap && !snap_steps))
    return fail(c, LUDVM_E_ARG, "null array");
  if (npan < 1 || npan > kMarchMaxPan || ncoef < 4 || ncoef > kMarchMaxCoef)
    return fail(c, LUDVM_E_ARG, "ensemble: 1 <= Npanels <= 256 and 4 <= Ncoeffs <= 64");
  if (members > ((size_t)1 << 24)) return fail(c, LUDVM_E_ARG, "ensemble: too many members");
  if (scalar_count != 12 * members) return fail(c, LUDVM_E_ARG, "ensemble: scalars must hold 12 values per member");
  if (nsnap > LUDVM_ENSEMBLE_MAX_SNAPSHOTS) return fail(c, LUDVM_E_ARG, "ensemble: too many snapshot steps");
  for (size_t k = 0; k < nsnap; ++k)
    if (snap_steps[k] < 1 || (k && snap_steps[k] <= snap_steps[k - 1]))
      return fail(c, LUDVM_E_ARG, "ensemble: snapshot steps must be >= 1 and strictly increasing");
  const size_t P = (size_t)npan, NC = (size_t)ncoef;
  const size_t tab_doubles = 8 * P + NC * P + (NC - 1) * P;
  const size_t krow = 7 + 2 * P;
  const size_t row_doubles = kMarchRowHead + 2 * NC + 2 * P;
  const size_t init_doubles = kEnsInitHead + NC;
  const size_t nrec = nsnap + 1;

  // every member inside the limits and inside the arrays given, before anything touches the device
  size_t work_doubles = 0;
  for (size_t mi = 0; mi < members; ++mi) {
    const long long* d = desc + mi * LUDVM_ENSEMBLE_DESC;
    const long long nt = d[0], kin_off = d[1], nfree = d[2], free_off = d[3], row_off = d[4], wake_off = d[5];
    const std::string who = "ensemble: member " + std::to_string(mi) + ": ";
    if (nt < 2 || nt - 1 > LUDVM_ENSEMBLE_MAX_STEPS)
      return fail(c, LUDVM_E_ARG, who + "1 <= steps <= " + std::to_string(LUDVM_ENSEMBLE_MAX_STEPS) + " (it can be run on its own)");
    if (nfree < 0 || nfree + 2 * (nt - 1) > LUDVM_ENSEMBLE_MAX_WAKE)
      return fail(c, LUDVM_E_ARG, who + "free vortices + 2 steps <= " + std::to_string(LUDVM_ENSEMBLE_MAX_WAKE) + " (it can be run on its own)");
    const size_t cap = (size_t)(nfree + 2 * (nt - 1));
    if (kin_off < 0 || (size_t)kin_off + (size_t)nt > kin_rows) return fail(c, LUDVM_E_ARG, who + "kinematics rows outside the table");
    if (free_off < 0 || (size_t)free_off + (size_t)nfree > free_count) return fail(c, LUDVM_E_ARG, who + "free vortices outside the array");
    if (row_off < 0 || (size_t)row_off + (size_t)(nt - 1) > rows_count) return fail(c, LUDVM_E_ARG, who + "output rows outside the array");
    if (wake_off < 0 || (size_t)wake_off + nrec * 3 * cap > wake_doubles) return fail(c, LUDVM_E_ARG, who + "wake records outside the array");
    const double* sc = scalars + 12 * mi;
    if (sc[8] != 0.0 && !(sc[9] > 0.0 && sc[10] >= 1.0 && sc[11] > 0.0))
      return fail(c, LUDVM_E_ARG, who + "'Ramesh' needs maxerror > 0, maxiter >= 1, epsilon > 0");
    work_doubles += 5 * (cap + P) + 2 * M + (I ? (cap + 7) / 8 : 0);      // (integrals: a tag byte per wake vortex)
  }

  HIPCHK(c, hipSetDevice(c->device));
  // inputs: tables | kin | init | free | snapshot steps | member records
  const size_t in_tab = Arena::need(members * tab_doubles, 8), in_kin = Arena::need(kin_rows * krow, 8);
  const size_t in_init = Arena::need(members * init_doubles, 8), in_free = Arena::need(3 * free_count + 1, 8);
  const size_t in_snap = Arena::need(nsnap + 1, 8), in_mem = Arena::need(members, sizeof(EnsembleMember));
  // (probes: points and offsets behind the inputs, rows behind the outputs)
  const size_t in_probe = nprobe ? 2 * Arena::need(nprobe, 8) + (shift_x ? Arena::need(shift_rows, 8) : 0) : 0;
  // (tracers: seeds, release steps, tile minima, offsets, record steps and the members' tracer records behind those;
  // current positions in the work memory, records behind the outputs)
  const size_t ttiles = (M + kBlock - 1) / kBlock;
  const size_t in_tracer = M ? 3 * Arena::need(M, 8) + Arena::need(ttiles, 8) + (tr.shift_x ? Arena::need(tr.shift_rows, 8) : 0) +
                                   Arena::need(ntrec + 1, 8) + Arena::need(members, sizeof(EnsembleTracers))
                             : 0;
  // (survey: points, offsets and the members' survey records behind those; the sums behind the outputs)
  const bool sshift = K && sv.shift_rows;
  const size_t in_survey = K ? 2 * Arena::need(K, 8) + (sshift ? Arena::need(sv.shift_rows, 8) : 0) +
                                   Arena::need(members, sizeof(EnsembleSurvey))
                             : 0;
  // (bins: the table and the members' bin records behind those; the bin sums behind the outputs)
  // (gradient sums: the members' bin records -- a null table without bins -- and their gradient records; the sums behind the
  // outputs)
  const size_t in_bins = (B ? Arena::need(sv.bin_rows, sizeof(int)) : 0) + (B || G ? Arena::need(members, sizeof(EnsembleSurveyBins)) : 0);
  const size_t in_grad = G ? Arena::need(members, sizeof(EnsembleSurveyGrad)) : 0;
  // (integrals: the members' integral records; rows and energy behind the outputs, the tags in the work memory)
  const size_t in_integ = I ? Arena::need(members, sizeof(EnsembleIntegrals)) : 0;
  CHK(ensure(c, c->ens_in, in_tab + in_kin + in_init + in_free + in_snap + in_mem + in_probe + in_tracer + in_survey + in_bins + in_grad +
                               in_integ));
  CHK(ensure(c, c->ens_work, work_doubles * 8));
  const size_t out_rows = Arena::need(rows_count * row_doubles, 8), out_wakes = Arena::need(wake_doubles, 8);
  const size_t out_n = Arena::need(members * nrec, 8);
  const size_t out_probe = nprobe ? 2 * Arena::need(kin_rows * nprobe, 8) : 0;
  const size_t trec_doubles = members * (ntrec + 1) * 2 * M;
  const size_t out_tracer = M ? Arena::need(trec_doubles, 8) : 0;
  const size_t out_survey = K ? Arena::need(members * 5 * K, 8) : 0;
  const size_t out_bins = B ? Arena::need(members * B * 5 * K, 8) : 0;
  const size_t out_grad = G ? Arena::need(members * 5 * K, 8) + (B ? Arena::need(members * B * 5 * K, 8) : 0) : 0;
  const size_t out_integ = I ? Arena::need(kin_rows * kIntegralSums, 8) + (E ? Arena::need(kin_rows, 8) : 0) : 0;
  CHK(ensure(c, c->ens_out, out_rows + out_wakes + out_n + out_probe + out_tracer + out_survey + out_bins + out_grad + out_integ));
  Arena in(c->ens_in.p), out(c->ens_out.p);
  double* d_tab = in.take<double>(members * tab_doubles);
  double* d_kin = in.take<double>(kin_rows * krow);
  double* d_init = in.take<double>(members * init_doubles);
  double* d_free = in.take<double>(3 * free_count + 1);
  long long* d_snap = in.take<long long>(nsnap + 1);
  EnsembleMember* d_mem = in.take<EnsembleMember>(members);
  double* d_rows = out.take<double>(rows_count * row_doubles);
  double* d_wakes = out.take<double>(wake_doubles);
  long long* d_n = out.take<long long>(members * nrec);
  double *d_px = nullptr, *d_pz = nullptr, *d_shift = nullptr, *d_pu = nullptr, *d_pw = nullptr;
  if (nprobe) {
    d_px = in.take<double>(nprobe);
    d_pz = in.take<double>(nprobe);
    if (shift_x) d_shift = in.take<double>(shift_rows);
    d_pu = out.take<double>(kin_rows * nprobe);
    d_pw = out.take<double>(kin_rows * nprobe);
  }
  double *d_sx = nullptr, *d_sz = nullptr, *d_tshift = nullptr, *d_trows = nullptr;
  long long *d_rel = nullptr, *d_tmin = nullptr, *d_trec = nullptr;
  EnsembleTracers* d_tr = nullptr;
  if (M) {
    d_sx = in.take<double>(M);
    d_sz = in.take<double>(M);
    d_rel = in.take<long long>(M);
    d_tmin = in.take<long long>(ttiles);
    if (tr.shift_x) d_tshift = in.take<double>(tr.shift_rows);
    d_trec = in.take<long long>(ntrec + 1);
    d_tr = in.take<EnsembleTracers>(members);
    d_trows = out.take<double>(trec_doubles);
  }
  double *d_vx = nullptr, *d_vz = nullptr, *d_vshift = nullptr, *d_vsums = nullptr;
  EnsembleSurvey* d_sv = nullptr;
  if (K) {
    d_vx = in.take<double>(K);
    d_vz = in.take<double>(K);
    if (sshift) d_vshift = in.take<double>(sv.shift_rows);
    d_sv = in.take<EnsembleSurvey>(members);
    d_vsums = out.take<double>(members * 5 * K);
  }
  int* d_btab = nullptr;
  double* d_bsums = nullptr;
  EnsembleSurveyBins* d_sb = nullptr;
  if (B) {
    d_btab = in.take<int>(sv.bin_rows);
    d_bsums = out.take<double>(members * B * 5 * K);
  }
  if (B || G) d_sb = in.take<EnsembleSurveyBins>(members);
  double *d_gsums = nullptr, *d_bgsums = nullptr;
  EnsembleSurveyGrad* d_sg = nullptr;
  if (G) {
    d_sg = in.take<EnsembleSurveyGrad>(members);
    d_gsums = out.take<double>(members * 5 * K);
    if (B) d_bgsums = out.take<double>(members * B * 5 * K);
  }
  double *d_isums = nullptr, *d_energy = nullptr;
  EnsembleIntegrals* d_ig = nullptr;
  if (I) {
    d_ig = in.take<EnsembleIntegrals>(members);
    d_isums = out.take<double>(kin_rows * kIntegralSums);
    if (E) d_energy = out.take<double>(kin_rows);
  }

  std::vector<EnsembleMember> hm(members);
  std::vector<EnsembleIntegrals> hi(I ? members : 0);
  std::vector<EnsembleSurvey> hv(K ? members : 0);
  std::vector<EnsembleSurveyBins> hb(B || G ? members : 0);
  std::vector<EnsembleSurveyGrad> hg(G ? members : 0);
  std::vector<EnsembleTracers> ht(M ? members : 0);
  std::vector<long long> tmin(ttiles, std::numeric_limits<long long>::max());     // earliest release step of each tile
  for (size_t k = 0; k < M; ++k) tmin[k / kBlock] = std::min(tmin[k / kBlock], tr.release[k]);
  double* work = static_cast<double*>(c->ens_work.p);
  for (size_t mi = 0; mi < members; ++mi) {
    const long long* d = desc + mi * LUDVM_ENSEMBLE_DESC;
    const double* sc = scalars + 12 * mi;
    EnsembleMember& e = hm[mi];
    MarchSetup& m = e.m;
    m.npan = npan; m.ncoef = ncoef;
    m.U = sc[0]; m.chord = sc[1]; m.rho = sc[2]; m.dt = sc[3]; m.piv = sc[4];
    m.kelvin0 = sc[7] - sc[6];          // sum(Gamma_free) - IC
    m.vc4 = (sc[5] * sc[5]) * (sc[5] * sc[5]);
    m.method = sc[8] != 0.0 ? 1 : 0;
    m.maxerror = sc[9]; m.maxiter = (int)sc[10]; m.epsilon = sc[11];
    const double* t = d_tab + mi * tab_doubles;
    m.detadx = t; m.eta = t + P; m.xpan = t + 2 * P; m.cm1 = t + 3 * P; m.wq = t + 4 * P; m.opcs = t + 5 * P;
    m.hcsd = t + 6 * P; m.wx = t + 7 * P; m.cproj = t + 8 * P; m.ssin = t + 8 * P + NC * P;
    e.nt = d[0]; e.nfree = d[2];
    e.cap = d[2] + 2 * (d[0] - 1);
    const size_t cap = (size_t)e.cap, slab = cap + P;
    e.kin = d_kin + (size_t)d[1] * krow;
    e.init = d_init + mi * init_doubles;
    e.free_x = d_free + 3 * (size_t)d[3]; e.free_z = e.free_x + d[2]; e.free_g = e.free_z + d[2];
    e.xa = work; e.za = work + slab; e.xb = work + 2 * slab; e.zb = work + 3 * slab; e.g = work + 4 * slab;
    work += 5 * slab;
    if (M) {
      EnsembleTracers& t = ht[mi];
      t.seed_x = d_sx; t.seed_z = d_sz; t.release = d_rel; t.tile_min = d_tmin; t.M = (long long)M;
      t.shift = d_tshift ? d_tshift + (size_t)d[1] : nullptr;
      t.cur_x = work; t.cur_z = work + M;
      work += 2 * M;
      t.rec = d_trows + mi * (ntrec + 1) * 2 * M;
    }
    if (K) {
      EnsembleSurvey& v = hv[mi];
      v.x = d_vx; v.z = d_vz; v.K = (long long)K;
      v.shift = d_vshift ? d_vshift + (size_t)d[1] : nullptr;
      v.first = sv.first; v.stop = sv.stop; v.every = sv.every;
      v.sums = d_vsums + mi * 5 * K;
    }
    if (B) {
      hb[mi].bin_of_step = d_btab + (size_t)d[1];
      hb[mi].sums = d_bsums + mi * B * 5 * K;
    } else if (G) {
      hb[mi].bin_of_step = nullptr;
      hb[mi].sums = nullptr;
    }
    if (G) {
      hg[mi].sums = d_gsums + mi * 5 * K;
      hg[mi].bin_sums = B ? d_bgsums + mi * B * 5 * K : nullptr;
    }
    if (I) {
      EnsembleIntegrals& q = hi[mi];
      q.tags = reinterpret_cast<unsigned char*>(work);
      work += (cap + 7) / 8;
      q.sums = d_isums + (size_t)d[1] * kIntegralSums;
      q.energy = E ? d_energy + (size_t)d[1] : nullptr;
      q.first = ig.first; q.stop = ig.stop; q.every = ig.every;
    }
    e.rows = d_rows + (size_t)d[4] * row_doubles;
    e.rec = d_wakes + (size_t)d[5];
    e.rec_n = d_n + mi * nrec;
    e.px = d_px; e.pz = d_pz; e.P = (long long)nprobe;
    e.shift = d_shift ? d_shift + (size_t)d[1] : nullptr;
    e.pu_rows = nprobe ? d_pu + (size_t)d[1] * nprobe : nullptr;
    e.pw_rows = nprobe ? d_pw + (size_t)d[1] * nprobe : nullptr;
  }
  HIPCHK(c, hipMemcpyAsync(d_tab, tables, members * tab_doubles * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_kin, kin, kin_rows * krow * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_init, init, members * init_doubles * 8, hipMemcpyHostToDevice, c->stream));
  if (free_count) HIPCHK(c, hipMemcpyAsync(d_free, free_xzg, 3 * free_count * 8, hipMemcpyHostToDevice, c->stream));
  if (nsnap) HIPCHK(c, hipMemcpyAsync(d_snap, snap_steps, nsnap * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_mem, hm.data(), members * sizeof(EnsembleMember), hipMemcpyHostToDevice, c->stream));
  if (nprobe) {
    HIPCHK(c, hipMemcpyAsync(d_px, probe_x, nprobe * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pz, probe_z, nprobe * 8, hipMemcpyHostToDevice, c->stream));
    if (shift_x) HIPCHK(c, hipMemcpyAsync(d_shift, shift_x, shift_rows * 8, hipMemcpyHostToDevice, c->stream));
    // (rows of `kin` that no member owns stay 0)
    HIPCHK(c, hipMemsetAsync(d_pu, 0, kin_rows * nprobe * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_pw, 0, kin_rows * nprobe * 8, c->stream));
  }
  if (M) {
    HIPCHK(c, hipMemcpyAsync(d_sx, tr.seed_x, M * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_sz, tr.seed_z, M * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rel, tr.release, M * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tmin, tmin.data(), ttiles * 8, hipMemcpyHostToDevice, c->stream));
    if (tr.shift_x) HIPCHK(c, hipMemcpyAsync(d_tshift, tr.shift_x, tr.shift_rows * 8, hipMemcpyHostToDevice, c->stream));
    if (ntrec) HIPCHK(c, hipMemcpyAsync(d_trec, tr.rec_steps, ntrec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tr, ht.data(), members * sizeof(EnsembleTracers), hipMemcpyHostToDevice, c->stream));
    // (a record whose step a member does not have stays 0)
    HIPCHK(c, hipMemsetAsync(d_trows, 0, trec_doubles * 8, c->stream));
  }
  if (K) {
    HIPCHK(c, hipMemcpyAsync(d_vx, sv.x, K * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_vz, sv.z, K * 8, hipMemcpyHostToDevice, c->stream));
    if (sshift) HIPCHK(c, hipMemcpyAsync(d_vshift, sv.shift_x, sv.shift_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_sv, hv.data(), members * sizeof(EnsembleSurvey), hipMemcpyHostToDevice, c->stream));
    // (the kernel adds to the sums)
    HIPCHK(c, hipMemsetAsync(d_vsums, 0, members * 5 * K * 8, c->stream));
  }
  if (B) {
    HIPCHK(c, hipMemcpyAsync(d_btab, sv.bin_of_step, sv.bin_rows * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // (the kernel adds to the bin sums)
    HIPCHK(c, hipMemsetAsync(d_bsums, 0, members * B * 5 * K * 8, c->stream));
  }
  if (B || G) HIPCHK(c, hipMemcpyAsync(d_sb, hb.data(), members * sizeof(EnsembleSurveyBins), hipMemcpyHostToDevice, c->stream));
  if (G) {
    HIPCHK(c, hipMemcpyAsync(d_sg, hg.data(), members * sizeof(EnsembleSurveyGrad), hipMemcpyHostToDevice, c->stream));
    // (the kernel adds to the gradient sums)
    HIPCHK(c, hipMemsetAsync(d_gsums, 0, members * 5 * K * 8, c->stream));
    if (B) HIPCHK(c, hipMemsetAsync(d_bgsums, 0, members * B * 5 * K * 8, c->stream));
  }
  if (I) {
    HIPCHK(c, hipMemcpyAsync(d_ig, hi.data(), members * sizeof(EnsembleIntegrals), hipMemcpyHostToDevice, c->stream));
    // (row 0 of a member and rows of `kin` that no member owns stay 0; the energy is NaN wherever no sample lands)
    HIPCHK(c, hipMemsetAsync(d_isums, 0, kin_rows * kIntegralSums * 8, c->stream));
    if (E) {
      std::fill(ig.energy, ig.energy + kin_rows, std::numeric_limits<double>::quiet_NaN());
      HIPCHK(c, hipMemcpyAsync(d_energy, ig.energy, kin_rows * 8, hipMemcpyHostToDevice, c->stream));
    }
  }
  // ONE launch: a workgroup per member, all of its time steps inside
  if (I) {
    const dim3 grid((unsigned)members), block(kBlock);
    const EnsembleMember* am = d_mem; const long long* as = d_snap; const EnsembleTracers* at = d_tr;
    const long long* ar = d_trec; const EnsembleSurvey* av = d_sv; const EnsembleSurveyBins* ab = d_sb;
    const EnsembleSurveyGrad* ag = d_sg; const EnsembleIntegrals* ai = d_ig;
#define LUDVM_ENS_INTEGRALS(SURVEY)                                                                                                      \
  do {                                                                                                                                   \
    if (M && nprobe)                                                                                                                     \
      hipLaunchKernelGGL((ensemble_integrals<true, true, SURVEY>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, \
                         ab, ag, ai);                                                                                                    \
    else if (M)                                                                                                                          \
      hipLaunchKernelGGL((ensemble_integrals<false, true, SURVEY>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec,    \
                         av, ab, ag, ai);                                                                                                \
    else if (nprobe)                                                                                                                     \
      hipLaunchKernelGGL((ensemble_integrals<true, false, SURVEY>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec,    \
                         av, ab, ag, ai);                                                                                                \
    else                                                                                                                                 \
      hipLaunchKernelGGL((ensemble_integrals<false, false, SURVEY>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec,   \
                         av, ab, ag, ai);                                                                                                \
  } while (0)
    // SURVEY: 3 graded, 2 binned, 1 plain, 0 none -- the kernel the call without integrals launches, with phases 2i and 2e
    if (G) LUDVM_ENS_INTEGRALS(3);
    else if (B) LUDVM_ENS_INTEGRALS(2);
    else if (K) LUDVM_ENS_INTEGRALS(1);
    else LUDVM_ENS_INTEGRALS(0);
#undef LUDVM_ENS_INTEGRALS
  } else if (G) {
    const dim3 grid((unsigned)members), block(kBlock);
    const EnsembleMember* am = d_mem; const long long* as = d_snap; const EnsembleTracers* at = d_tr;
    const long long* ar = d_trec; const EnsembleSurvey* av = d_sv; const EnsembleSurveyBins* ab = d_sb;
    const EnsembleSurveyGrad* ag = d_sg;
    if (M && nprobe) hipLaunchKernelGGL((ensemble_graded<true, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab, ag);
    else if (M) hipLaunchKernelGGL((ensemble_graded<false, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab, ag);
    else if (nprobe) hipLaunchKernelGGL((ensemble_graded<true, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab, ag);
    else hipLaunchKernelGGL((ensemble_graded<false, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab, ag);
  } else if (B) {
    const dim3 grid((unsigned)members), block(kBlock);
    const EnsembleMember* am = d_mem; const long long* as = d_snap; const EnsembleTracers* at = d_tr;
    const long long* ar = d_trec; const EnsembleSurvey* av = d_sv; const EnsembleSurveyBins* ab = d_sb;
    if (M && nprobe) hipLaunchKernelGGL((ensemble_binned<true, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab);
    else if (M) hipLaunchKernelGGL((ensemble_binned<false, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab);
    else if (nprobe) hipLaunchKernelGGL((ensemble_binned<true, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab);
    else hipLaunchKernelGGL((ensemble_binned<false, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av, ab);
  } else if (K) {
    const dim3 grid((unsigned)members), block(kBlock);
    const EnsembleMember* am = d_mem; const long long* as = d_snap; const EnsembleTracers* at = d_tr;
    const long long* ar = d_trec; const EnsembleSurvey* av = d_sv;
    if (M && nprobe) hipLaunchKernelGGL((ensemble_surveyed<true, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av);
    else if (M) hipLaunchKernelGGL((ensemble_surveyed<false, true>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av);
    else if (nprobe) hipLaunchKernelGGL((ensemble_surveyed<true, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av);
    else hipLaunchKernelGGL((ensemble_surveyed<false, false>), grid, block, 0, c->stream, am, as, (int)nsnap, at, ar, (int)ntrec, av);
  } else if (M && nprobe)
    hipLaunchKernelGGL(ensemble_traced<true>, dim3((unsigned)members), dim3(kBlock), 0, c->stream, (const EnsembleMember*)d_mem,
                       (const long long*)d_snap, (int)nsnap, (const EnsembleTracers*)d_tr, (const long long*)d_trec, (int)ntrec);
  else if (M)
    hipLaunchKernelGGL(ensemble_traced<false>, dim3((unsigned)members), dim3(kBlock), 0, c->stream, (const EnsembleMember*)d_mem,
                       (const long long*)d_snap, (int)nsnap, (const EnsembleTracers*)d_tr, (const long long*)d_trec, (int)ntrec);
  else if (nprobe)
    hipLaunchKernelGGL(ensemble_march<true>, dim3((unsigned)members), dim3(kBlock), 0, c->stream, (const EnsembleMember*)d_mem,
                       (const long long*)d_snap, (int)nsnap);
  else
    hipLaunchKernelGGL(ensemble_march<false>, dim3((unsigned)members), dim3(kBlock), 0, c->stream, (const EnsembleMember*)d_mem,
                       (const long long*)d_snap, (int)nsnap);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(rows, d_rows, rows_count * row_doubles * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(wakes, d_wakes, wake_doubles * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(wake_n, d_n, members * nrec * 8, hipMemcpyDeviceToHost, c->stream));
  if (nprobe) {
    HIPCHK(c, hipMemcpyAsync(probe_u, d_pu, kin_rows * nprobe * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(probe_w, d_pw, kin_rows * nprobe * 8, hipMemcpyDeviceToHost, c->stream));
  }
  if (M) HIPCHK(c, hipMemcpyAsync(tr.rows, d_trows, trec_doubles * 8, hipMemcpyDeviceToHost, c->stream));
  if (K) HIPCHK(c, hipMemcpyAsync(sv.sums, d_vsums, members * 5 * K * 8, hipMemcpyDeviceToHost, c->stream));
  if (B) HIPCHK(c, hipMemcpyAsync(sv.bin_sums, d_bsums, members * B * 5 * K * 8, hipMemcpyDeviceToHost, c->stream));
  if (G) HIPCHK(c, hipMemcpyAsync(sv.grad_sums, d_gsums, members * 5 * K * 8, hipMemcpyDeviceToHost, c->stream));
  if (G && B) HIPCHK(c, hipMemcpyAsync(sv.bin_grad_sums, d_bgsums, members * B * 5 * K * 8, hipMemcpyDeviceToHost, c->stream));
  if (I) HIPCHK(c, hipMemcpyAsync(ig.sums, d_isums, kin_rows * kIntegralSums * 8, hipMemcpyDeviceToHost, c->stream));
  if (E) HIPCHK(c, hipMemcpyAsync(ig.energy, d_energy, kin_rows * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));     // (hm, ht, hv, hb, hg, hi and tmin live on this frame)
  return LUDVM_OK;
}

}  // namespace

extern "C" {

int ludvm_ensemble_run(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                       const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                       size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                       size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n) {
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, nullptr, nullptr, 0, nullptr, 0, nullptr,
                           nullptr);
}

int ludvm_ensemble_run_probed(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                              const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                              size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                              size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n, const double* probe_x,
                              const double* probe_z, size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u,
                              double* probe_w) {
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w);
}

int ludvm_ensemble_run_traced(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                              const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                              size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                              size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n, const double* probe_x,
                              const double* probe_z, size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u,
                              double* probe_w, const double* seed_x, const double* seed_z, const long long* release, size_t ntracer,
                              const double* tshift_x, size_t tshift_rows, const long long* trec_steps, size_t ntrec,
                              double* tracer_rows, size_t tracer_doubles) {
  EnsembleTracerArgs tr;
  tr.seed_x = seed_x; tr.seed_z = seed_z; tr.release = release; tr.count = ntracer;
  tr.shift_x = tshift_x; tr.shift_rows = tshift_rows;
  tr.rec_steps = trec_steps; tr.nrec = ntrec;
  tr.rows = tracer_rows; tr.doubles = tracer_doubles;
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w, tr);
}

int ludvm_ensemble_run_surveyed(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                                const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                                size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                                size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n, const double* probe_x,
                                const double* probe_z, size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u,
                                double* probe_w, const double* seed_x, const double* seed_z, const long long* release, size_t ntracer,
                                const double* tshift_x, size_t tshift_rows, const long long* trec_steps, size_t ntrec,
                                double* tracer_rows, size_t tracer_doubles, const double* survey_x, const double* survey_z,
                                size_t nsurvey, const double* sshift_x, size_t sshift_rows, long long first, long long stop,
                                long long every, double* survey_sums, size_t survey_doubles) {
  EnsembleTracerArgs tr;
  tr.seed_x = seed_x; tr.seed_z = seed_z; tr.release = release; tr.count = ntracer;
  tr.shift_x = tshift_x; tr.shift_rows = tshift_rows;
  tr.rec_steps = trec_steps; tr.nrec = ntrec;
  tr.rows = tracer_rows; tr.doubles = tracer_doubles;
  EnsembleSurveyArgs sv;
  sv.x = survey_x; sv.z = survey_z; sv.count = nsurvey;
  sv.shift_x = sshift_x; sv.shift_rows = sshift_rows;
  sv.first = first; sv.stop = stop; sv.every = every;
  sv.sums = survey_sums; sv.doubles = survey_doubles;
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w, tr, sv);
}

int ludvm_ensemble_run_surveyed_binned(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                                       const double* tables, const double* kin, size_t kin_rows, const double* init,
                                       const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                                       size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                                       long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                                       const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w, const double* seed_x,
                                       const double* seed_z, const long long* release, size_t ntracer, const double* tshift_x,
                                       size_t tshift_rows, const long long* trec_steps, size_t ntrec, double* tracer_rows,
                                       size_t tracer_doubles, const double* survey_x, const double* survey_z, size_t nsurvey,
                                       const double* sshift_x, size_t sshift_rows, long long first, long long stop, long long every,
                                       double* survey_sums, size_t survey_doubles, const int* bin_of_step, size_t bin_rows, int nbins,
                                       double* bin_sums, size_t bin_doubles) {
  EnsembleTracerArgs tr;
  tr.seed_x = seed_x; tr.seed_z = seed_z; tr.release = release; tr.count = ntracer;
  tr.shift_x = tshift_x; tr.shift_rows = tshift_rows;
  tr.rec_steps = trec_steps; tr.nrec = ntrec;
  tr.rows = tracer_rows; tr.doubles = tracer_doubles;
  EnsembleSurveyArgs sv;
  sv.x = survey_x; sv.z = survey_z; sv.count = nsurvey;
  sv.shift_x = sshift_x; sv.shift_rows = sshift_rows;
  sv.first = first; sv.stop = stop; sv.every = every;
  sv.sums = survey_sums; sv.doubles = survey_doubles;
  sv.bin_of_step = bin_of_step; sv.bin_rows = bin_rows; sv.nbins = nbins;
  sv.bin_sums = bin_sums; sv.bin_doubles = bin_doubles;
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w, tr, sv);
}

int ludvm_ensemble_run_surveyed_graded(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                                       const double* tables, const double* kin, size_t kin_rows, const double* init,
                                       const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                                       size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                                       long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                                       const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w, const double* seed_x,
                                       const double* seed_z, const long long* release, size_t ntracer, const double* tshift_x,
                                       size_t tshift_rows, const long long* trec_steps, size_t ntrec, double* tracer_rows,
                                       size_t tracer_doubles, const double* survey_x, const double* survey_z, size_t nsurvey,
                                       const double* sshift_x, size_t sshift_rows, long long first, long long stop, long long every,
                                       double* survey_sums, size_t survey_doubles, const int* bin_of_step, size_t bin_rows, int nbins,
                                       double* bin_sums, size_t bin_doubles, double* grad_sums, size_t grad_doubles,
                                       double* bin_grad_sums, size_t bin_grad_doubles) {
  EnsembleTracerArgs tr;
  tr.seed_x = seed_x; tr.seed_z = seed_z; tr.release = release; tr.count = ntracer;
  tr.shift_x = tshift_x; tr.shift_rows = tshift_rows;
  tr.rec_steps = trec_steps; tr.nrec = ntrec;
  tr.rows = tracer_rows; tr.doubles = tracer_doubles;
  EnsembleSurveyArgs sv;
  sv.x = survey_x; sv.z = survey_z; sv.count = nsurvey;
  sv.shift_x = sshift_x; sv.shift_rows = sshift_rows;
  sv.first = first; sv.stop = stop; sv.every = every;
  sv.sums = survey_sums; sv.doubles = survey_doubles;
  sv.bin_of_step = bin_of_step; sv.bin_rows = bin_rows; sv.nbins = nbins;
  sv.bin_sums = bin_sums; sv.bin_doubles = bin_doubles;
  sv.grad_sums = grad_sums; sv.grad_doubles = grad_doubles;
  sv.bin_grad_sums = bin_grad_sums; sv.bin_grad_doubles = bin_grad_doubles;
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w, tr, sv);
}

int ludvm_ensemble_run_integrals(ludvm_ctx* c, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                                 const double* tables, const double* kin, size_t kin_rows, const double* init,
                                 const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                                 size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                                 long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                                 const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w, const double* seed_x,
                                 const double* seed_z, const long long* release, size_t ntracer, const double* tshift_x,
                                 size_t tshift_rows, const long long* trec_steps, size_t ntrec, double* tracer_rows,
                                 size_t tracer_doubles, const double* survey_x, const double* survey_z, size_t nsurvey,
                                 const double* sshift_x, size_t sshift_rows, long long first, long long stop, long long every,
                                 double* survey_sums, size_t survey_doubles, const int* bin_of_step, size_t bin_rows, int nbins,
                                 double* bin_sums, size_t bin_doubles, double* grad_sums, size_t grad_doubles,
                                 double* bin_grad_sums, size_t bin_grad_doubles, double* integral_sums, size_t integral_doubles,
                                 double* energy, size_t energy_doubles, long long energy_first, long long energy_stop,
                                 long long energy_every) {
  EnsembleTracerArgs tr;
  tr.seed_x = seed_x; tr.seed_z = seed_z; tr.release = release; tr.count = ntracer;
  tr.shift_x = tshift_x; tr.shift_rows = tshift_rows;
  tr.rec_steps = trec_steps; tr.nrec = ntrec;
  tr.rows = tracer_rows; tr.doubles = tracer_doubles;
  EnsembleSurveyArgs sv;
  sv.x = survey_x; sv.z = survey_z; sv.count = nsurvey;
  sv.shift_x = sshift_x; sv.shift_rows = sshift_rows;
  sv.first = first; sv.stop = stop; sv.every = every;
  sv.sums = survey_sums; sv.doubles = survey_doubles;
  sv.bin_of_step = bin_of_step; sv.bin_rows = bin_rows; sv.nbins = nbins;
  sv.bin_sums = bin_sums; sv.bin_doubles = bin_doubles;
  sv.grad_sums = grad_sums; sv.grad_doubles = grad_doubles;
  sv.bin_grad_sums = bin_grad_sums; sv.bin_grad_doubles = bin_grad_doubles;
  EnsembleIntegralArgs ig;
  ig.sums = integral_sums; ig.doubles = integral_doubles;
  ig.energy = energy; ig.energy_doubles = energy_doubles;
  ig.first = energy_first; ig.stop = energy_stop; ig.every = energy_every;
  return ensemble_run_body(c, members, npan, ncoef, scalars, scalar_count, tables, kin, kin_rows, init, free_xzg, free_count, desc,
                           snap_steps, nsnap, rows, rows_count, wakes, wake_doubles, wake_n, probe_x, probe_z, nprobe, shift_x,
                           shift_rows, probe_u, probe_w, tr, sv, ig);
}

}  // extern "C"
