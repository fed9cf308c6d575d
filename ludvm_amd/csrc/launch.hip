// libludvm_hip.so -- C-ABI implementation (see include/ludvm_hip.h for the contract and the reference file:line each entry point
// replaces; ctx.hpp for how the library is divided into translation units).  gfx950 only; no CPU path: every entry point either
// runs the HIP kernels or returns an error code.
// This unit: plans and launches of the pair kernels (direct with partial slabs, symmetric with fixed-point accumulators), the
// kernel stopwatch, the fixed-point probe.
#include "ctx.hpp"
#include "sym_prepare_kernels.hpp"

namespace ludvm_host {

// The plan itself is plan_rule.hpp; these hand it the context's settings.
PlanKnobs plan_knobs(const ludvm_ctx* c) {
  PlanKnobs k;
  k.small_tile_max = c->small_tile_max;
  k.small_tile_max_f64 = c->small_tile_max_f64;
  k.tune_tpl = c->tune_tpl;
  k.tune_split = c->tune_split;
  k.grid_kernel = c->grid_kernel;
  k.few_packed = c->few_packed;
  return k;
}
static_assert(kPlanF32 == LUDVM_PREC_F32 && kPlanF32X2 == LUDVM_PREC_F32X2 && kPlanF64 == LUDVM_PREC_F64, "plan_rule.hpp takes the ABI's precision codes");

Plan make_plan(const ludvm_ctx* c, long long nt_launch, long long ns, int precision, bool small_ok, long long plan_nt, bool grid_patch) {
  const DirectPlan d = direct_plan(plan_knobs(c), nt_launch, ns, precision, small_ok, plan_nt, grid_patch);
  Plan p{};
  p.tpl = d.tpl;
  p.tile = d.tile;
  p.nsplit = d.nsplit;
  p.chunk = d.chunk;
  p.nt_pad = d.nt_pad;
  p.grid = dim3((unsigned)d.grid_x, (unsigned)d.grid_y, 1);
  return p;
}

int timed_begin(ludvm_ctx* c, TimedLaunch& t, bool& active) {
  active = c->timing;
  if (!active) return LUDVM_OK;
  if (!c->pool.empty()) {
    t = c->pool.back();
    c->pool.pop_back();
  } else {
    HIPCHK(c, hipEventCreate(&t.e0));
    HIPCHK(c, hipEventCreate(&t.e1));
  }
  HIPCHK(c, hipEventRecord(t.e0, c->stream));
  return LUDVM_OK;
}

int timed_end(ludvm_ctx* c, TimedLaunch& t, bool active) {
  if (!active) return LUDVM_OK;
  HIPCHK(c, hipEventRecord(t.e1, c->stream));
  c->pending.push_back(t);
  return LUDVM_OK;
}

int drain_timing(ludvm_ctx* c) {
  for (auto& t : c->pending) {
    HIPCHK(c, hipEventSynchronize(t.e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, t.e0, t.e1));
    c->total_ms += ms;
    c->launches += 1;
    c->pool.push_back(t);
  }
  c->pending.clear();
  return LUDVM_OK;
}

// Launch the main pair kernel described by `a` (sources, targets and vc4 filled in by the caller)
// under plan `p`; a.part / a.u / a.w / a.nt_pad / a.chunk are completed here.  With more than one
// split the results are left in c->part for a finisher; with one split they go to (u, w).
int launch_pair(ludvm_ctx* c, PairArgs a, const Plan& p, int precision, void* u, void* w) {
  const size_t elt = precision == LUDVM_PREC_F64 ? sizeof(double) : sizeof(float);
  a.chunk = p.chunk;
  a.nt_pad = p.nt_pad;
  a.nsplit = p.nsplit;
  a.u = u;
  a.w = w;
  a.part = nullptr;
  if (p.nsplit > 1 || u == nullptr) {
    CHK(ensure(c, c->part, (size_t)p.nsplit * 2 * (size_t)p.nt_pad * elt));
    a.part = c->part.p;
  }
  dim3 grid = p.grid;
  // a single split asked to land in the slab (fused finisher): the kernel distinguishes by
  // gridDim.y, so give it the direct pointers into slab row 0
  if (p.nsplit == 1 && u == nullptr) {
    a.u = c->part.p;
    a.w = static_cast<char*>(c->part.p) + (size_t)p.nt_pad * elt;
  }
  // which instantiation, and how many workgroups of it: plan_rule.hpp (few array targets with their results in the slab:
  // several source splits per workgroup -- sized from the host's target count; never when THAT lives on the device.  A
  // source count on the device -- the march's chord sums, the launch pair_f64_few exists for -- does not matter)
  DirectPlan d{};
  d.tpl = p.tpl; d.tile = p.tile; d.nsplit = p.nsplit; d.chunk = p.chunk; d.nt_pad = p.nt_pad;
  d.grid_x = grid.x; d.grid_y = grid.y;
  const DirectVariant v = direct_variant(plan_knobs(c), d, precision, a.scx != nullptr, a.nt, a.grid_nz, a.part != nullptr,
                                         a.nt_dev != 0);
  void (*kernel)(PairArgs) = nullptr;
#define LUDVM_PAIR_F32(TPL, TILE, HILO, GRID, LOCAL) \
  case direct_key(TPL, TILE, HILO, GRID, LOCAL): kernel = pair_f32<TPL, TILE, HILO, GRID, LOCAL>; break;
  if (v.kernel == kDirectF64Few) {
    kernel = pair_f64_few<kTileF64Few>;
  } else if (v.kernel == kDirectF64) {
    kernel = v.tile == kTileF64Few ? pair_f64<kTileF64Few> : pair_f64<kTileF64>;
  } else {
    switch (direct_key(v.tpl, v.tile, v.hilo, v.grid, v.local)) {
      // array (and generic-grid) targets: plain, hi+lo, local origins
      LUDVM_PAIR_F32(1, kTileF32Small, false, 0, false) LUDVM_PAIR_F32(1, kTileF32Small, true, 0, false) LUDVM_PAIR_F32(1, kTileF32Small, false, 0, true)
      LUDVM_PAIR_F32(1, kTileF32, false, 0, false) LUDVM_PAIR_F32(2, kTileF32, false, 0, false) LUDVM_PAIR_F32(4, kTileF32, false, 0, false)
      LUDVM_PAIR_F32(1, kTileF32, true, 0, false) LUDVM_PAIR_F32(2, kTileF32, true, 0, false) LUDVM_PAIR_F32(4, kTileF32, true, 0, false)
      LUDVM_PAIR_F32(1, kTileF32, false, 0, true) LUDVM_PAIR_F32(2, kTileF32, false, 0, true) LUDVM_PAIR_F32(4, kTileF32, false, 0, true)
      // flow-field grids: 4 points of a row, a 2 x 4 patch, a 4 x 4 patch per lane
      LUDVM_PAIR_F32(4, kTileF32Small, false, 1, false) LUDVM_PAIR_F32(4, kTileF32, false, 1, false)
      LUDVM_PAIR_F32(4, kTileF32Small, false, 1, true) LUDVM_PAIR_F32(4, kTileF32, false, 1, true)
      LUDVM_PAIR_F32(8, kTileF32Small, false, 2, false) LUDVM_PAIR_F32(8, kTileF32, false, 2, false)
      LUDVM_PAIR_F32(8, kTileF32Small, false, 2, true) LUDVM_PAIR_F32(8, kTileF32, false, 2, true)
      LUDVM_PAIR_F32(16, kTileF32, false, 2, false) LUDVM_PAIR_F32(16, kTileF32, false, 2, true)
      default: break;
    }
  }
#undef LUDVM_PAIR_F32
  if (!kernel) return fail(c, LUDVM_E_ARG, "no direct pair kernel for this launch plan");
  grid = dim3((unsigned)v.blocks_x, (unsigned)v.blocks_y, 1);
  TimedLaunch t{};
  bool active = false;
  CHK(timed_begin(c, t, active));
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  CHK(timed_end(c, t, active));
  return LUDVM_OK;
}

// pair kernel + split reduction into (u, w) device arrays of the precision's type
int induce_device(ludvm_ctx* c, const PairArgs& a, long long nt, long long ns, int precision, void* u, void* w,
                  long long plan_nt) {
  if (nt == 0) return LUDVM_OK;
  const size_t elt = precision == LUDVM_PREC_F64 ? sizeof(double) : sizeof(float);
  if (ns == 0) {
    HIPCHK(c, hipMemsetAsync(u, 0, (size_t)nt * elt, c->stream));
    HIPCHK(c, hipMemsetAsync(w, 0, (size_t)nt * elt, c->stream));
    return LUDVM_OK;
  }
  const bool grid_generic = grid_is_generic(plan_knobs(c), a.grid_nz);
  // (whatever form of the grid kernel runs -- LUDVM_GRID_KERNEL can force one --: the plan, and with it the bits, stays the same)
  const bool grid_patch = a.grid_nz > 0 && !grid_generic && precision == LUDVM_PREC_F32;
  Plan p = make_plan(c, nt, ns, precision, !grid_generic, plan_nt, grid_patch);
  CHK(launch_pair(c, a, p, precision, u, w));
  if (p.nsplit > 1) {
    if (precision == LUDVM_PREC_F64)
      hipLaunchKernelGGL(finish_sum<double>, dim3(blocks_for(nt)), dim3(kBlock), 0, c->stream,
                         static_cast<const double*>(c->part.p), nt, p.nt_pad, p.nsplit, static_cast<double*>(u),
                         static_cast<double*>(w));
    else
      hipLaunchKernelGGL(finish_sum<float>, dim3(blocks_for(nt)), dim3(kBlock), 0, c->stream,
                         static_cast<const float*>(c->part.p), nt, p.nt_pad, p.nsplit, static_cast<float*>(u),
                         static_cast<float*>(w));
    HIPCHK(c, hipGetLastError());
  }
  return LUDVM_OK;
}

static_assert(64 * 8 == LUDVM_SYM_TILE, "the multi-GPU entry points always use the 512-vortex tile");

// The launch rule itself is sym_rule.hpp; these hand it the context's settings.
SymKnobs sym_knobs(const ludvm_ctx* c) {
  SymKnobs k;
  k.sym_mode = c->sym_mode;
  k.self_order = c->self_order;
  k.tile_t = c->tune_sym_t;
  k.tune_split = c->tune_split;
  k.tune_rsplit = c->tune_sym_rsplit;
  k.quad = c->sym_quad;
  k.quad_min_tiles = c->sym_quad_min_tiles;
  k.tail_items = c->sym_tail_items;
  return k;
}
long long sym_threshold(const ludvm_ctx* c, bool march) { return sym_min_n(sym_knobs(c), march); }
bool use_symmetric(const ludvm_ctx* c, long long n, double vc4, bool march) {
  return sym_use(sym_knobs(c), n, (float)vc4 > 0.0f, march);
}
bool use_self_order(const ludvm_ctx* c, long long n) { return sym_self_order(sym_knobs(c), n); }
// (local origins fit both tiles: a 512-vortex tile keeps its targets twice)
int sym_tile_t(const ludvm_ctx* c, long long n, bool hilo) { return sym_tile(sym_knobs(c), n, hilo); }

// Symmetric kernel over I tiles [i_first, i_first + i_count) of the tile ring of (x, z, g)[0, n); raw fixed-point
// sums are ADDED into acc_u / acc_w (n each, zeroed by the caller).  The partition of the work into partial sums
// is a function of n and T alone (sym_geometry).  n_dev (march): the vortex count is read on the device; it lies in
// [n_lo, n], and the grid is sized for the largest wave count any such n needs.
int launch_sym_tiles(ludvm_ctx* c, int T, const SymOperands& o, long long n, long long i_first, long long i_count, double vc4,
                     const long long* n_dev, long long n_lo, bool sharded) {
  if (n >= (1LL << 31)) return fail(c, LUDVM_E_ARG, "the symmetric kernel indexes vortices with 32 bits: n < 2^31");
  SymArgs a{};
  a.x = o.x; a.z = o.z; a.g = o.g; a.n = n;
  a.n_dev = n_dev;
  a.xl = o.xl; a.zl = o.zl;
  a.cx = o.cx; a.cz = o.cz;
  const SymKnobs k = sym_knobs(c);
  const SymVariant v = sym_variant(k, n, T, o.xl && o.zl);
  const SymGeom& gm = v.g;
  a.tune_split = k.tune_split;
  a.tune_rsplit = v.tune_rsplit;
  a.shard_rank = (n_dev && sharded) ? c->shard_rank : 0;       // (host-sized launches get their tile block as arguments)
  a.shard_world = (n_dev && sharded) ? c->shard_world : 1;
  a.tail_items = k.tail_items;
  a.ntiles = gm.ntiles;
  a.dmax = gm.dmax;
  a.i_first = i_first;
  a.i_count = i_count;
  a.ysplit = gm.ysplit;
  a.rsplit = gm.rsplit;
  a.ytail = gm.ytail;
  a.rbulk = gm.rbulk;
  a.xcd_run = c->xcd_run;
  a.acc_u = o.acc_u;
  a.acc_w = o.acc_w;
  a.scale = o.scale;
  a.bad = o.bad;
  a.vc4 = (float)vc4;
  // workgroups: 4 / rsplit items (tile, d-chunk) each
  long long blocks = sym_blocks(i_count, gm.ysplit, gm.rsplit, gm.ytail, gm.rbulk, c->xcd_run);
  if (n_dev) blocks = std::max(blocks, sym_grid_bound(k, v, false, n_lo, n, c->xcd_run));
  if (!n_dev && i_count == 0) return LUDVM_OK;     // an owner without tiles (fewer tiles than owners)
  blocks = std::max<long long>(blocks, 1);         // (n_dev: the share is decided on the device; surplus waves leave)
  // Large launches: the quad variant (four I tiles of a workgroup share each partner tile: a quarter of the atomics) plus a
  // launch of the plain kernel restricted to the diagonal tiles; owners of a sharded ring must own whole quads.
  if (v.quad) {
    if (i_first % 4 != 0 || (i_count % 4 != 0 && i_first + i_count != gm.ntiles))
      return fail(c, LUDVM_E_ARG, "symmetric kernel, quad variant: an owner's tile block must start and end on multiples of 4 tiles");
    TimedLaunch tq{};
    bool act = false;
    CHK(timed_begin(c, tq, act));
    SymArgs d = a;
    d.diag_only = 1;
    const long long dblocks = std::max<long long>(1, sym_blocks(n_dev ? gm.ntiles : i_count, 1, 1, 0, 1, c->xcd_run));
    hipLaunchKernelGGL((pair_sym_f32<8, false, 1>), dim3((unsigned)dblocks), dim3(kBlock), 0, c->stream, d);
    long long qblocks = quad_blocks(n_dev ? gm.ntiles : i_count, v.q.ysplit, c->xcd_run);
    // (the device derives the chunks from its own vortex count)
    if (n_dev) qblocks = std::max(qblocks, sym_grid_bound(k, v, true, n_lo, n, c->xcd_run));
    hipLaunchKernelGGL((pair_sym_quad_f32<8>), dim3((unsigned)std::max<long long>(qblocks, 1)), dim3(kBlock), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    CHK(timed_end(c, tq, act));
    return LUDVM_OK;
  }
  TimedLaunch t{};
  bool active = false;
  CHK(timed_begin(c, t, active));
  const dim3 grid((unsigned)blocks);
  const dim3 blk(kBlock);
#define LUDVM_SYM_LAUNCH(TT, HH)                                                                              \
  switch (gm.rsplit) {                                                                                        \
    case 0: hipLaunchKernelGGL((pair_sym_f32<TT, HH, 0>), grid, blk, 0, c->stream, a); break;                 \
    case 1: hipLaunchKernelGGL((pair_sym_f32<TT, HH, 1>), grid, blk, 0, c->stream, a); break;                 \
    case 2: hipLaunchKernelGGL((pair_sym_f32<TT, HH, 2>), grid, blk, 0, c->stream, a); break;                 \
    default: hipLaunchKernelGGL((pair_sym_f32<TT, HH, 4>), grid, blk, 0, c->stream, a); break;                \
  }
  if (v.hilo) { LUDVM_SYM_LAUNCH(4, true) }
  else if (v.T == 8) { LUDVM_SYM_LAUNCH(8, false) }
  else { LUDVM_SYM_LAUNCH(4, false) }
#undef LUDVM_SYM_LAUNCH
  HIPCHK(c, hipGetLastError());
  CHK(timed_end(c, t, active));
  return LUDVM_OK;
}

// The symmetric kernel's accumulators: [2 NaN counters | acc_u nt_pad | acc_w nt_pad] 64-bit integers, in the context's
// own buffer or in the caller's (ludvm_set_shard).  *acc points at acc_u; the counters sit at acc[-2], acc[-1].
int acc_buffer(ludvm_ctx* c, long long nt_pad, long long** acc) {
  const size_t bytes = ((size_t)2 * (size_t)nt_pad + 2) * sizeof(long long);
  if (c->ext_acc) {
    if (bytes > c->ext_acc_bytes) return fail(c, LUDVM_E_NOMEM, "the accumulator buffer given to ludvm_set_shard is too small");
    *acc = static_cast<long long*>(c->ext_acc) + 2;
    return LUDVM_OK;
  }
  CHK(ensure(c, c->acc, bytes));
  *acc = static_cast<long long*>(c->acc.p) + 2;
  return LUDVM_OK;
}

bool sharded_at(const ludvm_ctx* c, long long n) { return (c->shard_world > 1 || c->comm_force) && n >= c->shard_min_n; }

// tile block of a shard owner (whole quads of 4 tiles: sym_rule.hpp, shard_block)
void shard_tiles(const ludvm_ctx* c, long long ntiles, long long* first, long long* count) {
  unsigned long long f, cnt;
  shard_block((unsigned long long)ntiles, c->shard_rank, c->shard_world, &f, &cnt);
  *first = (long long)f;
  *count = (long long)cnt;
}

// Fixed-point scale record for circulations g[0, n) into (scale, bad); `partial` = workspace for the chunk sums.
int launch_sym_prepare(ludvm_ctx* c, const float* g, long long n, double vc4, SymScale* scale, long long* bad) {
  const long long nparts = (n + kPrepChunk - 1) / kPrepChunk;
  if (nparts <= 1) {
    hipLaunchKernelGGL(sym_prepare, dim3(1), dim3(kPrepBlock), 0, c->stream, g, n, vc4, scale, bad, (double*)nullptr);
  } else {
    CHK(ensure(c, c->symsc, 128 + (size_t)nparts * sizeof(double)));
    // (the record itself may live in c->symsc: re-derive the pointers after a grow)
    double* partial = reinterpret_cast<double*>(static_cast<char*>(c->symsc.p) + 128);
    hipLaunchKernelGGL(sym_prepare, dim3((unsigned)nparts), dim3(kPrepBlock), 0, c->stream, g, n, vc4, scale, bad, partial);
    hipLaunchKernelGGL(sym_prepare_final, dim3(1), dim3(64), 0, c->stream, partial, (int)nparts, vc4, scale, bad);
  }
  HIPCHK(c, hipGetLastError());
  return LUDVM_OK;
}

// Symmetric self-interaction of all of (x, z, g)[0, n) with the context's accumulators: zero them, derive the
// fixed-point scale from sum|Gamma| (unless the caller -- the march -- maintains it: scale / bad given), run the
// kernel.  The raw sums are left in c->acc as [acc_u | acc_w], each nt_pad 64-bit integers.
int launch_sym(ludvm_ctx* c, SymOperands o, long long n, double vc4, long long* nt_pad_out, const long long** acc_out,
               const long long** bad_out, const long long* n_dev, long long n_lo) {
  const long long nt_pad = (n + 63) / 64 * 64;
  long long* acc = nullptr;
  CHK(acc_buffer(c, nt_pad, &acc));
  CHK(ensure(c, c->symsc, 128 + (size_t)((n + kPrepChunk - 1) / kPrepChunk) * sizeof(double)));
  HIPCHK(c, hipMemsetAsync(acc - 2, 0, ((size_t)2 * (size_t)nt_pad + 2) * sizeof(long long), c->stream));
  o.acc_u = acc;
  o.acc_w = acc + nt_pad;
  if (!o.scale) {
    CHK(launch_sym_prepare(c, o.g, n, vc4, ctx_scale(c), ctx_bad(c)));
    o.scale = ctx_scale(c);
    o.bad = ctx_bad(c);
  }
  const bool sharded = sharded_at(c, n);      // (n: exact, or the march's bound -- the same number on every owner)
  if (sharded) o.bad = acc - 2;               // counted where the all-reduce sees it
  const int T = sym_tile_t(c, n, o.xl && o.zl);
  const long long ntiles = (n + 64LL * T - 1) / (64LL * T);
  long long first = 0, count = ntiles;
  if (sharded) shard_tiles(c, ntiles, &first, &count);
  CHK(launch_sym_tiles(c, T, o, n, first, count, vc4, n_dev, n_lo, sharded));
  if (sharded) CHK(reduce_accumulators(c, acc, nt_pad));
  *nt_pad_out = nt_pad;
  *acc_out = acc;
  *bad_out = o.bad;
  return LUDVM_OK;
}

}  // namespace ludvm_host

extern "C" {

/* ---- measurement ---------------------------------------------------------------------------- */

int ludvm_fixed_point_probe(ludvm_ctx* c, const float* values, size_t n, int scale_log2, long long* units) {
  if (!c) return LUDVM_E_ARG;
  if (n && (!values || !units)) return fail(c, LUDVM_E_ARG, "null array");
  if (scale_log2 < -120 || scale_log2 > 120) return fail(c, LUDVM_E_ARG, "scale_log2 must lie in [-120, 120]");
  if (n == 0) return LUDVM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->arena, Arena::need(n, 4) + Arena::need(n, 8)));
  Arena ar(c->arena.p);
  float* dv = ar.take<float>(n);
  long long* du = ar.take<long long>(n);
  HIPCHK(c, hipMemcpyAsync(dv, values, n * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(fx_probe, dim3(blocks_for((long long)n)), dim3(kBlock), 0, c->stream, dv, (long long)n,
                     (float)std::ldexp(1.0, scale_log2), du);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(units, du, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LUDVM_OK;
}

int ludvm_kernel_timing(ludvm_ctx* c, int enable) {
  if (!c) return LUDVM_E_ARG;
  c->timing = enable != 0;
  return LUDVM_OK;
}

int ludvm_kernel_time_ms(ludvm_ctx* c, int reset, double* avg_ms, long long* launches) {
  if (!c) return LUDVM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(drain_timing(c));
  if (avg_ms) *avg_ms = c->launches ? c->total_ms / (double)c->launches : 0.0;
  if (launches) *launches = c->launches;
  if (reset) {
    c->total_ms = 0.0;
    c->launches = 0;
  }
  return LUDVM_OK;
}

}  // extern "C"
