// The direct launch plan: how a launch of the direct (non-symmetric) pair kernels divides its sources and targets -- source
// tile, targets per lane, source splits, slab rows -- and which instantiation of pair_kernels.hpp serves it.
// Integer code (the origin-class index arithmetic for host and device, the rest for the host), and nothing else: no kernel, no HIP header.  Any C++17 compiler builds it, which is how Python
// asks (tools/plan_rule.py compiles a few lines of main() around this file); launch.hip fills PlanKnobs from the context and
// dispatches from the DirectVariant it gets back.  Every constant and every predicate of the plan is stated here and nowhere
// else (the symmetric kernels' rule: sym_rule.hpp).
#pragma once
#include <cstddef>
#include <cstdio>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace ludvm {

constexpr int kPlanBlock = 256;          // lanes of a workgroup (= kBlock, pair_kernels.hpp asserts it)
constexpr int kTileF32 = 1024;
// Small source sets (a young wake, a chord-sized launch): with 1024-source tiles a launch of a few hundred sources is
// one tile walked by one wave per SIMD, which issues at ~40 % of the SIMD's rate; 256-source tiles give 4x more splits
// (more workgroups, shorter walks): one self-advection step 21 -> 9-11 us up to 4096 vortices, 46 -> 37 us at
// 12 288, no gain at 16 384 [MI355X].  LUDVM_SMALL_TILE_MAX (sources) overrides the switch-over, 0 disables.
constexpr int kTileF32Small = 256;
constexpr int kTileF64 = 512;
constexpr int kTileF64Few = 128;         // fp64 launches with few targets (chord points): short tiles, more workgroups
                                         // (64: more slabs than the shorter walks save, profiles/r06_march_chain_ab.txt)
constexpr long long kFewTargets = 256;
constexpr long long kTargetBlocks = 16384;  // total workgroups aimed for (2048 resident at 8/CU)
constexpr int kMaxSplit = 2048;
constexpr long long kPatch4MinTargets = 1LL << 20;   // flow-field grids: the 4 x 4 patch from this many grid points
constexpr int kFewGroupsMax = 4;                     // pair_f64_few: source splits a workgroup works at once, at most
constexpr long long kSmallTileMaxDefault = 14000;    // direct fp32 launches with at most this many sources use 256-source tiles
constexpr long long kSmallTileMaxF64Default = 12000; // fp64 launches with at most this many sources use 128-source tiles
constexpr long long kTpl2MinTargets = 131072;        // two targets per lane from this many targets
constexpr long long kSmallTileMaxTargets = 65536;    // the 256-source tile serves at most this many targets

// what launch.hip reads from the context (the defaults are the product's; the measurement build's switches change them)
struct PlanKnobs {
  long long small_tile_max = kSmallTileMaxDefault;
  long long small_tile_max_f64 = kSmallTileMaxF64Default;
  int tune_tpl = 0, tune_split = 0;      // ludvm_set_tuning (0 = the rule)
  int grid_kernel = 2;                   // 1 = 4 points of a row per lane; 2 = patch by size; 3 / 4 = always the 2 x 4 / 4 x 4 patch
  bool few_packed = true;
};

enum PlanPrecision { kPlanF32 = 0, kPlanF32X2 = 1, kPlanF64 = 2 };     // (= LUDVM_PREC_*)

struct DirectPlan {
  int tpl;
  int tile;
  int nsplit;
  long long chunk;
  long long nt_pad;
  long long grid_x, grid_y;
};

inline long long plan_max(long long a, long long b) { return a > b ? a : b; }
inline long long plan_min(long long a, long long b) { return a < b ? a : b; }

// a flow-field grid of nz points per row takes the generic (one grid point per target slot) path, not a row / patch kernel
inline bool grid_is_generic(const PlanKnobs& k, long long grid_nz) { return grid_nz > 0 && !(grid_nz % 4 == 0 && k.tune_tpl == 0); }

// small_ok = false: the launch has no 256-source-tile kernel (generic flow-field grids), keep the chunk a multiple of 1024
// plan_nt: the target count that DECIDES the plan -- tile size, targets per lane and the split of the sources into
// partial sums, i.e. everything the rounding of a result depends on -- when the launch itself covers only a part of a
// larger target set (a block of rows of a flow-field grid: the block then carries the whole grid's bits); 0 = nt.
inline DirectPlan direct_plan(const PlanKnobs& k, long long nt_launch, long long ns, int precision, bool small_ok = true,
                              long long plan_nt = 0, bool grid_patch = false) {
  DirectPlan p{};
  const long long nt = plan_nt > 0 ? plan_nt : nt_launch;
  const bool f64 = precision == kPlanF64;
  p.tile = f64 ? ((nt <= kFewTargets || ns <= k.small_tile_max_f64) ? kTileF64Few : kTileF64) : kTileF32;
  if (!f64 && small_ok && ns <= k.small_tile_max) p.tile = kTileF32Small;
  if (f64) {
    p.tpl = 1;
  } else if (k.tune_tpl == 1 || k.tune_tpl == 2 || k.tune_tpl == 4) {
    p.tpl = k.tune_tpl;
  } else {
    p.tpl = nt >= kTpl2MinTargets ? 2 : 1;
  }
  // the small tile exists for TPL = 1 (and for the 4-points-per-lane grid kernel, whose TPL the launch fixes itself)
  if (p.tile == kTileF32Small && (p.tpl != 1 || nt > kSmallTileMaxTargets)) p.tile = kTileF32;
  // target tiles = workgroups per source split.  The flow-field patch kernels hold 8 or 16 grid points per lane, not tpl:
  // counted with tpl, a 4096 x 4096 grid looked like 32 768 workgroups and got ONE source split -- 4096 workgroups that
  // each walk all the sources for a quarter of a second, and a launch that ends over half such a lifetime (config 5:
  // 8.05e12 pairs/s with one split, 8.13e12 with four, 8.15e12 with eight [MI355X])
  const long long per_wg = grid_patch ? (long long)kPlanBlock * 4 * (nt >= kPatch4MinTargets ? 4 : 2) : (long long)kPlanBlock * p.tpl;
  const long long ttiles = plan_max(1, (nt + per_wg - 1) / per_wg);
  const long long max_split = plan_max(1, (ns + p.tile - 1) / p.tile);
  long long nsplit = k.tune_split > 0 ? k.tune_split : (kTargetBlocks + ttiles - 1) / ttiles;
  nsplit = plan_max(1, plan_min(plan_min(nsplit, max_split), kMaxSplit));
  long long chunk = (plan_max(ns, 1) + nsplit - 1) / nsplit;
  chunk = (chunk + p.tile - 1) / p.tile * p.tile;
  p.chunk = chunk;
  p.nsplit = (int)plan_max(1, (ns + chunk - 1) / chunk);
  p.nt_pad = (nt_launch + 63) / 64 * 64;
  p.grid_x = plan_max(1, (nt_launch + (long long)kPlanBlock * p.tpl - 1) / ((long long)kPlanBlock * p.tpl));
  p.grid_y = p.nsplit;
  return p;
}

// rows of the patch of grid points a lane owns (4 columns), 0 = the row kernel.  Every variant performs the same
// operations on the same operands for a given grid point, so the choice never changes a result bit.
inline int grid_patch_rows(const PlanKnobs& k, long long nt, int tile) {
  if (k.grid_kernel == 1) return 0;
  if (k.grid_kernel == 3 || tile == kTileF32Small) return 2;       // (the 4 x 4 patch exists for 1024-source tiles)
  if (k.grid_kernel == 4) return 4;
  return nt >= kPatch4MinTargets ? 4 : 2;
}

// workgroups of a flow-field grid launch: 256 lanes of 4 row points (patch_rows = 0), or of patch_rows x 4 patches
inline long long grid_kernel_blocks(long long nt, long long grid_nz, int patch_rows) {
  if (patch_rows > 0) {
    const long long nrows = nt / grid_nz, patches = ((nrows + patch_rows - 1) / patch_rows) * (grid_nz / 4);
    return (patches + kPlanBlock - 1) / kPlanBlock;
  }
  return (nt + (long long)kPlanBlock * 4 - 1) / ((long long)kPlanBlock * 4);
}

// pair_f64_few: source splits a workgroup works at once for nt_few array targets; 0 = the launch is not that kernel's
// (more than half a workgroup of targets, several target blocks, one split, no slab, a grid, a target count on the device)
inline int few_groups(const PlanKnobs& k, const DirectPlan& p, long long nt, long long grid_nz, bool slab, bool nt_on_device) {
  const long long nt_few = nt_on_device ? 0 : nt;
  if (!(p.tile == kTileF64Few && k.few_packed && slab && grid_nz == 0 && nt_few >= 1 && 2 * nt_few <= kPlanBlock &&
        p.grid_x == 1 && p.nsplit > 1))
    return 0;
  return (int)plan_min(kPlanBlock / nt_few, kFewGroupsMax);
}

enum DirectKernel { kDirectF32 = 0, kDirectF64 = 1, kDirectF64Few = 2 };

// What launch_pair launches: the instantiation pair_f32<tpl, tile, hilo, grid, local>, pair_f64<tile> or pair_f64_few<tile>,
// and its workgroup counts (blocks_x target blocks x blocks_y source splits, or groups of splits).
struct DirectVariant {
  int kernel;
  int tpl, tile;
  bool hilo;
  int grid;          // 0: array or generic-grid targets; 1: 4 points of a grid row per lane; 2: a patch of rows x 4 per lane
  bool local;
  int groups;        // pair_f64_few: splits per workgroup (0 otherwise)
  long long blocks_x, blocks_y;
};

// one integer per pair_f32 instantiation (launch.hip switches on it)
constexpr int direct_key(int tpl, int tile, bool hilo, int grid, bool local) {
  return (((tpl * 2048 + tile) * 2 + (hilo ? 1 : 0)) * 4 + grid) * 2 + (local ? 1 : 0);
}

// local: the positions are offsets from class origins (PairArgs::scx given); slab: the launch has a partial slab to write to
// (PairArgs::part given: more than one split, or a fused finisher reads the results there); nt: the launch's own target
// count (a.nt); nt_on_device: the TARGET count is completed on the device (PairArgs::nt_dev: the march's roll-up, whose
// targets are the wake) -- a SOURCE count that lives there (PairArgs::ns_dev: the march's chord sums, whose targets are the
// npan + 3 points the host knows) changes nothing here: the plan was made from the host's bound on it
inline DirectVariant direct_variant(const PlanKnobs& k, const DirectPlan& p, int precision, bool local, long long nt, long long grid_nz,
                                    bool slab, bool nt_on_device) {
  DirectVariant v{};
  v.tpl = p.tpl;
  v.tile = p.tile;
  v.blocks_x = p.grid_x;
  v.blocks_y = p.grid_y;
  if (precision == kPlanF64) {
    v.tpl = 1;
    v.groups = few_groups(k, p, nt, grid_nz, slab, nt_on_device);
    v.kernel = v.groups > 0 ? kDirectF64Few : kDirectF64;
    if (v.groups > 0) {
      v.blocks_x = 1;
      v.blocks_y = (p.nsplit + v.groups - 1) / v.groups;
    }
    return v;
  }
  v.kernel = kDirectF32;
  v.local = local;
  const int tpl_array = (p.tpl == 1 || p.tpl == 2) ? p.tpl : 4;
  const bool grid_kernel = grid_nz > 0 && !grid_is_generic(k, grid_nz);
  const bool small_array = p.tile == kTileF32Small && !(grid_nz > 0);
  // local-origin fp32 (LUDVM_PREC_F32 wherever the library lays the positions out itself) replaces hi+lo positions; the grid
  // kernels are plain or local fp32 (a hi+lo launch over a grid generates its points in the array kernels)
  v.hilo = !local && precision == kPlanF32X2;
  if ((local || !(small_array || v.hilo)) && grid_kernel) {
    // flow-field grid: a 2 x 4 patch (or 4 points of a row) per lane; the plan's target blocks are recomputed for it
    const int prows = grid_patch_rows(k, nt, p.tile);
    v.blocks_x = grid_kernel_blocks(nt, grid_nz, prows);
    v.grid = prows > 0 ? 2 : 1;
    v.tpl = prows == 4 ? 16 : (prows == 2 ? 8 : 4);
    if (prows == 4) v.tile = kTileF32;
  } else if (p.tile == kTileF32Small && (local || small_array)) {
    v.tpl = 1;
  } else {
    v.tile = kTileF32;       // (the 256-source tile exists for array targets with one target per lane and the grid kernels)
    v.tpl = tpl_array;
  }
  return v;
}

// ---- origin classes of the local-origin kernels (pair_kernels.hpp, kOriginShift: what they are) -----------------------------
constexpr int kOriginShift = 8;
constexpr int kOriginBlock = 1 << kOriginShift;   // = the 256-vortex tile of pair_sym_f32<4>
// origin record of vortex i
__host__ __device__ inline long long origin_slot(long long i) { return 2 * (i >> kOriginShift) + (i & 1); }
// Which vortex lends origin class (block b, index parity p) its origin when n vortices are stored (n > 256 b): the
// middle one of the class, or its newest while the class is less than half full; a class without a member yet (the
// odd one of a block that holds a single vortex) borrows the block's first vortex, so that its record is a number.
__host__ __device__ inline long long origin_index(long long b, int p, long long n) {
  const long long first = b << kOriginShift;
  const long long mid = first + kOriginBlock / 2 + p;
  if (mid < n) return mid;
  const long long last = (n - 1) - (((n - 1) ^ p) & 1);       // the newest stored index of parity p
  return last >= first ? last : first;
}

// ---- launch rule of the marched observers (march_kernels.hpp: probes, tracers, survey) ---------------------------------------
// `count` points in tiles of point_tile (one workgroup each, padded to `pad` columns of the slab [split][2][pad]); the sources --
// at most ns_ub = n_ub + nfoil, n_ub the step's anchor-derived bound of the wake size after its solve -- in `nsplit` splits of
// `chunk` sources, a multiple of the src_tile sources a kernel stages at once, chosen so that tiles x splits comes to about
// `groups` workgroups, with at most max_split splits (the tracer and survey finishers add them one after the other).  A
// function of count and ns_ub alone: the summation order of a step does not depend on where the calls of a run begin.
struct ObserverRule { long long point_tile, src_tile, groups, max_split; };
struct ObserverPlan { long long tiles, pad, chunk; int nsplit; };

enum ObserverKind { kObsProbes = 0, kObsTracers, kObsTracersF32x2, kObsSurvey, kObsSurveyF32, kObserverKinds };
// probes: one wavefront per tile, about one per SIMD of the device, no cap (their finisher sums the splits as a tree);
// the others: 256 lanes x 2 (float64) or x 4 (fp32) points, about four workgroups per CU
constexpr ObserverRule kObserverRules[kObserverKinds] = {
    {64, 256, 1024, 1024}, {512, 256, 1024, 64}, {1024, 256, 1024, 64}, {512, 256, 1024, 64}, {1024, 256, 1024, 64}};

inline long long observer_tiles(const ObserverRule& r, long long count) { return (count + r.point_tile - 1) / r.point_tile; }
// the splits a step may have, whatever the wake size (count >= 1)
inline long long observer_want(const ObserverRule& r, long long count) {
  return plan_min(r.max_split, plan_max(1, r.groups / observer_tiles(r, count)));
}
inline ObserverPlan observer_plan(const ObserverRule& r, long long count, long long ns_ub) {
  ObserverPlan p;
  p.tiles = observer_tiles(r, count);
  p.pad = p.tiles * r.point_tile;
  const long long want = observer_want(r, count);
  ns_ub = plan_max(ns_ub, 1);
  p.chunk = plan_max(r.src_tile, ((ns_ub + want - 1) / want + r.src_tile - 1) / r.src_tile * r.src_tile);
  p.nsplit = (int)((ns_ub + p.chunk - 1) / p.chunk);       // <= want
  return p;
}
// the slab of any step: nsplit <= observer_want whatever the wake size (probes: at most 1 MiB; the others: at most 16 MiB)
inline size_t observer_slab_bytes(const ObserverRule& r, long long count) {
  return (size_t)observer_want(r, count) * 2 * (size_t)(observer_tiles(r, count) * r.point_tile) * 8;
}

// ---- launch rule of the wake energy (march_kernels.hpp: march_energy_partial; ludvm_march_set_integrals) ---------------------
// The points are the step's own sources, so points and sources both grow with the run: the plan of a step is
// observer_plan(kEnergyRule, ns_ub, ns_ub), a function of the step's anchor-derived bound alone.  512 points per workgroup (256
// lanes x 2), 256-source tiles, about four workgroups per CU, at most 64 splits (the finisher adds them one after the other).
// A constant of its own: kObserverRules is the table of the observers whose points the user supplies.
constexpr ObserverRule kEnergyRule = {512, 256, 1024, 64};
inline ObserverPlan energy_plan(long long ns_ub) { return observer_plan(kEnergyRule, plan_max(ns_ub, 1), ns_ub); }
// the slab [split][pad] of any step of a run whose sources never exceed ns_cap: nsplit <= observer_want, so
// nsplit x tiles <= max(groups, tiles)
inline size_t energy_slab_bytes(long long ns_cap) {
  const long long tiles = observer_tiles(kEnergyRule, plan_max(ns_cap, 1));
  return (size_t)plan_max(kEnergyRule.groups, tiles) * (size_t)kEnergyRule.point_tile * 8;
}

// ---- launch rule of the hi+lo fp32 field sums (field_kernels.hpp: field_hilo_f32, analytic vorticity and velocity gradient) -----
// Targets in workgroups of kFieldHiloTargets (256 lanes x kFieldHiloPerLane points), sources in tiles of kFieldHiloTile; the
// sources in `nsplit` splits of `chunk` sources, a multiple of the tile, so that target workgroups x splits comes to about
// kFieldHiloGroups (eight workgroups per CU), with at most kFieldHiloMaxSplit splits (the finishers add them one after the
// other).  A function of plan_nt -- the whole grid's points when the launch is a block of its rows -- and ns alone: everything
// the rounding of a result depends on.
constexpr int kFieldHiloPerLane = 4;
constexpr int kFieldHiloTile = 256;
constexpr long long kFieldHiloTargets = (long long)kPlanBlock * kFieldHiloPerLane;
constexpr long long kFieldHiloGroups = 2048;
constexpr long long kFieldHiloMaxSplit = 64;
struct FieldHiloPlan { long long chunk; int nsplit; };

inline FieldHiloPlan field_hilo_plan(long long plan_nt, long long ns) {
  const long long tiles = plan_max(1, (plan_nt + kFieldHiloTargets - 1) / kFieldHiloTargets);
  const long long want = plan_min(kFieldHiloMaxSplit, plan_max(1, kFieldHiloGroups / tiles));
  ns = plan_max(ns, 1);
  FieldHiloPlan p;
  p.chunk = ((ns + want - 1) / want + kFieldHiloTile - 1) / kFieldHiloTile * kFieldHiloTile;
  p.nsplit = (int)((ns + p.chunk - 1) / p.chunk);          // <= want
  return p;
}
// workgroups over the targets of one launch, and the columns of a slab row (the lanes past nt store nothing)
inline long long field_hilo_blocks(long long nt) { return plan_max(1, (nt + kFieldHiloTargets - 1) / kFieldHiloTargets); }
inline long long field_hilo_pad(long long nt) { return (nt + 63) / 64 * 64; }

// the instantiation's name as a profiler prints it
inline void direct_kernel_name(const DirectVariant& v, char* out, size_t len) {
  if (v.kernel == kDirectF64Few) std::snprintf(out, len, "pair_f64_few<%d>", v.tile);
  else if (v.kernel == kDirectF64) std::snprintf(out, len, "pair_f64<%d>", v.tile);
  else std::snprintf(out, len, "pair_f32<%d, %d, %s, %d, %s>", v.tpl, v.tile, v.hilo ? "true" : "false", v.grid,
                     v.local ? "true" : "false");
}

}  // namespace ludvm
