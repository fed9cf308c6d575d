// The symmetric launch rule: which kernel serves a self-interaction launch of n vortices -- direct or symmetric, 256- or
// 512-vortex tiles, 1, 2 or 4 waves per work item or mixed granularity, the quad variant -- and the geometry of that launch.
// Integer code for host AND device (the kernels of pair_sym_kernels.hpp re-derive their geometry from a vortex count they
// read on the device), and nothing else: no kernel, no HIP header.  Any C++17 compiler builds it, which is how Python asks
// (tools/sym_rule.py compiles a few lines of main() around this file); launch.hip fills SymKnobs from the context.
// Every threshold and every predicate of the rule is stated here and nowhere else.
#pragma once
#include <cstddef>
#include <cstdio>
#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace ludvm {

// Launch geometry as a function of the vortex count alone (not of the owner's share, not of a host-side bound):
// the partition of the work into partial sums -- and with it every bit of the result -- is then the same for a
// march step sized from an upper bound, for one GPU and for G GPUs that own I-tile blocks of the same ring.
constexpr long long kSymTargetWaves = 8 * 65536;   // (I, d-chunk) work items aimed for over the whole ring
constexpr long long kSymMaxSplit = 64;
constexpr long long kSymMaxSplitTuned = 1024;      // what ludvm_set_tuning may ask for (measurements)
constexpr long long kXcds = 8;                        // XCDs of an MI355X: workgroup b is dispatched to XCD b % 8
constexpr long long kSymMaxRsplit = 4;
constexpr long long kSymMinItems = 10500;          // measured (profiles/r02_atomics_cost_and_lds_reduction.txt, table 4)
// Mixed granularity (rsplit = 0): a launch ends when its last waves do, and a launch of equal work items drains over about
// half an item's lifetime.  So the items that are dispatched LAST -- those of the highest d-chunks, in every owner's order
// -- are worked by four waves each (a quarter of the rotation steps per wave, partial sums added through LDS), the bulk
// before them by as many waves per item as the size rule gives (`rbulk` = 1 or 2; where the rule gives four there is
// nothing finer and the launch keeps one granularity).  Which items those are is a function of the vortex count alone (their
// d-chunk), so the partition into partial sums is the same for every owner of a sharded ring.  History [MI355X]: the first
// form (bulk always by single waves, 3072 items for the end, chunk counts that could leave the end empty) lost as often
// as it won (profiles/r03_mixed_granularity_negative_result.txt) and was shelved; with the bulk following the rule, no empty
// chunks and 1536 items for the end it is never slower than one granularity under sustained load and 1-5 % faster from
// 57 000 vortices up to the quad variant's range (profiles/r03_mixed_granularity_by_rule.txt), and is the default there.
// ludvm_set_sym_tuning(.., -1) / LUDVM_SYM_MIXED=1: at every size; -2 / LUDVM_SYM_MIXED=0: nowhere.
constexpr long long kSymTailItems = 1536;          // (half of 256 CUs x 4 SIMDs x 3 waves: measured, see above)
struct SymGeom { long long ntiles, dmax, dtot; int ysplit, rsplit, ytail, rbulk; };
// Placement of a launch's (unit, d-chunk) work items on the 8 XCDs (unit = I tile, or quad of I tiles): workgroup b runs
// on XCD b % 8.  The launch's `ys` d-chunks are cut into at most 8 RUNS of K = ceil(ys / 8) consecutive chunks, and in run r
// XCD x takes eighth (x + r) % 8 of the units.  Within a run an XCD works on neighbouring units whose ring offsets grow
// chunk by chunk, i.e. on overlapping partner tiles, which its L2 serves (round 2's point: memory-side fetches 2 GB ->
// 0.03 GB per N = 2^20 launch); and because the eighths ROTATE from run to run, every XCD meets every eighth once: all get
// the same number of items to within K - 1.  With a fixed eighth per XCD (rounds 2 and 3 until this) a unit count that is
// not a multiple of 8 left seven XCDs waiting for the eighth one: 129 tiles = 7 x 16 + 17, 6 % of the launch; 489 quads
// (N = 1e6) = 7 x 61 + 62, 1.4 % [MI355X].  (Rotating with EVERY chunk balances to within one item, and was measured
// first: same speed, but every chunk then meets new partner tiles: 1.0 GB of fetches per N = 1e6 launch instead of 0.03.)
struct XcdShare { unsigned lo, n; };
__host__ __device__ inline XcdShare xcd_share(unsigned units, unsigned e) {
  const unsigned lo = (unsigned)((unsigned long long)units * e / (unsigned)kXcds);
  return XcdShare{lo, (unsigned)((unsigned long long)units * (e + 1) / (unsigned)kXcds) - lo};
}
__host__ __device__ inline unsigned xcd_run(unsigned ys, int k) {
  return k > 0 ? (unsigned)k : (ys > 0 ? (ys + (unsigned)kXcds - 1) / (unsigned)kXcds : 1);
}
// items of XCD x in chunks [y0, y0 + ny) of a launch of ys chunks
__host__ __device__ inline unsigned long long xcd_items(unsigned units, unsigned ys, unsigned x, unsigned y0, unsigned ny,
                                                         int k = 0) {
  const unsigned K = xcd_run(ys, k);
  unsigned long long t = 0;
  for (unsigned y = y0; y < y0 + ny;) {
    const unsigned r = y / K, y_end = (r + 1) * K < y0 + ny ? (r + 1) * K : y0 + ny;
    t += (unsigned long long)xcd_share(units, (x + r) % (unsigned)kXcds).n * (y_end - y);
    y = y_end;
  }
  return t;
}
// item q of XCD x's list over chunks [y0, y0 + ny) (run by run, chunk-major within a run): its chunk and unit; false
// beyond the list
__host__ __device__ inline bool xcd_item(unsigned units, unsigned ys, unsigned x, unsigned y0, unsigned ny, unsigned q,
                                         unsigned& y_out, unsigned& unit, int k = 0) {
  const unsigned K = xcd_run(ys, k);
  y_out = y0; unit = 0;
  for (unsigned y = y0; y < y0 + ny;) {
    const unsigned r = y / K, y_end = (r + 1) * K < y0 + ny ? (r + 1) * K : y0 + ny;
    const XcdShare s = xcd_share(units, (x + r) % (unsigned)kXcds);
    const unsigned cnt = s.n * (y_end - y);
    if (q < cnt) {               // (s.n > 0 here)
      const unsigned c = q / s.n;
      y_out = y + c;
      unit = s.lo + (q - c * s.n);
      return true;
    }
    q -= cnt;
    y = y_end;
  }
  return false;
}
// Workgroups per XCD of a launch over i_count I tiles (the largest XCD's; surplus workgroups leave at once).  With
// rsplit = 0 an XCD's first workgroups hold 4 / rbulk bulk items each (d-chunks below ysplit - ytail), the rest one
// four-wave item each.
__host__ __device__ inline long long sym_blocks_xcd(long long i_count, long long ysplit, int rsplit, long long ytail,
                                                    int rbulk = 1, int k = 0) {
  long long most = 0;
  for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
    long long wg;
    if (rsplit == 0) {
      const unsigned y1 = (unsigned)(ysplit - ytail);
      wg = ((long long)xcd_items((unsigned)i_count, (unsigned)ysplit, x, 0, y1, k) * rbulk + 3) / 4 +
           (long long)xcd_items((unsigned)i_count, (unsigned)ysplit, x, y1, (unsigned)ytail, k);
    } else {
      const long long ipb = 4 / rsplit;
      wg = ((long long)xcd_items((unsigned)i_count, (unsigned)ysplit, x, 0, (unsigned)ysplit, k) + ipb - 1) / ipb;
    }
    most = wg > most ? wg : most;
  }
  return most;
}
__host__ __device__ inline long long sym_blocks(long long i_count, long long ysplit, int rsplit, long long ytail = 0,
                                                int rbulk = 1, int k = 0) {
  return kXcds * sym_blocks_xcd(i_count, ysplit, rsplit, ytail, rbulk, k);
}

// Tile block of owner `rank` of `world` on a ring of ntiles tiles: whole quads of 4 consecutive tiles (the quad variant of
// the kernel adds the partial sums of a quad's four waves in fp32 before they are converted, so a quad must not be cut
// between two owners; the last block ends with the ring)
__host__ __device__ inline void shard_block(unsigned long long ntiles, int rank, int world, unsigned long long* first,
                                            unsigned long long* count) {
  const unsigned long long quads = (ntiles + 3) / 4;
  unsigned long long lo = 4 * (quads * (unsigned long long)rank / (unsigned long long)world);
  unsigned long long hi = 4 * (quads * (unsigned long long)(rank + 1) / (unsigned long long)world);
  if (lo > ntiles) lo = ntiles;
  if (hi > ntiles) hi = ntiles;
  *first = lo;
  *count = hi - lo;
}

// (I: long long on the host, unsigned on the device -- the kernel's prologue runs once per wave and a 64-bit division
// costs ~100 instructions there; both give the same numbers for n < 2^31)
template <typename I>
__host__ __device__ inline void sym_geometry_t(I n, int T, int tune_split, int tune_rsplit, I tail_items, I& ntiles, I& dmax,
                                               I& dtot, int& ysplit, int& rsplit, int& ytail, int& rbulk) {
  const I W = (I)(64 * T);
  ntiles = (n + W - 1) / W;
  dmax = ntiles > 0 ? (ntiles - 1) / 2 : 0;
  dtot = dmax + ((ntiles % 2 == 0 && ntiles > 1) ? 1 : 0);
  const I nt1 = ntiles > 0 ? ntiles : 1;
  // (kSymTargetWaves / nt1 rounded up is at least kSymMaxSplit whenever nt1 <= kSymTargetWaves / kSymMaxSplit: no division)
  I ys = tune_split > 0 ? (I)tune_split
                        : (nt1 <= (I)(kSymTargetWaves / kSymMaxSplit) ? (I)kSymMaxSplit : ((I)kSymTargetWaves + nt1 - 1) / nt1);
  if (ys > (I)kSymMaxSplit && tune_split <= 0) ys = (I)kSymMaxSplit;
  if (ys > (I)kSymMaxSplitTuned) ys = (I)kSymMaxSplitTuned;
  if (ys > dtot) ys = dtot;
  if (ys < 1) ys = 1;
  // no empty chunks: with `per` offsets per chunk, ceil(dtot / per) chunks cover the ring (96 offsets in 64 chunks would be 48
  // chunks of 2 and 16 empty ones -- waves that leave at once, and a mixed launch's fine-grained end without any work)
  if (dtot > 0) {
    const I per0 = (dtot + ys - 1) / ys;
    ys = (dtot + per0 - 1) / per0;
  }
  I rs = 1;
  ytail = 0;
  rbulk = 1;
  if (tune_rsplit == -4) {                     // the quad variant, whatever the size: single-wave geometry
    rs = 1;
  } else if (tune_rsplit == 1 || tune_rsplit == 2 || tune_rsplit == 4) {
    rs = (I)tune_rsplit;
  } else if (tune_rsplit == -1) {              // mixed: the last d-chunks by four waves per item
    rs = 0;
    const I yt = (tail_items + nt1 - 1) / nt1;
    ytail = (int)(yt > ys ? ys : yt);
    I rb = 1;                                  // the bulk before them by as many waves per item as the size rule gives
    while (rb < (I)kSymMaxRsplit && nt1 * ys * rb < (I)kSymMinItems) rb *= 2;
    rbulk = (int)rb;
  } else {                                     // by size: the smallest number of waves per item that gives enough work items
    while (rs < (I)kSymMaxRsplit && nt1 * ys * rs < (I)kSymMinItems) rs *= 2;
    // ... and, where that leaves room below four waves per item, the items dispatched last finer than the bulk (mixed
    // granularity).  tune_rsplit = -2: one granularity per launch, as until round 3
    if (tune_rsplit != -2 && rs < (I)kSymMaxRsplit) {
      rbulk = (int)rs;
      rs = 0;
      const I yt = (tail_items + nt1 - 1) / nt1;
      ytail = (int)(yt > ys ? ys : yt);
    }
  }
  ysplit = (int)ys;
  rsplit = (int)rs;
}
__host__ __device__ inline SymGeom sym_geometry(long long n, int T, int tune_split, int tune_rsplit,
                                                 long long tail_items = kSymTailItems) {
  SymGeom g;
  sym_geometry_t<long long>(n, T, tune_split, tune_rsplit, tail_items, g.ntiles, g.dmax, g.dtot, g.ysplit, g.rsplit, g.ytail,
                            g.rbulk);
  return g;
}

// Quad variant (pair_sym_quad_f32, described at the kernel): four consecutive I tiles per workgroup, their d-chunks.
constexpr unsigned kQuad = 4;
constexpr unsigned kQuadSplit = 128;
struct QuadGeom { unsigned ntiles, dmax, dtot, Dtot; int ysplit, per, nlong, pshort; };
template <typename I>
__host__ __device__ inline QuadGeom quad_geometry(I n, int T, int tune_split) {
  QuadGeom g;
  const I W = (I)(64 * T);
  const I nt = (n + W - 1) / W;
  g.ntiles = (unsigned)nt;
  g.dmax = nt > 0 ? (unsigned)((nt - 1) / 2) : 0;
  g.dtot = g.dmax + ((nt % 2 == 0 && nt > 1) ? 1u : 0u);
  g.Dtot = g.dtot + (kQuad - 1);
  // d-chunks per quad.  An item of `per` rounds lives per x ~0.17 ms; a launch drains over about half the lifetime of the
  // items dispatched LAST, while every item pays ~4 % of one round for its own targets (loads, I-side conversions and
  // atomics).  Uniform chunks (measured at N = 1e6, same box: 64 chunks 112.0 ms, 128: 111.6, 256: 111.6;
  // tools/ab_quad_chunks.sh) cannot have both small; so the chunks TAPER: with u = Dtot / 128 rounded up, the first seven
  // eighths of the offsets go in chunks of 2 u rounds and the last eighth -- the highest chunk numbers, which every XCD
  // dispatches last -- in chunks of u / 4 (at least 1) rounds.  A function of the vortex count alone, like everything
  // about the partition.  ludvm_set_tuning(.., k > 0) asks for k uniform chunks instead (measurements).
  if (tune_split > 0) {
    unsigned ys = (unsigned)tune_split;
    if (ys > (unsigned)kSymMaxSplitTuned) ys = (unsigned)kSymMaxSplitTuned;
    if (ys > g.Dtot) ys = g.Dtot;
    if (ys < 1) ys = 1;
    g.per = (int)((g.Dtot + ys - 1) / ys);
    g.ysplit = (int)((g.Dtot + (unsigned)g.per - 1) / (unsigned)g.per);     // (no empty chunk at the end)
    g.nlong = g.ysplit;
    g.pshort = g.per;
    return g;
  }
  const unsigned u = (g.Dtot + kQuadSplit - 1) / kQuadSplit;
  const unsigned P = 2 * (u > 0 ? u : 1), ps = u / 4 > 0 ? u / 4 : 1;
  const unsigned nlong = (g.Dtot - g.Dtot / 8) / P;
  const unsigned rest = g.Dtot - nlong * P;
  g.per = (int)P;
  g.pshort = (int)ps;
  g.nlong = (int)nlong;
  g.ysplit = (int)(nlong + (rest + ps - 1) / ps);
  if (g.ysplit < 1) g.ysplit = 1;
  return g;
}
// ring offsets D in [lo, hi) of d-chunk yq of a quad
__host__ __device__ inline void quad_chunk(const QuadGeom& g, unsigned yq, int& lo, int& hi) {
  const bool lg = (int)yq < g.nlong;
  lo = 1 + (lg ? (int)yq * g.per : g.nlong * g.per + ((int)yq - g.nlong) * g.pshort);
  hi = lo + (lg ? g.per : g.pshort);
  if (hi > (int)g.Dtot + 1) hi = (int)g.Dtot + 1;
}
// workgroups of a quad launch over I tiles [i_first, i_first + i_count) (i_first a multiple of 4): one per (quad, d-chunk),
// the same number for each XCD
__host__ __device__ inline long long quad_blocks(long long i_count, int ysplit, int k = 0) {
  const unsigned quads = (unsigned)((i_count + kQuad - 1) / kQuad);
  long long most = 0;
  for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
    const long long wg = (long long)xcd_items(quads, (unsigned)ysplit, x, 0, (unsigned)ysplit, k);
    most = wg > most ? wg : most;
  }
  return kXcds * most;
}

// ---- which launch is symmetric, with which tile and which variant ----------------------------------------------------
constexpr long long kSymMinN = 16384;   // below this the direct kernel's launch is as fast
// Vortices per lane of the symmetric kernel: 8 (tile 512, 158-162 VGPRs: 3 waves/SIMD) from ~4e4 vortices up, where
// halving the rotation / LDS-read cost per pair wins 2-7 % (with the rotation steps of a tile pair shared by two or four
// waves below ~8e4); 4 (tile 256, 70-90 VGPRs) below, where more and smaller tiles balance better, and for hi+lo
// positions (not instantiated for the 512-vortex tile: hi+lo is instruction-bound either way).
// Round 6 (profiles/r06_mid_size_variant_table.txt: every candidate forced at 22 sizes, ordered sheet, sustained load): between
// 35 000 and 44 000 vortices the two tiles alternate within +-2 % with the parity of their tile counts; the one size where the
// pick lost more (36 000: 512-vortex tiles 3.5 % behind) is what moved the switch from 34 816 to 36 864 = 72 tiles of 512.
constexpr long long kSymT8MinN = 36864;
// The symmetric kernel accumulates in fixed point, which needs the bound sum|Gamma| / (sqrt(2) v_core) on the raw
// sums: point vortices (v_core = 0, or so small that v_core^4 vanishes in fp32) take the direct kernel.
// In the march a symmetric step is an OVERLAPPED step: chord sums and solve run beside the kernel instead of in front
// of it (~40 us of a ~60 us serial step at 1e4 vortices), so it pays earlier there: from ~11 000 vortices [MI355X]
// (profiles/r02_march_symmetric_threshold.txt).
constexpr long long kSymMinNMarch = 11264;
// The quad variant takes launches of at least this many 512-vortex tiles whose items the size rule gives one wave each.
constexpr long long kSymQuadMinTiles = 640;
// A symmetric launch on plain fp32 device arrays (ludvm_induce_dev_f32, the self path of ludvm_advect_dev_f32) of at least
// this many vortices is evaluated in Morton order: one O(N) pre-pass (bounding box, keys, stable sort, gather), the pair
// kernel on the ordered copies, the way back fused into the finisher.  The pair kernel has no data-dependent path; what
// the order changes is its operands' statistics -- a tile is then a small box, the high bits of every dx, dz, r^2 and rsq
// of a tile pair nearly constant -- and with them the power per operation and the clock the chip holds under this
// energy-limited kernel.  Measured [MI355X] on the uniform cloud of bench.py, same box, the two modes alternating, medians
// of 6 blocks of 10 whole calls, pre-pass included (profiles/self_order_ab.txt): 327 680 vortices +1.2 % (unordered arm's own
// block-to-block spread 0.8 %), 524 288 +2.2 % (0.1 %), 1e6 +3.0 % (0.5 %); the pre-pass itself 0.14 / 0.16 / 0.22 ms.  The
// threshold is the smallest of these sizes whose gain exceeds max(1.5 %, 3 x that spread).  A shed wake is coherent as
// stored and gains nothing; the resident wake and the march do not come this way.
constexpr long long kSelfOrderMin = 524288;

// What a context can override; the defaults are the library's.
struct SymKnobs {
  int sym_mode = 1;                             // 0: never symmetric; 1: from kSymMinN / kSymMinNMarch; > 1: from this size
  int self_order = 1;                           // device-pointer self launches in Morton order: 0 never, 1 from kSelfOrderMin, 2 always
  int tile_t = 0;                               // 4 or 8: that many vortices per lane at every size (0: by size)
  int tune_split = 0;                           // > 0: this many d-chunks
  int tune_rsplit = 0;                          // 1, 2, 4: waves per item; -1: mixed everywhere; -2: nowhere; -4: quad (0: by size)
  bool quad = true;
  long long quad_min_tiles = kSymQuadMinTiles;
  long long tail_items = kSymTailItems;
  long long t8_min_n = kSymT8MinN;
};

inline long long sym_min_n(const SymKnobs& k, bool march) {
  return k.sym_mode == 1 ? (march ? kSymMinNMarch : kSymMinN) : (long long)k.sym_mode;
}
// core: (float)v_core^4 > 0
inline bool sym_use(const SymKnobs& k, long long n, bool core, bool march) {
  return k.sym_mode != 0 && core && n >= sym_min_n(k, march);
}
// (asked only of launches that sym_use gave to the symmetric kernel)
inline bool sym_self_order(const SymKnobs& k, long long n) {
  return k.self_order == 2 || (k.self_order == 1 && n >= kSelfOrderMin);
}
inline int sym_tile(const SymKnobs& k, long long n, bool hilo) {
  if (hilo) return 4;                 // hi+lo positions: 256-vortex tile only
  if (k.tile_t == 4 || k.tile_t == 8) return k.tile_t;
  return n >= k.t8_min_n ? 8 : 4;
}

// The launch of n vortices in tiles of 64 T: the kernel's template arguments, what it is handed, whether the quad variant
// (plus a launch of the plain kernel restricted to the diagonal tiles) takes it.  A function of the vortex count (the
// march's bound) alone, so every owner of a sharded ring makes the same choice.
struct SymVariant {
  int T;
  bool hilo;
  int tune_rsplit;      // what the kernel re-derives its geometry with (n_dev launches)
  SymGeom g;
  bool quad;
  QuadGeom q;           // (quad only)
};
inline SymVariant sym_variant(const SymKnobs& k, long long n, int T, bool hilo) {
  SymVariant v{};
  v.T = hilo ? 4 : T;
  v.hilo = hilo;
  // (hi+lo positions keep one granularity per launch: the mixed form was measured on plain fp32 positions only)
  v.tune_rsplit = (hilo && k.tune_rsplit == 0) ? -2 : k.tune_rsplit;
  v.g = sym_geometry(n, v.T, k.tune_split, v.tune_rsplit, k.tail_items);
  const bool one_wave_items = v.g.rsplit == 1 || (v.g.rsplit == 0 && v.g.rbulk == 1);      // what the size rule gives at this size
  v.quad = v.T == 8 && !hilo && v.g.ntiles >= 16 &&
           (k.tune_rsplit == -4 || (k.quad && one_wave_items && k.tune_rsplit == 0 && v.g.ntiles >= k.quad_min_tiles));
  if (v.quad) v.q = quad_geometry<long long>(n, 8, k.tune_split);
  return v;
}
// the kernel's name as rocprofv3 prints it
inline void sym_kernel_name(const SymVariant& v, char* out, size_t len) {
  if (v.quad) std::snprintf(out, len, "pair_sym_quad_f32<8>");
  else std::snprintf(out, len, "pair_sym_f32<%d, %s, %d, %s>", v.T, v.hilo ? "true" : "false", v.g.rsplit,
                     v.g.rsplit != 1 ? "true" : "false");
}

// Workgroups that cover a launch whose vortex count is read on the device and lies in [n_lo, n] (the march): the most that
// any tile count in that range needs -- of the quad kernel, or of the plain one under the waves-per-item rule v.g.rsplit,
// which picked the instantiation.
inline long long sym_grid_bound(const SymKnobs& k, const SymVariant& v, bool quad_kernel, long long n_lo, long long n, int xcd_run) {
  const long long W = 64LL * v.T;
  long long most = 0;
  for (long long nt = ((n_lo > 1 ? n_lo : 1) + W - 1) / W; nt <= (n + W - 1) / W; ++nt) {
    const SymGeom q = sym_geometry(nt * W, v.T, k.tune_split, v.g.rsplit == 0 ? -1 : v.g.rsplit, k.tail_items);
    const long long b = quad_kernel ? quad_blocks(nt, quad_geometry<long long>(nt * W, v.T, k.tune_split).ysplit, xcd_run)
                                    : sym_blocks(q.ntiles, q.ysplit, v.g.rsplit, q.ytail, q.rbulk, xcd_run);
    most = b > most ? b : most;
  }
  return most;
}

}  // namespace ludvm
