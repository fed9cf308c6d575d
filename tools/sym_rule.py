"""The library's symmetric launch rule, asked of the library's own header (no engine, no GPU needed): ludvm_amd/csrc/sym_rule.hpp
states which kernel serves a self-interaction launch of n vortices, in plain C++17.  This module compiles, once per process, a
few lines of main() around it with the host C++ compiler and returns what they print: constants() -- the rule's thresholds --,
rule(sizes, march, t8_switch) -- a Rule per size (a range is walked by the program itself).
t8_switch: the size at which the 512-vortex tile took over in an earlier round (34816 through round 5), for that round's tables."""
import collections
import functools
import os
import shutil
import subprocess
import tempfile

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ludvm_amd", "csrc", "sym_rule.hpp")
# argv: march (0 / 1), T = 8 switch (0: the library's), only the first quad size of each range (0 / 1); stdin: lo hi step ...
MAIN = r'''#include <cstdlib>
using namespace ludvm;
int main(int, char** argv) {
  SymKnobs k;
  const bool march = std::atoi(argv[1]), first_quad = std::atoi(argv[3]);
  if (std::atoll(argv[2]) > 0) k.t8_min_n = std::atoll(argv[2]);
  std::printf("%lld %lld %lld %lld %lld\n", kSymMinN, kSymMinNMarch, kSymT8MinN, kSymQuadMinTiles, kSelfOrderMin);
  for (long long lo, hi, step; std::scanf("%lld %lld %lld", &lo, &hi, &step) == 3;)
    for (long long n = lo; n <= hi; n += step) {
      const bool sym = sym_use(k, n, true, march);
      const SymVariant v = sym_variant(k, n, sym_tile(k, n, false), false);
      if (first_quad && !(sym && v.quad)) continue;
      char name[64];
      sym_kernel_name(v, name, sizeof name);
      std::printf("%lld %d %d %d %d %d %d %d %d %d %d %d %s\n", n, (int)sym, v.T, v.g.rsplit, v.g.rbulk, v.g.ytail, v.g.ysplit,
                  (int)v.quad, v.q.ysplit, v.q.nlong, v.q.per, v.q.pshort, name);
      if (first_quad) break;
    }
}
'''
# The second program, `cover`: the PARTITION the header states -- which (tile, d-chunk) work items each XCD's workgroups get, which
# ring offsets a chunk holds, which tiles an owner holds -- enumerated from the header's own functions (xcd_item, quad_chunk,
# shard_block, sym_geometry), for one launch (`dump`) or exhaustively with the loops inside the program (`items`, `ring`, `quad`,
# `owners`, `device`), which print one line per property: name, cases checked, failures, first counter-example.
# The tile-pair predicates of the two kernels are restated here ONCE (pair_valid, quad_valid); tests/test_sym_shapes_host.py
# pins them to the kernels' source lines.
COVER_MAIN = r'''#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>
using namespace ludvm;
struct Fail { long long n = 0; char first[240] = ""; };
#define FAIL(f, ...) do { if (!(f).n++) std::snprintf((f).first, sizeof((f).first), __VA_ARGS__); } while (0)
static void report(const char* name, long long checked, const Fail& f) {
  std::printf("%s %lld %lld %s\n", name, checked, f.n, f.n ? f.first : "-");
}
typedef std::vector<std::pair<unsigned, unsigned>> Items;      // (d-chunk, unit)
// XCD x's list over chunks [y0, y0 + ny), read from xcd_item; its length against xcd_items, and false from there on
static Items xcd_list(unsigned units, unsigned ys, unsigned x, unsigned y0, unsigned ny, int k, Fail& f) {
  Items out;
  const unsigned long long want = xcd_items(units, ys, x, y0, ny, k);
  unsigned y, u;
  for (unsigned long long q = 0; q <= (unsigned long long)units * ny; ++q) {
    if (!xcd_item(units, ys, x, y0, ny, (unsigned)q, y, u, k)) break;
    out.push_back({y, u});
  }
  if (out.size() != want) FAIL(f, "xcd_items %llu, xcd_item lists %zu (units %u ys %u xcd %u y0 %u ny %u run %d)", want, out.size(), units, ys, x, y0, ny, k);
  for (unsigned extra : {0u, 1u, 7u, 4096u})
    if (xcd_item(units, ys, x, y0, ny, (unsigned)want + extra, y, u, k))
      FAIL(f, "xcd_item true at %llu + %u (units %u ys %u xcd %u y0 %u ny %u run %d)", want, extra, units, ys, x, y0, ny, k);
  return out;
}
// over the 8 XCDs: exactly units x [y0, y0 + ny), each once
static void check_cover(unsigned units, unsigned ys, unsigned y0, unsigned ny, int k, Fail& f) {
  std::vector<unsigned char> seen((size_t)units * ny, 0);
  for (unsigned x = 0; x < (unsigned)kXcds; ++x)
    for (const auto& it : xcd_list(units, ys, x, y0, ny, k, f)) {
      if (it.first < y0 || it.first >= y0 + ny || it.second >= units) { FAIL(f, "item (%u, %u) outside units %u chunks [%u, %u) run %d", it.first, it.second, units, y0, y0 + ny, k); continue; }
      if (seen[(size_t)(it.first - y0) * units + it.second]++) FAIL(f, "item (%u, %u) twice (units %u ys %u y0 %u ny %u run %d)", it.first, it.second, units, ys, y0, ny, k);
    }
  for (size_t i = 0; i < seen.size(); ++i)
    if (!seen[i]) { FAIL(f, "item (%u, %u) missing (units %u ys %u y0 %u ny %u run %d)", y0 + (unsigned)(i / units), (unsigned)(i % units), units, ys, y0, ny, k); break; }
}
// workgroups XCD x needs under pair_sym_f32's packing: 4 / R items per workgroup; mixed: 4 / rbulk bulk items per workgroup, the
// tail's one each, counted from the end of the bulk's workgroups as the kernel counts them
static long long wg_needed(unsigned i_count, const SymGeom& g, unsigned x, int k, Fail& f) {
  // (item counts from xcd_items: `items` shows that they are the lengths of xcd_item's lists)
  if (g.rsplit == 0) {
    const unsigned y1 = (unsigned)(g.ysplit - g.ytail);
    const long long nb = (long long)xcd_items(i_count, (unsigned)g.ysplit, x, 0, y1, k);
    const long long nt = (long long)xcd_items(i_count, (unsigned)g.ysplit, x, y1, (unsigned)g.ytail, k);
    const long long ipb = 4 / g.rbulk, nb1 = (nb * g.rbulk + 3) / 4;      // nb1: as the kernel counts the bulk's workgroups
    if (nb1 * ipb < nb) FAIL(f, "bulk workgroups %lld x %lld items < %lld", nb1, ipb, nb);
    return nb1 + nt;
  }
  const long long ipb = 4 / g.rsplit;
  return ((long long)xcd_items(i_count, (unsigned)g.ysplit, x, 0, (unsigned)g.ysplit, k) + ipb - 1) / ipb;
}
// pair_sym_f32: does the item (I, chunk y) of a launch meet a partner tile in round dd, and which (round_of)
static bool pair_valid(const SymGeom& g, unsigned I, int y, int dd, unsigned& J) {
  const bool even = (g.ntiles % 2 == 0) && g.ntiles > 1;
  const int dtot = (int)g.dtot, per = (int)((g.dtot + g.ysplit - 1) / g.ysplit), ntiles = (int)g.ntiles;
  const int d_lo = 1 + y * per;
  int d_hi = d_lo + per;
  if (d_hi > dtot + 1) d_hi = dtot + 1;
  const int d = d_lo + dd;
  J = I + (unsigned)d;
  if (J >= (unsigned)ntiles) J -= (unsigned)ntiles;
  return dd < per && d < d_hi && !(even && d == dtot && (int)I >= ntiles / 2);
}
// pair_sym_quad_f32: does wave w of the quad at I0 meet the partner tile at offset D (valid_of), for an owner of [i_first, i_first + i_count)
static bool quad_valid(const QuadGeom& g, unsigned I0, int w, int D, unsigned i_first, unsigned i_count) {
  const bool even = (g.ntiles % 2 == 0) && g.ntiles > 1;
  const int dtot = (int)g.dtot, dmax = (int)g.dmax;
  const unsigned ntiles = g.ntiles;
  const int d = D - w;
  const unsigned Iw = I0 + (unsigned)w;
  const bool own = Iw < i_first + i_count && Iw < ntiles;
  return own && ((d >= 1 && d <= (int)dmax) || (even && d == dtot && Iw < ntiles / 2));
}
// every unordered pair of distinct tiles exactly once?  cnt: ntiles x ntiles, [min][max]
static void check_pairs(const std::vector<unsigned char>& cnt, unsigned nt, const char* what, long long a, long long b, Fail& f) {
  for (unsigned i = 0; i < nt; ++i)
    for (unsigned j = i + 1; j < nt; ++j)
      if (cnt[(size_t)i * nt + j] != 1) { FAIL(f, "%s: tile pair (%u, %u) met %d times (tiles %u, %lld, %lld)", what, i, j, (int)cnt[(size_t)i * nt + j], nt, a, b); return; }
}
static void mark(std::vector<unsigned char>& cnt, unsigned nt, unsigned I, unsigned J) {
  const unsigned lo = I < J ? I : J, hi = I < J ? J : I;
  if (cnt[(size_t)lo * nt + hi] < 250) ++cnt[(size_t)lo * nt + hi];
}
static const int kRsplits[] = {0, -1, -2, 1, 2, 4};
static const int kSplits[] = {0, 1, 2, 3, 5, 64, 1024};
static const int kQuadSplits[] = {0, 1, 2, 3, 5, 128, 1024};
static const int kRuns[] = {0, 1, 3, 8};

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  auto arg = [&](int i, long long dflt) { return argc > i ? std::atoll(argv[i]) : dflt; };
  if (cmd == "consts") {
    std::printf("%lld %lld %lld %lld %lld %u %u %lld\n", kSymMinItems, kSymTailItems, kSymMaxSplit, kSymMaxSplitTuned, kXcds, kQuad, kQuadSplit, kSymMaxRsplit);
  } else if (cmd == "dump") {      // n T tune_split tune_rsplit tail_items xcd_run i_first i_count (< 0: the ring) quad
    const long long n = arg(2, 0);
    const int T = (int)arg(3, 8), ts = (int)arg(4, 0), tr = (int)arg(5, 0), k = (int)arg(7, 0);
    const long long tail = arg(6, kSymTailItems);
    const bool quad = arg(10, 0) != 0;
    Fail f;
    const SymGeom g = sym_geometry(n, T, ts, tr, tail);
    const unsigned i_first = (unsigned)arg(8, 0), i_count = arg(9, -1) < 0 ? (unsigned)g.ntiles : (unsigned)arg(9, -1);
    if (quad) {
      const QuadGeom q = quad_geometry<long long>(n, T, ts);
      const unsigned quads = (i_count + kQuad - 1) / kQuad;
      std::printf("quadgeom %u %u %u %u %d %d %d %d %lld\n", q.ntiles, q.dmax, q.dtot, q.Dtot, q.ysplit, q.per, q.nlong, q.pshort, quad_blocks(i_count, q.ysplit, k) / kXcds);
      for (int yq = 0; yq < q.ysplit; ++yq) { int lo, hi; quad_chunk(q, (unsigned)yq, lo, hi); std::printf("chunk %d %d %d\n", yq, lo, hi); }
      for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
        std::printf("xcd %u all", x);
        for (const auto& it : xcd_list(quads, (unsigned)q.ysplit, x, 0, (unsigned)q.ysplit, k, f)) std::printf(" %u:%u", it.first, i_first + kQuad * it.second);
        std::printf("\n");
      }
    } else {
      const int per = g.dtot > 0 ? (int)((g.dtot + g.ysplit - 1) / g.ysplit) : 0;
      std::printf("geom %lld %lld %lld %d %d %d %d %d %lld\n", g.ntiles, g.dmax, g.dtot, g.ysplit, g.rsplit, g.ytail, g.rbulk, per,
                  sym_blocks_xcd(i_count, g.ysplit, g.rsplit, g.ytail, g.rbulk, k));
      for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
        const unsigned y1 = g.rsplit == 0 ? (unsigned)(g.ysplit - g.ytail) : (unsigned)g.ysplit;
        std::printf("xcd %u %s", x, g.rsplit == 0 ? "bulk" : "all");
        for (const auto& it : xcd_list(i_count, (unsigned)g.ysplit, x, 0, y1, k, f)) std::printf(" %u:%u", it.first, i_first + it.second);
        std::printf("\n");
        if (g.rsplit == 0) {
          std::printf("xcd %u tail", x);
          for (const auto& it : xcd_list(i_count, (unsigned)g.ysplit, x, y1, (unsigned)g.ytail, k, f)) std::printf(" %u:%u", it.first, i_first + it.second);
          std::printf("\n");
        }
      }
    }
    report("lists", 1, f);
  } else if (cmd == "shard") {     // ntiles world
    for (int r = 0; r < (int)arg(3, 1); ++r) {
      unsigned long long f, c;
      shard_block((unsigned long long)arg(2, 0), r, (int)arg(3, 1), &f, &c);
      std::printf("%llu %llu\n", f, c);
    }
  } else if (cmd == "find") {      // smallest ring (tiles) at which code -1 gives rbulk = argv[2], with tune_split argv[3]
    const int want = (int)arg(2, 1), ts = (int)arg(3, 0);
    for (long long nt = 1; nt <= 4096; ++nt)
      if (sym_geometry(nt * 256, 4, ts, -1, kSymTailItems).rbulk == want) { std::printf("%lld\n", nt); return 0; }
    std::printf("0\n");
  } else if (cmd == "items") {     // ntmax; the tile counts are dealt to up to 16 threads
    const long long ntmax = arg(2, 700);
    struct Part { Fail cover, chunks, ranges, blocks, tiles; long long ncover = 0, ngeom = 0; };
    const unsigned nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Part> parts(nthreads);
    auto work = [&](unsigned tid) {
      Part& p = parts[tid];
      for (long long nt = 1 + tid; nt <= ntmax; nt += nthreads) {
        std::set<std::tuple<unsigned, unsigned, unsigned, unsigned>> done;       // (chunks, first, count, chunks per run) of this tile count
        for (int tr : kRsplits) for (int ts : kSplits) for (long long tail : {kSymTailItems, (long long)17}) {
          if (tail != kSymTailItems && ts >= 64) continue;      // (a second cut between bulk and tail: at the small splits)
          const SymGeom g = sym_geometry(nt * 512, 8, ts, tr, tail);
          // (the partition is a function of the tile count: both tiles, a full and a one-member last tile give the same geometry)
          for (long long n : {nt * 256, nt * 256 - 255, nt * 512 - 511}) {
            const SymGeom h = sym_geometry(n, n == nt * 512 - 511 ? 8 : 4, ts, tr, tail);
            if (std::memcmp(&g, &h, sizeof g) != 0) FAIL(p.tiles, "geometry of %lld tiles differs between the tiles (split %d code %d)", nt, ts, tr);
          }
          ++p.ngeom;
          if (g.ntiles != nt) FAIL(p.chunks, "ntiles %lld for %lld", g.ntiles, nt);
          const long long per = g.dtot > 0 ? (g.dtot + g.ysplit - 1) / g.ysplit : 0;
          if (g.dtot > 0 ? !((g.ysplit - 1) * per < g.dtot && g.dtot <= g.ysplit * per) : g.ysplit != 1)
            FAIL(p.chunks, "tiles %lld split %d code %d: dtot %lld ysplit %d per %lld", nt, ts, tr, g.dtot, g.ysplit, per);
          if (g.ytail < 0 || g.ytail > g.ysplit || !(g.rbulk == 1 || g.rbulk == 2 || g.rbulk == 4) ||
              !(g.rsplit == 0 || g.rsplit == 1 || g.rsplit == 2 || g.rsplit == 4) || (g.rsplit != 0 && g.ytail != 0) ||
              ((tr == 1 || tr == 2 || tr == 4) && g.rsplit != tr) || (tr == -1 && g.rsplit != 0) || (tr == -2 && g.rsplit == 0))
            FAIL(p.ranges, "tiles %lld split %d code %d: rsplit %d ytail %d ysplit %d rbulk %d", nt, ts, tr, g.rsplit, g.ytail, g.ysplit, g.rbulk);
          for (int k : kRuns) {
            const unsigned y1 = g.rsplit == 0 ? (unsigned)(g.ysplit - g.ytail) : (unsigned)g.ysplit, K = xcd_run((unsigned)g.ysplit, k);
            if (done.insert({(unsigned)g.ysplit, 0u, y1, K}).second) { check_cover((unsigned)nt, (unsigned)g.ysplit, 0, y1, k, p.cover); ++p.ncover; }
            if (g.rsplit == 0 && done.insert({(unsigned)g.ysplit, y1, (unsigned)g.ytail, K}).second) {
              check_cover((unsigned)nt, (unsigned)g.ysplit, y1, (unsigned)g.ytail, k, p.cover); ++p.ncover;
            }
            const long long have = sym_blocks_xcd(nt, g.ysplit, g.rsplit, g.ytail, g.rbulk, k);
            for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
              const long long need = wg_needed((unsigned)nt, g, x, k, p.blocks);
              if (have < need) FAIL(p.blocks, "tiles %lld split %d code %d run %d: sym_blocks_xcd %lld < %lld of XCD %u", nt, ts, tr, k, have, need, x);
            }
          }
        }
      }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; ++t) pool.emplace_back(work, t);
    for (auto& t : pool) t.join();
    Part all;
    auto add = [](Fail& to, const Fail& from) { if (!to.n && from.n) std::memcpy(to.first, from.first, sizeof to.first); to.n += from.n; };
    for (const Part& p : parts) {
      add(all.cover, p.cover); add(all.chunks, p.chunks); add(all.ranges, p.ranges); add(all.blocks, p.blocks); add(all.tiles, p.tiles);
      all.ncover += p.ncover; all.ngeom += p.ngeom;
    }
    report("cover", all.ncover, all.cover); report("chunks", all.ngeom, all.chunks); report("ranges", all.ngeom, all.ranges);
    report("blocks", all.ngeom * 4, all.blocks); report("tiles", all.ngeom, all.tiles);
  } else if (cmd == "ring") {      // ntmax
    const long long ntmax = arg(2, 700);
    Fail plain, chunked;
    long long nchunked = 0;
    for (long long nt = 1; nt <= ntmax; ++nt) {
      // the set itself: I + d for d = 1 .. dmax, and d = NT / 2 for I < NT / 2 on an even ring
      const long long dmax = (nt - 1) / 2;
      std::vector<unsigned char> cnt((size_t)nt * nt, 0);
      for (long long I = 0; I < nt; ++I) {
        for (long long d = 1; d <= dmax; ++d) mark(cnt, (unsigned)nt, (unsigned)I, (unsigned)((I + d) % nt));
        if (nt % 2 == 0 && nt > 1 && I < nt / 2) mark(cnt, (unsigned)nt, (unsigned)I, (unsigned)(I + nt / 2));
      }
      check_pairs(cnt, (unsigned)nt, "the set", 0, 0, plain);
      // ... and what the kernel's rounds meet, chunk by chunk
      int last_ys = -1;
      for (int ts : kSplits) {
        const SymGeom g = sym_geometry(nt * 512, 8, ts, 1, kSymTailItems);
        if (g.ysplit == last_ys) continue;
        last_ys = g.ysplit;
        if (g.dmax != dmax) FAIL(chunked, "dmax %lld of %lld tiles", g.dmax, nt);
        const int per = g.dtot > 0 ? (int)((g.dtot + g.ysplit - 1) / g.ysplit) : 0;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (unsigned I = 0; I < (unsigned)nt; ++I)
          for (int y = 0; y < g.ysplit; ++y)
            for (int dd = 0; dd < per; ++dd) { unsigned J; if (pair_valid(g, I, y, dd, J)) mark(cnt, (unsigned)nt, I, J); }
        check_pairs(cnt, (unsigned)nt, "rounds", ts, g.ysplit, chunked);
        ++nchunked;
      }
    }
    report("ring_set", ntmax, plain); report("ring_rounds", nchunked, chunked);
  } else if (cmd == "quad") {      // ntmax of the chunk check, ntmax of the pair check
    const long long ntmax = arg(2, 5000), ntpairs = arg(3, 400);
    Fail tiling, pairs, blocks, cover;
    long long ntiling = 0, npairs = 0;
    for (long long nt = 16; nt <= ntmax; ++nt)
      for (int ts : kQuadSplits) {
        const QuadGeom q = quad_geometry<long long>(nt * 512, 8, ts);
        const QuadGeom qu = quad_geometry<unsigned>((unsigned)(nt * 512 - 511), 8, ts);
        if (std::memcmp(&q, &qu, sizeof q) != 0) FAIL(tiling, "tiles %lld split %d: the device's geometry differs", nt, ts);
        int next = 1;
        for (int yq = 0; yq < q.ysplit; ++yq) {
          int lo, hi;
          quad_chunk(q, (unsigned)yq, lo, hi);
          if (lo != next || hi <= lo || hi - lo > (yq < q.nlong ? q.per : q.pshort)) { FAIL(tiling, "tiles %lld split %d chunk %d: [%d, %d) after %d", nt, ts, yq, lo, hi, next); break; }
          next = hi;
        }
        if (next != (int)q.Dtot + 1 || q.Dtot != q.dtot + 3) FAIL(tiling, "tiles %lld split %d: chunks end at %d, Dtot %u", nt, ts, next, q.Dtot);
        ++ntiling;
        const bool wanted = nt <= ntpairs || nt == 639 || nt == 640 || nt == 641 || nt == 1023 || nt == 1024 || nt == 2047;
        if (!wanted) continue;
        const unsigned quads = (unsigned)((nt + kQuad - 1) / kQuad);
        for (int k : kRuns) {
          check_cover(quads, (unsigned)q.ysplit, 0, (unsigned)q.ysplit, k, cover);
          const long long have = quad_blocks(nt, q.ysplit, k) / kXcds;
          for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
            const long long need = (long long)xcd_list(quads, (unsigned)q.ysplit, x, 0, (unsigned)q.ysplit, k, blocks).size();
            if (have < need) FAIL(blocks, "tiles %lld split %d run %d: quad_blocks / 8 = %lld < %lld of XCD %u", nt, ts, k, have, need, x);
          }
        }
        std::vector<unsigned char> cnt((size_t)nt * nt, 0);
        for (unsigned quad = 0; quad < quads; ++quad)
          for (int yq = 0; yq < q.ysplit; ++yq) {
            int lo, hi;
            quad_chunk(q, (unsigned)yq, lo, hi);
            for (int D = lo; D < hi; ++D) {
              unsigned J = kQuad * quad + (unsigned)D;
              if (J >= (unsigned)nt) J -= (unsigned)nt;
              for (int w = 0; w < (int)kQuad; ++w)
                if (quad_valid(q, kQuad * quad, w, D, 0, (unsigned)nt)) {
                  if (J >= (unsigned)nt || J == kQuad * quad + (unsigned)w) FAIL(pairs, "tiles %lld split %d: quad %u wave %d offset %d meets tile %u", nt, ts, quad, w, D, J);
                  else mark(cnt, (unsigned)nt, kQuad * quad + (unsigned)w, J);
                }
            }
          }
        check_pairs(cnt, (unsigned)nt, "quad rounds", ts, q.ysplit, pairs);
        ++npairs;
      }
    report("quad_chunks", ntiling, tiling); report("quad_pairs", npairs, pairs); report("quad_blocks", npairs * 4, blocks);
    report("quad_cover", npairs * 4, cover);
  } else if (cmd == "owners") {    // ntmax of the block check, ntmax of the item check, largest world
    const long long ntmax = arg(2, 5000), ntitems = arg(3, 120);
    const int wmax = (int)arg(4, 17);
    Fail part, items, qitems;
    long long npart = 0, nitems = 0;
    for (long long nt = 1; nt <= ntmax; ++nt)
      for (int world = 1; world <= wmax; ++world) {
        unsigned long long next = 0, f, c;
        for (int r = 0; r < world; ++r) {
          shard_block((unsigned long long)nt, r, world, &f, &c);
          if (f != next || f % 4 != 0 || ((f + c) % 4 != 0 && f + c != (unsigned long long)nt)) FAIL(part, "tiles %lld world %d rank %d: block [%llu, %llu) after %llu", nt, world, r, f, f + c, next);
          next = f + c;
        }
        if (next != (unsigned long long)nt) FAIL(part, "tiles %lld world %d: the blocks end at %llu", nt, world, next);
        ++npart;
        if (nt > ntitems) continue;
        // the owners' items together are the single owner's: plain (tile, chunk), and quad (first tile of the quad, chunk) with
        // the waves that hold a tile of the owner's
        for (int ts : {0, 2, 3}) {
          const SymGeom g = sym_geometry(nt * 512, 8, ts, 1, kSymTailItems);
          std::vector<unsigned char> seen((size_t)nt * g.ysplit, 0);
          for (int r = 0; r < world; ++r) {
            shard_block((unsigned long long)nt, r, world, &f, &c);
            for (unsigned x = 0; x < (unsigned)kXcds; ++x)
              for (const auto& it : xcd_list((unsigned)c, (unsigned)g.ysplit, x, 0, (unsigned)g.ysplit, 0, items))
                if (it.first >= (unsigned)g.ysplit || f + it.second >= (unsigned long long)nt) FAIL(items, "tiles %lld world %d rank %d: item (%u, %llu) outside the ring", nt, world, r, it.first, f + it.second);
                else ++seen[(size_t)it.first * nt + f + it.second];
          }
          for (size_t i = 0; i < seen.size(); ++i)
            if (seen[i] != 1) { FAIL(items, "tiles %lld world %d split %d: item (%llu, %llu) held %d times", nt, world, ts, (unsigned long long)(i / nt), (unsigned long long)(i % nt), (int)seen[i]); break; }
          ++nitems;
          if (nt < 16) continue;
          const QuadGeom q = quad_geometry<long long>(nt * 512, 8, ts);
          std::vector<unsigned char> wseen((size_t)nt * q.ysplit, 0);      // (tile of a wave, chunk)
          for (int r = 0; r < world; ++r) {
            shard_block((unsigned long long)nt, r, world, &f, &c);
            const unsigned quads = (unsigned)((c + kQuad - 1) / kQuad);
            for (unsigned x = 0; x < (unsigned)kXcds; ++x)
              for (const auto& it : xcd_list(quads, (unsigned)q.ysplit, x, 0, (unsigned)q.ysplit, 0, qitems))
                for (unsigned w = 0; w < kQuad; ++w) {
                  const unsigned I = (unsigned)f + kQuad * it.second + w;
                  if (it.first >= (unsigned)q.ysplit) FAIL(qitems, "tiles %lld world %d rank %d: chunk %u of %d", nt, world, r, it.first, q.ysplit);
                  else if (I < f + c && I < (unsigned)nt) ++wseen[(size_t)it.first * nt + I];
                }
          }
          for (size_t i = 0; i < wseen.size(); ++i)
            if (wseen[i] != 1) { FAIL(qitems, "tiles %lld world %d split %d: wave (%llu, %llu) held %d times", nt, world, ts, (unsigned long long)(i / nt), (unsigned long long)(i % nt), (int)wseen[i]); break; }
        }
      }
    report("owner_blocks", npart, part); report("owner_items", nitems, items); report("owner_quad_items", nitems, qitems);
  } else if (cmd == "device") {    // stdin: n ...; every tile, every code and split, every run: the grid covers what the device derives
    Fail bound, rule, width;
    long long nb = 0;
    for (long long n; std::scanf("%lld", &n) == 1;)
      for (int hilo = 0; hilo < 2; ++hilo) for (int T : {4, 8}) for (int tr : {0, -1, -2, 1, 2, 4, -4}) for (int ts : {0, 1, 2, 3, 64}) for (int xr : kRuns) {
        if (hilo && T == 8) continue;
        SymKnobs k;
        k.tune_split = ts; k.tune_rsplit = tr;
        if (n < 16 * 512) k.quad_min_tiles = 16;
        const SymVariant v = sym_variant(k, n, T, hilo != 0);
        const long long n_lo = n > 256 ? n - 256 : 1;
        const long long have = sym_grid_bound(k, v, false, n_lo, n, xr), qhave = v.quad ? sym_grid_bound(k, v, true, n_lo, n, xr) : 0;
        for (long long nd = n_lo; nd <= n; ++nd) {
          // what pair_sym_f32 re-derives from the count it reads: the code of its instantiation
          unsigned ntiles, dmax, dtot; int ys, rs, yt, rb;
          const int R = v.g.rsplit;
          sym_geometry_t<unsigned>((unsigned)nd, v.T, ts, R == 0 ? -1 : R, (unsigned)k.tail_items, ntiles, dmax, dtot, ys, rs, yt, rb);
          const SymGeom h = sym_geometry(nd, v.T, ts, R == 0 ? -1 : R, k.tail_items);
          if (h.ntiles != ntiles || h.dmax != dmax || h.dtot != dtot || h.ysplit != ys || h.rsplit != rs || h.ytail != yt || h.rbulk != rb)
            FAIL(width, "n %lld (%lld on the device) T %d code %d split %d: 32- and 64-bit geometry differ", n, nd, v.T, tr, ts);
          if (rs != R) FAIL(rule, "n %lld (%lld on the device) T %d code %d split %d: host instantiates %d waves per item, the device derives %d", n, nd, v.T, tr, ts, R, rs);
          const SymGeom dg{(long long)ntiles, (long long)dmax, (long long)dtot, ys, rs, yt, rb};
          ++nb;
          if (nd != n_lo && nd != n && (nd - 1) % (64 * v.T) != 0 && nd % (64 * v.T) != 0) continue;      // (a function of the tile count)
          if (!v.quad)
            for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
              const long long need = wg_needed(ntiles, dg, x, xr, bound);
              if (have < kXcds * need) FAIL(bound, "n %lld (%lld on the device) T %d code %d split %d run %d: sym_grid_bound %lld < 8 x %lld", n, nd, v.T, tr, ts, xr, have, need);
            }
          else {
            const QuadGeom q = quad_geometry<unsigned>((unsigned)nd, 8, ts);
            const unsigned quads = (q.ntiles + kQuad - 1) / kQuad;
            for (unsigned x = 0; x < (unsigned)kXcds; ++x) {
              const long long need = (long long)xcd_items(quads, (unsigned)q.ysplit, x, 0, (unsigned)q.ysplit, xr);
              if (qhave < kXcds * need) FAIL(bound, "n %lld (%lld on the device) quad split %d run %d: sym_grid_bound %lld < 8 x %lld", n, nd, ts, xr, qhave, need);
            }
          }
        }
      }
    report("device_bound", nb, bound); report("device_rule", nb, rule); report("device_width", nb, width);
  } else {
    std::fprintf(stderr, "cover: unknown command\n");
    return 2;
  }
  return 0;
}
'''
# symmetric = 0: the direct kernel takes the launch (kernel None); the other fields say what a symmetric launch would be.
# quad_*: the quad variant's d-chunks per quad, how many of them are long, rounds per long and per short chunk (0 without quad)
Rule = collections.namedtuple("Rule", "n symmetric T rsplit rbulk ytail ysplit quad quad_chunks quad_long quad_per quad_pershort kernel")


@functools.lru_cache(maxsize=None)
def _program(name="dump", tmp=tempfile.TemporaryDirectory(prefix="sym_rule_")):       # (removed when the process ends)
    """A program built from HEADER -- the file the library's units include -- with the compiler oracle/Makefile uses: `dump`
    (MAIN) or `cover` (COVER_MAIN)."""
    cxx = next(c for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "hipcc", "/opt/rocm/bin/hipcc") if c and shutil.which(c))
    with open(os.path.join(tmp.name, name + ".cpp"), "w") as f:
        f.write(f'#include "{HEADER}"\n' + {"dump": MAIN, "cover": COVER_MAIN}[name])
    subprocess.run([cxx, {"dump": "-O1", "cover": "-O2"}[name], "-std=c++17", "-pthread", "-x", "c++", "-o", os.path.join(tmp.name, name), f.name],
                   check=True, timeout=300)
    return os.path.join(tmp.name, name)


def _ask(ranges, *flags):
    return subprocess.run([_program(), *(str(int(f or 0)) for f in flags)], capture_output=True, text=True, check=True, timeout=300,
                          input="".join("%d %d %d\n" % r for r in ranges)).stdout.splitlines()


def constants():
    return dict(zip(("kSymMinN", "kSymMinNMarch", "kSymT8MinN", "kSymQuadMinTiles", "kSelfOrderMin"), map(int, _ask([], 0, 0, 0)[0].split())))


def rule(sizes, march=False, t8_switch=None, first_quad=False):
    """first_quad: of a range, only the first size that takes the quad variant"""
    ranges = [(sizes.start, sizes.stop - 1, sizes.step)] if isinstance(sizes, range) else [(n, n, 1) for n in sizes]
    rows = [Rule(*map(int, l.split()[:12]), l.split(None, 12)[12]) for l in _ask(ranges, march, t8_switch, first_quad)[1:]]
    return [r if r.symmetric else r._replace(kernel=None) for r in rows]


# ---- the partition (the `cover` program) ------------------------------------------------------------------------------------------
# Cover: one launch.  per: ring offsets per d-chunk (rounds of an item); blocks_xcd: workgroups per XCD the launch rule sizes
# (sym_blocks_xcd, or quad_blocks / 8); xcds[x]: {'all' | 'bulk' | 'tail': [(d-chunk, tile)]} in the order of the XCD's workgroups --
# for the quad variant the tile is the quad's first; chunks: the quad's [(lo, hi)] ring offsets per d-chunk (None otherwise).
Cover = collections.namedtuple("Cover", "ntiles dmax dtot ysplit rsplit ytail rbulk per blocks_xcd xcds chunks Dtot")
Check = collections.namedtuple("Check", "checked failures first")


def _cover(args, stdin=""):
    return subprocess.run([_program("cover"), *map(str, args)], capture_output=True, text=True, check=True, timeout=600,
                          input=stdin).stdout.splitlines()


def cover_constants():
    return dict(zip(("kSymMinItems", "kSymTailItems", "kSymMaxSplit", "kSymMaxSplitTuned", "kXcds", "kQuad", "kQuadSplit", "kSymMaxRsplit"),
                    map(int, _cover(["consts"])[0].split())))


@functools.lru_cache(maxsize=None)
def cover(n, T, tune_split=0, tune_rsplit=0, tail_items=None, xcd_run=0, i_first=0, i_count=-1, quad=False):
    """The geometry and every XCD's item list of one launch, the lists read from xcd_item."""
    tail = cover_constants()["kSymTailItems"] if tail_items is None else tail_items
    lines = _cover(["dump", n, T, tune_split, tune_rsplit, tail, xcd_run, i_first, i_count, int(quad)])
    head = lines[0].split()
    xcds, chunks = [dict() for _ in range(8)], None
    for l in lines[1:]:
        w = l.split()
        if w[0] == "xcd":
            xcds[int(w[1])][w[2]] = [tuple(map(int, it.split(":"))) for it in w[3:]]
        elif w[0] == "chunk":
            chunks = (chunks or []) + [(int(w[2]), int(w[3]))]
        elif w[0] == "lists":
            assert int(w[2]) == 0, l
    if quad:
        ntiles, dmax, dtot, Dtot, ysplit, per, nlong, pshort, blocks = map(int, head[1:])
        return Cover(ntiles, dmax, dtot, ysplit, 1, 0, 1, (per, nlong, pshort), blocks, xcds, chunks, Dtot)
    ntiles, dmax, dtot, ysplit, rsplit, ytail, rbulk, per, blocks = map(int, head[1:])
    return Cover(ntiles, dmax, dtot, ysplit, rsplit, ytail, rbulk, per, blocks, xcds, None, None)


def cover_check(command, *args, stdin=""):
    """One of the program's exhaustive checks ('items', 'ring', 'quad', 'owners', 'device'): {property: Check}."""
    out = {}
    for l in _cover([command, *args], stdin):
        name, checked, failures, first = l.split(None, 3)
        out[name] = Check(int(checked), int(failures), first)
    return out


def smallest_mixed_ring(rbulk, tune_split=0):
    """The smallest tile count at which code -1 (mixed granularity at every size) works its bulk by `rbulk` waves per item."""
    return int(_cover(["find", rbulk, tune_split])[0])


def shard_blocks(ntiles, world):
    """[(first tile, tiles)] of the owners 0 .. world - 1 of a ring, from shard_block."""
    return [tuple(map(int, l.split())) for l in _cover(["shard", ntiles, world])]
