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
# symmetric = 0: the direct kernel takes the launch (kernel None); the other fields say what a symmetric launch would be.
# quad_*: the quad variant's d-chunks per quad, how many of them are long, rounds per long and per short chunk (0 without quad)
Rule = collections.namedtuple("Rule", "n symmetric T rsplit rbulk ytail ysplit quad quad_chunks quad_long quad_per quad_pershort kernel")


@functools.lru_cache(maxsize=None)
def _program(tmp=tempfile.TemporaryDirectory(prefix="sym_rule_")):       # (removed when the process ends)
    """The dump program, built from HEADER -- the file the library's units include -- with the compiler oracle/Makefile uses."""
    cxx = next(c for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "hipcc", "/opt/rocm/bin/hipcc") if c and shutil.which(c))
    with open(os.path.join(tmp.name, "dump.cpp"), "w") as f:
        f.write(f'#include "{HEADER}"\n' + MAIN)
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "c++", "-o", os.path.join(tmp.name, "dump"), f.name], check=True, timeout=300)
    return os.path.join(tmp.name, "dump")


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
