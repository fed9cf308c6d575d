"""The library's direct launch plan, asked of the library's own header (no engine, no GPU needed): ludvm_amd/csrc/plan_rule.hpp
states how a launch of the direct pair kernels divides its sources and targets and which instantiation serves it, in plain
C++17.  This module compiles, once per process, a few lines of main() around it with the host C++ compiler and returns what
they print: constants() -- the plan's constants and default knobs --, plan(cases) -- a Plan per case --, origin_index(b, p, n)
-- which vortex lends origin class (block b, index parity p) of n stored vortices its origin --, observer_plan(kind, count, ns_ub)
-- the launch of a marched observer's kernels (probes, tracers, survey) over `count` points with at most ns_ub sources,
field_hilo_plan(plan_nt, ns) -- the source splits of the hi+lo fp32 field sums (analytic vorticity, velocity gradient).
A case is a dict: precision ('f32' | 'f32x2' | 'f64'), ns, nt, and optionally local (positions on local origins: what
LUDVM_PREC_F32 is wherever the library lays the positions out itself), grid_nz (> 0: a flow-field grid of that many points per
row, nt = its points), slab (the results stay in the partial slabs for a fused finisher), plan_nt (the whole grid's points
when the launch is a block of its rows), nt_on_device (the TARGET count is completed on the device: the march's roll-up, whose
targets are the wake; a source count that lives there -- the march's chord sums -- is planned from the host's bound on it: give
that bound as ns), and the knobs small_tile_max, small_tile_max_f64, tune_tpl, tune_split, grid_kernel
(1 row | 2 patch by size | 3 patch2 | 4 patch4), few_packed (None / absent = the product's)."""
import collections
import functools
import os
import shutil
import subprocess
import tempfile

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ludvm_amd", "csrc", "plan_rule.hpp")
CONSTANTS = ("kPlanBlock", "kTileF32", "kTileF32Small", "kTileF64", "kTileF64Few", "kFewTargets", "kTargetBlocks", "kMaxSplit",
             "kPatch4MinTargets", "kFewGroupsMax", "kSmallTileMaxDefault", "kSmallTileMaxF64Default", "kTpl2MinTargets",
             "kSmallTileMaxTargets")
KNOBS = ("small_tile_max", "small_tile_max_f64", "tune_tpl", "tune_split", "grid_kernel", "few_packed")
PRECISIONS = {"f32": 0, "f32x2": 1, "f64": 2}
# stdin: precision ns nt local grid_nz slab plan_nt nt_on_device, then the six knobs (-1 = the product's); with an argument:
# stdin: b p n per line -> origin_index; with the argument 'observer': stdin: kind count ns_ub per line -> ObserverPlan
OBSERVER_KINDS = ("probes", "tracers", "tracers_f32x2", "survey", "survey_f32")       # (= ObserverKind)
MAIN = r'''
using namespace ludvm;
int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "observer") == 0) {
    for (long long kind, count, ns; std::scanf("%lld %lld %lld", &kind, &count, &ns) == 3;) {
      const ObserverRule& r = kObserverRules[kind];
      const ObserverPlan p = observer_plan(r, count, ns);
      std::printf("%lld %lld %lld %d %lld %zu %lld %lld\n", p.tiles, p.pad, p.chunk, p.nsplit, observer_want(r, count),
                  observer_slab_bytes(r, count), r.point_tile, r.src_tile);
    }
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "field_hilo") == 0) {
    for (long long nt, ns; std::scanf("%lld %lld", &nt, &ns) == 2;) {
      const FieldHiloPlan p = field_hilo_plan(nt, ns);
      std::printf("%lld %d %lld %d %d\n", p.chunk, p.nsplit, kFieldHiloTargets, kFieldHiloTile, kFieldHiloPerLane);
    }
    return 0;
  }
  if (argc > 1) {
    for (long long b, p, n; std::scanf("%lld %lld %lld", &b, &p, &n) == 3;) std::printf("%lld\n", origin_index(b, (int)p, n));
    return 0;
  }
  std::printf("''' + " ".join(["%lld"] * len(CONSTANTS)) + r'''\n", ''' + ", ".join(f"(long long){c}" for c in CONSTANTS) + r''');
  long long prec, ns, nt, local, grid_nz, slab, plan_nt, nt_dev, kn[6];
  while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &prec, &ns, &nt, &local, &grid_nz, &slab, &plan_nt,
                    &nt_dev, &kn[0], &kn[1], &kn[2], &kn[3], &kn[4], &kn[5]) == 14) {
    PlanKnobs k;
    if (kn[0] >= 0) k.small_tile_max = kn[0];
    if (kn[1] >= 0) k.small_tile_max_f64 = kn[1];
    if (kn[2] >= 0) k.tune_tpl = (int)kn[2];
    if (kn[3] >= 0) k.tune_split = (int)kn[3];
    if (kn[4] >= 0) k.grid_kernel = (int)kn[4];
    if (kn[5] >= 0) k.few_packed = kn[5] != 0;
    // (as induce_device hands a launch to the plan)
    const bool generic = grid_is_generic(k, grid_nz);
    const bool patch = grid_nz > 0 && !generic && prec == kPlanF32;
    const DirectPlan p = direct_plan(k, nt, ns, (int)prec, !generic, plan_nt, patch);
    // (launch_pair gives a launch a slab when it has more than one split or its caller reads the results there)
    const bool part = slab != 0 || p.nsplit > 1;
    const DirectVariant v = direct_variant(k, p, (int)prec, local != 0, nt, grid_nz, part, nt_dev != 0);
    char name[96];
    direct_kernel_name(v, name, sizeof name);
    std::printf("%d %d %d %d %d %d %d %lld %lld %d %lld %lld %d %s\n", v.kernel, v.tpl, v.tile, (int)v.hilo, v.grid, (int)v.local, v.groups,
                v.blocks_x, v.blocks_y, p.nsplit, p.chunk, p.nt_pad, p.tpl, name);
  }
}
'''
# family: 'f32' | 'f64' | 'f64_few'; tpl / tile / hilo / grid / local: the instantiation's template arguments; groups: source
# splits a pair_f64_few workgroup works at once; blocks_x x blocks_y workgroups; nsplit slab rows of chunk sources each (the
# last one may hold fewer), nt_pad elements per slab row and component; plan_tpl: targets per lane the plan counted with
Plan = collections.namedtuple("Plan", "family tpl tile hilo grid local groups blocks_x blocks_y nsplit chunk nt_pad plan_tpl kernel")
FAMILIES = ("f32", "f64", "f64_few")


@functools.lru_cache(maxsize=None)
def _program(tmp=tempfile.TemporaryDirectory(prefix="plan_rule_")):       # (removed when the process ends)
    """The dump program, built from HEADER -- the file the library's units include -- with the compiler oracle/Makefile uses."""
    cxx = next(c for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "hipcc", "/opt/rocm/bin/hipcc") if c and shutil.which(c))
    with open(os.path.join(tmp.name, "dump.cpp"), "w") as f:
        f.write(f'#include "{HEADER}"\n#include <cstring>\n' + MAIN)
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "c++", "-o", os.path.join(tmp.name, "dump"), f.name], check=True, timeout=300)
    return os.path.join(tmp.name, "dump")


def _ask(lines, *args):
    return subprocess.run([_program(), *args], capture_output=True, text=True, check=True, timeout=300, input="".join(lines)).stdout.splitlines()


def constants():
    return dict(zip(CONSTANTS, map(int, _ask([])[0].split())))


def plan(cases):
    lines = []
    for c in cases:
        unknown = set(c) - {"precision", "ns", "nt", "local", "grid_nz", "slab", "plan_nt", "nt_on_device", *KNOBS}
        if unknown:
            raise ValueError(f"plan_rule.plan: unknown fields {sorted(unknown)}")
        knobs = [-1 if c.get(k) is None else int(c[k]) for k in KNOBS]
        lines.append("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
            PRECISIONS[c["precision"]], c["ns"], c["nt"], bool(c.get("local")), c.get("grid_nz") or 0, bool(c.get("slab")),
            c.get("plan_nt") or 0, bool(c.get("nt_on_device")), *knobs))
    rows = []
    for l in _ask(lines)[1:]:
        f = l.split(None, 13)
        rows.append(Plan(FAMILIES[int(f[0])], int(f[1]), int(f[2]), bool(int(f[3])), int(f[4]), bool(int(f[5])), *map(int, f[6:13]), f[13]))
    assert len(rows) == len(lines)
    return rows


def origin_index(queries):
    """[index] for (b, p, n) triples: pair_kernels' origin classes, from the header the kernels include"""
    out = _ask(["%d %d %d\n" % q for q in queries], "origin")
    assert len(out) == len(queries)
    return [int(l) for l in out]


# tiles x nsplit workgroups; pad columns per slab row and component; nsplit splits of chunk sources (the last may hold fewer,
# or none); want: the splits any step may have; slab_bytes: what the setter allocates; point_tile, src_tile: the rule's
ObserverPlan = collections.namedtuple("ObserverPlan", "tiles pad chunk nsplit want slab_bytes point_tile src_tile")


def observer_plan(kind, count, ns_ub):
    """The launch of observer `kind` (one of OBSERVER_KINDS) with `count` >= 1 points in a step whose sources number at most
    ns_ub; arrays of counts and bounds give a list over their product (count-major)."""
    counts, bounds = ([int(v) for v in (a if hasattr(a, "__len__") else [a])] for a in (count, ns_ub))
    k = OBSERVER_KINDS.index(kind)
    out = _ask(["%d %d %d\n" % (k, c, n) for c in counts for n in bounds], "observer")
    assert len(out) == len(counts) * len(bounds)
    rows = [ObserverPlan(*map(int, l.split())) for l in out]
    return rows if hasattr(count, "__len__") or hasattr(ns_ub, "__len__") else rows[0]


# nsplit splits of chunk sources (the last may hold fewer); targets: points of one workgroup (256 lanes x per_lane); tile:
# sources staged at once
FieldHiloPlan = collections.namedtuple("FieldHiloPlan", "chunk nsplit targets tile per_lane")


def field_hilo_plan(plan_nt, ns):
    """The source splits of field_hilo_f32 for plan_nt targets (the whole grid's points when the launch is a block of its rows)
    and ns sources: a function of the two counts alone."""
    return FieldHiloPlan(*map(int, _ask(["%d %d\n" % (int(plan_nt), int(ns))], "field_hilo")[0].split()))
