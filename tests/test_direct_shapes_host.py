"""CPU tier of the direct-kernel shape table (tests/direct_shapes_common.py): what the library's own plan (plan_rule.hpp through
tools/plan_rule.py) makes of the table -- every instantiation launch_pair can launch is met, each with a ragged last target
block, a ragged last source tile, a split of several tiles and a split of exactly one source --, every case sits on its side
of its route's precondition, and the float64 reference would notice a lost, doubled or misplaced source.  The GPU tier
(tests/test_gpu_direct_shapes.py) runs the same table through the production entry points."""
import os
import re

import numpy as np
import pytest

import direct_shapes_common as D
from oracle import g8_cases as G8

plan_rule = D.plan_rule
CSRC = os.path.join(D.ROOT, "ludvm_amd", "csrc")

# Every instantiation launch_pair can launch, and where the table meets it: 'product', or the measurement build
# (libludvm_hip_exp.so) with the switch that forces it at these sizes.  In a product build the 1024-source tile with one
# target per lane takes over above small_tile_max = 14000 sources (at any size only for grids whose rows are no multiple of 4
# points: they have no 256-source-tile kernel), the 4 x 4 patch from 2^20 grid points, the 1024-source
# tile of the 2 x 4 patch above 14000 sources or 65536 grid points, pair_f64<512> above 256 targets AND 12000 sources (the
# table has that one product pair), and the row kernels only run under LUDVM_GRID_KERNEL=row.
EXPECTED = {
    "pair_f32<1, 256, false, 0, false>": "product",
    "pair_f32<1, 256, true, 0, false>": "product",
    "pair_f32<1, 256, false, 0, true>": "product",
    "pair_f32<1, 1024, false, 0, false>": "product",        # (generic flow-field grids; array targets: tile1024)
    "pair_f32<1, 1024, true, 0, false>": "tile1024",
    "pair_f32<1, 1024, false, 0, true>": "product",         # (generic flow-field grids; array targets: tile1024)
    "pair_f32<2, 1024, false, 0, false>": "product",
    "pair_f32<2, 1024, true, 0, false>": "product",
    "pair_f32<2, 1024, false, 0, true>": "product",
    "pair_f32<4, 1024, false, 0, false>": "product",
    "pair_f32<4, 1024, true, 0, false>": "product",
    "pair_f32<4, 1024, false, 0, true>": "product",
    "pair_f32<4, 256, false, 1, false>": "grid_row",
    "pair_f32<4, 256, false, 1, true>": "grid_row",
    "pair_f32<4, 1024, false, 1, false>": "grid_row_tile1024",
    "pair_f32<4, 1024, false, 1, true>": "grid_row_tile1024",
    "pair_f32<8, 256, false, 2, false>": "product",
    "pair_f32<8, 256, false, 2, true>": "product",
    "pair_f32<8, 1024, false, 2, false>": "tile1024",
    "pair_f32<8, 1024, false, 2, true>": "tile1024",
    "pair_f32<16, 1024, false, 2, false>": "grid_patch4_tile1024",
    "pair_f32<16, 1024, false, 2, true>": "grid_patch4_tile1024",
    "pair_f64<128>": "product",
    "pair_f64<512>": "product",
    "pair_f64_few<128>": "product",
}
# Where one of the four shapes cannot occur, per instantiation: nowhere -- with the forced splits every family walks several
# tiles in one split, and every source list of the table has a size one past a tile.  (pair_f64_few runs only with more than
# one split and at most 128 targets, all in its one workgroup row: its "target block" is the group of nt lanes, ragged
# whenever 256 is no multiple of nt.)
CANNOT = {}


def _met(kernel):
    return [(f, b, c, p) for f, b, c, p in D.planned_table() if p.kernel == kernel]


def test_the_table_names_every_instantiation_launch_pair_can_launch():
    first = {}
    for family, build, case, p in D.planned_table():
        rank = 0 if build == "product" else 1
        if p.kernel not in first or rank < first[p.kernel][0]:
            first[p.kernel] = (rank, build)
    assert sorted(first) == sorted(EXPECTED), sorted(set(first) ^ set(EXPECTED))
    for kernel, where in EXPECTED.items():
        builds = {b for _, b, _, p in D.planned_table() if p.kernel == kernel}
        assert where in builds, (kernel, where, sorted(builds))
        assert ("product" in builds) == (where == "product"), (kernel, sorted(builds))      # marked as what it is
    # ... and these are all the instantiations there are: launch.hip's dispatch names the same set
    with open(os.path.join(CSRC, "launch.hip")) as f:
        launch = f.read()
    named = set()
    for tpl, tile, hilo, grid, local in re.findall(r"LUDVM_PAIR_F32\((\d+), (\w+), (\w+), (\d), (\w+)\)", launch):
        tile = {"kTileF32": plan_rule.constants()["kTileF32"], "kTileF32Small": plan_rule.constants()["kTileF32Small"]}[tile]
        named.add(f"pair_f32<{tpl}, {tile}, {hilo}, {grid}, {local}>")
    assert named == {k for k in EXPECTED if k.startswith("pair_f32")}, sorted(named ^ set(EXPECTED))
    # plan_rule.hpp is the only statement of the plan: the library's units include it and restate none of its constants
    texts = {}
    for name in ("launch.hip", "ctx.hpp", "pair_kernels.hpp", "context.hip"):
        with open(os.path.join(CSRC, name)) as f:
            texts[name] = f.read()
    assert '#include "plan_rule.hpp"' in texts["pair_kernels.hpp"] and '#include "pair_kernels.hpp"' in texts["ctx.hpp"]
    assert "direct_plan(plan_knobs(c)" in texts["launch.hip"] and "direct_variant(plan_knobs(c)" in texts["launch.hip"]
    restated = r"constexpr[^;=]*\b(" + "|".join(c for c in plan_rule.CONSTANTS) + r") ="
    assert not re.search(restated, "".join(texts.values()))


@pytest.mark.parametrize("kernel", sorted(EXPECTED))
def test_each_instantiation_meets_the_four_ragged_shapes(kernel):
    """a ragged last target block, a ragged last source tile, a split of more than one tile, a split of exactly one source"""
    seen = set()
    for family, build, case, p in _met(kernel):
        ns, nt = case["ns"], case["nt"]
        sizes = D.split_sizes(ns, p)
        assert sum(sizes) == ns and all(s >= 1 for s in sizes) and p.chunk % p.tile == 0, (case, p)
        if p.family == "f64_few":
            per_block = nt
            ragged_t = 256 % nt != 0
        elif p.grid == 2:
            rows = p.tpl // 4
            per_block = None
            ragged_t = ((-(-(nt // case["grid_nz"]) // rows)) * (case["grid_nz"] // 4)) % 256 != 0 or (nt // case["grid_nz"]) % rows != 0
        else:
            per_block = 256 * p.tpl
            ragged_t = nt % per_block != 0
        if ragged_t:
            seen.add("ragged target block")
        if sizes[-1] % p.tile != 0:
            seen.add("ragged source tile")
        if max(sizes) > p.tile:
            seen.add("split of several tiles")
        if sizes[-1] == 1:
            seen.add("split of one source")
        # the launch covers its targets and its splits
        if per_block and p.family != "f64_few":
            assert p.blocks_x * per_block >= nt > (p.blocks_x - 1) * per_block and p.blocks_y == p.nsplit, (case, p)
        if p.family == "f64_few":
            assert p.groups == min(256 // nt, 4) and p.blocks_y * p.groups >= p.nsplit > (p.blocks_y - 1) * p.groups, (case, p)
    want = {"ragged target block", "ragged source tile", "split of several tiles", "split of one source"} - CANNOT.get(kernel, set())
    assert seen >= want, (kernel, sorted(want - seen))


def test_the_few_targets_kernel_is_met_at_every_group_count_boundary():
    groups = {}
    for family, build, case, p in D.planned_table():
        if family == "f64" and build == "product":
            groups.setdefault(case["nt"], set()).add((p.family, p.groups, p.nsplit))
    few = {nt: {g for f, g, _ in v if f == "f64_few"} for nt, v in groups.items()}
    assert [few[nt] for nt in (63, 64, 65, 85, 86, 127, 128, 129, 257)] == [{4}, {4}, {3}, {3}, {2}, {2}, {2}, set(), set()]
    assert few[1] == few[2] == few[42] == {4} and few[43] == {4}
    for g in (2, 3, 4):         # split counts that are and are not multiples of the group count
        ns_ = {n % g == 0 for nt, v in groups.items() for f, gg, n in v if f == "f64_few" and gg == g}
        assert ns_ == {True, False}, g
    # one split is the unpacked kernel's even at few targets, and so is every launch of the LUDVM_FEW_PACKED=0 build
    assert all(p.family == "f64" for f, b, c, p in D.planned_table() if f == "f64" and (p.nsplit == 1 or b == "few_unpacked"))
    # the hand-over at 129 targets, and pair_f64<512> on the far side of small_tile_max_f64 only
    (lo, hi) = [p for f, b, c, p in D.planned_table() if f == "f64_product_pair"]
    assert (lo.kernel, hi.kernel) == ("pair_f64<128>", "pair_f64<512>")


def _library_constants():
    with open(os.path.join(CSRC, "ctx.hpp")) as f:
        ctx = f.read()

    def one(pattern, conv=int):
        m = re.findall(pattern, ctx)
        assert len(m) == 1, (pattern, m)
        return conv(m[0])
    k = dict(plan_rule.constants())
    k.update(kOrderMin=one(r"constexpr size_t kOrderMin = (\d+);"),
             kSmallSidePairsF64=one(r"constexpr double kSmallSidePairsF64 = ([0-9.]+);", float),
             kMaxExtentOverCore=one(r"constexpr double kMaxExtentOverCore = ([0-9.]+);", float),
             kMaxExtentOverCoreCloud=one(r"constexpr double kMaxExtentOverCoreCloud = ([0-9.]+);", float))
    return k


@pytest.mark.filterwarnings("ignore:All-NaN slice:RuntimeWarning")      # (a last block of one point has a class without a member)
def test_every_case_sits_on_its_side_of_its_routes_precondition():
    """with at least 10 % margin (sizes that ARE a threshold of the table -- 2048 points a side -- sit exactly on it)"""
    k = _library_constants()
    # induce(..., 'f32') runs fp32 on local origins from kOrderMin points on BOTH sides: the local table starts there
    assert min(D.N_LOCAL) == k["kOrderMin"] and max(D.NS_PLAIN + D.NT_PLAIN) > k["kOrderMin"]
    # (the plain and hi+lo entries -- induce_dev, induce_f32, precision 'f32x2' -- take any size as it is: no precondition)
    # induce(..., 'f64') is float64 whatever the size; 'f32' would also be below kOrderMin while ns nt <= kSmallSidePairsF64
    assert 1.1 * max(D.NS_F64) * max(D.NT_F64) < k["kSmallSidePairsF64"]
    # the product's tiles: 256-source fp32 tiles and 128-source fp64 tiles up to the small-tile bounds
    assert 1.1 * D.SIDE_CAP < k["kSmallTileMaxDefault"] and 1.1 * D.SIDE_CAP < k["kSmallTileMaxF64Default"]
    assert D.F64_PRODUCT_PAIR[0][0] == k["kSmallTileMaxF64Default"] == D.F64_PRODUCT_PAIR[1][0] - 1
    assert all(nt > k["kFewTargets"] for _, nt in D.F64_PRODUCT_PAIR) and all(nt > k["kFewTargets"] for nt in D.NT_F64_512)
    assert max(D.NT_PLAIN + D.N_LOCAL) * 1.1 < k["kTpl2MinTargets"]          # the rule's TPL is 1 everywhere in the table
    # below kSymMinN every self-interaction is the direct kernel's
    import sym_rule
    assert 1.1 * D.SIDE_CAP < sym_rule.constants()["kSymMinN"]
    # kept / reordered, and the extent of the origin classes against the sparse bounds
    for layout in D.LAYOUTS:
        for ns, nt in D.local_shapes(layout):
            g, xs, zs, xt, zt, vc = D.local_inputs(layout, ns, nt)
            sides = [("sources", xs, zs, layout in ("cloud", "self"))]
            if layout != "self":
                sides.append(("targets", xt, zt, layout in ("cloud", "mixed")))
            for what, x, z, want_reordered in sides:
                reordered, extent = G8.predicted_order(x, z)
                assert reordered == want_reordered, (layout, ns, nt, what)
                bound = k["kMaxExtentOverCoreCloud"] if reordered else k["kMaxExtentOverCore"]
                assert extent / vc < 0.9 * bound, (layout, ns, nt, what, extent / vc, bound)
    # the host flow field's sources: ordered from kOrderMin on, their class extents under the bound either way
    for ns in D.NS_GRID:
        g, xs, zs, vc = D.grid_inputs(ns)
        if ns >= k["kOrderMin"]:
            reordered, extent = G8.predicted_order(xs, zs)
        else:
            reordered, extent = False, G8.class_extent_mean(xs, zs)
        bound = k["kMaxExtentOverCoreCloud"] if reordered else k["kMaxExtentOverCore"]
        assert extent / vc < 0.9 * bound, (ns, extent / vc, bound)


def test_no_case_is_larger_than_it_needs_to_be():
    for family, build, case, p in D.planned_table():
        if family == "f64_product_pair":
            continue
        assert case["ns"] <= D.SIDE_CAP and case["nt"] <= D.SIDE_CAP, case
    for arrays in (D.plain_inputs(3073, 2049), D.hilo_sheet_inputs(3073, 2049), D.local_inputs("mixed", 2049, 2305)):
        for a in arrays[:5]:          # what every entry point is handed is exactly what the reference saw
            assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    X, Z = D.grid_points(7, 37)
    assert np.array_equal(X, X.astype(np.float32)) and np.array_equal(Z, Z.astype(np.float32))


def _last_split_firsts(family, ns, nt):
    return sorted({(p.nsplit - 1) * p.chunk for f, b, c, p in D.planned_table()
                   if f == family and c["ns"] == ns and c["nt"] == nt})


def _sensitivity(name, inputs, tol, firsts, local):
    """Each change to the reference moves at least one target by more than 10 x the case's tolerance."""
    g, xs, zs, xt, zt, vc = inputs
    ns, nt = len(xs), len(xt)
    ur, wr = D.cached_reference(name, inputs)
    need = 10 * tol * max(np.abs(ur).max(), np.abs(wr).max())

    def moved(du, dw):
        return max(np.abs(du).max(), np.abs(dw).max())
    # dropping the last source, the first source of the last split (of every plan the table runs the case under), counting
    # one source twice: the change IS that source's contribution
    for k in sorted({ns - 1, ns // 2, *firsts}):
        assert moved(*D.contribution(g[k], xs[k], zs[k], xt, zt, vc)) > need, (name, "source", k)
    # reading the targets shifted by one index (one target: there is no other index)
    if nt > 1:
        assert moved(np.roll(ur, -1) - ur, np.roll(wr, -1) - wr) > need, (name, "targets shifted")
    # swapping the two origin classes of the last block: its sources move by the difference of the classes' origins (a last
    # block of one source has one origin, lent to both classes: nothing to swap)
    if local:
        b = (ns - 1) // 256
        o0, o1 = plan_rule.origin_index([(b, 0, ns), (b, 1, ns)])      # (the kernels' own rule, from their header)
        if o0 != o1:
            sl = slice(256 * b, ns)
            sign = np.where(np.arange(256 * b, ns) % 2 == 0, 1.0, -1.0)
            xsw, zsw = xs[sl] + sign * (xs[o1] - xs[o0]), zs[sl] + sign * (zs[o1] - zs[o0])
            u0, w0 = D.contribution(g[sl], xs[sl], zs[sl], xt, zt, vc)
            u1, w1 = D.contribution(g[sl], xsw, zsw, xt, zt, vc)
            assert moved(u1 - u0, w1 - w0) > need, (name, "origin classes swapped")
        else:
            assert ns - 256 * b == 1


def test_the_reference_would_notice_a_lost_doubled_or_misplaced_source_plain_hilo_f64():
    for ns in D.NS_PLAIN:
        for nt in D.NT_PLAIN:
            _sensitivity(("plain", ns, nt), D.plain_inputs(ns, nt), D.TOL["plain"], _last_split_firsts("plain", ns, nt), False)
            _sensitivity(("hilo", ns, nt), D.plain_inputs(ns, nt), D.TOL["hilo"], _last_split_firsts("hilo", ns, nt), False)
            _sensitivity(("hilo_sheet", ns, nt), D.hilo_sheet_inputs(ns, nt), D.TOL["hilo"], _last_split_firsts("hilo", ns, nt), False)
    for ns in D.NS_F64 + D.NS_F64_512:
        for nt in D.NT_F64 + D.NT_F64_512:
            fam = "f64" if ns in D.NS_F64 and nt in D.NT_F64 else "f64_512"
            _sensitivity(("f64", ns, nt), D.f64_inputs(ns, nt), D.TOL["f64"], _last_split_firsts(fam, ns, nt), False)


@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_the_reference_would_notice_a_lost_doubled_or_misplaced_source_local(layout):
    for ns, nt in D.local_shapes(layout):
        _sensitivity((layout, ns, nt), D.local_inputs(layout, ns, nt), D.TOL["local"],
                     _last_split_firsts("local_" + layout, ns, nt), True)


def test_the_reference_would_notice_a_lost_source_advect_and_grids():
    for ns in D.NS_ADVECT:
        g, xs, zs, vc = D.advect_inputs(ns)
        for t_first, nt in D.advect_ranges(ns):
            inputs = (g, xs, zs, xs[t_first:t_first + nt], zs[t_first:t_first + nt], vc)
            firsts = sorted({(p.nsplit - 1) * p.chunk for f, b, c, p in D.planned_table()
                             if f == "advect" and c["ns"] == ns and c["nt"] == nt})
            # (a vortex induces nothing on itself: a one-target range is not asked about its own source)
            firsts = [k for k in firsts if not (nt == 1 and k == t_first)]
            g_, xs_, zs_, xt_, zt_, _ = inputs
            ur, wr = D.cached_reference(("advect", ns, t_first, nt), inputs)
            need = 10 * D.TOL["plain"] * max(np.abs(ur).max(), np.abs(wr).max())
            for k in sorted({ns - 1 if not (nt == 1 and t_first == ns - 1) else ns - 2, *firsts}):
                du, dw = D.contribution(g[k], xs[k], zs[k], xt_, zt_, vc)
                assert max(np.abs(du).max(), np.abs(dw).max()) > need, (ns, t_first, nt, k)
            if nt > 1:     # t_first off by one
                assert max(np.abs(np.roll(ur, -1) - ur).max(), np.abs(np.roll(wr, -1) - wr).max()) > need, (ns, t_first, nt)
    for ns in D.NS_GRID:
        g, xs, zs, vc = D.grid_inputs(ns)
        for nx, nz, _ in D.grid_shapes():
            xt, zt = D.grid_points(nx, nz)
            fam_firsts = sorted({(p.nsplit - 1) * p.chunk for f, b, c, p in D.planned_table()
                                 if f.startswith("grid") and c["ns"] == ns and c["nt"] == nx * nz})
            _sensitivity(("grid", ns, nx, nz), (g, xs, zs, xt, zt, vc), D.TOL["plain"], fam_firsts, False)
