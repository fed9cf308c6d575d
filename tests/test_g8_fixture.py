"""CPU tier of G8 (tests/golden/g8_fp32_routes.npz, oracle/g8_cases.py): the inputs regenerate, both oracles are pinned to
the reference's numbers at the sizes where the fp32 routes change, and every pair of cases still straddles the library's
threshold.  A threshold that moves fails here: move the case pair with it and regenerate G8 (python oracle/gen_golden.py g8).
The GPU tier runs the same cases through the production entry points (tests/test_gpu_g8.py)."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import grouped, load_golden
from oracle import c_oracle
from oracle import g8_cases as G8
from oracle import ludvm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ludvm_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_rule  # noqa: E402
import sym_rule  # noqa: E402
REGEN = "regenerate G8 with the case pair at the new value (oracle/g8_cases.py, python oracle/gen_golden.py g8)"


@pytest.fixture(scope="module")
def g8():
    return grouped(load_golden("g8_fp32_routes.npz"))


def _targets(c, ref):
    inp = G8.inputs(c)
    return inp, G8.targets(c, inp, ref["idx"])


def test_g8_inputs_regenerate_and_the_fixture_is_the_tables(g8):
    assert sorted(g8) == sorted(G8.BY_NAME)
    for c in G8.CASES:
        ref = g8[c["name"]]
        inp = G8.inputs(c)
        assert np.array_equal(ref["sha256"], G8.digest(inp)), c["name"]
        assert np.array_equal(ref["params"], G8.params(c)), c["name"]
        assert np.array_equal(ref["idx"], G8.sample(c)), c["name"]
        assert len(np.unique(ref["idx"])) == len(ref["idx"]) == (512 if c["nt"] == 512 else 256)
        for k, v in inp.items():        # what every entry point is handed is exactly what the reference saw
            assert v.dtype == np.float64 and np.array_equal(v, v.astype(np.float32).astype(np.float64)), (c["name"], k)
        assert len(inp["xs"]) == c["ns"], c["name"]
        if c["kind"] != "grid":
            assert len(inp.get("xt", inp["xs"])) == c["nt"], c["name"]
        if c["kind"] == "grid":
            x1, z1 = G8.grid_axes(c)
            assert (len(x1), len(z1)) == (c["nx"], c["nz"]) and c["nt"] == c["nx"] * c["nz"]
            nx, nz = c["nx"], c["nz"]
            corners = {0, nz - 1, (nx - 1) * nz, nx * nz - 1}
            assert corners <= set(ref["idx"].tolist()), c["name"]
        elif c["nt"] > 512:
            assert np.array_equal(ref["idx"][:64], np.arange(64)) and np.array_equal(ref["idx"][-64:], np.arange(c["nt"] - 64, c["nt"]))


def test_g8_python_oracle_is_bit_identical(g8):
    """oracle/ludvm_oracle.py on every G8 case: the reference's arithmetic, so the same bits (rows are independent: chunked
    by target rows as test_g1_row_chunking_is_bit_identical relies on)."""
    for c in G8.CASES:
        ref = g8[c["name"]]
        inp, (xp, zp) = _targets(c, ref)
        rows = max(1, (1 << 24) // c["ns"])
        u, w = O.induced_velocity(inp["g"], inp["xs"], inp["zs"], xp, zp, c["v_core"], rows_per_chunk=rows)
        assert np.array_equal(u, ref["u"]) and np.array_equal(w, ref["w"]), c["name"]
        if "foil_x" in inp:
            u, w = O.induced_velocity(inp["foil_g"], inp["foil_x"], inp["foil_z"], xp, zp, c["v_core"])
            assert np.array_equal(u, ref["u_foil"]) and np.array_equal(w, ref["w_foil"]), c["name"]


@pytest.mark.skipif(not c_oracle.available(), reason="oracle/libpair_oracle.so not built")
def test_g8_c_oracle_matches_the_reference(g8):
    """oracle/pair_oracle.c (what the GPU tests use at large N) within test_c_oracle_matches_goldens' bound: same terms, only
    the order of the row sum differs."""
    for c in G8.CASES:
        ref = g8[c["name"]]
        inp, (xp, zp) = _targets(c, ref)
        srcs = [(inp["g"], inp["xs"], inp["zs"], "u", "w")]
        if "foil_x" in inp:
            srcs.append((inp["foil_g"], inp["foil_x"], inp["foil_z"], "u_foil", "w_foil"))
        for g, xs, zs, ku, kw in srcs:
            u, w = c_oracle.induced_velocity(g, xs, zs, xp, zp, c["v_core"])
            scale = np.abs(g).sum()
            bound = 1e-13 * max(1.0, np.abs(ref[ku]).max(), np.abs(ref[kw]).max()) * max(1.0, scale)
            np.testing.assert_allclose(u, ref[ku], rtol=1e-11, atol=bound, err_msg=c["name"])
            np.testing.assert_allclose(w, ref[kw], rtol=1e-11, atol=bound, err_msg=c["name"])


def _library_constants():
    """The symmetric rule's thresholds from the rule itself (tools/sym_rule.py), the direct kernels' plan constants from the plan
    itself (tools/plan_rule.py), the routing constants of the entry points from the source."""
    rule = sym_rule.constants()
    plan = plan_rule.constants()
    ctx = open(os.path.join(CSRC, "ctx.hpp")).read()

    def one(pattern, text, conv=int):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return conv(m[0])
    return {
        "kSymMinN": rule["kSymMinN"],
        "kSymT8MinN": rule["kSymT8MinN"],
        "kPatch4MinTargets": plan["kPatch4MinTargets"],
        "tpl2_min_targets": plan["kTpl2MinTargets"],
        "kOrderMin": one(r"constexpr size_t kOrderMin = (\d+);", ctx),
        "kSmallSidePairsF64": one(r"constexpr double kSmallSidePairsF64 = ([0-9.]+);", ctx, float),
        "small_tile_max": plan["kSmallTileMaxDefault"],
        "sym_quad_min_tiles": rule["kSymQuadMinTiles"],
        "kMaxExtentOverCore": one(r"constexpr double kMaxExtentOverCore = ([0-9.]+);", ctx, float),
        "kMaxExtentOverCoreCloud": one(r"constexpr double kMaxExtentOverCoreCloud = ([0-9.]+);", ctx, float),
    }


def test_g8_pairs_straddle_the_librarys_thresholds():
    """Each pair of G8 cases is (t - 1, t), t = the first size on the far side of the library's current threshold."""
    k = _library_constants()
    first = {
        "small_tile_max": k["small_tile_max"] + 1,           # plan_rule.hpp direct_plan: ns <= small_tile_max -> 256-source tiles
        "kSymMinN": k["kSymMinN"],                           # use_symmetric: n >= kSymMinN
        "kSymT8MinN": k["kSymT8MinN"],                       # sym_tile_t: n >= kSymT8MinN -> T = 8
        "sym_quad_min_tiles": sym_rule.rule(range(1, 4000000), first_quad=True)[0].n,    # the first size the rule itself marks quad
        "kOrderMin": k["kOrderMin"],                         # ludvm_induce_f64: min(ns, nt) < kOrderMin -> float64 / hi+lo
        "kSmallSidePairsF64": int(k["kSmallSidePairsF64"] // 512) + 1,     # ns * 512 <= 2^28 -> float64 (512 targets)
        "tpl2_min_targets": k["tpl2_min_targets"],           # direct_plan: nt >= 131072 -> 2 targets per lane
    }
    for lo, hi, const in G8.PAIRS:
        a, b = G8.BY_NAME[lo], G8.BY_NAME[hi]
        key = "ns" if a["ns"] != b["ns"] else "nt"
        t = first[const]
        assert (a[key], b[key]) == (t - 1, t), f"{const} moved: the first size on its far side is now {t}; {REGEN}"
    for c in G8.CASES:
        if c["threshold"] is not None and c["threshold"][0] in k:
            name, value = c["threshold"]
            assert k[name] == value, f"{c['name']}: {name} is {k[name]}, the case table says {value}; {REGEN}"


def test_g8_grid_and_extent_cases_sit_on_their_sides():
    k = _library_constants()
    ff = {n: G8.BY_NAME[n] for n in ("ff_default", "ff_small", "ff_fine", "ff_ragged")}
    # 2 x 4 patch below kPatch4MinTargets grid points, 4 x 4 from there (plan_rule.hpp grid_patch_rows)
    assert ff["ff_default"]["nt"] < k["kPatch4MinTargets"] <= ff["ff_fine"]["nt"], REGEN
    assert ff["ff_default"]["ns"] > k["small_tile_max"] and ff["ff_fine"]["ns"] > k["small_tile_max"], REGEN
    # 256-source tiles: at most small_tile_max sources and 65 536 grid points (direct_plan)
    assert ff["ff_small"]["ns"] <= k["small_tile_max"] and ff["ff_small"]["nt"] <= 65536 == plan_rule.constants()["kSmallTileMaxTargets"], REGEN
    # the patch kernels need rows of a multiple of 4 points; the generic grid path takes the others
    assert ff["ff_ragged"]["nz"] % 4 != 0 and all(ff[n]["nz"] % 4 == 0 for n in ("ff_default", "ff_small", "ff_fine"))
    # the first G8 flow field is the reference's default grid (flowfield(), LUDVM.py:1186)
    assert (ff["ff_default"]["nx"], ff["ff_default"]["nz"]) == (500, 400)
    # extent bounds: the host restatement of order.hip's decision puts each case on its side, with a margin
    margin = {False: 0.05, True: 0.10}        # (Morton order on the device may differ from this estimate in its key rounding)
    for c in G8.CASES:
        if c["extent_side"] is None:
            continue
        inp = G8.inputs(c)
        reordered, extent = G8.predicted_order(inp["xs"], inp["zs"])
        assert reordered == c["reordered"], c["name"]
        bound = k["kMaxExtentOverCoreCloud"] if reordered else k["kMaxExtentOverCore"]
        ratio = extent / c["v_core"]
        if c["extent_side"] == "above":
            assert ratio > (1 + margin[reordered]) * bound, (c["name"], ratio, bound, REGEN)
        else:
            assert ratio < (1 - margin[reordered]) * bound, (c["name"], ratio, bound, REGEN)


def test_the_rule_takes_each_g8_threshold_pair_to_its_two_routes():
    """What the launch rule itself (ludvm_amd/csrc/sym_rule.hpp through tools/sym_rule.py) says at the pairs of self-interaction
    cases: each side gets the route its case is in the table for -- direct | symmetric, 256- | 512-vortex tiles, plain | quad --
    and the march turns symmetric at its own, lower size.  DESIGN 4.2's quad geometry at the headline size."""
    sizes = [G8.BY_NAME[name]["ns"] for lo, hi, const in G8.PAIRS[1:4] for name in (lo, hi)]
    assert sizes == [16383, 16384, 36863, 36864, 327168, 327169]
    route = [(bool(r.symmetric), r.T, bool(r.quad), r.kernel) for r in sym_rule.rule(sizes)]
    assert route[0][0] is False and route[0][3] is None                                  # the direct kernel
    assert route[1] == route[2] == (True, 4, False, "pair_sym_f32<4, false, 4, true>")
    assert route[3] == (True, 8, False, "pair_sym_f32<8, false, 4, true>")
    assert route[4] == (True, 8, False, "pair_sym_f32<8, false, 0, true>")               # (mixed, the bulk by single waves)
    assert route[5] == (True, 8, True, "pair_sym_quad_f32<8>")
    below, above = sym_rule.rule([11263, 11264], march=True)
    assert not below.symmetric and above.symmetric and (above.T, above.kernel) == (4, "pair_sym_f32<4, false, 4, true>")
    assert not any(r.symmetric for r in sym_rule.rule([11263, 11264]))                   # ... outside the march: from kSymMinN
    big, = sym_rule.rule([1000000])
    assert big.quad and (big.quad_chunks, big.quad_long, big.quad_per, big.quad_pershort) == (119, 53, 16, 2)     # 53 + 66 = 119
