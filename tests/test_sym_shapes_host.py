"""CPU tier of the symmetric-kernel shape table (tests/sym_shapes_common.py).

The partition -- which (tile, d-chunk) work items each XCD's workgroups hold, which ring offsets a chunk holds, which tiles an owner
of a sharded ring holds, how many workgroups a launch whose count is read on the device may need -- is enumerated from
ludvm_amd/csrc/sym_rule.hpp itself by tools/sym_rule.py's `cover` program (the loops run inside the compiled program; Python gets
counts and the first counter-example), exhaustively over 1 .. 700 tiles.  The two kernels' tile-pair predicates, restated once in
that program, are pinned to the kernels' source lines.  Then: the GPU table reaches every shape it is there for (asserted from the
rule), and its float64 reference would notice a lost or doubled tile pair, a lost quarter of the rotation steps, a lost last
vortex and swapped parity origins at more than ten tolerances."""
import collections
import os
import time

import numpy as np
import pytest

import sym_shapes_common as S
from observer_sources_common import fast_iv

sym_rule = S.sym_rule
KERNELS = os.path.join(S.ROOT, "ludvm_amd", "csrc", "pair_sym_kernels.hpp")
# (the wake entries' bounds, tests/test_gpu_rollup_edges.py TOL; the induce entries' are the same or tighter, oracle/g8_cases.py TOL)
TOL = {"plain": 1e-5, "local": 1e-5, "hilo": 3e-6}


def _passes(checks, *names):
    for name in names:
        c = checks[name]
        print(f"{name}: {c.checked} cases, {c.failures} failures")
        assert c.checked > 0 and c.failures == 0, (name, c)


# ---- the partition, from the header ------------------------------------------------------------------------------------------------
def test_every_item_is_held_by_exactly_one_workgroup_slot_for_1_to_700_tiles():
    """Over the 8 XCDs the items are units x [y0, y0 + ny), each once (the mixed form: bulk and tail chunks separately), xcd_item is
    false from xcd_items on, sym_blocks_xcd covers every XCD's workgroups under the kernel's packing, the chunks are
    (ysplit - 1) per < dtot <= ysplit per with per = ceil(dtot / ysplit), 0 <= ytail <= ysplit, rbulk in {1, 2, 4}; both tiles, every
    tune_rsplit in {0, -1, -2, 1, 2, 4}, tune_split in {0, 1, 2, 3, 5, 64, 1024}, xcd_run in {0, 1, 3, 8}"""
    t0 = time.time()
    checks = sym_rule.cover_check("items", 700)
    print(f"items: {time.time() - t0:.1f} s")
    _passes(checks, "cover", "chunks", "ranges", "blocks", "tiles")


def _source_line(text, marker):
    lines = [l.strip() for l in text.splitlines() if marker in l]
    assert len(lines) == 1, (marker, lines)
    return lines[0]


def test_the_ring_of_tile_pairs_and_the_kernels_predicates():
    """{I, I + d mod NT} over I and d = 1 .. dmax, plus d = NT / 2 for I < NT / 2 on an even ring, is every unordered pair of distinct
    tiles once -- as a set, and as the rounds of pair_sym_f32's items meet it chunk by chunk (1 .. 700 tiles, every split).  The
    predicate the program walks is the kernel's: its text is taken from the kernel source, and this test fails when that line
    changes."""
    with open(KERNELS) as f:
        src = f.read()
    valid = _source_line(src, "rd.valid =")
    assert valid.startswith("rd.valid = rd.diag || (active && dd < per && d < d_hi && !(even && d == dtot && I >= ntiles / 2));"), valid
    assert _source_line(src, "const int d = rd.diag ?") == "const int d = rd.diag ? 0 : d_lo + dd;"
    assert _source_line(src, "const int per = a.diag_only") == \
        "const int per = a.diag_only ? 0 : (int)(((unsigned)dtot + (unsigned)ysplit - 1) / (unsigned)ysplit);"
    assert _source_line(src, "const int d_lo =") == "const int d_lo = 1 + y * per;"
    assert src.count("if (d_hi > dtot + 1) d_hi = dtot + 1;") == 1
    assert src.count("const bool even = (ntiles % 2 == 0) && ntiles > 1;") == 2          # both kernels
    assert _source_line(src, "const int dtot = (int)dmax + (even ? 1 : 0);")
    # ... and the program's restatement is that text (casts apart)
    prog = sym_rule.COVER_MAIN.replace("(int)I", "I")
    assert "return dd < per && d < d_hi && !(even && d == dtot && I >= ntiles / 2);" in prog
    assert "const int d_lo = 1 + y * per;" in prog and "if (d_hi > dtot + 1) d_hi = dtot + 1;" in prog
    _passes(sym_rule.cover_check("ring", 700), "ring_set", "ring_rounds")


def test_the_quad_variants_chunks_and_pairs():
    """quad_chunk tiles [1, Dtot + 1) without gap or overlap for 16 .. 5000 tiles and tune_split in {0, 1, 2, 3, 5, 128, 1024}; the
    waves of every quad, at offsets D - w kept to 1 .. dmax plus the half-way rule, meet every unordered pair of distinct tiles once
    (16 .. 300 tiles and a few larger rings; the diagonal tiles are the diag_only launch's); quad_blocks covers every XCD's
    workgroups.  The predicate is pinned to the kernel's text."""
    with open(KERNELS) as f:
        src = f.read()
    own = "const bool own = Iw < i_first + i_count && Iw < ntiles;"
    ret = "return own && ((d >= 1 && d <= (int)dmax) || (even && d == dtot && Iw < ntiles / 2));"
    assert _source_line(src, "const bool own =") == own and _source_line(src, "return own &&") == ret
    assert _source_line(src, "const int d = D - w;") and _source_line(src, "unsigned J = I0 + (unsigned)(D_lo + dd);")
    assert own in sym_rule.COVER_MAIN and ret in sym_rule.COVER_MAIN
    _passes(sym_rule.cover_check("quad", 5000, 300), "quad_chunks", "quad_pairs", "quad_blocks", "quad_cover")


def test_owner_blocks_of_a_sharded_ring():
    """shard_block over world 1 .. 17 partitions a ring of 1 .. 5000 tiles into consecutive blocks of whole quads (the last one ends
    with the ring; empty owners allowed), and the owners' items together are the single owner's, for plain and quad launches
    (1 .. 120 tiles)"""
    _passes(sym_rule.cover_check("owners", 5000, 120, 17), "owner_blocks", "owner_items", "owner_quad_items")


def _switch_sizes():
    """vortex counts on both sides of every switch of the rule: its thresholds, and every size at which the rule's pick changes"""
    c = sym_rule.constants()
    marks = {c["kSymMinN"], c["kSymMinNMarch"], c["kSymT8MinN"], 512 * c["kSymQuadMinTiles"], 16 * 512, 2, 257, 513}
    for march in (False, True):
        rows = sym_rule.rule(range(256, 512 * c["kSymQuadMinTiles"] + 2048, 256), march=march)
        for a, b in zip(rows, rows[1:]):
            if (a.symmetric, a.T, a.rsplit, a.rbulk, a.quad) != (b.symmetric, b.T, b.rsplit, b.rbulk, b.quad):
                marks.add(b.n)
    sizes = set()
    for m in marks:
        sizes.update(n for n in (m - 257, m - 256, m - 1, m, m + 1, m + 255, m + 256, m + 257) if n >= 2)
    return sorted(sizes)


def test_the_grid_of_a_launch_whose_count_is_read_on_the_device():
    """For n on both sides of every switch in the header and n_lo = n - 256: sym_grid_bound is at least the workgroups of the geometry
    the device re-derives for every count in [n_lo, n] (both tiles, hi+lo, every code, split and XCD run), that geometry's
    waves-per-item rule is the host's instantiation, and the 32-bit and 64-bit forms of sym_geometry_t agree"""
    sizes = _switch_sizes()
    assert len(sizes) > 60
    _passes(sym_rule.cover_check("device", stdin=" ".join(map(str, sizes))), "device_bound", "device_rule", "device_width")


# ---- the table reaches everything ---------------------------------------------------------------------------------------------------
def _idle_beside_active(g, R):
    """some workgroup holds an idle wave beside an active item: an XCD's item count is no multiple of the 4 / R items per workgroup"""
    return any(len(x["all"]) % (4 // R) != 0 for x in g.xcds)


def test_the_table_reaches_every_shape_it_is_there_for():
    table = S.table()
    fam = collections.Counter(c.family for c in table)
    print("symmetric shape table:", dict(fam), "+", len(S.owner_cases()), "owner cases; rings of", S.TILES, "tiles, quad", S.QUAD_TILES)
    for form in ("plain", "local", "hilo"):
        for T in ((4,) if form == "hilo" else S.TS):
            W = 64 * T
            for R in S.RS:
                cases = [(c, S.geometry(c)) for c in table if c.family == form and c.T == T and c.code == R]
                assert all(g.rsplit == R and g.ytail == 0 for _, g in cases)
                has = lambda p: any(p(c, g) for c, g in cases)      # noqa: E731
                what = (form, T, R)
                assert has(lambda c, g: g.ntiles == 1) and has(lambda c, g: g.ntiles == 2), what
                assert has(lambda c, g: g.per > 1 and g.ntiles % 2 == 1) and has(lambda c, g: g.per > 1 and g.ntiles % 2 == 0), what
                # the half-way offset d = dtot sits in the last chunk; that chunk has an invalid trailing round when ysplit per > dtot
                assert has(lambda c, g: g.ntiles % 2 == 0 and g.per > 1 and g.ysplit * g.per > g.dtot), what
                assert has(lambda c, g: c.n % W == 1 and c.n > W) and has(lambda c, g: c.n % W == 0), what
                assert {c.n % W for c, _ in cases} >= {1, 63, 64, 65, W - 1, 0}, what
                if R < 4:        # (a four-wave item fills its workgroup: no wave of it is idle beside an active item)
                    assert has(lambda c, g: _idle_beside_active(g, R)), what
                assert has(lambda c, g: g.blocks_xcd * 8 * (4 // R) > g.ntiles * g.ysplit), what       # surplus slots that leave
    # the mixed form
    mixed = [(c, S.geometry(c)) for c in table if c.family in ("mixed", "mixed_big")]
    assert all(g.rsplit == 0 for _, g in mixed)
    for form in ("plain", "local"):
        for T in S.TS:
            assert any(0 < g.ytail < g.ysplit and g.rbulk == 4 for c, g in mixed if c.form == form and c.T == T), (form, T)
            assert any(g.ytail == g.ysplit for c, g in mixed if c.form == form and c.T == T), (form, T)       # (no bulk at all)
        for rb, tiles, split in S.mixed_big_rings():
            # the smallest ring with that bulk, whatever the split: asked of the rule
            assert all(tiles <= t for t in (sym_rule.smallest_mixed_ring(rb, s) for s in (0, 1, 2, 3, 5, 64, 1024)) if t), (rb, tiles)
            assert any(g.rbulk == rb and g.ntiles == tiles and 0 < g.ytail < g.ysplit and c.n % 256 == 65
                       for c, g in mixed if c.form == form and c.family == "mixed_big"), (form, rb, tiles)
        # a bulk workgroup of two two-wave items with an idle pair of waves, on some XCD
        assert any(g.rbulk == 2 and any(len(x["bulk"]) % 2 for x in g.xcds) for c, g in mixed if c.form == form), form
    assert [t for _, t, _ in S.mixed_big_rings()] == sorted((t for _, t, _ in S.mixed_big_rings()))
    # the quad variant
    for form in ("plain", "local"):
        quad = [(c, S.geometry(c)) for c in table if c.family == "quad" and c.form == form]
        assert {g.ntiles % 4 for _, g in quad} == {0, 1, 2, 3}, form                          # last quads of 4, 1, 2, 3 tiles
        assert any(c.split == 0 and g.per[2] < g.per[0] for c, g in quad), form               # tapered: short chunks behind long ones
        assert any(c.split > 0 and g.per[2] == g.per[0] and g.per[0] > 1 for c, g in quad), form          # uniform, several rounds
        assert any(g.ntiles % 2 == 0 for _, g in quad) and any(g.ntiles % 2 == 1 for _, g in quad), form
        assert {c.n % 512 for c, _ in quad} == {1, 0}, form
        assert all(g.ntiles >= 16 for _, g in quad)
    # owners: one without a tile, one whose block is a single ragged quad
    owners = [(kind, n, world, sym_rule.shard_blocks(-(-n // 512), world)) for kind, n, world, _ in S.owner_cases()]
    for kind in S.OWNER_TILES:
        mine = [(n, w, b) for k, n, w, b in owners if k == kind]
        assert any(cnt == 0 for _, _, b in mine for _, cnt in b), kind
        assert any(0 < cnt < 4 for _, _, b in mine for _, cnt in b), kind
    # the placement runs change the lists, not the items
    for c in table:
        if c.family == "xcd" and c.code != S.QUAD:
            a, b = S.geometry(c), S.geometry(c._replace(build="exp"))
            flat = lambda g: sorted(it for x in g.xcds for lst in x.values() for it in lst)      # noqa: E731
            assert flat(a) == flat(b), c


# ---- what the reference would notice ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iv():
    return fast_iv()


def _origin_index(b, p, n):
    """plan_rule.hpp origin_index: the vortex that lends class (block b, parity p) its origin"""
    first = b << 8
    mid = first + 128 + p
    if mid < n:
        return mid
    last = (n - 1) - (((n - 1) ^ p) & 1)
    return last if last >= first else first


def _moves(du, dw, scale, tol):
    return max(np.abs(du).max(), np.abs(dw).max()) / (tol * scale)


def _mutations(form, n, T, g, x, z, vc):
    """name -> (du, dw)[n]: what each defect of the partition would add to the all-pairs sums"""
    W = 64 * T
    nt = -(-n // W)
    idx = np.arange(n)
    tile = lambda I: idx[S.tile_slice(I, W, n)]      # noqa: E731
    # the tile pair: the last tile (the ragged one) and the one in front of it -- of a one-tile ring, the tile with itself (its
    # diagonal round)
    I, J = max(nt - 2, 0), nt - 1
    out = {}

    def both(ti, sj):
        a, b = S.pair_delta(g, x, z, vc, ti, sj, n), S.pair_delta(g, x, z, vc, sj, ti, n)
        return (a[0] + b[0], a[1] + b[1]) if J != I else a
    out["one tile pair left out"] = both(tile(I), tile(J))
    if nt % 2 == 0:
        out["a half-way pair counted twice"] = both(tile(0), tile(nt // 2))
    # one wave's quarter of the rotation steps: lane l's T targets against the T sources of home lane (l + k) % 64, k in [0, 16)
    # (the first wave's of a four-wave item: the quarter that holds a pair even when a tile has two members)
    du, dw = np.zeros(n), np.zeros(n)
    for ti, sj in S.rotation_quarter(I, J, W, n, 0, 16):
        for l in range(64):
            t, s = ti[l][ti[l] < n], sj[l][sj[l] < n]
            if len(t) and len(s):
                a = S.pair_delta(g, x, z, vc, t, s, n)
                du += a[0]
                dw += a[1]
                if J != I:
                    b = S.pair_delta(g, x, z, vc, s, t, n)
                    du += b[0]
                    dw += b[1]
    out["a quarter of the rotation steps left out"] = (du, dw)
    # (for the tile in front of the last one -- on a sheet its neighbours; a one-tile ring: for its own tile)
    near = tile(max(nt - 2, 0))
    out["the last vortex dropped as a partner for one tile"] = S.pair_delta(g, x, z, vc, near[near != n - 1], np.array([n - 1]), n)
    if form == "local":
        # the records of one block's two classes swapped, as the lanes of the NEXT tile read them for their partner (tile 0's last
        # block; of a one-tile ring, block 0 as the tile's own lanes read it): every even source of the block appears shifted by
        # (odd origin - even origin), every odd one by the opposite
        b0 = W // 256 - 1 if nt > 1 else 0
        blk = idx[256 * b0:min(256 * (b0 + 1), n)]
        o0, o1 = _origin_index(b0, 0, n), _origin_index(b0, 1, n)
        sx, sz = np.asarray(x, float).copy(), np.asarray(z, float).copy()
        sign = np.where(blk % 2 == 0, 1.0, -1.0)
        sx[blk] += sign * (x[o1] - x[o0])
        sz[blk] += sign * (z[o1] - z[o0])
        tg = tile(1) if nt > 1 else tile(0)
        a, b = S.D.contribution(g[blk], sx[blk], sz[blk], x[tg], z[tg], vc), S.D.contribution(g[blk], x[blk], z[blk], x[tg], z[tg], vc)
        du, dw = np.zeros(n), np.zeros(n)
        du[tg], dw[tg] = a[0] - b[0], a[1] - b[1]
        out["the two parity origins of a block swapped"] = (du, dw)
    return out


@pytest.mark.parametrize("form", ["plain", "local", "hilo"])
def test_the_reference_notices_a_wrong_partition_at_ten_tolerances(iv, form):
    """every input of the table (every distinct form, size and tile), every defect: no case is exempt"""
    shapes = sorted({(c.n, 4 if form == "hilo" else c.T) for c in S.table() if c.form == form})
    shapes += sorted({(n, 8) for _, n, _, _ in S.owner_cases()} - set(shapes)) if form == "plain" else []
    least = {}
    for n, T in shapes:
        g, x, z, vc = S.inputs(form, n)
        ur, wr = S.reference(iv, (form, n, 0), g, x, z, vc)
        scale = max(np.abs(ur).max(), np.abs(wr).max())
        for name, (du, dw) in _mutations(form, n, T, np.asarray(g, float), np.asarray(x, float), np.asarray(z, float), vc).items():
            m = _moves(du, dw, scale, TOL[form])
            if m < least.get(name, (np.inf,))[0]:
                least[name] = (m, n, T)
            assert m > 10.0, (form, n, T, name, m)
    for name, (m, n, T) in least.items():
        print(f"{form}: {name}: at least {m:.3g} tolerances (n = {n}, T = {T})")
    assert "a half-way pair counted twice" in least and ("the two parity origins of a block swapped" in least) == (form == "local")
