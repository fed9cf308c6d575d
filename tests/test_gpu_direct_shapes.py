"""GPU tier of the direct-kernel shape table (tests/direct_shapes_common.py): every direct pair-kernel instantiation by value
against the float64 oracle at ALL targets, at the ragged shapes where an index can go wrong, through the production entry
points -- forced launch shapes by set_tuning, forced tiles and kernel forms by engines of the measurement build.

Besides the values: device-pointer entries write between sentinel guards into NaN-filled outputs and read from buffers that
hold NaN beyond their counts; launches whose sums are formed by the same operations in the same order return the same bits
(targets per lane at a fixed tile and split; a target prefix of a larger launch; the packed and the unpacked few-targets
kernel; the row, 2 x 4 and 4 x 4 grid kernels).  tests/test_direct_shapes_host.py shows on the CPU that the table reaches
every instantiation and that the reference would notice a lost, doubled or misplaced source."""
import contextlib
import os

import numpy as np
import pytest

import direct_shapes_common as D

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
GUARD = 256


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


@pytest.fixture(scope="module")
def exp():
    """engines of the measurement build, by key of D.EXP, made when first asked for and closed with the module (constructed as
    test_grid_patch_kernels_equal_the_row_kernel_bit_for_bit constructs its engines: the switch is read at creation)"""
    from ludvm_amd import Engine, _ffi
    made = {}

    def get(build):
        if build not in made:
            env = D.EXP[build][1]
            assert not any(k in os.environ for k in env)
            os.environ.update(env)
            try:
                made[build] = Engine(0, lib_path=_ffi.EXP_LIB_PATH)
            finally:
                for k in env:
                    del os.environ[k]
        return made[build]
    yield get
    for e in made.values():
        e.close()


@contextlib.contextmanager
def restored(*engines):
    """Every test leaves the engines as it found them: the rule's launch shapes, the symmetric kernel on, the own stream."""
    try:
        yield
    finally:
        for e in engines:
            e.set_tuning(0, 0)
            e.set_symmetric(1)
            e.set_stream(None)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


class Guarded:
    """n float32 elements inside a larger torch buffer: inputs with NaN on both sides (an over-read that is used shows as NaN),
    outputs with GUARD sentinel elements on both sides and NaN where the results go."""

    def __init__(self, torch, n, values=None):
        self.n = n
        dev = torch.device("cuda", 0)
        if values is not None:
            host = np.full(n + 2 * GUARD, np.nan, np.float32)
            host[GUARD:GUARD + n] = values
            self.t = torch.from_numpy(host).to(dev)
        else:
            self.t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.output = values is None

    def ptr(self, first=0):
        return self.t.data_ptr() + 4 * (GUARD + first)

    def arm(self):
        self.t[GUARD:GUARD + self.n] = float("nan")

    def read(self, what):
        host = self.t.cpu().numpy()
        out = host[GUARD:GUARD + self.n].copy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + self.n:] == SENTINEL), ("guard overwritten", what)
        assert np.isfinite(out).all(), ("output not written or not finite", what, int((~np.isfinite(out)).sum()))
        return out


def _check(worst, family, got, ref, what):
    err = D.rel_err(got[0], got[1], ref[0], ref[1])
    worst[family] = max(worst.get(family, 0.0), err)
    assert err <= D.TOL[family], (what, err, D.TOL[family])


def _cross_tpl_bits(results, shapes, splits, what):
    """GRID 0: a target's sum is formed by the same operations in the same order whatever the targets per lane are (tile and
    splits fixed)"""
    for shape in shapes:
        for s in splits:
            one = results[shape + (1, s)]
            for tpl in (2, 4):
                assert _same_bits(one, results[shape + (tpl, s)]), (what, "TPL 1 vs", tpl, shape, s)


def test_plain_fp32_device_and_host_entries_by_value_with_guards(eng, exp):
    """pair_f32<1, 256 | 1024, false>, <2 | 4, 1024, false> through induce_dev (guarded buffers) and induce_f32, finish_sum<float>"""
    import torch
    big = exp("tile1024")
    worst = {}
    with restored(eng, big):
        for e in (eng, big):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        res = {eng: {}, big: {}}
        for ns in D.NS_PLAIN:
            src = [Guarded(torch, ns, a) for a in D.plain_inputs(ns, max(D.NT_PLAIN))[1:3] + D.plain_inputs(ns, max(D.NT_PLAIN))[:1]]
            for nt in D.NT_PLAIN:
                g, xs, zs, xt, zt, vc = D.plain_inputs(ns, nt)
                ref = D.cached_reference(("plain", ns, nt), (g, xs, zs, xt, zt, vc))
                tgt = [Guarded(torch, nt, a) for a in (xt, zt)]
                out = [Guarded(torch, nt), Guarded(torch, nt)]
                for e in (eng, big):
                    for tpl in D.TPLS:
                        for s in D.SPLITS_PLAIN:
                            what = ("induce_dev", "tile1024" if e is big else "product", ns, nt, tpl, s)
                            e.set_tuning(tpl, s)
                            for o in out:
                                o.arm()
                            e.induce_dev(src[0].ptr(), src[1].ptr(), src[2].ptr(), ns, tgt[0].ptr(), tgt[1].ptr(), nt, vc,
                                         out[0].ptr(), out[1].ptr())
                            torch.cuda.synchronize()
                            got = (out[0].read(what), out[1].read(what))
                            _check(worst, "plain", got, ref, what)
                            res[e][(ns, nt, tpl, s)] = got
                # the host entry is the same launch on uploaded copies: the same bits
                for tpl, s in ((1, 0), (2, 3), (4, 5)):
                    eng.set_tuning(tpl, s)
                    assert _same_bits(eng.induce_f32(g, xs, zs, xt, zt, vc), res[eng][(ns, nt, tpl, s)]), ("induce_f32", ns, nt, tpl, s)
        shapes = [(ns, nt) for ns in D.NS_PLAIN for nt in D.NT_PLAIN]
        _cross_tpl_bits(res[big], shapes, D.SPLITS_PLAIN, "plain, 1024-source tile")
        for shape in shapes:
            for s in D.SPLITS_PLAIN:
                for tpl in (2, 4):       # the product's 1024-tile launches are the measurement build's
                    assert _same_bits(res[eng][shape + (tpl, s)], res[big][shape + (tpl, s)]), (shape, tpl, s)
        # the first 257 targets of the nt = 1025 launch are the nt = 257 launch (the knobs held fixed)
        for e in (eng, big):
            for ns in D.NS_PLAIN:
                for tpl in D.TPLS:
                    for s in D.SPLITS_PLAIN[1:]:
                        a, b = res[e][(ns, 1025, tpl, s)], res[e][(ns, 257, tpl, s)]
                        assert _same_bits((a[0][:257], a[1][:257]), b), ("prefix", ns, tpl, s)
    print(f"plain fp32: worst error / max|u| = {worst['plain']:.2e} (bound {D.TOL['plain']:.0e})")


@pytest.mark.parametrize("inputs", ["cloud", "sheet"])
def test_hilo_host_entry_by_value(eng, exp, inputs):
    """pair_f32<1, 256 | 1024, true>, <2 | 4, 1024, true> through induce(..., 'f32x2'): on the plain table's cloud, and on a sheet
    at x0 = -50 with neighbours 1e-3 apart"""
    big = exp("tile1024")
    worst = {}
    make = D.plain_inputs if inputs == "cloud" else D.hilo_sheet_inputs
    with restored(eng, big):
        res = {eng: {}, big: {}}
        for ns in D.NS_PLAIN:
            for nt in D.NT_PLAIN:
                g, xs, zs, xt, zt, vc = make(ns, nt)
                ref = D.cached_reference(("plain" if inputs == "cloud" else "hilo_sheet", ns, nt), (g, xs, zs, xt, zt, vc))
                for e in (eng, big):
                    for tpl in D.TPLS:
                        for s in D.SPLITS_PLAIN:
                            e.set_tuning(tpl, s)
                            got = e.induce(g, xs, zs, xt, zt, vc, precision="f32x2")
                            _check(worst, "hilo", got, ref, (inputs, "tile1024" if e is big else "product", ns, nt, tpl, s))
                            res[e][(ns, nt, tpl, s)] = got
        shapes = [(ns, nt) for ns in D.NS_PLAIN for nt in D.NT_PLAIN]
        _cross_tpl_bits(res[big], shapes, D.SPLITS_PLAIN, "hi+lo, 1024-source tile")
        if inputs == "cloud":        # (the cloud's targets are a prefix of the longer cloud's)
            for ns in D.NS_PLAIN:
                for tpl in D.TPLS:
                    for s in D.SPLITS_PLAIN[1:]:
                        a, b = res[eng][(ns, 1025, tpl, s)], res[eng][(ns, 257, tpl, s)]
                        assert _same_bits((a[0][:257], a[1][:257]), b), ("prefix", ns, tpl, s)
    print(f"hi+lo, {inputs}: worst error / max|u| = {worst['hilo']:.2e} (bound {D.TOL['hilo']:.0e})")


@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_local_origin_host_entry_by_value(eng, exp, layout):
    """pair_f32<1, 256 | 1024, false, 0, true>, <2 | 4, 1024, false, 0, true> through induce(..., 'f32') with both sides from 2048
    points on: a last origin block of one member (its odd class has none), block edges, Morton gather and scatter"""
    big = exp("tile1024")
    worst = {}
    with restored(eng, big):
        res = {}
        for ns, nt in D.local_shapes(layout):
            g, xs, zs, xt, zt, vc = D.local_inputs(layout, ns, nt)
            assert (xt is xs) == (layout == "self")
            ref = D.cached_reference((layout, ns, nt), (g, xs, zs, xt, zt, vc))
            for e in (eng, big):
                for tpl in D.TPLS:
                    for s in D.SPLITS_LOCAL:
                        e.set_tuning(tpl, s)
                        got = e.induce(g, xs, zs, xt, zt, vc, precision="f32")
                        _check(worst, "local", got, ref, (layout, "tile1024" if e is big else "product", ns, nt, tpl, s))
                        if e is big:
                            res[(ns, nt, tpl, s)] = got
        _cross_tpl_bits(res, D.local_shapes(layout), D.SPLITS_LOCAL, "local origins, 1024-source tile, " + layout)
    print(f"local origins, {layout}: worst error / max|u| = {worst['local']:.2e} (bound {D.TOL['local']:.0e})")


def test_float64_kernels_by_value_and_the_packed_few_targets_kernel_bit_for_bit(eng, exp):
    """pair_f64_few<128> at every group-count boundary (split counts that are and are not multiples of the group count),
    pair_f64<128>, the hand-over at 129 targets, finish_sum<double>; wake_induce_on_points from an odd first source; the packed
    kernel's slab is the unpacked kernel's, bit for bit (the claim at pair_f64_few)"""
    packed, unpacked = exp("few_packed"), exp("few_unpacked")
    worst = {}
    with restored(eng, packed, unpacked):
        for ns in D.NS_F64:
            g, xs, zs = D.f64_inputs(ns, max(D.NT_F64))[:3]
            eng.wake_clear()
            eng.wake_append(np.r_[np.full(D.WAKE_SRC_FIRST, 7.0), xs], np.r_[np.full(D.WAKE_SRC_FIRST, 7.0), zs],
                            np.r_[np.full(D.WAKE_SRC_FIRST, 1e3), g])         # (a source that is wrongly read is not missed)
            for nt in D.NT_F64:
                g, xs, zs, xt, zt, vc = D.f64_inputs(ns, nt)
                ref = D.cached_reference(("f64", ns, nt), (g, xs, zs, xt, zt, vc))
                for s in D.SPLITS_F64:
                    for e in (eng, packed, unpacked):
                        e.set_tuning(0, s)
                    got = eng.induce(g, xs, zs, xt, zt, vc, precision="f64")
                    _check(worst, "f64", got, ref, ("induce f64", ns, nt, s))
                    wk = eng.wake_induce_on_points(D.WAKE_SRC_FIRST, ns, xt, zt, vc)
                    assert _same_bits(wk, got), ("wake_induce_on_points", ns, nt, s)
                    a, b = (e.induce(g, xs, zs, xt, zt, vc, precision="f64") for e in (packed, unpacked))
                    assert _same_bits(a, b) and _same_bits(a, got), ("LUDVM_FEW_PACKED 1 | 0", ns, nt, s)
        eng.wake_clear()
    print(f"float64: worst error / max|u| = {worst['f64']:.2e} (bound {D.TOL['f64']:.0e})")


def test_float64_512_source_tile_by_value(eng, exp):
    """pair_f64<512>: forced at small sizes by the measurement build, and the one product pair across small_tile_max_f64"""
    e512 = exp("f64_tile512")
    worst = {}
    with restored(eng, e512):
        for ns in D.NS_F64_512:
            for nt in D.NT_F64_512:
                g, xs, zs, xt, zt, vc = D.f64_inputs(ns, nt)
                ref = D.cached_reference(("f64", ns, nt), (g, xs, zs, xt, zt, vc))
                for s in D.SPLITS_F64:
                    e512.set_tuning(0, s)
                    _check(worst, "f64", e512.induce(g, xs, zs, xt, zt, vc, precision="f64"), ref, ("tile 512", ns, nt, s))
        for ns, nt in D.F64_PRODUCT_PAIR:
            g, xs, zs, xt, zt, vc = D.f64_inputs(ns, nt)
            ref = D.cached_reference(("f64", ns, nt), (g, xs, zs, xt, zt, vc))
            _check(worst, "f64", eng.induce(g, xs, zs, xt, zt, vc, precision="f64"), ref, ("product", ns, nt))
    print(f"float64, 512-source tile: worst error / max|u| = {worst['f64']:.2e} (bound {D.TOL['f64']:.0e})")


def test_fused_euler_step_by_value_with_guards(eng, exp):
    """advect_dev: the pair kernels with their results in the slab (one split included) and finish_advect_f32 with its t_first,
    dt = 1 so that the product is exact: |x_out - (x + u_ref)| <= 1e-5 max|u_ref| + 2^-22 (one fp32 ulp of |x| < 4: the sum's
    rounding)"""
    import torch
    big = exp("tile1024")
    worst = 0.0
    with restored(eng, big):
        for e in (eng, big):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        for ns in D.NS_ADVECT:
            g, xs, zs, vc = D.advect_inputs(ns)
            assert np.abs(xs).max() < 4 and np.abs(zs).max() < 4
            src = [Guarded(torch, ns, a) for a in (xs, zs, g)]
            for t_first, nt in D.advect_ranges(ns):
                sl = slice(t_first, t_first + nt)
                ur, wr = D.cached_reference(("advect", ns, t_first, nt), (g, xs, zs, xs[sl], zs[sl], vc))
                bound = D.TOL["plain"] * max(np.abs(ur).max(), np.abs(wr).max()) + 2.0**-22
                out = [Guarded(torch, nt), Guarded(torch, nt)]
                res = {}
                for e in (eng, big):
                    for tpl in D.TPLS:
                        for s in D.SPLITS_ADVECT:
                            what = ("advect_dev", "tile1024" if e is big else "product", ns, t_first, nt, tpl, s)
                            e.set_tuning(tpl, s)
                            for o in out:
                                o.arm()
                            e.advect_dev(src[0].ptr(), src[1].ptr(), src[2].ptr(), ns, t_first, nt, vc, 1.0, out[0].ptr(), out[1].ptr())
                            torch.cuda.synchronize()
                            xo, zo = out[0].read(what), out[1].read(what)
                            err = max(np.abs(xo - (xs[sl] + ur)).max(), np.abs(zo - (zs[sl] + wr)).max())
                            worst = max(worst, err / bound)
                            assert err <= bound, (what, err, bound)
                            res[(e is big, tpl, s)] = (xo, zo)
                for s in D.SPLITS_ADVECT:
                    for tpl in (2, 4):
                        assert _same_bits(res[(True, 1, s)], res[(True, tpl, s)]), ("TPL 1 vs", tpl, ns, t_first, nt, s)
                        assert _same_bits(res[(False, tpl, s)], res[(True, tpl, s)]), (tpl, ns, t_first, nt, s)
    print(f"fused Euler step: worst error / bound = {worst:.2f}")


def test_flowfield_grids_by_value_with_guards(eng, exp):
    """host flowfield (local origins) and flowfield_dev (plain, guarded buffers) on small grids: the 2 x 4 patch kernels at 1, 2, 3
    and 5 rows, the generic path (rows of 1, 3, 5, 37 points, or a forced TPL), and through the measurement build the row kernels,
    the 1024-source tile and the 4 x 4 patch -- which return the 2 x 4 patch's bits"""
    import torch
    builds = ("tile1024", "grid_row", "grid_row_tile1024", "grid_patch4_tile1024")
    engines = {"product": eng, **{b: exp(b) for b in builds}}
    worst = {}
    args = (D.GRID_XMIN, D.GRID_ZMIN, D.GRID_DR)
    with restored(*engines.values()):
        for e in engines.values():
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        for ns in D.NS_GRID:
            g, xs, zs, vc = D.grid_inputs(ns)
            src = [Guarded(torch, ns, a) for a in (xs, zs, g)]
            for nx, nz, tpls in D.grid_shapes():
                xt, zt = D.grid_points(nx, nz)
                ref = D.cached_reference(("grid", ns, nx, nz), (g, xs, zs, xt, zt, vc))
                out = [Guarded(torch, nx * nz), Guarded(torch, nx * nz)]
                res = {}
                for build, e in engines.items():
                    for tpl in (tpls if build == "product" else (0,)):
                        for s in D.SPLITS_GRID:
                            what = (build, ns, nx, nz, tpl, s)
                            e.set_tuning(tpl, s)
                            u, w = e.flowfield(*args, nx, nz, g, xs, zs, vc)
                            assert u.shape == (nx, nz)
                            _check(worst, "local", (u.ravel(), w.ravel()), ref, ("flowfield",) + what)
                            for o in out:
                                o.arm()
                            e.flowfield_dev(*args, nx, nz, src[0].ptr(), src[1].ptr(), src[2].ptr(), ns, vc, out[0].ptr(), out[1].ptr())
                            torch.cuda.synchronize()
                            got = (out[0].read(what), out[1].read(what))
                            _check(worst, "plain", got, ref, ("flowfield_dev",) + what)
                            res[(build, tpl, s)] = (u.ravel(), w.ravel()) + got
                if nz % 4 == 0:      # the forms of the grid kernel at one tile: the same bits
                    for s in D.SPLITS_GRID:
                        assert _same_bits(res[("grid_row", 0, s)], res[("product", 0, s)]), ("row | patch2, 256-source tile", ns, nx, nz, s)
                        for b in ("grid_row_tile1024", "grid_patch4_tile1024"):
                            assert _same_bits(res[(b, 0, s)], res[("tile1024", 0, s)]), (b, ns, nx, nz, s)
                for s in D.SPLITS_GRID:      # the generic path: targets per lane change no bit
                    if all((("product", tpl, s) in res) for tpl in D.TPLS):
                        for tpl in (2, 4):
                            assert _same_bits(res[("product", 1, s)], res[("product", tpl, s)]), ("generic, TPL 1 vs", tpl, ns, nx, nz, s)
    print(f"flow-field grids: worst error / max|u| = local {worst['local']:.2e}, plain {worst['plain']:.2e} (bound 1e-05)")
