"""GPU tier: parity of the HIP pair kernels with the oracle, through the C ABI (ctypes)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import c_oracle
from oracle import ludvm_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


def _rel(u, w, ur, wr):
    scale = max(np.abs(ur).max(), np.abs(wr).max(), 1e-300)
    return max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale


def _kernel_mass(g, xw, zw, xp, zp, vc):
    """sum_w |Gamma_w K_pw| per target: the natural error scale of an fp32 sum (tier T1)."""
    dx = xp[:, None] - xw[None, :]
    dz = zp[:, None] - zw[None, :]
    k = np.abs(g)[None, :] / (2 * np.pi * np.sqrt((dx * dx + dz * dz) ** 2 + vc**4))
    return (k * np.abs(dz)).sum(1), (k * np.abs(dx)).sum(1)


# Tolerances relative to max|u| of the call (tier T1).  Every G1 case has fewer than 2048 points on a side, and
# such a call runs in float64 whatever fp32 precision was asked for (ludvm_induce_f64: too few points to make 128-point
# origin classes compact, and nothing to gain from fp32 at that size) -- round 3 allowed 5e-4 / 2e-3 here for the random
# 1023-vortex clouds in fp32 on local origins.  hi+lo ('f32x2') and the plain-fp32 entry (below) do run fp32 kernels.
# "off50": coordinates offset by -50 with separations ~1e-3 -- plain fp32 positions lose the difference there.
TOL = {"f32": {"vc065": 1e-11, "vc0013": 1e-11, "off50": 1e-11},
       "f32x2": {"vc065": 1e-5, "vc0013": 1e-5, "off50": 1e-5},
       "f64": {"vc065": 1e-12, "vc0013": 1e-12, "off50": 1e-12}}


@pytest.mark.parametrize("precision", ["f32", "f32x2", "f64"])
def test_g1_golden_kats(eng, g1_cases, precision):
    for name, c in g1_cases.items():
        if "inviscid" in name:
            continue
        tag = "off50" if "off50" in name else ("vc0013" if name.endswith("vc0013") else "vc065")
        u, w = eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], float(c["v_core"]), precision=precision)
        assert u.dtype == np.float64 and u.shape == c["u"].shape
        err = _rel(u, w, c["u"], c["w"])
        fp32_kernels = precision == "f32x2" or (precision == "f32" and min(len(c["xw"]), len(c["xp"])) >= 2048)
        assert err <= (1e-5 if fp32_kernels else TOL[precision][tag]), (name, precision, err)
        if precision != "f64":
            mu, mw = _kernel_mass(c["g"].astype(float), c["xw"], c["zw"], c["xp"], c["zp"], float(c["v_core"]))
            lim = 1e-10 if not fp32_kernels else (1e-4 if precision == "f32" else 2e-6)
            assert np.all(np.abs(u - c["u"]) <= lim * mu + 1e-30), name
            assert np.all(np.abs(w - c["w"]) <= lim * mw + 1e-30), name


def test_g1_golden_kats_through_the_plain_fp32_entry(eng, g1_cases):
    """ludvm_induce_f32 (host float32 buffers: the caller's fp32 coordinates are used as they are, direct kernel) on the
    reference's KATs: 1e-5 of max|u| at v_core = 0.065, 5e-4 at v_core = 1.3e-3 with O(1) coordinates (SURVEY 8d T1 "without
    recentring"), and the loss SURVEY H2 predicts once the coordinates sit at -50."""
    tol = {"vc065": 1e-5, "vc0013": 5e-4, "off50": 5e-2}
    worst = {}
    for name, c in g1_cases.items():
        if "inviscid" in name:
            continue
        tag = "off50" if "off50" in name else ("vc0013" if name.endswith("vc0013") else "vc065")
        u, w = eng.induce_f32(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], float(c["v_core"]))
        err = _rel(u.astype(float), w.astype(float), c["u"], c["w"])
        assert err <= tol[tag], (name, err)
        worst[tag] = max(worst.get(tag, 0.0), err)
    assert worst["off50"] > 1e-4           # (what local origins, hi+lo positions and the float64 route are for)


def test_hilo_positions_remove_the_offset_cancellation(eng, g1_cases):
    c = g1_cases["p257x1023_off50_vc0013"]   # |x| ~ 55, separations ~ 1e-3, v_core = 1.3e-3
    e32 = _rel(*(a.astype(float) for a in eng.induce_f32(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 1.3e-3)), c["u"], c["w"])
    e2 = _rel(*eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 1.3e-3, precision="f32x2"), c["u"], c["w"])
    assert e2 < 1e-5 and 20 * e2 < e32


@pytest.mark.parametrize("precision", ["f32", "f32x2", "f64"])
def test_inviscid(eng, g1_cases, precision):
    c = g1_cases["p129x333_inviscid"]
    u, w = eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 0.0, precision=precision)
    assert _rel(u, w, c["u"], c["w"]) <= (1e-12 if precision == "f64" else 2e-5)
    # coincident source/target with v_core = 0: NaN exactly where the reference's 0/0 gives NaN
    c = g1_cases["p3x3_inviscid_self"]
    u, w = eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 0.0, precision=precision)
    assert np.array_equal(np.isnan(u), np.isnan(c["u"])) and np.array_equal(np.isnan(w), np.isnan(c["w"]))
    ok = ~np.isnan(c["u"])
    np.testing.assert_allclose(u[ok], c["u"][ok], rtol=1e-5, atol=1e-7)


def test_empty_and_ragged_shapes(eng):
    rng = np.random.default_rng(3)
    u, w = eng.induce([], [], [], [0.0, 1.0], [0.0, 1.0], 0.065)
    assert np.array_equal(u, [0, 0]) and np.array_equal(w, [0, 0])
    u, w = eng.induce([1.0], [0.0], [0.0], [], [], 0.065)
    assert u.shape == (0,) and w.shape == (0,)
    for ns in (1, 3, 1023, 1024, 1025, 4097):
        for nt in (1, 63, 255, 256, 257, 513, 1025):
            xs, zs, g = rng.uniform(-3, 0, ns), rng.uniform(-1, 1, ns), rng.standard_normal(ns)
            xt, zt = rng.uniform(-3, 0, nt), rng.uniform(-1, 1, nt)
            ur, wr = O.induced_velocity(g, xs, zs, xt, zt, 0.065)
            u, w = eng.induce(g, xs, zs, xt, zt, 0.065, precision="f64")
            assert _rel(u, w, ur, wr) <= 1e-12, (ns, nt)
            u, w = eng.induce_f32(g, xs, zs, xt, zt, 0.065)          # the fp32 direct kernels on the caller's coordinates
            assert _rel(u.astype(float), w.astype(float), ur, wr) <= 2e-5, (ns, nt)
    # both sides from 2048 points on: fp32 on local origins (these random arrays are taken in Morton order on the device)
    for ns, nt in ((2048, 2048), (2049, 4097), (4097, 2300), (30001, 2051)):
        xs, zs, g = rng.uniform(-3, 0, ns), rng.uniform(-1, 1, ns), rng.standard_normal(ns)
        xt, zt = rng.uniform(-3, 0, nt), rng.uniform(-1, 1, nt)
        ur, wr = c_oracle.induced_velocity(g, xs, zs, xt, zt, 0.065)
        u, w = eng.induce(g, xs, zs, xt, zt, 0.065, precision="f32")
        assert _rel(u, w, ur, wr) <= 1e-5, (ns, nt)


def test_a_non_finite_target_poisons_only_itself(eng):
    """The reference's sum gives NaN exactly at a target whose position is NaN and nowhere else (LUDVM.py:556-569).  fp32 on
    local origins refers a class of 128 targets to its middle member: when THAT one is not a number the class takes the
    coordinate origin instead -- on a compact (kept as stored) and on an unordered (Morton-ordered) target set."""
    rng = np.random.default_rng(8)
    ns = 3000
    xs, zs, g = rng.uniform(-3, 0, ns), rng.uniform(-1, 1, ns), rng.standard_normal(ns)
    for layout in ("sheet", "cloud"):
        nt = 5000
        xt = np.linspace(-3.0, 0.0, nt) if layout == "sheet" else rng.uniform(-3, 0, nt)
        zt = 0.1 * np.sin(3 * xt) if layout == "sheet" else rng.uniform(-1, 1, nt)
        bad = [128, 129, 2500]                    # 128 / 129: the middle members of block 0's two classes (as stored)
        xt[bad[0]], zt[bad[1]], xt[bad[2]] = np.nan, np.inf, -np.inf
        ok = np.ones(nt, bool)
        ok[bad] = False
        ur, wr = c_oracle.induced_velocity(g, xs, zs, xt[ok], zt[ok], 0.065)
        for prec in ("f32", "f32x2", "f64"):
            u, w = eng.induce(g, xs, zs, xt, zt, 0.065, precision=prec)
            assert not np.isfinite(u[bad[0]]) and not np.isfinite(w[bad[2]]), (layout, prec)
            assert np.isfinite(u[ok]).all() and np.isfinite(w[ok]).all(), (layout, prec, int((~np.isfinite(u[ok])).sum()))
            assert _rel(u[ok], w[ok], ur, wr) <= (1e-12 if prec == "f64" else 1e-5), (layout, prec)


def test_strided_and_integer_inputs(eng, g1_cases):
    c = g1_cases["p80x1_int_vc065"]       # circulation = np.array([1]) (int64), LUDVM.py:751
    assert c["g"].dtype.kind == "i"
    u, w = eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 0.065, precision="f64")
    assert _rel(u, w, c["u"], c["w"]) < 1e-12
    big = np.random.default_rng(1).uniform(-5, 0, (3, 2, 700))
    gam = np.random.default_rng(2).standard_normal(700)
    args = (gam[:650], big[1, 0, :650], big[1, 1, :650], big[2, 0, :300], big[2, 1, :300])
    assert not args[1].flags["C_CONTIGUOUS"] or args[1].base is not None
    ur, wr = O.induced_velocity(*args, 0.065)
    assert _rel(*eng.induce(*args, 0.065, precision="f64"), ur, wr) < 1e-12


def test_launch_shapes_agree_and_are_reproducible(eng):
    rng = np.random.default_rng(11)
    n = 20000
    xs, zs, g = rng.uniform(-10, 0, n), rng.uniform(-2, 2, n), rng.standard_normal(n) / n
    ur, wr = c_oracle.induced_velocity(g, xs, zs, xs, zs, 0.065)
    results = {}
    try:
        eng.set_symmetric(0)      # the property under test belongs to the direct kernel (no atomics)
        for tpl in (1, 2, 4):
            for splits in (1, 3, 16):
                eng.set_tuning(tpl, splits)
                u, w = eng.induce(g, xs, zs, xs, zs, 0.065, precision="f32")
                assert _rel(u, w, ur, wr) < 1e-5, (tpl, splits)
                u2, w2 = eng.induce(g, xs, zs, xs, zs, 0.065, precision="f32")
                assert np.array_equal(u, u2) and np.array_equal(w, w2)   # no atomics: bitwise reproducible
                results[(tpl, splits)] = (u, w)
    finally:
        eng.set_tuning(0, 0)
        eng.set_symmetric(1)
    # the launch shapes agree: a target's sum is formed by the same operations in the same order whatever the targets per
    # lane are (bitwise at equal splits); another split count is another partition into fp32 partial sums -- each within
    # 1e-5 of the reference, so within 2e-5 max|u| of each other
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    for splits in (1, 3, 16):
        for tpl in (2, 4):
            assert np.array_equal(results[(1, splits)][0], results[(tpl, splits)][0]), (tpl, splits)
            assert np.array_equal(results[(1, splits)][1], results[(tpl, splits)][1]), (tpl, splits)
    for tpl in (1, 2, 4):
        for sa, sb in ((1, 3), (1, 16), (3, 16)):
            for k in (0, 1):
                assert np.abs(results[(tpl, sa)][k] - results[(tpl, sb)][k]).max() <= 2e-5 * scale, (tpl, sa, sb)


def test_linearity_and_antisymmetry(eng):
    rng = np.random.default_rng(21)
    n = 5000
    xs, zs = rng.uniform(-10, 0, n), rng.uniform(-2, 2, n)
    g1, g2 = rng.standard_normal(n), rng.standard_normal(n)
    u1, w1 = eng.induce(g1, xs, zs, xs, zs, 0.065)
    u2, w2 = eng.induce(2.0 * g1, xs, zs, xs, zs, 0.065)
    assert np.array_equal(2.0 * u1, u2) and np.array_equal(2.0 * w1, w2)   # power-of-two scaling is exact
    ua, wa = eng.induce(g1 + g2, xs, zs, xs, zs, 0.065)
    ub, wb = eng.induce(g2, xs, zs, xs, zs, 0.065)
    assert np.abs(ua - (u1 + ub)).max() < 1e-4 * np.abs(ua).max()
    # K(i->j) = -K(j->i): the linear impulse of self-induction vanishes, sum_i G_i u_i = 0
    assert abs(np.sum(g1 * u1)) < 1e-5 * np.sum(np.abs(g1 * u1))
    assert abs(np.sum(g1 * w1)) < 1e-5 * np.sum(np.abs(g1 * w1))
    # a single vortex induces nothing on itself
    u, w = eng.induce([3.0], [0.5], [0.25], [0.5], [0.25], 0.065)
    assert u[0] == 0.0 and w[0] == 0.0


def test_host_entry_uses_symmetric_kernel_for_self_interaction(eng):
    rng = np.random.default_rng(41)
    n = 30000
    x, z, g = rng.uniform(-10, 0, n), rng.uniform(-2, 2, n), rng.standard_normal(n) / n
    ur, wr = c_oracle.induced_velocity(g, x, z, x, z, 0.065)
    try:
        for prec, tol in (("f32", 1e-5), ("f32x2", 2e-6)):
            eng.set_symmetric(0)
            ud, wd = eng.induce(g, x, z, x, z, 0.065, precision=prec)
            eng.set_symmetric(1)
            eng.kernel_timing(True)
            eng.kernel_time_ms(reset=True)
            us, ws = eng.induce(g, x, z, x, z, 0.065, precision=prec)      # same objects -> symmetric path
            _, launches = eng.kernel_time_ms(reset=True)
            eng.kernel_timing(False)
            assert launches == 1
            assert _rel(us, ws, ur, wr) < tol and _rel(ud, wd, ur, wr) < tol
            assert not np.array_equal(us, ud)                               # a different kernel did run
    finally:
        eng.set_symmetric(1)
        eng.kernel_timing(False)


def test_host_float32_entry(eng):
    rng = np.random.default_rng(4)
    xs, zs, g = rng.uniform(-10, 0, 3000), rng.uniform(-2, 2, 3000), rng.standard_normal(3000)
    xt, zt = rng.uniform(-10, 0, 700), rng.uniform(-2, 2, 700)
    u, w = eng.induce_f32(g, xs, zs, xt, zt, 0.065)
    assert u.dtype == np.float32
    ur, wr = O.induced_velocity(g.astype(np.float32).astype(float), xs.astype(np.float32).astype(float),
                                zs.astype(np.float32).astype(float), xt.astype(np.float32).astype(float),
                                zt.astype(np.float32).astype(float), 0.065)
    assert _rel(u, w, ur, wr) < 1e-5


def test_device_pointer_entries_with_torch(eng):
    import torch
    rng = np.random.default_rng(8)
    n = 30000
    x, z, g = (rng.uniform(-10, 0, n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32),
               (rng.standard_normal(n) / n).astype(np.float32))
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                       du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
        ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), x.astype(float),
                                           z.astype(float), 0.065)
        assert _rel(du.cpu().numpy(), dw.cpu().numpy(), ur, wr) < 1e-5
        # fused Euler step on a target sub-range
        lo, cnt = 1000, 12345
        xo, zo = torch.empty(cnt, device=dev), torch.empty(cnt, device=dev)
        eng.advect_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, lo, cnt, 0.065, 0.05, xo.data_ptr(), zo.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_allclose(xo.cpu().numpy(), x[lo:lo + cnt] + 0.05 * ur[lo:lo + cnt], rtol=0, atol=2e-6)
        np.testing.assert_allclose(zo.cpu().numpy(), z[lo:lo + cnt] + 0.05 * wr[lo:lo + cnt], rtol=0, atol=2e-6)
        # the shard step with a world of one is the same thing
        from ludvm_amd.sharded import HipShardKernel, ShardedWake
        for symmetric in (True, False):
            wake = ShardedWake(x, z, g, 0.065, 0.05, HipShardKernel(eng), dev, symmetric=symmetric)
            wake.step()
            xs1, zs1 = wake.positions()
            np.testing.assert_allclose(xs1, x + 0.05 * ur, rtol=0, atol=2e-6)
            np.testing.assert_allclose(zs1, z + 0.05 * wr, rtol=0, atol=2e-6)
            wake.step()   # second step reads the re-laid-out buffers
            assert np.isfinite(wake.positions()[0]).all()
    finally:
        eng.set_stream(None)


def test_flowfield_grid_and_vorticity(eng):
    rng = np.random.default_rng(13)
    ns = 2000
    xs, zs, g = rng.uniform(-10, 0, ns), rng.uniform(-2, 2, ns), rng.standard_normal(ns) / 50
    xmin, zmin, dr, nx, nz = -10.0, -4.0, 0.125, 80, 64
    u, w = eng.flowfield(xmin, zmin, dr, nx, nz, g, xs, zs, 0.065)
    assert u.shape == (nx, nz) and u.dtype == np.float32
    X, Z = np.meshgrid(np.arange(xmin, 0, dr), np.arange(zmin, 4, dr), indexing="ij")
    assert X.shape == (nx, nz)
    ur, wr = O.induced_velocity(g, xs, zs, X.ravel(), Z.ravel(), 0.065, rows_per_chunk=1024)
    assert _rel(u.ravel(), w.ravel(), ur, wr) < 1e-5
    ome = eng.vorticity(u, w, dr)
    omr = O.vorticity(u[None].astype(float), w[None].astype(float), X, Z)[0]
    np.testing.assert_allclose(ome, omr, rtol=0, atol=1e-4 * np.abs(omr).max())
    with pytest.raises(Exception):
        eng.vorticity(u[:1], w[:1], dr)


def test_grid_patch_kernels_equal_the_row_kernel_bit_for_bit():
    """Flow-field grids run with a patch of grid points per lane -- 4 x 4 from 2^20 grid points, 2 x 4 below (dx, dx^2
    and Gamma dx shared along each row, dz and Gamma dz along each column: 5.25 / 5.75 instead of 6.5 packed operations
    per two pairs and target); LUDVM_GRID_KERNEL = row | patch2 | patch4 forces one form (row: 4 points of one row per
    lane).  Same operations on the same operands in the same order -> the same bits, for row counts that are and are not
    multiples of the patch, one and several source splits, small- and large-tile source sets, local-origin sources."""
    import os
    from ludvm_amd import Engine, _ffi
    res = {}
    for kind in ("row", "patch2", "patch4", "patch"):
        os.environ["LUDVM_GRID_KERNEL"] = kind          # a switch of the measurement build (-DLUDVM_EXPERIMENTS)
        try:
            e = Engine(0, lib_path=_ffi.EXP_LIB_PATH)
        finally:
            del os.environ["LUDVM_GRID_KERNEL"]
        try:
            out = []
            r = np.random.default_rng(17)
            for ns, nx, nz in ((700, 37, 48), (20000, 64, 36), (3000, 1, 8), (5000, 301, 260), (20000, 1027, 1024)):
                xs, zs, g = r.uniform(-10, 0, ns) - 20.0, r.uniform(-2, 2, ns), r.standard_normal(ns) / 50
                u, w, ome = e.flowfield_rows(-30.0, -2.0, 0.0173, nx, nz, 0, nx, g, xs, zs, 0.065, vorticity=nx > 1)
                out.append((u, w, ome))
                if nx > 1000 and kind == "patch":
                    # a block of rows of a grid large enough for the 4 x 4 patch: its patches start at another row, the
                    # bits stay (what a GPU of several evaluates, ludvm_amd/distributed.py)
                    ub, wb, ob = e.flowfield_rows(-30.0, -2.0, 0.0173, nx, nz, 301, 405, g, xs, zs, 0.065)
                    assert np.array_equal(ub, u[301:706]) and np.array_equal(wb, w[301:706]) and np.array_equal(ob, ome[301:706])
            res[kind] = out
        finally:
            e.close()
    for kind in ("patch2", "patch4", "patch"):
        for a, b in zip(res[kind], res["row"]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), kind
            assert (a[2] is None and b[2] is None) or np.array_equal(a[2], b[2]), kind


def test_flowfield_row_blocks_are_bitwise_the_full_grid(eng):
    """ludvm_flowfield_rows_f32: any block of rows -- one row, ragged blocks, the grid's own edges -- is bit for bit what
    the whole-grid call returns for those rows, velocity and vorticity (halo rows are evaluated internally; the grid's
    first and last row keep the reference's one-sided differences, LUDVM.py:1233-1248)."""
    rng = np.random.default_rng(23)
    ns, nx, nz = 4000, 37, 44
    xs, zs, g = rng.uniform(-10, 0, ns) - 15.0, rng.uniform(-2, 2, ns), rng.standard_normal(ns) / 50
    args = (-25.0, -2.0, 0.07, nx, nz)
    u, w, ome = eng.flowfield_rows(*args, 0, nx, g, xs, zs, 0.065)
    uf, wf, of = eng.flowfield_vorticity(*args, g, xs, zs, 0.065)
    assert np.array_equal(u, uf) and np.array_equal(w, wf) and np.array_equal(ome, of)
    for first, count in ((0, 1), (0, 5), (5, 1), (6, 13), (19, 17), (36, 1), (30, 7), (12, 0)):
        ub, wb, ob = eng.flowfield_rows(*args, first, count, g, xs, zs, 0.065)
        assert ub.shape == (count, nz)
        assert np.array_equal(ub, u[first:first + count]) and np.array_equal(wb, w[first:first + count])
        assert np.array_equal(ob, ome[first:first + count]), (first, count)
    ub, wb, ob = eng.flowfield_rows(*args, 3, 4, g, xs, zs, 0.065, vorticity=False)
    assert ob is None and np.array_equal(ub, u[3:7])
    with pytest.raises(Exception):
        eng.flowfield_rows(*args, 30, 8, g, xs, zs, 0.065)        # rows outside the grid


def test_self_interaction_calls_small_and_large_through_the_host_entry(eng):
    """LUDVM.induced_velocity called with the same arrays as sources and targets (what the reference's roll-up passes,
    LUDVM.py:1105): uploaded once; small calls take the packed path, large ones the symmetric kernel; every precision
    against the oracle, and repeated calls return the same bits."""
    rng = np.random.default_rng(29)
    for n, tol32 in ((700, 1e-5), (30000, 1e-5)):
        x, z, g = rng.uniform(-10, 0, n) - 30.0, rng.uniform(-2, 2, n), rng.standard_normal(n) / n
        ur, wr = c_oracle.induced_velocity(g, x, z, x, z, 0.065)
        for prec, tol in (("f32", tol32), ("f32x2", 1e-5), ("f64", 1e-12)):
            u, w = eng.induce(g, x, z, x, z, 0.065, precision=prec)
            assert _rel(u, w, ur, wr) < tol, (n, prec)
            u2, w2 = eng.induce(g, x, z, x, z, 0.065, precision=prec)
            assert np.array_equal(u, u2) and np.array_equal(w, w2), (n, prec)


def test_flowfield_over_a_far_wake_keeps_1e5(eng):
    """The reference evaluates flowfield in float64 (LUDVM.py:1206, :1216-1217).  Over a config-2 wake -- |x| ~ 50,
    vortices 1e-3 apart, v_core = 1.3e-3 -- plain fp32 coordinates lose three digits; the host entry
    stores the sources as offsets from the origin of their 256-source block and refers the float64 grid points to
    those origins: 1e-5 of max|u| against the oracle, at the speed of the plain fp32 grid kernel.  The fused
    velocity + vorticity call returns exactly what the two separate calls return."""
    rng = np.random.default_rng(41)
    ns = 30000
    xs = -50.0 + np.sort(rng.uniform(0, 30, ns))
    zs = 0.3 * np.sin(0.7 * xs) + 1e-3 * rng.standard_normal(ns)
    g = rng.standard_normal(ns) * 1e-3
    vc = 1.3e-3
    import torch
    dev = torch.device("cuda", 0)
    for k, (xmin, zmin, dr, nx, nz) in enumerate(((-35.0, -0.6, 0.01, 96, 120), (-30.3, 0.1, 0.0013, 41, 37))):   # nz % 4 == 0 and not
        u, w = eng.flowfield(xmin, zmin, dr, nx, nz, g, xs, zs, vc)
        X, Z = np.meshgrid(xmin + np.arange(nx) * dr, zmin + np.arange(nz) * dr, indexing="ij")
        ur, wr = c_oracle.induced_velocity(g, xs, zs, X.ravel(), Z.ravel(), vc)
        err = _rel(u.ravel(), w.ravel(), ur, wr)
        assert err < 1e-5, (nx, nz, err)
        u2, w2, ome2 = eng.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, xs, zs, vc)
        assert np.array_equal(u, u2) and np.array_equal(w, w2)
        assert np.array_equal(ome2, eng.vorticity(u, w, dr))
        if k == 0:
            # the grid that crosses the sheet, with plain fp32 coordinates for comparison (device fp32 entry: the caller's
            # layout is used as it is)
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            try:
                dx, dz, dg = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (xs, zs, g))
                du, dw = torch.empty(nx * nz, device=dev), torch.empty(nx * nz, device=dev)
                eng.flowfield_dev(xmin, zmin, dr, nx, nz, dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), ns, vc, du.data_ptr(),
                                  dw.data_ptr())
                torch.cuda.synchronize()
                plain = _rel(du.cpu().numpy(), dw.cpu().numpy(), ur, wr)
                assert plain > 20 * err, (plain, err)
            finally:
                eng.set_stream(None)


def _cloud(n, seed=77):
    """n vortices uniformly random in a 10 x 4 box centred at x = -55: the order a caller's array or a turbulence cloud
    (LUDVM.generate_flowfield_turbulence, LUDVM.py:98-130) has -- none -- at the distance config 2's wake ends at."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-60.0, -50.0, n), rng.uniform(-2.0, 2.0, n), rng.standard_normal(n) * 1e-2


@pytest.mark.parametrize("n,vc,route", [(100_000, 1.3e-3, "f32x2"), (1_000_000, 1.3e-3, "f32x2"), (1_000_000, 5e-3, "f32")])
def test_fp32_accuracy_does_not_depend_on_the_callers_order(eng, n, vc, route):
    """VERDICT r3 item 3.  The reference's float64 sum (LUDVM.py:565-569) is order-independent; the fp32 kernels' local
    origins need compact 256-vortex blocks, which a shed wake's stored order gives and a random cloud's does not: measured
    before [MI355X, profiles/r04_unordered_accuracy.txt] 1.3e-4 (1e5 vortices) / 5e-5 (1e6) of max|u| at v_core = 1.3e-3,
    4.7e-4 / 1.7e-4 on 512 separate targets.  Now: sources and targets of a host-pointer call are taken in Morton order on
    the device when their own order is not compact (results back in the caller's order), sides of fewer than 2048 points run
    in float64, sets too sparse for their core (mean class extent > 150 v_core in Morton order -- calibrated in
    profiles/r04_extent_rule_calibration.txt; 4096 targets in this box; 1e6 vortices at v_core = 1.3e-3 sit at 267) take hi+lo
    positions, and the resident wake is told the order and the extent (ludvm_spatial_order).  1e-5 of max|u| on sampled
    targets against the C oracle: symmetric and direct kernel, self-interaction and separate targets, stateless call and
    wake roll-up; `route` = what the rule picks for the wake (1e6 vortices at v_core = 5e-3: fp32 in Morton order)."""
    x, z, g = _cloud(n)
    rng = np.random.default_rng(3)
    sel = rng.choice(n, 512, replace=False)
    ur, wr = c_oracle.induced_velocity(g, x, z, x[sel], z[sel], vc)
    try:
        scale = None
        for sym in (1, 0):
            eng.set_symmetric(sym)
            u, w = eng.induce(g, x, z, x, z, vc, precision="f32")
            if scale is None:
                scale = max(np.abs(u).max(), np.abs(w).max())         # max|u| over ALL vortices (good to 1e-5 by this very test)
                assert scale > 0.5 * max(np.abs(ur).max(), np.abs(wr).max())
            err = max(np.abs(u[sel] - ur).max(), np.abs(w[sel] - wr).max()) / scale
            assert err < 1e-5, (n, sym, err)
        eng.set_symmetric(1)
        # separate targets: 4096 of them (too sparse in any order: hi+lo) and 512 (fewer than 2048: float64, or hi+lo at 1e6 sources)
        big = rng.choice(n, 4096, replace=False)
        ub, wb = c_oracle.induced_velocity(g, x, z, x[big], z[big], vc)
        u, w = eng.induce(g, x, z, x[big].copy(), z[big].copy(), vc, precision="f32")
        assert max(np.abs(u - ub).max(), np.abs(w - wb).max()) / scale < 1e-5
        u, w = eng.induce(g, x, z, x[sel].copy(), z[sel].copy(), vc, precision="f32")
        # 512 targets: float64 while the call is small as a whole (<= 2^28 pairs), hi+lo positions beyond (round 5)
        assert max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale < (1e-11 if 512 * n <= 2**28 else 2e-6)
        # the resident wake keeps the caller's slots, so the caller stores the cloud in the order the engine names
        # (and picks hi+lo positions when even that order leaves the classes too wide for the core, as LUDVM.time_loop does)
        order, reordered, extent = eng.spatial_order(x, z, with_extent=True)
        assert reordered and np.array_equal(np.sort(order), np.arange(n))
        assert 0.3 * np.sqrt(128 * 40.0 / n) < extent < 3 * 2 * np.sqrt(128 * 40.0 / n)      # ~ 2 sides of a 128-point cell
        prec = "f32x2" if extent > 150 * vc else "f32"
        assert prec == route
        slot = np.empty(n, np.int64)
        slot[order] = np.arange(n)
        for sym in (1, 0):
            eng.set_symmetric(sym)
            eng.wake_clear()
            eng.wake_append(x[order], z[order], g[order])
            u, w = eng.wake_advect(2.0 ** -10, [], [], [], vc, precision=prec, return_velocity=True)
            err = max(np.abs(u[slot[sel]] - ur).max(), np.abs(w[slot[sel]] - wr).max()) / scale
            assert err < 1e-5, (n, sym, err)
        # the order is a pure function of the positions
        order2, _ = eng.spatial_order(x, z)
        assert np.array_equal(order, order2)
    finally:
        eng.set_symmetric(1)
        eng.wake_clear()


@pytest.mark.parametrize("n", [8192, 20000])
def test_a_thin_sheet_near_the_extent_bound_keeps_its_tier_in_its_own_order_and_in_a_scrambled_one(eng, n):
    """ADVICE r5 (order.hip:77).  Two thresholds decide a LUDVM_PREC_F32 call's route: the thin-set rule (class extents within
    3 x of a line across the bounding box: the given order stays, no keys, no sort) and the extent bound (mean class extent
    <= 300 v_core for a set kept as given, 150 v_core in Morton order; beyond: hi+lo positions).  The calibration of round 4
    covered Morton-ordered clouds and config 2's wake; this pins a SHEET just inside both lines: a wavy sheet stored along
    itself whose mean class extent is ~280 v_core -- kept as given (identity order), fp32 on local origins, 1e-5 of max|u|
    against the float64 oracle on every point -- and the same sheet stored in four interleaved strands (classes span 4 x the
    line bound: over the 3 x rule), which takes the sort and keeps the tier too."""
    vc = 1.3e-3
    s = np.arange(n, dtype=np.float64)
    spacing = 280.0 * vc / 256.0 / 1.02                  # a class = every other one of 256 consecutive points
    x = -40.0 + spacing * s
    z = 0.02 * np.sin(2 * np.pi * s / 2000.0)            # gentle: ~2 % on the class extent
    g = np.random.default_rng(11).standard_normal(n) * 1e-3
    ur, wr = c_oracle.induced_velocity(g, x, z, x, z, vc)
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    order, reordered, extent = eng.spatial_order(x, z, with_extent=True)
    assert not reordered and np.array_equal(order, np.arange(n))
    assert 250 * vc < extent < 300 * vc, extent / vc     # just inside the bound of a set that is compact as given
    try:
        for sym in (1, 0):
            eng.set_symmetric(sym)
            u, w = eng.induce(g, x, z, x, z, vc, precision="f32")
            err = max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale
            assert err < 1e-5, (n, sym, err)
        # four interleaved strands: stored point k is sheet point 4 (k mod n/4) + k // (n/4)
        perm = np.arange(n).reshape(n // 4, 4).T.ravel()
        xp, zp, gp = x[perm].copy(), z[perm].copy(), g[perm].copy()
        order, reordered, extent_p = eng.spatial_order(xp, zp, with_extent=True)
        assert reordered and np.array_equal(np.sort(order), np.arange(n))
        assert extent_p < 1.3 * extent                   # Morton order of a line is the line again, up to key resolution
        for sym in (1, 0):
            eng.set_symmetric(sym)
            u, w = eng.induce(gp, xp, zp, xp, zp, vc, precision="f32")
            # (150 v_core applies to a reordered set: at ~280 this one takes hi+lo positions -- either way the tier holds)
            err = max(np.abs(u - ur[perm]).max(), np.abs(w - wr[perm]).max()) / scale
            assert err < 1e-5, (n, sym, err)
    finally:
        eng.set_symmetric(1)


def test_a_shed_wake_keeps_its_order_and_its_bits(eng):
    """The spatial order applies only where the given order is not compact: a shed wake -- single sheet, the alternating
    TEV / LEV order, rolled up -- is evaluated as stored (ludvm_spatial_order: identity), so its results are the bits they
    were before the order existed; a cloud that is ALREADY in Morton order is left alone as well."""
    from test_gpu_wake import _late_time_wake
    rng = np.random.default_rng(5)
    for layout in ("sheet", "interleaved"):
        x, z = _late_time_wake(layout, 40000, rng)
        order, reordered = eng.spatial_order(x, z)
        assert not reordered and np.array_equal(order, np.arange(40000)), layout
    # a sheet wound into a spiral (a rolled-up starting vortex): compact along the sheet, though not monotone in space
    s = np.linspace(0.0, 1.0, 30000)
    x, z = -40.0 + (0.02 + s) * np.cos(40 * s), (0.02 + s) * np.sin(40 * s)
    assert not eng.spatial_order(x, z)[1]
    # fewer than 2048 points: never
    assert not eng.spatial_order(*_cloud(2000)[:2])[1]
    xc, zc, _ = _cloud(50000)
    order, reordered = eng.spatial_order(xc, zc)
    assert reordered
    assert not eng.spatial_order(xc[order], zc[order])[1]
    # odd sizes, degenerate sets: always a permutation; points on a line or all in one place need no order
    for n in (2048, 2049, 65537, 300_001):
        xo, zo, _ = _cloud(n, seed=n)
        order, reordered = eng.spatial_order(xo, zo)
        assert reordered and np.array_equal(np.sort(order), np.arange(n)), n
        # neighbours in the order are neighbours in space: the mean step is a few point spacings, not the box size
        step = np.hypot(np.diff(xo[order]), np.diff(zo[order])).mean()
        assert step < 3.0 * np.sqrt(40.0 / n) and step < 0.1 * np.hypot(np.diff(xo), np.diff(zo)).mean(), (n, step)
    line = np.linspace(-60.0, -50.0, 5000)
    assert not eng.spatial_order(line, np.zeros(5000))[1]
    assert not eng.spatial_order(np.full(5000, -55.0), np.full(5000, 0.25))[1]
    shuffled = np.random.default_rng(2).permutation(line)
    order, reordered = eng.spatial_order(shuffled, np.zeros(5000))          # a shuffled line IS put back in order
    assert reordered and np.all(np.diff(shuffled[order]) >= -10.0 / 65535)


@pytest.mark.parametrize("vc,tol", [(0.01, 1e-5), (1.3e-3, 3e-7)])
def test_flowfield_over_an_unordered_cloud_keeps_1e5(eng, vc, tol):
    """LUDVM.flowfield over a turbulence cloud (sources in no order).  v_core = 0.01: the host entry takes the sources in
    Morton order (the sum over sources does not care), the float64 grid points are referred to compact source classes.
    v_core = 1.3e-3: 2e5 sources in a 10 x 4 box are too sparse for that core in ANY order (mean class extent ~600 v_core;
    ctx.hpp, too_sparse) and the grid kernels have no hi+lo variant: the rows are evaluated in float64 and
    returned as float32."""
    x, z, g = _cloud(200_000, seed=9)
    xmin, zmin, dr, nx, nz = -55.3, -0.2, 0.004, 48, 64
    u, w = eng.flowfield(xmin, zmin, dr, nx, nz, g, x, z, vc)
    assert u.dtype == np.float32
    X, Z = np.meshgrid(xmin + np.arange(nx) * dr, zmin + np.arange(nz) * dr, indexing="ij")
    ur, wr = c_oracle.induced_velocity(g, x, z, X.ravel(), Z.ravel(), vc)
    assert _rel(u.ravel(), w.ravel(), ur, wr) < tol
    extent = eng.spatial_order(x, z, with_extent=True)[2]
    assert (extent > 150 * vc) == (vc < 0.005)
    # the fused call (velocity + vorticity) takes the same route and returns the same velocities
    u2, w2, ome2 = eng.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, x, z, vc)
    assert np.array_equal(u, u2) and np.array_equal(w, w2) and np.isfinite(ome2).all()


def test_flowfield_float64_mode_and_row_blocks(eng):
    """ludvm_flowfield_rows_f64: float64 pair sums, grid coordinates and stencil -- the oracle's fields (the reference's
    arithmetic, LUDVM.py:1206-1292) to 1e-12 of their maxima, vorticity included; any block of rows is bit for bit the
    whole-grid call; no sources gives zeros."""
    rng = np.random.default_rng(23)
    ns, nx, nz = 1500, 37, 52
    xs, zs, g = rng.uniform(-3, 0, ns), rng.uniform(-1, 1, ns), rng.standard_normal(ns) / ns
    xmin, zmin, dr, vc = -3.2, -1.1, 0.043, 0.065
    u, w, ome = eng.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, xs, zs, vc, precision="f64")
    assert u.dtype == np.float64 and u.shape == (nx, nz)
    x1, z1 = xmin + np.arange(nx) * dr, zmin + np.arange(nz) * dr
    X, Z = np.meshgrid(x1, z1, indexing="ij")
    ur, wr = O.induced_velocity(g, xs, zs, X.ravel(), Z.ravel(), vc)
    ur, wr = ur.reshape(nx, nz), wr.reshape(nx, nz)
    orr = O.vorticity(ur[None], wr[None], X, Z)[0]
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    assert np.abs(u - ur).max() <= 1e-12 * scale and np.abs(w - wr).max() <= 1e-12 * scale
    assert np.abs(ome - orr).max() <= 1e-10 * np.abs(orr).max()
    for first, count in ((0, 1), (0, 7), (5, 20), (36, 1), (30, 7)):
        ub, wb, ob = eng.flowfield_rows(xmin, zmin, dr, nx, nz, first, count, g, xs, zs, vc, precision="f64")
        assert np.array_equal(ub, u[first:first + count]) and np.array_equal(wb, w[first:first + count])
        assert np.array_equal(ob, ome[first:first + count])
    u0, w0, o0 = eng.flowfield_vorticity(xmin, zmin, dr, 5, 6, [], [], [], vc, precision="f64")
    assert not u0.any() and not w0.any() and not o0.any()


def test_fp32_flowfield_vorticity_against_the_float64_oracle_at_config5_resolution(eng):
    """The reference differences float64 fields (LUDVM.py:1224-1292); the fp32 flow field differences sums that carry
    ~1e-6 of max|u| of rounding, and the stencil divides by 2 dr: at BASELINE config 5's dr = 8 / 4096 that is a factor
    256.  A 64 x 64 patch of that grid inside a 1e5-vortex synthetic wake against the oracle's float64 fields and THEIR
    stencil: u, w to 3e-6 of max|u| (measured 1e-6), vorticity to 2e-4 of max|omega| (measured ~7e-5: the stated accuracy of
    ome_ff in fp32; a float64 run has the reference's)."""
    from oracle import c_oracle
    rng = np.random.default_rng(20260101)
    n = 100_000
    xs, zs, g = rng.uniform(-10, 0, n), rng.uniform(-2, 2, n), rng.standard_normal(n) / n
    dr, nx, nz, vc = 8.0 / 4096, 64, 64, 0.065
    xmin, zmin = -8.0 + 1800 * dr, -4.0 + 2100 * dr            # a patch of config 5's grid, inside the wake
    u, w, ome = eng.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, xs, zs, vc)
    x1, z1 = xmin + np.arange(nx) * dr, zmin + np.arange(nz) * dr
    X, Z = np.meshgrid(x1, z1, indexing="ij")
    ur, wr = c_oracle.induced_velocity(g, xs, zs, X.ravel(), Z.ravel(), vc)
    ur, wr = ur.reshape(nx, nz), wr.reshape(nx, nz)
    orr = O.vorticity(ur[None], wr[None], X, Z)[0]
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    ev = max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale
    eo = np.abs(ome - orr).max() / np.abs(orr).max()
    print(f"fp32 flow field at dr = 8/4096: velocity error {ev:.2e} of max|u|, vorticity error {eo:.2e} of max|omega|")
    assert ev <= 3e-6 and eo <= 2e-4, (ev, eo)
    # the float64 mode on the same patch: the oracle's vorticity to rounding
    u64, w64, o64 = eng.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, xs, zs, vc, precision="f64")
    assert np.abs(o64 - orr).max() <= 1e-9 * np.abs(orr).max()


def test_flowfield_row_blocks_with_halo_equal_the_full_grid(eng):
    """Multi-GPU flow field on one GPU: the row blocks of 3 owners (each with its halo rows) reproduce
    the single-launch fields bit for bit in (u, w) and in the vorticity."""
    import torch
    from ludvm_amd.sharded import HipFlowfieldKernel, ShardedFlowfield, flowfield_rows
    rng = np.random.default_rng(5)
    ns, nx, nz, dr = 3000, 50, 33, 0.2
    dev = torch.device("cuda", 0)
    xs, zs, gs = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in
                  (rng.uniform(-10, 0, ns), rng.uniform(-2, 2, ns), rng.standard_normal(ns) / 50))
    ff = ShardedFlowfield(HipFlowfieldKernel(eng), dev)
    try:
        u, w, ome = ff.compute(-10.0, -3.0, dr, nx, nz, xs, zs, gs, 0.065)     # world of one: the full grid
        assert u.shape == (nx, nz)
        for world in (3, 7):
            for rank in range(world):
                ff.world, ff.rank = world, rank
                ub, wb, ob = ff.compute(-10.0, -3.0, dr, nx, nz, xs, zs, gs, 0.065)
                r0, r1 = flowfield_rows(nx, world, rank)
                # grid x of a block row = (xmin + h0*dr) + i*dr instead of xmin + (h0+i)*dr (double rounding),
                # and a different launch shape sums the sources in a different order
                assert torch.allclose(ub, u[r0:r1], rtol=0, atol=1e-5 * float(u.abs().max()))
                assert torch.allclose(wb, w[r0:r1], rtol=0, atol=1e-5 * float(w.abs().max()))
                assert torch.allclose(ob, ome[r0:r1], rtol=0, atol=1e-3 * float(ome.abs().max()))
    finally:
        eng.set_stream(None)


def test_error_reporting(eng):
    from ludvm_amd import LudvmHipError
    eng.wake_clear()
    with pytest.raises(LudvmHipError) as ei:
        eng.wake_read(0, 5)
    assert ei.value.code == 1 and "wake" in str(ei.value)
    with pytest.raises(LudvmHipError):
        eng.set_tuning(3, 0)
    with pytest.raises(ValueError):
        eng.induce([1.0, 2.0], [0.0], [0.0], [0.0], [0.0], 0.065)


def test_full_size_config3_properties(eng):
    """N = 1e6 all-pairs (BASELINE config 3), direct and symmetric kernels: sampled targets against the
    C oracle, impulse invariant; BOTH kernels are bitwise reproducible (the symmetric one accumulates in 64-bit fixed
    point, whose integer atomics commute) and the direct one is exactly linear under power-of-two scaling."""
    import torch
    n = 1_000_000
    rng = np.random.default_rng(20260101)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    sel = rng.choice(n, 1024, replace=False)
    ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float),
                                       x[sel].astype(float), z[sel].astype(float), 0.065)
    gd = g.astype(float)
    try:
        def run(gam):
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), gam.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                           du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            return du.cpu().numpy().copy(), dw.cpu().numpy().copy()
        res = {}
        for mode in (0, 1):
            eng.set_symmetric(mode)
            u, w = run(dg)
            res[mode] = (u, w)
            assert _rel(u[sel], w[sel], ur, wr) < 1e-5, mode
            assert abs(np.sum(gd * u)) < 1e-4 * np.sum(np.abs(gd * u))
            assert abs(np.sum(gd * w)) < 1e-4 * np.sum(np.abs(gd * w))
            u2, w2 = run(dg)
            u4, w4 = run(dg * 4.0)
            assert np.array_equal(u, u2) and np.array_equal(w, w2), mode
            if mode == 0:
                assert np.array_equal(u4, 4.0 * u) and np.array_equal(w4, 4.0 * w)
            else:
                # the fp32 partial sums scale exactly, their truncation to the fixed-point grid need not
                scale = max(np.abs(u).max(), np.abs(w).max())
                assert np.abs(u4 - 4.0 * u).max() < 1e-6 * scale
        scale = max(np.abs(res[0][0]).max(), np.abs(res[0][1]).max())
        assert np.abs(res[0][0] - res[1][0]).max() < 1e-5 * scale and np.abs(res[0][1] - res[1][1]).max() < 1e-5 * scale
    finally:
        eng.set_symmetric(1)
        eng.set_stream(None)


@pytest.mark.parametrize("n", [16384, 16385, 20000, 36863, 36864, 36865, 40959, 40960, 40961, 65536 + 255, 98304, 98305, 131072,
                               131072 + 511, 200000, 327168, 327169])
def test_symmetric_kernel_tile_edges(eng, n):
    """Symmetric self-interaction at sizes around its tilings (256-vortex tiles below 36 864 vortices (kSymT8MinN),
    512 from there; the quad variant plus a diagonal launch from 640 tiles of 512, i.e. from 327 169 vortices; odd and even
    tile counts, ragged last tile) against the C oracle and the direct kernel."""
    import torch
    rng = np.random.default_rng(n)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    sel = np.r_[0:300, n - 300:n, rng.choice(n, 400, replace=False)]
    ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float),
                                       x[sel].astype(float), z[sel].astype(float), 0.065)
    try:
        out = {}
        for mode in (0, 1):
            eng.set_symmetric(mode)
            du.fill_(float("nan")); dw.fill_(float("nan"))
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                           du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            out[mode] = (du.cpu().numpy().copy(), dw.cpu().numpy().copy())
            assert np.isfinite(out[mode][0]).all()
            assert _rel(out[mode][0][sel], out[mode][1][sel], ur, wr) < 1e-5, mode
        scale = max(np.abs(out[0][0]).max(), np.abs(out[0][1]).max())
        assert np.abs(out[0][0] - out[1][0]).max() < 1e-5 * scale
        assert np.abs(out[0][1] - out[1][1]).max() < 1e-5 * scale
    finally:
        eng.set_symmetric(1)
        eng.set_stream(None)


@pytest.mark.parametrize("ranks,n", [(2, 70000), (3, 100000), (8, 300001), (3, 600001), (8, 1100000)])
def test_symmetric_tile_ring_partition(eng, ranks, n):
    """Multi-GPU building block on one GPU: the owners of the tile ring, run one after the other with
    separate accumulators, add up (integer sums: what the all-reduce does) to BIT FOR BIT the self-interaction
    one owner of all tiles computes, and one owner's block step equals the direct advection of that block.  The two
    largest sizes run the quad variant of the kernel (from 640 tiles: four I tiles per workgroup share each partner tile,
    J-side sums added in LDS before one atomic): owners own whole quads (LUDVM_SYM_OWNER_ALIGN)."""
    import torch
    from ludvm_amd._ffi import SYM_OWNER_ALIGN, SYM_TILE
    tile = SYM_TILE * SYM_OWNER_ALIGN
    n_loc = ((n + ranks - 1) // ranks + tile - 1) // tile * tile
    n_pad = n_loc * ranks
    rng = np.random.default_rng(n)
    x = np.r_[rng.uniform(-10, 0, n), np.full(n_pad - n, 1e6)].astype(np.float32)
    z = np.r_[rng.uniform(-2, 2, n), np.full(n_pad - n, 1e6)].astype(np.float32)
    g = np.r_[rng.standard_normal(n) / n, np.zeros(n_pad - n)].astype(np.float32)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        scale = torch.zeros([32], dtype=torch.uint8, device=dev)
        eng.sym_scale_dev(dg.data_ptr(), n_pad, 0.065, scale.data_ptr())
        tiles = n_loc // SYM_TILE

        def accumulate(first, count, acc):
            base = acc.data_ptr()
            eng.sym_accumulate_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n_pad, first, count, 0.065, scale.data_ptr(),
                                   base, base + 8 * n_pad, base + 16 * n_pad)
        total = torch.zeros([2 * n_pad + 1], dtype=torch.int64, device=dev)
        for r in range(ranks):
            acc = torch.zeros_like(total)
            accumulate(r * tiles, tiles, acc)
            total += acc
        one = torch.zeros_like(total)
        accumulate(0, ranks * tiles, one)
        torch.cuda.synchronize()
        assert torch.equal(total, one) and int(total[-1]) == 0
        # ... and the whole-array entry point produces exactly these sums too
        du, dw = torch.empty(n_pad, device=dev), torch.empty(n_pad, device=dev)
        eng.set_symmetric(1)
        eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n_pad, dx.data_ptr(), dz.data_ptr(), n_pad, 0.065,
                       du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
        us, ws = du.cpu().numpy().copy(), dw.cpu().numpy().copy()
        eng.set_symmetric(0)
        eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n_pad, dx.data_ptr(), dz.data_ptr(), n_pad, 0.065,
                       du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
        ud, wd = du.cpu().numpy(), dw.cpu().numpy()
        sc = max(np.abs(ud[:n]).max(), np.abs(wd[:n]).max())
        assert np.abs(us[:n] - ud[:n]).max() < 1e-5 * sc and np.abs(ws[:n] - wd[:n]).max() < 1e-5 * sc
        # padding vortices (zero strength, 1e6 away) only feel the far field of the net circulation
        assert np.abs(us[n:]).max() < 1e-6 * sc and np.abs(ws[n:]).max() < 1e-6 * sc
        # block step of the last owner from the summed integers: the same velocities, bit for bit
        lo = (ranks - 1) * n_loc
        xo, zo = torch.empty(n_loc, device=dev), torch.empty(n_loc, device=dev)
        base = total.data_ptr()
        eng.advect_from_sums_dev(base + 8 * lo, base + 8 * (n_pad + lo), scale.data_ptr(), base + 16 * n_pad, dx.data_ptr(),
                                 dz.data_ptr(), lo, n_loc, 0.05, xo.data_ptr(), zo.data_ptr())
        torch.cuda.synchronize()
        assert np.abs(xo.cpu().numpy() - (x[lo:] + 0.05 * us[lo:])).max() < 1e-6      # (fma vs mul + add)
        np.testing.assert_allclose(xo.cpu().numpy(), x[lo:] + 0.05 * ud[lo:], rtol=0, atol=1e-5 * sc * 0.05 + 1e-6)
        np.testing.assert_allclose(zo.cpu().numpy(), z[lo:] + 0.05 * wd[lo:], rtol=0, atol=1e-5 * sc * 0.05 + 1e-6)
    finally:
        eng.set_symmetric(1)
        eng.set_stream(None)


@pytest.mark.parametrize("gscale", [1e-18, 1.0, 1e9])
def test_symmetric_kernel_fixed_point_scale_follows_the_circulations(eng, gscale):
    """The fixed-point scale is derived from sum|Gamma| / v_core per launch, so circulations of any magnitude -- and a
    mix of one dominant vortex with many weak ones -- keep fp32 accuracy: 1e-5 of max|u| against the oracle, and the weak
    vortices' own contribution (the field with the dominant one removed) is still resolved to 1e-3 of ITS maximum
    wherever fp32 itself can resolve it."""
    import torch
    n = 40000
    rng = np.random.default_rng(5)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n * gscale).astype(np.float32)
    big = g.copy()
    big[123] = np.float32(1e4 * np.abs(g).max())           # one vortex 10^4 times stronger than any other
    dev = torch.device("cuda", 0)
    dx, dz = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    sel = np.r_[0:200, rng.choice(n, 300, replace=False)]
    try:
        out = {}
        for name, gam in (("plain", g), ("dominant", big)):
            dg = torch.from_numpy(gam).to(dev)
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                           du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            u, w = du.cpu().numpy().astype(np.float64), dw.cpu().numpy().astype(np.float64)
            ur, wr = c_oracle.induced_velocity(gam.astype(float), x.astype(float), z.astype(float), x[sel].astype(float),
                                               z[sel].astype(float), 0.065)
            assert np.isfinite(u).all() and _rel(u[sel], w[sel], ur, wr) < 1e-5, name
            out[name] = (u[sel], w[sel], ur, wr)
        # what the weak vortices contribute, recovered from the two fields by linearity
        g1 = np.zeros(n); g1[123] = float(big[123]) - float(g[123])
        u1, w1 = c_oracle.induced_velocity(g1, x.astype(float), z.astype(float), x[sel].astype(float), z[sel].astype(float), 0.065)
        weak_u = out["dominant"][0] - u1
        scale = np.abs(out["plain"][2]).max()
        far = np.abs(u1) < 50 * scale              # targets where fp32 itself can still resolve the weak part
        assert far.sum() > 50 and np.abs(weak_u[far] - out["plain"][2][far]).max() < 1e-3 * scale
    finally:
        eng.set_stream(None)


def test_fixed_point_conversion_is_exact(eng):
    """fx_add's float -> 64-bit integer conversion through the kernel's own code (ludvm_fixed_point_probe): trunc(v * 2^k),
    exactly, for every |v * 2^k| < 2^63 -- small negative partial sums included (round 2 split the signed product: for
    t in (-2^31, 0) its remainder t + 2^32 is not an fp32 number and the result was off by up to 128 units)."""
    import math
    from fractions import Fraction
    rng = np.random.default_rng(77)
    special = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, -100.0, 100.25, -100.75, -2.0**31 + 128, 2.0**31 - 128, -2.0**31, 2.0**31,
               -2.0**32, 2.0**32 - 256, -(2.0**32 - 256), 2.0**32 + 512, -(2.0**32 + 512), 2.0**62, -2.0**62,
               float(np.float32(2.0**63 - 2.0**39)), -float(np.float32(2.0**63 - 2.0**39)), 1e-30, -1e-30, 3.0**20, -(3.0**20)]
    rand = np.concatenate([rng.standard_normal(2000) * s for s in (1.0, 1e3, 2.0**31, 2.0**40, 2.0**61)])
    v = np.concatenate([np.array(special), rand]).astype(np.float32)
    for k in (0, 7, -9):
        vals = v if k == 0 else (v * np.float32(2.0 ** -k)).astype(np.float32)
        keep = np.abs(vals.astype(np.float64) * 2.0**k) < 2.0**63
        vals = vals[keep]
        got = eng.fixed_point_probe(vals, k)
        want = np.array([math.trunc(Fraction(float(x)) * Fraction(2) ** k) for x in vals], dtype=object)
        assert all(int(a) == int(b) for a, b in zip(got, want)), [(float(x), int(a), int(b)) for x, a, b in zip(vals, got, want) if int(a) != int(b)][:5]


def test_symmetric_kernel_propagates_nan_like_the_reference(eng):
    """A NaN source position poisons the sum at every target in the reference (LUDVM.py:565-569); the fixed-point
    accumulators cannot hold a NaN, so the launch counts non-finite partial sums and the finisher returns NaN."""
    import torch
    n = 30000
    rng = np.random.default_rng(3)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    x[12345] = np.nan
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.zeros_like(dx), torch.zeros_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for mode in (0, 1):
            eng.set_symmetric(mode)
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                           du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            assert torch.isnan(du).all() and torch.isnan(dw).all(), mode
        # a clean launch afterwards is clean again
        dx[12345] = -1.0
        eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                       du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
        assert torch.isfinite(du).all() and torch.isfinite(dw).all()
    finally:
        eng.set_symmetric(1)
        eng.set_stream(None)


def test_symmetric_inviscid_self_pairs_are_nan_like_the_reference(eng):
    import torch
    n = 20000
    rng = np.random.default_rng(77)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        # v_core = 0 with targets == sources: every target coincides with one source -> NaN (0/0), as in
        # the reference, in both kernels
        for mode in (0, 1):
            eng.set_symmetric(mode)
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.0,
                           du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            assert torch.isnan(du).all() and torch.isnan(dw).all()
    finally:
        eng.set_symmetric(1)
        eng.set_stream(None)


def test_full_size_config5_flowfield(eng):
    """BASELINE config 5 at full size: 4096 x 4096 grid over N = 1e6 vortices (1.7e13 pairs).  Sampled
    grid points against the C oracle; linearity in the circulations (exact for a power of two); vorticity
    finite and consistent with the stencil on a sampled interior point."""
    import torch
    n, nx, nz = 1_000_000, 4096, 4096
    rng = np.random.default_rng(20260101)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    xmin, zmin, dr = -8.0, -4.0, 8.0 / nx
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du = torch.empty(nx * nz, dtype=torch.float32, device=dev)
    dw, dome = torch.empty_like(du), torch.empty_like(du)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.flowfield_dev(xmin, zmin, dr, nx, nz, dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, 0.065, du.data_ptr(),
                          dw.data_ptr())
        eng.vorticity_dev(du.data_ptr(), dw.data_ptr(), nx, nz, dr, dome.data_ptr())
        torch.cuda.synchronize()
        sel = rng.choice(nx * nz, 512, replace=False)
        xt, zt = xmin + (sel // nz) * dr, zmin + (sel % nz) * dr
        ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), xt, zt, 0.065)
        sel_t = torch.from_numpy(sel).to(dev)
        u, w = du[sel_t].cpu().numpy(), dw[sel_t].cpu().numpy()
        assert _rel(u, w, ur, wr) < 1e-5
        assert bool(torch.isfinite(dome).all())
        i, j = 1234, 2345
        p = i * nz + j
        ome_ref = (float(dw[p + nz]) - float(dw[p - nz])) / (2 * dr) - (float(du[p + 1]) - float(du[p - 1])) / (2 * dr)
        assert abs(float(dome[p]) - ome_ref) <= 1e-3 * abs(ome_ref) + 1e-4
        # doubling every circulation doubles the field exactly -- for the SAME launch geometry (a one-row
        # launch splits the sources differently from the full grid, so it matches that only to rounding)
        u_full = du[:nz].clone()
        r1u, r1w, r2u, r2w = (torch.empty(nz, dtype=torch.float32, device=dev) for _ in range(4))
        dg2 = dg * 2.0
        eng.flowfield_dev(xmin, zmin, dr, 1, nz, dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, 0.065, r1u.data_ptr(),
                          r1w.data_ptr())
        eng.flowfield_dev(xmin, zmin, dr, 1, nz, dx.data_ptr(), dz.data_ptr(), dg2.data_ptr(), n, 0.065, r2u.data_ptr(),
                          r2w.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(r2u, 2.0 * r1u) and torch.equal(r2w, 2.0 * r1w)
        assert float((r1u - u_full).abs().max()) < 1e-5 * float(u_full.abs().max())
    finally:
        eng.set_stream(None)


def test_full_size_config4_self_advection_step(eng):
    """BASELINE config 4's workload on one GPU: one symmetric self-advection step of N = 8e6 vortices (6.4e13 ordered
    pairs), and the direct variant's step of ONE owner of eight (rank 3: targets [3e6, 4e6) against all 8e6 sources,
    ludvm_advect_dev_f32 -- what `--symmetric 0` runs per rank).  256 sampled velocities against the C oracle at
    1e-5 max|u| with NO absolute floor (|u| ~ 2e-5 here, so with the run's dt = 0.05 a displacement is one
    ulp of x and (x1 - x0) / dt bounded nothing):
      * the symmetric kernel's fixed-point sums themselves, converted as finish_sym does (sum / scale / 2 pi);
      * the displacements of a step with dt = 2^16 (dt u exact, |dt u| ~ 1: the rounding of x + dt u is 1e-7 of max|u|),
        which also passes through the Euler finishers -- both variants;
    and conservation of the linear impulse sum_i G_i u_i (the pair forces cancel exactly in exact arithmetic)."""
    import torch
    from ludvm_amd.sharded import HipShardKernel, ShardedWake
    n = 8_000_000
    rng = np.random.default_rng(20260101)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    dev = torch.device("cuda", 0)
    dt = 65536.0
    try:
        wake = ShardedWake(x, z, g, 0.065, dt, HipShardKernel(eng), dev, symmetric=True)
        assert wake.n_loc % 512 == 0 and wake.pairs_per_step == float(n) * n
        wake.step()
        x1, z1 = wake.positions()
        sel = np.sort(rng.choice(n, 256, replace=False))
        ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), x[sel].astype(float),
                                           z[sel].astype(float), 0.065)
        scale = max(np.abs(ur).max(), np.abs(wr).max())
        assert 1e-5 < scale < 1e-3                      # (the regime the old absolute floor of 2-4e-5 swallowed)
        # (a) the raw fixed-point sums (the step leaves them in the wake's accumulator: u | w | NaN counter)
        rec = wake._scale.cpu().numpy()
        inv = float(rec[8:16].view(np.float64)[0])      # SymScale {float scale, pad; double inv}
        assert float(rec[:4].view(np.float32)[0]) * inv == 1.0
        acc = wake._acc.cpu().numpy()
        assert acc[2 * wake.n_pad] == 0                 # no non-finite partial sum
        su, sw = acc[:n].astype(np.float64) * inv / (2 * np.pi), -acc[wake.n_pad:wake.n_pad + n].astype(np.float64) * inv / (2 * np.pi)
        assert np.abs(su[sel] - ur).max() < 1e-5 * scale and np.abs(sw[sel] - wr).max() < 1e-5 * scale
        gd = g.astype(float)
        for v in (su, sw):
            assert abs(np.sum(gd * v)) < 1e-3 * np.sum(np.abs(gd * v))
        # (b) through the Euler finisher: displacement / 2^16
        ud, wd = (x1.astype(float) - x) / dt, (z1.astype(float) - z) / dt
        assert np.abs(ud[sel] - ur).max() < 1e-5 * scale and np.abs(wd[sel] - wr).max() < 1e-5 * scale
        assert np.abs(ud - su).max() < 2e-6 * scale and np.abs(wd - sw).max() < 2e-6 * scale     # all 8e6: finisher == sums
        del wake
        # (c) the direct variant, owner 3 of 8
        lo, cnt = 3_000_000, 1_000_000
        dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
        ox, oz = torch.empty(cnt, dtype=torch.float32, device=dev), torch.empty(cnt, dtype=torch.float32, device=dev)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.advect_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, lo, cnt, 0.065, dt, ox.data_ptr(), oz.data_ptr())
        torch.cuda.synchronize()
        own = sel[(sel >= lo) & (sel < lo + cnt)]
        extra = np.sort(rng.choice(cnt, 256 - len(own), replace=False)) + lo
        tsel = np.unique(np.r_[own, extra])
        ur2, wr2 = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), x[tsel].astype(float),
                                             z[tsel].astype(float), 0.065)
        scale2 = max(np.abs(ur2).max(), np.abs(wr2).max())
        u2 = (ox.cpu().numpy().astype(float) - x[lo:lo + cnt]) / dt
        w2 = (oz.cpu().numpy().astype(float) - z[lo:lo + cnt]) / dt
        assert np.abs(u2[tsel - lo] - ur2).max() < 1e-5 * scale2 and np.abs(w2[tsel - lo] - wr2).max() < 1e-5 * scale2
        # ... and the two variants agree on the whole block
        assert np.abs(u2 - su[lo:lo + cnt]).max() < 1e-5 * scale and np.abs(w2 - sw[lo:lo + cnt]).max() < 1e-5 * scale
    finally:
        eng.set_stream(None)


def test_product_build_refuses_the_measurement_codes(eng):
    """The negative codes of ludvm_set_sym_tuning (force a kernel variant at every size) belong to the measurement build."""
    from ludvm_amd import LudvmHipError
    for code in (-1, -2, -4):
        with pytest.raises(LudvmHipError):
            eng.set_sym_tuning(8, code)
    eng.set_sym_tuning(8, 2)
    eng.set_sym_tuning(0, 0)


@pytest.mark.parametrize("n", [16384 + 77, 50000, 150001])
def test_symmetric_kernel_rotation_split_variants(exp_eng, n):
    """Every tiling of the symmetric kernel (256 / 512-vortex tiles) with a tile pair's 64 rotation steps done by
    1, 2 or 4 wavefronts, by the size rule (0, the default: the rule's number for the bulk and four for the work items
    dispatched last -- mixed granularity -- where the rule gives fewer than four), with the mixed form at every size (-1) or
    at none (-2) (ludvm_set_sym_tuning): sampled targets against the C oracle, all vortices against the direct kernel; every
    variant repeats bit for bit.  At the smallest size (2.7e8 pairs: a fraction of a second of the C oracle) the oracle is taken at
    ALL targets, for every variant."""
    import torch
    from ludvm_amd import LudvmHipError
    eng = exp_eng          # the measurement build: the negative codes force a variant at every size
    rng = np.random.default_rng(n)
    x = rng.uniform(-10, 0, n).astype(np.float32)
    z = rng.uniform(-2, 2, n).astype(np.float32)
    g = (rng.standard_normal(n) / n).astype(np.float32)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    du, dw = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    sel = np.r_[0:200, n - 200:n, rng.choice(n, 300, replace=False)]
    ur, wr = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), x[sel].astype(float),
                                       z[sel].astype(float), 0.065)
    everywhere = n == 16384 + 77
    if everywhere:
        ua, wa = c_oracle.induced_velocity(g.astype(float), x.astype(float), z.astype(float), x.astype(float), z.astype(float), 0.065)

    def velocities():
        du.fill_(float("nan")); dw.fill_(float("nan"))
        eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, 0.065,
                       du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
        return du.cpu().numpy().astype(float), dw.cpu().numpy().astype(float)

    try:
        eng.set_symmetric(0)
        ud, wd = velocities()
        eng.set_symmetric(2)
        for t in (4, 8):
            for r in (0, -1, -2, 1, 2, 4):
                eng.set_sym_tuning(t, r)
                u, w = velocities()
                assert _rel(u[sel], w[sel], ur, wr) < 1e-5, (t, r)
                assert _rel(u, w, ud, wd) < 1e-5, (t, r)
                if everywhere:
                    assert _rel(u, w, ua, wa) < 1e-5, (t, r, "all targets")
                u2, w2 = velocities()
                assert np.array_equal(u, u2) and np.array_equal(w, w2), (t, r)
        with pytest.raises(LudvmHipError):
            eng.set_sym_tuning(3, 1)
        with pytest.raises(LudvmHipError):
            eng.set_sym_tuning(4, 3)
    finally:
        eng.set_sym_tuning(0, 0)
        eng.set_symmetric(1)
        eng.set_stream(None)


@pytest.mark.parametrize("prec_code,win", [(2, {100: 1e-9}), (1, {50: 1e-6, 75: 1e-4, 100: 1e-2}),
                                           (0, {50: 1e-5, 75: 1e-3, 100: 6e-2})])
def test_integration_md_binding_drives_the_reference_loop(prec_code, win):
    """INTEGRATION.md option B as printed: the raw-ctypes binding of ludvm_induce_f64 is executed from the document
    and bound over `induced_velocity` of the CPU restatement of the reference class (the reference file itself does
    not travel to the GPU box); every call site of the reference's own time loop then runs through the C ABI.
    Against the reference's golden README run: identical LEV shedding; fp64 mode to rounding over the first 100
    steps; hi+lo fp32 inside SURVEY's T2 bound (1e-2 over the first 100 steps); fp32 in windows that widen with the
    flow's amplification (~10x per 12 steps), measured 3.5e-2 at step 100 with every sum -- the chord sums too -- in
    fp32 (deterministic kernels: the figure repeats)."""
    import os
    import re
    from conftest import CONFIG1, ROOT
    from ludvm_amd import _ffi
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"## B\..*?```python\n(.*?)```", text, re.S).group(1)
    assert "/path/to/ludvm_amd/csrc/libludvm_hip.so" in block and "v_core, 0, p(u), p(w))" in block
    block = block.replace("/path/to/ludvm_amd/csrc/libludvm_hip.so", _ffi.LIB_PATH)
    block = block.replace("v_core, 0, p(u), p(w))", f"v_core, {prec_code}, p(u), p(w))")
    _ffi.load()                       # one HIP runtime in the process before the document's own CDLL call
    ns = {}
    exec(compile(block, "INTEGRATION.md#B", "exec"), ns)

    class Bound(O.OracleLUDVM):
        induced_velocity = ns["induced_velocity"]

    g2 = load_golden("g2_config1.npz")
    sim = Bound(**CONFIG1)
    assert np.array_equal(sim.LEV_shed, g2["LEV_shed"])
    print("binding, precision", prec_code, {hi: max(float(np.abs(getattr(sim, n)[:hi] - g2[n][:hi]).max()) for n in ("Cl", "Cd", "Cm"))
                                            for hi in (50, 75, 100)})
    for name in ("Cl", "Cd", "Cm"):
        for hi, tol in win.items():
            assert np.abs(getattr(sim, name)[:hi] - g2[name][:hi]).max() <= tol, (name, hi)
    if prec_code == 2:
        np.testing.assert_allclose(sim.path["TEV"][50], g2["TEV_50"], rtol=0, atol=1e-9)
    ns["_hip"].ludvm_destroy(ns["_ctx"])


# ---------------------------------------------------------------------------------------------------------------------
# G3: the reference's own call trace through the HIP path
# ---------------------------------------------------------------------------------------------------------------------
def _g3_calls():
    from conftest import grouped
    g3 = load_golden("g3_boundary_trace.npz")
    by = grouped(g3)
    return [by[str(k)] for k in range(int(g3["ncalls"]))]


@pytest.mark.parametrize("precision", ["f64", "f32x2", "f32"])
def test_g3_boundary_trace_through_the_hip_path(eng, precision):
    """Every induced_velocity call the unmodified reference made in steps 1-5, 100 and 400 of the README run
    (tests/golden/g3_boundary_trace.npz: 63 calls at the call sites LUDVM.py:746, :751, :1054, :1105-1124 -- one-vortex and
    three-vortex wakes, Gamma = 0 phantom slots at (0, 0), the unit TEV with an INTEGER circulation [1], single targets, the
    80 bound vortices as sources) with the reference's arguments, through Engine.induce -> ludvm_induce_f64, against the
    reference's returns.  f64: 1e-12 of the call's max|u| (and exact zeros where the reference has them); f32 takes the
    float64 route at these sizes (< 2048 points a side: ludvm_hip.h) and is held to the same bound; f32x2 runs the fp32 hi+lo
    kernels: 1e-5 of max|u|, and 2e-6 of the kernel mass per target."""
    calls = _g3_calls()
    assert len(calls) == 63 and sorted({int(c["step"]) for c in calls}) == [1, 2, 3, 4, 5, 100, 400]
    assert sum(c["g"].dtype.kind == "i" for c in calls) == 7 and all(bool(c["viscous"]) for c in calls)
    compared = 0
    for k, c in enumerate(calls):
        u, w = eng.induce(c["g"], c["xw"], c["zw"], c["xp"], c["zp"], 0.065, precision=precision)
        assert u.dtype == np.float64 and u.shape == c["u"].shape == w.shape, k
        assert np.array_equal(np.isnan(u), np.isnan(c["u"])) and np.array_equal(np.isnan(w), np.isnan(c["w"])), k
        scale = max(np.abs(c["u"]).max(), np.abs(c["w"]).max())
        if scale == 0.0:                       # (a wake of Gamma = 0 slots only: the reference returns exact zeros)
            assert not u.any() and not w.any(), k
            continue
        err = max(np.abs(u - c["u"]).max(), np.abs(w - c["w"]).max()) / scale
        compared += 1
        assert err <= (1e-5 if precision == "f32x2" else 1e-12), (k, int(c["step"]), precision, err)
        if precision == "f32x2":
            mu, mw = _kernel_mass(c["g"].astype(float), c["xw"], c["zw"], c["xp"], c["zp"], 0.065)
            assert np.all(np.abs(u - c["u"]) <= 2e-6 * mu + 1e-30) and np.all(np.abs(w - c["w"]) <= 2e-6 * mw + 1e-30), k
    assert compared == 61                   # (calls 0 and 3: the step-1 wake is one Gamma = 0 slot)


@pytest.mark.parametrize("precision,tol", [("f64", 1e-12), ("f32x2", 1e-5), ("f32", 1e-5)])
def test_g3_roll_up_calls_equal_one_resident_wake_advect(eng, precision, tol):
    """The six roll-up calls of each traced step (LUDVM.py:1105-1124: wake -> TEV / LEV / FREE targets and bound vortices ->
    the same targets) are ONE ludvm_wake_advect on the resident wake in this build: with the traced sources loaded (phantom
    slots and all), the velocities it returns are u_wake + u_foil of the reference's calls in wake order, and the positions
    it leaves are x + dt (u_wake + u_foil) (:1108-1109, :1117-1118, :1126-1127)."""
    calls = _g3_calls()
    dt = 5e-2
    steps = sorted({int(c["step"]) for c in calls})
    for s in steps:
        mine = [c for c in calls if int(c["step"]) == s]
        roll = mine[-6:]                                   # (wake, foil) x (TEV, LEV, FREE)
        wake, foil = roll[0], roll[1]
        for a, b in zip(roll[0::2], roll[1::2]):           # the three wake calls share their sources; so do the foil calls
            assert np.array_equal(a["xw"], wake["xw"]) and np.array_equal(b["xw"], foil["xw"]) and len(b["g"]) == 80
            assert np.array_equal(a["xp"], b["xp"])
        xt = np.concatenate([c["xp"] for c in roll[0::2]])
        zt = np.concatenate([c["zp"] for c in roll[0::2]])
        assert np.array_equal(xt, wake["xw"]) and np.array_equal(zt, wake["zw"])       # targets = the wake, in its order
        u_ref = np.concatenate([a["u"] + b["u"] for a, b in zip(roll[0::2], roll[1::2])])
        w_ref = np.concatenate([a["w"] + b["w"] for a, b in zip(roll[0::2], roll[1::2])])
        eng.wake_clear()
        eng.wake_reserve(1024)
        eng.wake_append(wake["xw"], wake["zw"], wake["g"])
        u, w = eng.wake_advect(dt, foil["xw"], foil["zw"], foil["g"], 0.065, precision=precision, return_velocity=True)
        scale = max(np.abs(u_ref).max(), np.abs(w_ref).max())
        err = max(np.abs(u - u_ref).max(), np.abs(w - w_ref).max()) / scale
        assert err <= tol, (s, precision, err)
        x, z = eng.wake_read(0, len(xt))
        # the Euler update is done on the float64 masters whatever the pair kernels' precision
        assert np.abs(x - (xt + dt * u)).max() <= 1e-15 * max(1.0, np.abs(xt).max()) and np.abs(z - (zt + dt * w)).max() <= 1e-15, s
        assert max(np.abs(x - (xt + dt * u_ref)).max(), np.abs(z - (zt + dt * w_ref)).max()) <= tol * scale * dt + 1e-15, s
    eng.wake_clear()


def test_a_few_probe_points_in_a_large_wake_do_not_pay_the_float64_rate(eng):
    """LUDVM_PREC_F32 with fewer than 2048 points on ONE side used to run in float64 whatever the size of the
    other side.  1000 probe targets in a wake of 1e6 vortices (1e9 pairs, > 2^28): the call takes hi+lo positions -- the
    accuracy of the f32 tier (here <= 2e-6 of max|u| against the C oracle) at about a third of the float64 kernel time; with
    100 000 sources (1e8 pairs, <= 2^28) it still takes the float64 route and its 1e-12."""
    rng = np.random.default_rng(77)
    n = 1_000_000
    xw, zw = rng.uniform(-10, 0, n), rng.uniform(-2, 2, n)
    g = rng.standard_normal(n) / n
    xp, zp = rng.uniform(-10, 0, 1000), rng.uniform(-2, 2, 1000)
    ur, wr = c_oracle.induced_velocity(g, xw, zw, xp, zp, 0.065)
    ms = {}
    for prec in ("f64", "f32"):
        eng.induce(g, xw, zw, xp, zp, 0.065, precision=prec)              # (warm: buffers, first-use costs)
        eng.kernel_timing(True)
        eng.kernel_time_ms(reset=True)
        u, w = eng.induce(g, xw, zw, xp, zp, 0.065, precision=prec)
        ms[prec], launches = eng.kernel_time_ms(reset=True)
        eng.kernel_timing(False)
        assert launches >= 1
        assert _rel(u, w, ur, wr) <= (1e-12 if prec == "f64" else 2e-6), prec
    assert ms["f32"] < 0.6 * ms["f64"], ms
    # the same targets, a tenth of the sources: small as a whole -> float64, as before
    m = 100_000
    u, w = eng.induce(g[:m], xw[:m], zw[:m], xp, zp, 0.065, precision="f32")
    ur, wr = c_oracle.induced_velocity(g[:m], xw[:m], zw[:m], xp, zp, 0.065)
    assert _rel(u, w, ur, wr) <= 1e-12


def test_a_shed_sheet_keeps_its_order_without_a_sort(eng):
    """a thin, sheet-like set (every shed wake) is compact as stored; the library now sees that from the class
    extents alone (within 3 x of a line across the bounding box) and keeps the order -- reordered = 0 -- while a shuffled
    copy of the same sheet is still put in Morton order, and both calls agree to the f32 tier."""
    n = 40_000
    s = np.linspace(0.0, 1.0, n)
    x, z = -30.0 * s, 0.4 * np.sin(9.0 * s)                  # a wavy sheet, 30 chords long, stored in shedding order
    order, reordered, ext = eng.spatial_order(x, z, with_extent=True)
    assert reordered is False or reordered == 0
    assert np.array_equal(order, np.arange(n)) and ext < 3.0 * (30.0 + 0.8) * 256 / n
    perm = np.random.default_rng(5).permutation(n)
    order2, reordered2, ext2 = eng.spatial_order(x[perm], z[perm], with_extent=True)
    assert reordered2 and ext2 < 10.0 * ext
    g = np.full(n, 1.0 / n)
    u1, w1 = eng.induce(g, x, z, x, z, 5e-3, precision="f32")
    u2, w2 = eng.induce(g, x[perm], z[perm], x[perm], z[perm], 5e-3, precision="f32")
    ur, wr = c_oracle.induced_velocity(g, x, z, x, z, 5e-3)
    assert _rel(u1, w1, ur, wr) <= 1e-5 and _rel(u2, w2, ur[perm], wr[perm]) <= 1e-5
