"""GPU tier of the hi+lo fp32 route of the analytic vorticity and the velocity gradient: field_hilo_f32<omega | gradient> with
finish_scalar / finish_grad through Engine's precision='f32x2' and LUDVM.flowfield(field_precision='f32x2'), against the long
double closed forms of tests/gradient_common.py and tests/scalar_field_common.py at EVERY target and in every component, within
the bound derived in tests/gradient_f32x2_common.py (tests/test_gradient_f32x2_host.py shows on the CPU that the scheme meets it
with a margin of 15).

Shapes: source counts on both sides of the 256-source tile and of a split (the ragged tile is padded, the pad adds exact zeros),
a launch of several splits with a ragged last one at the smallest target count (one target already splits), target counts on
both sides of a workgroup's 1024 (256 lanes x 4 points).  Grids on a dyadic mesh (xmin + i dr is exact, so the device's mesh IS
the reference's)."""
import numpy as np
import pytest

import gradient_common as G
import gradient_f32x2_common as C
import scalar_field_common as S
from conftest import CONFIG1

pytestmark = pytest.mark.gpu

NS = (1, C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1)
NS_SPLIT = 3 * C.TILE + 77            # four splits of one tile each, the last one ragged (the plan is asserted below)
NT = (1, 63, C.WORKGROUP - 1, C.WORKGROUP, C.WORKGROUP + 1)
TIER = 2e-6                           # direct_shapes_common.TOL["hilo"]
GRID = dict(xmin=-8.0, zmin=-1.0, dr=0.0625)


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


def _ratio(got, val, bound, what):
    a = np.asarray(got).reshape(-1)
    assert a.dtype == np.float64 and a.shape == val.shape and np.isfinite(a).all(), (what, "not finite")
    err = np.abs(a - val)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if len(err) else 0.0
    assert np.all(err <= bound), (what, "worst error / bound", ratio, "at", int(np.argmax(err - bound)))
    return ratio


def _check_both(eng, key, inputs):
    """gradient and omega of one case by value -> the worst error / bound of each"""
    vals, bound = C.cached("grad", key, inputs)
    got = eng.gradient_field(*inputs, precision="f32x2")
    assert len(got) == 3
    rg = max(_ratio(a, v, bound, (key, name)) for name, a, v in zip(G.NAMES, got, vals))
    ome, obound = C.cached("omega", key, inputs)
    ro = _ratio(eng.scalar_field("omega", *inputs, precision="f32x2"), ome, obound, (key, "omega"))
    return rg, ro


@pytest.mark.parametrize("ns", NS + (NS_SPLIT,))
def test_points_by_value_at_ragged_tiles_splits_and_workgroup_edges(eng, ns):
    if ns == NS_SPLIT:
        assert C.plan(1, ns) == (C.TILE, 4) and ns % C.TILE != 0
    assert C.plan(1, C.TILE) == (C.TILE, 1) and C.plan(1, C.TILE + 1) == (C.TILE, 2)
    worst = (0.0, 0.0)
    for nt in NT:
        rg, ro = _check_both(eng, ("points", ns, nt), C.case(ns, nt))
        worst = (max(worst[0], rg), max(worst[1], ro))
    print(f"ns = {ns}: worst error / bound = {worst[0]:.3f} (gradient), {worst[1]:.3f} (omega)")


def test_no_sources_give_zeros_and_no_targets_nothing(eng):
    xt, zt = S.targets(5)
    g, xs, zs = S.wake_strip(7)
    assert all(np.array_equal(a, np.zeros(5)) for a in eng.gradient_field([], [], [], xt, zt, C.V_CORE, precision="f32x2"))
    assert np.array_equal(eng.scalar_field("omega", [], [], [], xt, zt, C.V_CORE, precision="f32x2"), np.zeros(5))
    assert all(np.array_equal(a, np.zeros((4, 3))) for a in eng.flowfield_gradient(0.0, 0.0, 0.5, 4, 3, [], [], [], C.V_CORE,
                                                                                   precision="f32x2"))
    assert np.array_equal(eng.flowfield_scalar("omega", 0.0, 0.0, 0.5, 4, 3, [], [], [], C.V_CORE, precision="f32x2"), np.zeros((4, 3)))
    assert all(a.shape == (0,) for a in eng.gradient_field(g, xs, zs, [], [], C.V_CORE, precision="f32x2"))
    assert eng.flowfield_scalar("omega", 0.0, 0.0, 0.5, 4, 3, g, xs, zs, C.V_CORE, row_first=4, precision="f32x2").shape == (0, 3)


# ---- the tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("strip", {}), ("small_core", dict(v_core=C.V_CORE_SMALL)), ("at_-5000", dict(shift=-5000.0))])
def test_the_hi_lo_tier_wherever_the_wake_is(eng, name, kw):
    inputs = C.case(3000, 1100, **kw)
    assert C.plan(1100, 3000)[1] >= 2
    rg, ro = _check_both(eng, ("tier", name), inputs)
    vals, _ = C.cached("grad", ("tier", name), inputs)
    got = eng.gradient_field(*inputs, precision="f32x2")
    err = max(np.abs(a - v).max() for a, v in zip(got, vals)) / max(np.abs(v).max() for v in vals)
    ome, _ = C.cached("omega", ("tier", name), inputs)
    oerr = np.abs(eng.scalar_field("omega", *inputs, precision="f32x2") - ome).max() / np.abs(ome).max()
    print(f"{name}: {err:.2e} of max|grad u|, {oerr:.2e} of max|omega|; worst error / bound = {rg:.3f}, {ro:.3f}")
    assert err <= TIER and oerr <= TIER


def test_sources_spread_over_twenty_thousand_chords(eng):
    """|x| <= 1e4 with targets among the sources: far pairs at r2 ~ 1e8 next to pairs inside a core -- the products' order keeps
    every factor inside fp32's range, so the far terms neither flush nor overflow"""
    rg, ro = _check_both(eng, ("wide",), C.wide_case(3000, 1100))
    print(f"wide: worst error / bound = {rg:.3f} (gradient), {ro:.3f} (omega)")


# ---- bits --------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)


def test_a_repeated_call_is_bit_identical(eng):
    inputs = C.case(3000, 1100)
    assert _same(eng.gradient_field(*inputs, precision="f32x2"), eng.gradient_field(*inputs, precision="f32x2"))
    assert _same(eng.scalar_field("omega", *inputs, precision="f32x2"), eng.scalar_field("omega", *inputs, precision="f32x2"))


@pytest.mark.parametrize("nx,nz", [(40, 28), (37, 31)])          # nz a multiple of 4, and not; both more than one workgroup
def test_grids_row_blocks_and_points_share_their_bits(eng, nx, nz):
    g, xs, zs = S.wake_strip(NS_SPLIT)
    xs = xs / 8.0                                     # (the strip over the mesh)
    assert nx * nz > C.WORKGROUP and C.plan(nx * nz, NS_SPLIT)[1] >= 2
    whole_g = eng.flowfield_gradient(**GRID, nx=nx, nz=nz, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, precision="f32x2")
    whole_o = eng.flowfield_scalar("omega", **GRID, nx=nx, nz=nz, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, precision="f32x2")
    # by value on the mesh the library generates
    xt, zt = S.grid_points(GRID["xmin"], GRID["zmin"], GRID["dr"], nx, nz)
    vals, bound = C.gradient_reference(g, xs, zs, xt, zt, C.V_CORE)
    for name, a, v in zip(G.NAMES, whole_g, vals):
        _ratio(a, v, bound, ("grid", nx, nz, name))
    ome, obound = C.omega_reference(g, xs, zs, xt, zt, C.V_CORE)
    _ratio(whole_o, ome, obound, ("grid", nx, nz, "omega"))
    # the same points as an array of as many targets: the same bits
    assert _same(tuple(a.reshape(-1) for a in whole_g), eng.gradient_field(g, xs, zs, xt, zt, C.V_CORE, precision="f32x2"))
    assert _same(whole_o.reshape(-1), eng.scalar_field("omega", g, xs, zs, xt, zt, C.V_CORE, precision="f32x2"))
    # blocks of rows (the first, an inner one that ends the grid, the last row alone) carry the whole-grid call's bits
    for first, count in ((0, 3), (5, nx - 5), (nx - 1, 1)):
        rows_g = eng.flowfield_gradient(**GRID, nx=nx, nz=nz, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, row_first=first,
                                        row_count=count, precision="f32x2")
        assert _same(rows_g, tuple(a[first:first + count] for a in whole_g)), (first, count)
        rows_o = eng.flowfield_scalar("omega", **GRID, nx=nx, nz=nz, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, row_first=first,
                                      row_count=count, precision="f32x2")
        assert _same(rows_o, whole_o[first:first + count]), (first, count)


def test_the_default_is_the_float64_route_bit_for_bit(eng):
    inputs = C.case(513, 257)
    g, xs, zs = inputs[:3]
    f32 = eng.gradient_field(*inputs, precision="f32x2")
    assert _same(eng.gradient_field(*inputs), eng.gradient_field(*inputs, precision="f64"))
    assert _same(eng.scalar_field("omega", *inputs), eng.scalar_field("omega", *inputs, precision="f64"))
    assert _same(eng.scalar_field("psi", *inputs), eng.scalar_field("psi", *inputs, precision="f64"))
    assert _same(eng.flowfield_gradient(**GRID, nx=9, nz=7, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE),
                 eng.flowfield_gradient(**GRID, nx=9, nz=7, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, precision="f64"))
    assert _same(eng.flowfield_scalar("omega", **GRID, nx=9, nz=7, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE),
                 eng.flowfield_scalar("omega", **GRID, nx=9, nz=7, circulation=g, xw=xs, zw=zs, v_core=C.V_CORE, precision="f64"))
    # ... inside the float64 bound, which the fp32 route is not: the two routes are two routes
    vals, b64 = G.reference(*inputs)
    assert all(np.all(np.abs(a - v) <= b64) for a, v in zip(eng.gradient_field(*inputs), vals))
    assert any(np.any(np.abs(a - v) > b64) for a, v in zip(f32, vals))


def test_omega_is_the_curl_of_the_gradient(eng):
    inputs = C.case(3000, 1100)
    _, bound = C.cached("grad", ("tier", "strip"), inputs)
    _, obound = C.cached("omega", ("tier", "strip"), inputs)
    _, uz, wx = eng.gradient_field(*inputs, precision="f32x2")
    ome = eng.scalar_field("omega", *inputs, precision="f32x2")
    assert np.abs(ome).max() > 0 and np.all(np.abs((wx - uz) - ome) <= bound + obound)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi_leave_the_context_usable(eng):
    from ludvm_amd import _ffi
    lib, ctx = eng._lib, eng._ctx
    inputs = C.case(300, 65)
    want_g = eng.gradient_field(*inputs, precision="f32x2")
    want_o = eng.scalar_field("omega", *inputs, precision="f32x2")
    good = lambda: _same(eng.gradient_field(*inputs, precision="f32x2"), want_g) and \
        _same(eng.scalar_field("omega", *inputs, precision="f32x2"), want_o)                       # noqa: E731
    buf = np.zeros(4)
    p = buf.ctypes.data_as(_ffi._pd)
    message = lambda: lib.ludvm_last_error(ctx).decode()                                             # noqa: E731
    PSI, OMEGA = _ffi.FIELD_KINDS["psi"], _ffi.FIELD_KINDS["omega"]
    # the stream function
    assert lib.ludvm_scalar_f32x2(ctx, PSI, p, p, p, 1, p, p, 1, 0.1, p) == _ffi.E_ARG
    assert "the stream function has no fp32 route" in message() and good()
    assert lib.ludvm_flowfield_scalar_rows_f32x2(ctx, PSI, 0.0, 0.0, 0.5, 2, 2, 0, 2, p, p, p, 1, 0.1, p) == _ffi.E_ARG
    assert "the stream function has no fp32 route" in message() and good()
    assert lib.ludvm_scalar_f32x2(ctx, 7, p, p, p, 1, p, p, 1, 0.1, p) == _ffi.E_ARG
    assert "unknown field kind" in message() and good()
    # no core, a core below fp32's reach, a core that is no number
    for vc in (0.0, 9.9e-7, -0.1, float("nan"), float("inf")):
        assert lib.ludvm_scalar_f32x2(ctx, OMEGA, p, p, p, 1, p, p, 1, vc, p) == _ffi.E_ARG
        assert "vcore" in message()
        assert lib.ludvm_flowfield_scalar_rows_f32x2(ctx, OMEGA, 0.0, 0.0, 0.5, 2, 2, 0, 2, p, p, p, 1, vc, p) == _ffi.E_ARG
        assert lib.ludvm_gradient_f32x2(ctx, p, p, p, 1, p, p, 1, vc, p, p, p) == _ffi.E_ARG
        assert "vcore" in message()
        assert lib.ludvm_flowfield_gradient_rows_f32x2(ctx, 0.0, 0.0, 0.5, 2, 2, 0, 2, p, p, p, 1, vc, p, p, p) == _ffi.E_ARG
        assert good()
    assert lib.ludvm_gradient_f32x2(ctx, p, p, p, 1, p, p, 1, 1e-6, p, p, p) == _ffi.OK                # (the smallest core)
    # rows outside the grid
    for first, count in ((2, 3), (5, 0), (0, 5)):
        assert lib.ludvm_flowfield_scalar_rows_f32x2(ctx, OMEGA, 0.0, 0.0, 0.5, 4, 4, first, count, p, p, p, 1, 0.1, p) == _ffi.E_ARG
        assert "rows outside the grid" in message()
        assert lib.ludvm_flowfield_gradient_rows_f32x2(ctx, 0.0, 0.0, 0.5, 4, 4, first, count, p, p, p, 1, 0.1, p, p, p) == _ffi.E_ARG
        assert "rows outside the grid" in message() and good()
    # null arrays with a non-zero count; no targets is a no-op
    assert lib.ludvm_gradient_f32x2(ctx, p, p, p, 1, p, p, 1, 0.1, p, None, p) == _ffi.E_ARG
    assert lib.ludvm_scalar_f32x2(ctx, OMEGA, None, p, p, 1, p, p, 1, 0.1, p) == _ffi.E_ARG
    assert "null array" in message()
    assert lib.ludvm_gradient_f32x2(ctx, None, None, None, 0, None, None, 0, 0.1, None, None, None) == _ffi.OK
    # through the engine: the library's message arrives
    from ludvm_amd import LudvmHipError
    with pytest.raises(LudvmHipError, match="vcore") as e:
        eng.gradient_field(*inputs[:5], 0.0, precision="f32x2")
    assert e.value.code == _ffi.E_ARG and good()


# ---- the class -------------------------------------------------------------------------------------------------------------------------
def test_class_fields_in_f32x2_next_to_the_float64_ones():
    """config 1's run: with field_precision='f32x2' omega_ff and the gradient fields are within the bound of the long double
    reference (and so of the float64 fields, which are within theirs), q_ff is formed from them, and u_ff, w_ff, ome_ff and
    psi_ff are bit for bit what the call without the keyword leaves"""
    from ludvm_amd import LUDVM
    sim = LUDVM(**CONFIG1, verbose=False)
    try:
        win = dict(xmin=-6.0, xmax=1.0, zmin=-1.0, zmax=1.0, dr=0.125)
        tsteps = [1, 200, 399]
        same = ("u_ff", "w_ff", "ome_ff", "psi_ff")
        new = ("omega_ff", "ux_ff", "uz_ff", "wx_ff")
        sim.flowfield(**win, tsteps=tsteps, psi=True, omega=True, grad=True)
        f64 = {n: getattr(sim, n).copy() for n in same + new}
        sim.flowfield(**win, tsteps=tsteps, psi=True, omega=True, grad=True, field_precision="f32x2")
        for n in same:
            assert np.array_equal(getattr(sim, n), f64[n]), n
        assert np.array_equal(sim.q_ff, -sim.ux_ff**2 - sim.uz_ff * sim.wx_ff)
        nx, nz = sim.x_ff.shape
        xt, zt = S.grid_points(win["xmin"], win["zmin"], win["dr"], nx, nz)
        for ii, s in enumerate(tsteps):
            g, xw, zw = sim._flowfield_sources(s)
            vals, bound = C.gradient_reference(g, xw, zw, xt, zt, sim.v_core)
            b64 = G.reference(g, xw, zw, xt, zt, sim.v_core)[1]
            for name, v in zip(("ux_ff", "uz_ff", "wx_ff"), vals):
                _ratio(getattr(sim, name)[ii], v, bound, ("step", s, name))
                assert np.all(np.abs(getattr(sim, name)[ii] - f64[name][ii]).ravel() <= bound + b64), (s, name)
            ome, obound = C.omega_reference(g, xw, zw, xt, zt, sim.v_core)
            _ratio(sim.omega_ff[ii], ome, obound, ("step", s, "omega_ff"))
            o64 = S.reference("omega", g, xw, zw, xt, zt, sim.v_core)[1]
            assert np.all(np.abs(sim.omega_ff[ii] - f64["omega_ff"][ii]).ravel() <= obound + o64), s
        # the two routes are two routes: some value of the last step differs
        assert any(not np.array_equal(getattr(sim, n)[2], f64[n][2]) for n in new)
    finally:
        sim.engine.close()
