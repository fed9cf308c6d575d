"""GPU tier of the velocity gradient: pair_grad_f64<128 | 512> and finish_grad through Engine.gradient_field / flowfield_gradient
and the class, against the long double closed forms of tests/gradient_common.py at EVERY target and in every component, within
the bound derived there (tests/test_gradient_host.py shows on the CPU that the helper is the gradient of the oracle's velocity
and that a plain float64 sum sits inside the bound).

Shapes: the table of tests/test_gpu_scalar_field.py -- source counts on both sides of the 128-source tile (the ragged tile is
bounded by its count), several splits, one product launch on the 512-source tile; target counts on both sides of a workgroup.
Grids on a dyadic mesh (xmin + i dr is exact, so the device's mesh IS the reference's)."""
import numpy as np
import pytest

import gradient_common as G
import scalar_field_common as S

pytestmark = pytest.mark.gpu

TILE = S.header_constant("kTileF64Few")
NS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 4099)
NT = (1, 83, 255, 256, 257)
# the one product launch on the 512-source tile: more sources than kSmallTileMaxF64Default AND more than kFewTargets targets
BIG = (S.header_constant("kSmallTileMaxF64Default") + 289, 257)
GRID = dict(xmin=-8.0, zmin=-1.0, dr=0.0625)
GRID_SHAPES = ((1, 1), (7, 5), (17, 33), (64, 64))
GRID_NS = 513


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


def _within(got, ref, what):
    """every component at every target inside the bound -> the worst error / bound"""
    vals, bound = ref
    worst = 0.0
    assert len(got) == 3
    for name, a, val in zip(G.NAMES, got, vals):
        a = np.asarray(a).reshape(-1)
        assert a.dtype == np.float64 and a.shape == val.shape and np.isfinite(a).all(), (what, name, "not finite")
        err = np.abs(a - val)
        ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if len(err) else 0.0
        assert np.all(err <= bound), (what, name, "worst error / bound", ratio, "at", int(np.argmax(err - bound)))
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("v_core", [S.V_CORE, 0.0])
def test_points_by_value_at_ragged_tiles_and_workgroup_edges(eng, v_core):
    assert BIG[0] > S.header_constant("kSmallTileMaxF64Default") and BIG[1] > S.header_constant("kFewTargets")
    worst = 0.0
    shapes = [(ns, nt) for ns in NS for nt in NT] + ([BIG] if v_core > 0 else [])
    for ns, nt in shapes:
        g, xs, zs = S.wake_strip(ns)
        xt, zt = S.targets(nt)
        ref = G.cached_reference(("points", ns, nt, v_core), (g, xs, zs, xt, zt, v_core))
        got = eng.gradient_field(g, xs, zs, xt, zt, v_core)
        worst = max(worst, _within(got, ref, (v_core, ns, nt)))
        if v_core == 0:
            assert np.array_equal(got[1], got[2]), (ns, nt)                  # no core: irrotational, bit for bit
        again = eng.gradient_field(g, xs, zs, xt, zt, v_core)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), ("not reproducible", ns, nt)
    print(f"v_core {v_core}: worst error / bound = {worst:.3f}")


def test_a_target_on_a_source_sees_the_cores_solid_rotation(eng):
    # one source: ux = 0 and uz = -wx = G / (2 pi v_core^2)
    ux, uz, wx = eng.gradient_field([2.0], [0.25], [-0.5], [0.25, 1.0], [-0.5, 0.0], S.V_CORE)
    ref = G.reference([2.0], [0.25], [-0.5], [0.25, 1.0], [-0.5, 0.0], S.V_CORE)
    rot = 2.0 / (2 * np.pi * S.V_CORE**2)
    assert ux[0] == 0 and abs(uz[0] - rot) <= ref[1][0] and abs(wx[0] + rot) <= ref[1][0]
    _within((ux, uz, wx), ref, "one source")
    # among the sources of three tiles: first and last slot of a tile, the last source of the ragged tile
    ns = 2 * TILE + 3
    g, xs, zs = S.wake_strip(ns)
    xt, zt = S.targets(83)
    on = [0, TILE - 1, TILE, ns - 1]
    xt[:len(on)], zt[:len(on)] = xs[on], zs[on]
    ref = G.reference(g, xs, zs, xt, zt, S.V_CORE)
    ratio = _within(eng.gradient_field(g, xs, zs, xt, zt, S.V_CORE), ref, "coincident")
    print(f"targets on sources: worst error / bound = {ratio:.3f}")


def test_grids_by_value_and_row_blocks_bit_for_bit(eng):
    g, xs, zs = S.wake_strip(GRID_NS, seed=1)
    xs = xs / 6.0                                             # [-10, 0]: the window below lies in the strip
    worst = 0.0
    for nx, nz in GRID_SHAPES:
        xt, zt = S.grid_points(GRID["xmin"], GRID["zmin"], GRID["dr"], nx, nz)
        ref = G.cached_reference(("grid", nx, nz), (g, xs, zs, xt, zt, S.V_CORE))
        args = (GRID["xmin"], GRID["zmin"], GRID["dr"], nx, nz, g, xs, zs, S.V_CORE)
        whole = eng.flowfield_gradient(*args)
        assert all(a.shape == (nx, nz) for a in whole)
        worst = max(worst, _within(whole, ref, ("grid", nx, nz)))
        # the point call at the mesh points: the same sums within the same bound
        _within(eng.gradient_field(g, xs, zs, xt, zt, S.V_CORE), ref, ("points of the grid", nx, nz))
        # blocks of rows planned for the whole grid carry its bits; so does a second call
        cut = min(3, nx)
        head = eng.flowfield_gradient(*args, row_first=0, row_count=cut)
        tail = eng.flowfield_gradient(*args, row_first=cut, row_count=nx - cut)
        for k in range(3):
            assert head[k].shape == (cut, nz) and tail[k].shape == (nx - cut, nz)
            assert np.array_equal(head[k], whole[k][:cut]) and np.array_equal(tail[k], whole[k][cut:]), (G.NAMES[k], nx, nz)
        assert all(np.array_equal(a, b) for a, b in zip(eng.flowfield_gradient(*args), whole)), (nx, nz)
    print(f"grids: worst error / bound = {worst:.3f}")


def test_the_curl_is_the_analytic_vorticity(eng):
    """wx - uz against Engine.scalar_field('omega') at points near and far from the cores, within the sum of both bounds"""
    for ns, nt in ((2 * TILE + 3, 257), (4099, 83)):
        g, xs, zs = S.wake_strip(ns)
        xt, zt = S.targets(nt)
        xt[:8], zt[:8] = xs[:8] + 0.01, zs[:8] - 0.005                      # inside a core's reach
        _, bound = G.reference(g, xs, zs, xt, zt, S.V_CORE)
        _, obound = S.reference("omega", g, xs, zs, xt, zt, S.V_CORE)
        _, uz, wx = eng.gradient_field(g, xs, zs, xt, zt, S.V_CORE)
        ome = eng.scalar_field("omega", g, xs, zs, xt, zt, S.V_CORE)
        assert np.abs(ome[:8]).max() > 1.0
        assert np.all(np.abs((wx - uz) - ome) <= bound + obound), (ns, nt, (np.abs((wx - uz) - ome) / (bound + obound)).max())


def test_error_paths_and_empty_sides(eng):
    from ludvm_amd import LudvmHipError, _ffi
    g, xs, zs = S.wake_strip(5)
    xt, zt = S.targets(3)
    for first, count in ((2, 3), (5, 0), (0, 5)):
        with pytest.raises(LudvmHipError, match="rows outside the grid") as e:
            eng.flowfield_gradient(0.0, 0.0, 0.5, 4, 4, g, xs, zs, S.V_CORE, row_first=first, row_count=count)
        assert e.value.code == _ffi.E_ARG
    with pytest.raises(ValueError):
        eng.gradient_field(g, xs, zs[:4], xt, zt, S.V_CORE)
    with pytest.raises(ValueError):
        eng.flowfield_gradient(0.0, 0.0, 0.5, 4, -1, g, xs, zs, S.V_CORE)
    lib, ctx = eng._lib, eng._ctx
    one = np.zeros(1)
    p = one.ctypes.data_as(_ffi._pd)
    assert lib.ludvm_gradient_f64(ctx, p, p, p, 1, p, p, 1, 0.1, p, None, p) == _ffi.E_ARG           # a null output
    assert lib.ludvm_gradient_f64(ctx, None, p, p, 1, p, p, 1, 0.1, p, p, p) == _ffi.E_ARG           # a null source array
    assert lib.ludvm_flowfield_gradient_rows_f64(ctx, 0.0, 0.0, 0.5, 2, 2, 0, 2, p, p, p, 1, 0.1, p, p, None) == _ffi.E_ARG
    assert lib.ludvm_gradient_f64(ctx, None, None, None, 0, None, None, 0, 0.1, None, None, None) == _ffi.OK   # no targets
    # no sources: zeros; no targets, no rows: nothing to do
    assert all(np.array_equal(a, np.zeros(3)) for a in eng.gradient_field([], [], [], xt, zt, S.V_CORE))
    assert all(np.array_equal(a, np.zeros((4, 3))) for a in eng.flowfield_gradient(0.0, 0.0, 0.5, 4, 3, [], [], [], S.V_CORE))
    assert all(a.shape == (0,) for a in eng.gradient_field(g, xs, zs, [], [], S.V_CORE))
    assert all(a.shape == (0, 3) for a in eng.flowfield_gradient(0.0, 0.0, 0.5, 4, 3, g, xs, zs, S.V_CORE, row_first=4))
    assert all(a.shape == (4, 0) for a in eng.flowfield_gradient(0.0, 0.0, 0.5, 4, 0, g, xs, zs, S.V_CORE))
    # the engine is usable afterwards
    assert all(np.isfinite(a).all() for a in eng.gradient_field(g, xs, zs, xt, zt, S.V_CORE))


def test_class_fields_next_to_the_other_fields():
    """a short README-like run (41 steps, dense history): ux_ff, uz_ff, wx_ff by value on the sources flowfield gathers, q_ff
    their determinant, the other five fields bit for bit what the call without the flag leaves, the point method the engine's"""
    from ludvm_amd import LUDVM
    sim = LUDVM(t0=0, tf=0.6, dt=1.5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012", verbose=False)
    try:
        win = dict(xmin=-1.0, xmax=1.5, zmin=-0.5, zmax=0.5, dr=0.1)
        tsteps = [0, 1, 20]
        others = ("u_ff", "w_ff", "ome_ff", "psi_ff", "omega_ff")
        sim.flowfield(**win, tsteps=tsteps, psi=True, omega=True)
        assert not any(hasattr(sim, n) for n in ("ux_ff", "uz_ff", "wx_ff", "q_ff"))
        plain = [getattr(sim, n).copy() for n in others]
        sim.flowfield(**win, tsteps=tsteps, psi=True, omega=True, grad=True)
        for n, before in zip(others, plain):
            assert np.array_equal(getattr(sim, n), before), n
        nx, nz = sim.x_ff.shape
        assert sim.ux_ff.shape == sim.uz_ff.shape == sim.wx_ff.shape == sim.q_ff.shape == (len(tsteps), nx, nz)
        assert np.array_equal(sim.q_ff, -sim.ux_ff**2 - sim.uz_ff * sim.wx_ff)
        xt, zt = S.grid_points(win["xmin"], win["zmin"], win["dr"], nx, nz)
        for ii, s in enumerate(tsteps):
            g, xw, zw = sim._flowfield_sources(s)
            ref = G.reference(g, xw, zw, xt, zt, sim.v_core)
            ratio = _within((sim.ux_ff[ii], sim.uz_ff[ii], sim.wx_ff[ii]), ref, ("step", s))
            print(f"gradient fields, step {s}, {len(g)} sources: worst error / bound = {ratio:.3f}")
            obound = S.reference("omega", g, xw, zw, xt, zt, sim.v_core)[1]
            assert np.all(np.abs((sim.wx_ff[ii] - sim.uz_ff[ii]).ravel() - sim.omega_ff[ii].ravel()) <= ref[1] + obound)
        assert np.abs(sim.q_ff[2]).max() > 0
        g, xw, zw = sim._flowfield_sources(20)
        px, pz = S.targets(83)
        for viscous, vc in ((True, sim.v_core), (False, 0)):
            got, want = sim.velocity_gradient(g, xw, zw, px, pz, viscous=viscous), sim.engine.gradient_field(g, xw, zw, px, pz, vc)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    finally:
        sim.engine.close()
