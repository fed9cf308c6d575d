"""GPU tier of the stream function and the analytic vorticity: pair_scalar_f64<PSI | OMEGA, 128 | 512> and finish_scalar through
Engine.scalar_field / flowfield_scalar and the class, against the long double closed forms of tests/scalar_field_common.py
at EVERY target, within the bounds derived there (tests/test_scalar_field_host.py shows on the CPU that the helper has the
contract's sign and gauge and that a plain float64 sum sits inside the bounds).

Shapes: source counts on both sides of the 128-source tile (the ragged tile is not padded: a padded slot would be 0 * ln(inf)),
several splits, one product launch on the 512-source tile; target counts on both sides of a workgroup.  Grids on a dyadic
mesh (xmin + i dr is exact, so the device's mesh IS the reference's whether or not the compiler fuses the multiply-add)."""
import numpy as np
import pytest

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
    val, bound = ref
    assert got.shape == val.shape and np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got - val)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    assert np.all(err <= bound), (what, "worst error / bound", ratio, "at", int(np.argmax(err - bound)))
    return ratio


@pytest.mark.parametrize("v_core", [S.V_CORE, 0.0])
@pytest.mark.parametrize("kind", S.KINDS)
def test_points_by_value_at_ragged_tiles_and_workgroup_edges(eng, kind, v_core):
    assert BIG[0] > S.header_constant("kSmallTileMaxF64Default") and BIG[1] > S.header_constant("kFewTargets")
    worst = 0.0
    shapes = [(ns, nt) for ns in NS for nt in NT] + ([BIG] if v_core > 0 else [])
    for ns, nt in shapes:
        g, xs, zs = S.wake_strip(ns)
        xt, zt = S.targets(nt)
        ref = S.cached_reference(("points", ns, nt, v_core), kind, (g, xs, zs, xt, zt, v_core))
        got = eng.scalar_field(kind, g, xs, zs, xt, zt, v_core)
        assert got.dtype == np.float64
        worst = max(worst, _within(got, ref, (kind, v_core, ns, nt)))
        if kind == "omega" and v_core == 0:
            assert np.all(got == 0), (ns, nt)
        assert np.array_equal(got, eng.scalar_field(kind, g, xs, zs, xt, zt, v_core)), ("not reproducible", ns, nt)
    print(f"{kind}, v_core {v_core}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", S.KINDS)
def test_a_target_on_a_source_is_finite_with_a_core(eng, kind):
    ns = 2 * TILE + 3
    g, xs, zs = S.wake_strip(ns)
    xt, zt = S.targets(83)
    on = [0, TILE - 1, TILE, ns - 1]                      # first and last slot of a tile, the last source of the ragged tile
    xt[:len(on)], zt[:len(on)] = xs[on], zs[on]
    ref = S.reference(kind, g, xs, zs, xt, zt, S.V_CORE)
    ratio = _within(eng.scalar_field(kind, g, xs, zs, xt, zt, S.V_CORE), ref, (kind, "coincident"))
    print(f"{kind}, targets on sources: worst error / bound = {ratio:.3f}")


@pytest.mark.parametrize("kind", S.KINDS)
def test_grids_by_value_and_row_blocks_bit_for_bit(eng, kind):
    g, xs, zs = S.wake_strip(GRID_NS, seed=1)
    xs = xs / 6.0                                             # [-10, 0]: the window below lies in the strip
    worst = 0.0
    for nx, nz in GRID_SHAPES:
        xt, zt = S.grid_points(GRID["xmin"], GRID["zmin"], GRID["dr"], nx, nz)
        ref = S.cached_reference(("grid", nx, nz), kind, (g, xs, zs, xt, zt, S.V_CORE))
        args = (kind, GRID["xmin"], GRID["zmin"], GRID["dr"], nx, nz, g, xs, zs, S.V_CORE)
        whole = eng.flowfield_scalar(*args)
        assert whole.shape == (nx, nz) and whole.dtype == np.float64
        worst = max(worst, _within(whole.ravel(), ref, (kind, "grid", nx, nz)))
        # the point call at the mesh points: the same sums within the same bounds
        _within(eng.scalar_field(kind, g, xs, zs, xt, zt, S.V_CORE), ref, (kind, "points of the grid", nx, nz))
        # blocks of rows planned for the whole grid carry its bits; so does a second call
        cut = min(3, nx)
        head = eng.flowfield_scalar(*args, row_first=0, row_count=cut)
        tail = eng.flowfield_scalar(*args, row_first=cut, row_count=nx - cut)
        assert head.shape == (cut, nz) and tail.shape == (nx - cut, nz)
        assert np.array_equal(head, whole[:cut]) and np.array_equal(tail, whole[cut:]), (kind, nx, nz)
        assert np.array_equal(eng.flowfield_scalar(*args), whole), (kind, nx, nz)
    print(f"{kind}, grids: worst error / bound = {worst:.3f}")


def test_error_paths_and_empty_sides(eng):
    from ludvm_amd import LudvmHipError, _ffi
    g, xs, zs = S.wake_strip(5)
    xt, zt = S.targets(3)
    with pytest.raises(LudvmHipError, match="unknown field kind") as e:
        eng.scalar_field(7, g, xs, zs, xt, zt, S.V_CORE)
    assert e.value.code == _ffi.E_ARG
    with pytest.raises(LudvmHipError, match="unknown field kind"):
        eng.flowfield_scalar(-1, 0.0, 0.0, 0.5, 4, 4, g, xs, zs, S.V_CORE)
    with pytest.raises(ValueError):
        eng.scalar_field("vorticity", g, xs, zs, xt, zt, S.V_CORE)
    for first, count in ((2, 3), (5, 0), (0, 5)):
        with pytest.raises(LudvmHipError, match="rows outside the grid") as e:
            eng.flowfield_scalar("psi", 0.0, 0.0, 0.5, 4, 4, g, xs, zs, S.V_CORE, row_first=first, row_count=count)
        assert e.value.code == _ffi.E_ARG
    for kind in S.KINDS:
        # no sources: zeros; no targets, no rows: nothing to do
        assert np.array_equal(eng.scalar_field(kind, [], [], [], xt, zt, S.V_CORE), np.zeros(3))
        assert np.array_equal(eng.flowfield_scalar(kind, 0.0, 0.0, 0.5, 4, 3, [], [], [], S.V_CORE), np.zeros((4, 3)))
        assert eng.scalar_field(kind, g, xs, zs, [], [], S.V_CORE).shape == (0,)
        assert eng.flowfield_scalar(kind, 0.0, 0.0, 0.5, 4, 3, g, xs, zs, S.V_CORE, row_first=4).shape == (0, 3)
        assert eng.flowfield_scalar(kind, 0.0, 0.0, 0.5, 4, 0, g, xs, zs, S.V_CORE).shape == (4, 0)
    # the engine is usable afterwards
    assert np.isfinite(eng.scalar_field("psi", g, xs, zs, xt, zt, S.V_CORE)).all()


def test_class_fields_next_to_the_velocity_fields():
    """a short README-like run (41 steps, dense history): psi_ff and omega_ff by value on the sources flowfield gathers, the
    velocity fields and the stencil's vorticity bit for bit what the call without the flags leaves, the point methods the
    engine's"""
    from ludvm_amd import LUDVM
    sim = LUDVM(t0=0, tf=0.6, dt=1.5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012", verbose=False)
    try:
        win = dict(xmin=-1.0, xmax=1.5, zmin=-0.5, zmax=0.5, dr=0.1)
        tsteps = [0, 1, 20]
        sim.flowfield(**win, tsteps=tsteps)
        assert not hasattr(sim, "psi_ff") and not hasattr(sim, "omega_ff")
        plain = [getattr(sim, n).copy() for n in ("u_ff", "w_ff", "ome_ff")]
        sim.flowfield(**win, tsteps=tsteps, psi=True, omega=True)
        for n, before in zip(("u_ff", "w_ff", "ome_ff"), plain):
            assert np.array_equal(getattr(sim, n), before), n
        nx, nz = sim.x_ff.shape
        assert sim.psi_ff.shape == sim.omega_ff.shape == (len(tsteps), nx, nz)
        xt, zt = S.grid_points(win["xmin"], win["zmin"], win["dr"], nx, nz)
        # (x_ff, z_ff are numpy's arange: the device's mesh to an ulp)
        assert np.abs(xt - sim.x_ff.ravel()).max() < 1e-14 and np.abs(zt - sim.z_ff.ravel()).max() < 1e-14
        for ii, s in enumerate(tsteps):
            g, xw, zw = sim._flowfield_sources(s)
            for kind, field in (("psi", sim.psi_ff), ("omega", sim.omega_ff)):
                ratio = _within(field[ii].ravel(), S.reference(kind, g, xw, zw, xt, zt, sim.v_core), (kind, "step", s))
                print(f"{kind}_ff, step {s}, {len(g)} sources: worst error / bound = {ratio:.3f}")
        assert np.abs(sim.omega_ff[2]).max() > 0 and np.abs(sim.psi_ff[2]).max() > 0
        g, xw, zw = sim._flowfield_sources(20)
        px, pz = S.targets(83)
        for viscous, vc in ((True, sim.v_core), (False, 0)):
            assert np.array_equal(sim.stream_function(g, xw, zw, px, pz, viscous=viscous), sim.engine.scalar_field("psi", g, xw, zw, px, pz, vc))
            assert np.array_equal(sim.vorticity(g, xw, zw, px, pz, viscous=viscous), sim.engine.scalar_field("omega", g, xw, zw, px, pz, vc))
    finally:
        sim.engine.close()
