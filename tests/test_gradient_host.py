"""CPU tier of the velocity gradient (ludvm_gradient_f64, ludvm_flowfield_gradient_rows_f64, Engine.gradient_field /
flowfield_gradient, LUDVM.velocity_gradient / flowfield(grad=True)).

What a GPU is not needed for: the reference helper the GPU tier is checked against (tests/gradient_common.py) IS the gradient of
the ORACLE's induced velocity -- centred differences converge to it at second order in every component -- and its curl is the
analytic vorticity's reference; the symbols are declared, bound and exported; the kernels compile without scratch; the class's
part (same sources, same mesh, attributes, refusals) on a small engine stub."""
import importlib.util
import inspect
import os
import re
import types

import numpy as np
import pytest

import gradient_common as G
import scalar_field_common as S
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import LUDVM, _ffi
from oracle import ludvm_oracle as O

NAMES = ("ludvm_gradient_f64", "ludvm_flowfield_gradient_rows_f64")


# ---- the reference helper ----------------------------------------------------------------------------------------------------------
def _case(ns=300, nt=50, clear=0.02):
    """a wake-like strip of `ns` sources in [-3, 0] and `nt` targets at least `clear` (and both steps h below) from every source"""
    rng = np.random.default_rng(11)
    g, xs, zs = S.wake_strip(ns, seed=5)
    xs = xs / 20.0
    xt, zt = rng.uniform(-3.2, 0.2, 40 * nt), rng.uniform(-1.5, 1.5, 40 * nt)
    far = np.hypot(xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]).min(axis=1) >= clear + 2e-3
    assert far.sum() >= nt
    return g, xs, zs, xt[far][:nt], zt[far][:nt]


def _differences(g, xs, zs, xt, zt, h):
    """centred differences of the oracle's velocity: u_x, u_z, w_x, w_z"""
    def vel(x, z):
        return O.induced_velocity(g, xs, zs, x, z, S.V_CORE)
    (ue, we), (uw_, ww_) = vel(xt + h, zt), vel(xt - h, zt)
    (un, wn), (us, ws) = vel(xt, zt + h), vel(xt, zt - h)
    return (ue - uw_) / (2 * h), (un - us) / (2 * h), (we - ww_) / (2 * h), (wn - ws) / (2 * h)


def test_the_reference_is_the_gradient_of_the_oracles_velocity():
    """300 sources, 50 targets at least 0.02 from every source, v_core = 0.0195: the error of the centred differences against the
    closed forms falls by 4 per halving of h (h = 1e-3, 5e-4) in u_x, u_z, w_x and in w_z = -u_x: ratio within [3.5, 4.5]"""
    g, xs, zs, xt, zt = _case()
    (ux, uz, wx), _ = G.reference(g, xs, zs, xt, zt, S.V_CORE)
    closed = (ux, uz, wx, -ux)
    err = {h: [np.abs(d - c).max() for d, c in zip(_differences(g, xs, zs, xt, zt, h), closed)] for h in (1e-3, 5e-4)}
    for k, name in enumerate(("u_x", "u_z", "w_x", "w_z")):
        ratio = err[1e-3][k] / err[5e-4][k]
        print(f"{name}: error {err[1e-3][k]:.3e} at h = 1e-3, {err[5e-4][k]:.3e} at 5e-4, ratio {ratio:.3f}")
        assert err[1e-3][k] < 1e-2 * np.abs(closed[k]).max(), name       # (the differences resolve the field: a wrong factor shows)
        assert 3.5 <= ratio <= 4.5, (name, ratio)


def test_the_curl_of_the_reference_is_the_analytic_vorticitys_reference():
    """w_x - u_z against scalar_field_common.reference('omega').  Both helpers hand out float64 values rounded from long double,
    so the difference of two rounded components carries their roundings, which the gradient's bound covers and omega's (small far
    from every core, where u_z and w_x are not) cannot: the tolerance is the sum of both bounds, as in the GPU tier.  The
    unrounded long double sums agree far inside that: to the gradient's bound at long double's precision (2^-63 for 2^-52)."""
    for ns, vc in ((300, S.V_CORE), (300, 0.3), (1, S.V_CORE), (300, 0.0)):
        g, xs, zs, xt, zt = _case(ns)
        (ux, uz, wx), bound = G.reference(g, xs, zs, xt, zt, vc)
        ome, obound = S.reference("omega", g, xs, zs, xt, zt, vc)
        assert np.all(np.abs((wx - uz) - ome) <= bound + obound), (ns, vc)
        (_, uzl, wxl), mag = G.reference_ld(g, xs, zs, xt, zt, vc)
        _, r2, s, vc4 = S._pairs(g, xs, zs, xt, zt, vc)
        omel = (-np.asarray(g, S.LD)[None, :] * vc4 / (S.PI * s**3)).sum(axis=1)
        assert np.all(np.abs((wxl - uzl) - omel) <= (ns + G.K) * 2.0**-63 * mag), (ns, vc)
        if vc > 0:
            assert np.abs(ome).max() > 0
        # the bound can tell a wrong sign or a factor of two in any component
        assert np.all(bound < 1e-9 * max(np.abs(c).max() for c in (ux, uz, wx)))


def test_a_point_on_a_source_has_the_core_s_solid_rotation():
    (ux, uz, wx), bound = G.reference([2.0], [0.25], [-0.5], [0.25], [-0.5], S.V_CORE)
    rot = 2.0 / (2 * np.pi * S.V_CORE**2)
    assert ux[0] == 0 and abs(uz[0] - rot) <= bound[0] and abs(wx[0] + rot) <= bound[0]


def test_the_float64_sum_sits_inside_the_bound():
    """a sequential float64 sum of float64 terms, formed as the kernel forms them, against the long double reference: inside the
    bound at sizes of the GPU table (the bound is not one only a lucky order meets)"""
    tile = S.header_constant("kTileF64Few")
    for ns in (1, tile - 1, tile + 1, 4099):
        g, xs, zs = S.wake_strip(ns)
        xt, zt = S.targets(83)
        dx, dz = xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]
        r2 = dx * dx + dz * dz
        y = 1.0 / np.sqrt(r2 * r2 + S.V_CORE**4)
        c = g * (y * y * y)
        e = c * r2
        ta, tb = e * (dx * dz), e * (dx * dx - dz * dz)
        A, B, C = np.zeros(len(xt)), np.zeros(len(xt)), np.zeros(len(xt))
        for j in range(ns):
            A, B, C = A + ta[:, j], B + tb[:, j], C + c[:, j]
        vC = S.V_CORE**4 * C
        got = (-A / np.pi, (B + vC) / (2 * np.pi), (B - vC) / (2 * np.pi))
        vals, bound = G.reference(g, xs, zs, xt, zt, S.V_CORE)
        for name, a, b in zip(G.NAMES, got, vals):
            assert np.all(np.abs(a - b) <= bound), (name, ns, (np.abs(a - b) / bound).max())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _prototype(name):
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1)


def test_symbols_are_declared_bound_exported_and_listed_as_additions():
    lib = _ffi.load()
    for name in NAMES:
        params = [p.strip() for p in _prototype(name).split(",")]
        assert len(params) == len(_ffi.SIGNATURES[name]), (name, params)
        assert params[0].startswith("ludvm_ctx*") and [p.split()[-1] for p in params[-3:]] == ["ux", "uz", "wx"]
        assert name in _ffi.ADDED_IN_ABI_7
        assert hasattr(lib, name)
        assert hasattr(_ffi.load(_ffi.EXP_LIB_PATH), name)
    assert _ffi.ABI_VERSION == 7


def test_a_null_context_is_refused():
    lib = _ffi.load()
    assert lib.ludvm_gradient_f64(None, None, None, None, 0, None, None, 0, 0.0, None, None, None) == _ffi.E_ARG
    assert lib.ludvm_flowfield_gradient_rows_f64(None, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None, 0, 0.0, None, None,
                                                 None) == _ffi.E_ARG


def test_gradient_kernels_compile_without_scratch():
    """pair_grad_f64<128 | 512> and finish_grad for gfx950 through tools/kernel_resources.py (no GPU needed): no scratch, no spill"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    K = {k: v for k, v in kr.resources(unit="flowfield.hip").items() if "pair_grad_f64" in k or "finish_grad" in k}
    tiles = (S.header_constant("kTileF64Few"), S.header_constant("kTileF64"))
    assert sorted(k for k in K if "pair_grad" in k) == sorted("_ZN5ludvm13pair_grad_f64ILi%dEEEvNS_8PairArgsE" % t for t in tiles)
    assert len(K) == 3
    for name, r in K.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) in (0, 3 * 8 * tiles[0], 3 * 8 * tiles[1]), (name, r)


# ---- the class on an engine stub -----------------------------------------------------------------------------------------------
class GradientStub(FakeEngine):
    """FakeEngine plus the scalar and gradient methods: the reference helpers' sums, every gradient call recorded"""

    def __init__(self):
        super().__init__()
        self.grad_calls = []

    def flowfield_scalar(self, kind, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None):
        x, z = S.grid_points(xmin, zmin, dr, nx, nz, row_first, row_count)
        return S.reference(kind, circulation, xw, zw, x, z, v_core)[0].reshape(-1, nz)

    def gradient_field(self, circulation, xw, zw, xp, zp, v_core):
        self.grad_calls.append(("points", np.array(circulation, float), np.array(xw, float), np.array(zw, float), v_core))
        return G.reference(circulation, xw, zw, xp, zp, v_core)[0]

    def flowfield_gradient(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None):
        self.grad_calls.append(("grid", np.array(circulation, float), np.array(xw, float), np.array(zw, float), v_core,
                                (xmin, zmin, dr, nx, nz, row_first, row_count)))
        x, z = S.grid_points(xmin, zmin, dr, nx, nz, row_first, row_count)
        return tuple(c.reshape(-1, nz) for c in G.reference(circulation, xw, zw, x, z, v_core)[0])


WINDOW = dict(xmin=-1.5, xmax=0.55, zmin=-0.5, zmax=0.5, dr=0.25)
TSTEPS = [0, 1, 9]
FIELDS = ("ux_ff", "uz_ff", "wx_ff", "q_ff")


@pytest.fixture(scope="module")
def sims():
    kw = dict(CONFIG1, tf=0.6)
    return LUDVM(**kw, verbose=False, engine=GradientStub()), LUDVM(**kw, verbose=False, engine=FakeEngine())


def test_flowfield_grad_hands_the_flowfield_sources_to_the_engine_and_leaves_the_other_fields(sims):
    sim, _ = sims
    eng = sim.engine
    sim.flowfield(**WINDOW, tsteps=TSTEPS, psi=True, omega=True)
    assert eng.grad_calls == [] and not any(hasattr(sim, n) for n in FIELDS)
    before = {n: getattr(sim, n).copy() for n in ("x_ff", "z_ff", "u_ff", "w_ff", "ome_ff", "psi_ff", "omega_ff")}
    sim.flowfield(**WINDOW, tsteps=TSTEPS, psi=True, omega=True, grad=True)
    for n, b in before.items():
        assert np.array_equal(getattr(sim, n), b), n
    nx, nz = sim.x_ff.shape
    assert all(getattr(sim, n).shape == (len(TSTEPS), nx, nz) for n in FIELDS)
    assert len(eng.grad_calls) == len(TSTEPS)
    for ii, s in enumerate(TSTEPS):
        g, xw, zw = sim._flowfield_sources(s)
        call = eng.grad_calls[ii]
        assert call[0] == "grid" and call[4] == sim.v_core
        assert np.array_equal(call[1], np.asarray(g, float)) and np.array_equal(call[2], xw) and np.array_equal(call[3], zw)
        assert call[5] == (WINDOW["xmin"], WINDOW["zmin"], WINDOW["dr"], nx, nz, 0, None)
        (ux, uz, wx), bound = G.reference(g, xw, zw, sim.x_ff.ravel(), sim.z_ff.ravel(), sim.v_core)
        for name, ref in (("ux_ff", ux), ("uz_ff", uz), ("wx_ff", wx)):
            assert np.all(np.abs(getattr(sim, name)[ii].ravel() - ref) <= bound + 1e-12), name   # (arange's mesh against xmin + i dr)
    assert np.array_equal(sim.q_ff, -sim.ux_ff * sim.ux_ff - sim.uz_ff * sim.wx_ff)
    assert np.abs(sim.q_ff[2]).max() > 0
    # grad alone: the scalar fields of an earlier call are not touched, the gradient is the same
    q = sim.q_ff.copy()
    sim.flowfield(**WINDOW, tsteps=TSTEPS, grad=True)
    assert np.array_equal(sim.q_ff, q) and np.array_equal(sim.psi_ff, before["psi_ff"])


def test_an_engine_without_the_methods_is_refused_by_name(sims):
    _, plain = sims
    with pytest.raises(RuntimeError, match="flowfield_gradient"):
        plain.flowfield(**WINDOW, tsteps=[1], grad=True)
    with pytest.raises(RuntimeError, match="gradient_field"):
        plain.velocity_gradient([1.0], [0.0], [0.0], [1.0], [1.0])
    plain.flowfield(**WINDOW, tsteps=[1])              # ... and the plain call goes on working
    assert not hasattr(plain, "q_ff")


def test_a_sharded_run_is_refused_before_any_engine_call():
    sim = LUDVM(**dict(CONFIG1, tf=0.6), verbose=False, engine=GradientStub())
    calls = dict(sim.engine.calls)
    sim._shard = types.SimpleNamespace(world=2)          # what a `distributed` run and every replica of a `devices` run carry
    with pytest.raises(ValueError, match="one GPU"):
        sim.flowfield(**WINDOW, tsteps=[1], grad=True)
    with pytest.raises(ValueError, match="one GPU"):
        sim.velocity_gradient([1.0], [0.0], [0.0], [1.0], [1.0])
    assert sim.engine.grad_calls == [] and sim.engine.calls == calls and not hasattr(sim, "q_ff")


def test_velocity_gradient_takes_induced_velocitys_arguments(sims):
    sim, _ = sims
    del sim.engine.grad_calls[:]
    g, xs, zs = S.wake_strip(5)
    xt, zt = S.targets(3)
    ux, uz, wx = sim.velocity_gradient(g, xs, zs, xt, zt)
    assert ux.shape == uz.shape == wx.shape == (3,)
    _, uz0, wx0 = sim.velocity_gradient(g, xs, zs, xt, zt, viscous=False)
    assert np.array_equal(uz0, wx0)                      # (no core: irrotational)
    assert [(c[0], c[4]) for c in sim.engine.grad_calls] == [("points", sim.v_core), ("points", 0)]
    names = [list(inspect.signature(getattr(LUDVM, m)).parameters) for m in ("induced_velocity", "stream_function", "velocity_gradient")]
    assert names[0] == names[1] == names[2]
