"""CPU tier of the stream function and the analytic vorticity (ludvm_scalar_f64, ludvm_flowfield_scalar_rows_f64,
Engine.scalar_field / flowfield_scalar, LUDVM.stream_function / vorticity / flowfield(psi=, omega=)).

What a GPU is not needed for: the symbols are declared, bound and exported; the reference helper the GPU tier is checked against
(tests/scalar_field_common.py) has the sign and the gauge of the contract -- central differences of its psi are the ORACLE's
induced velocity, its omega is the curl of that velocity, v_core = 0 is the point vortex; the kernels compile without scratch;
the class's part (same sources, same mesh, attributes, refusals) on a small engine stub."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

import scalar_field_common as S
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import LUDVM, _ffi
from oracle import ludvm_oracle as O

NAMES = ("ludvm_scalar_f64", "ludvm_flowfield_scalar_rows_f64")


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1)


def test_symbols_are_declared_bound_exported_and_listed_as_additions():
    lib = _ffi.load()
    for name in NAMES:
        params = [p.strip() for p in _prototype(name).split(",")]
        assert len(params) == len(_ffi.SIGNATURES[name]), (name, params)
        assert params[0].startswith("ludvm_ctx*") and params[1] == "int kind"
        assert name in _ffi.ADDED_IN_ABI_7
        assert hasattr(lib, name)
        assert hasattr(_ffi.load(_ffi.EXP_LIB_PATH), name)
    head = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    m = re.search(r"enum\s*\{\s*LUDVM_FIELD_PSI\s*=\s*(\d+)\s*,\s*LUDVM_FIELD_OMEGA\s*=\s*(\d+)\s*\}", head)
    assert _ffi.FIELD_KINDS == {"psi": int(m.group(1)), "omega": int(m.group(2))}
    doc = head[head.index("stream function and analytic vorticity"):head.index("---- measurement")]
    assert "LUDVM.py:565-566" in doc and "LUDVM.py:1186-1298" in doc
    assert _ffi.ABI_VERSION == 7


def test_a_null_context_is_refused_before_the_kind_is_looked_at():
    lib = _ffi.load()
    assert lib.ludvm_scalar_f64(None, 7, None, None, None, 0, None, None, 0, 0.0, None) == _ffi.E_ARG
    assert lib.ludvm_flowfield_scalar_rows_f64(None, 7, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None, 0, 0.0, None) == _ffi.E_ARG


# ---- the reference helper: sign, gauge, limits ---------------------------------------------------------------------------------
def _far_case(v_core, ns=97, nt=41):
    """sources of the wake strip near the origin and targets at least 0.5 away from every one of them"""
    rng = np.random.default_rng(7)
    g, xs, zs = S.wake_strip(ns, seed=3)
    xs = xs / 20.0                                      # [-3, 0]: the targets below see many sources at O(1) distances
    xt, zt = rng.uniform(-4.0, 1.0, 20 * nt), rng.uniform(-3.0, 3.0, 20 * nt)
    far = np.hypot(xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]).min(axis=1) >= 0.5 + 2e-3
    assert far.sum() >= nt
    return g, xs, zs, xt[far][:nt], zt[far][:nt], v_core


def _radial_derivatives(g, xs, zs, xt, zt, v_core):
    """psi = sum f(rho), rho = r^2: f'' .. f'''' per pair from the closed form (f' = G / (4 pi s), s' = rho / s), in float64"""
    dx, dz = xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]
    rho = dx * dx + dz * dz
    s = np.sqrt(rho * rho + v_core**4)
    k = np.asarray(g, float)[None, :] / (4 * np.pi)
    f2 = -k * rho / s**3
    f3 = -k * (s**-3 - 3 * rho**2 * s**-5)
    f4 = -k * (-9 * rho * s**-5 + 15 * rho**3 * s**-7)
    return dx, dz, f2, f3, f4


def _d3(d, f2, f3):          # d^3 f(rho) / d d^3 along one coordinate d (rho_d = 2 d, rho_dd = 2), summed over the sources
    return np.abs(8 * d**3 * f3 + 12 * d * f2).sum(axis=1)


def _d4(d, f2, f3, f4):
    return np.abs(16 * d**4 * f4 + 48 * d**2 * f3 + 12 * f2).sum(axis=1)


H = 1e-3


@pytest.mark.parametrize("v_core", [S.V_CORE, 0.3, 0.0])
def test_central_differences_of_the_reference_psi_are_the_oracles_velocity(v_core):
    """u = d psi / dz, w = -d psi / dx (LUDVM.py:565-568) with h = 1e-3; tolerance: ten times the truncation term
    h^2 / 6 max|d^3 psi|, the third derivatives from the closed form (sum over the sources of their magnitudes)"""
    g, xs, zs, xt, zt, vc = _far_case(v_core)
    u, w = O.induced_velocity(g, xs, zs, xt, zt, vc)

    def psi(x, z):
        return S.reference("psi", g, xs, zs, x, z, vc)[0]
    # (float64 values of the long double sums: the rounding, 2^-53 |psi| / h ~ 1e-14, is far below the truncation term)
    u_fd = (psi(xt, zt + H) - psi(xt, zt - H)) / (2 * H)
    w_fd = -(psi(xt + H, zt) - psi(xt - H, zt)) / (2 * H)
    dx, dz, f2, f3, _ = _radial_derivatives(g, xs, zs, xt, zt, vc)
    tol = 10 * H**2 / 6 * max(_d3(dz, f2, f3).max(), _d3(dx, f2, f3).max())
    assert 0 < tol < 1e-3 * max(np.abs(u).max(), np.abs(w).max())          # the check can tell a sign or a factor of 2
    assert np.abs(u_fd - u).max() <= tol, (np.abs(u_fd - u).max(), tol)
    assert np.abs(w_fd - w).max() <= tol, (np.abs(w_fd - w).max(), tol)


def test_the_reference_omega_is_the_curl_of_the_oracles_velocity():
    """omega = dw/dx - du/dz by the same differences, at a core wide enough (0.3) for the vorticity to be large 0.5 away from a
    source; tolerance: ten times h^2 / 6 (max|d^4 psi / dx^4| + max|d^4 psi / dz^4|) from the closed form"""
    g, xs, zs, xt, zt, vc = _far_case(0.3)

    def vel(x, z):
        return O.induced_velocity(g, xs, zs, x, z, vc)
    curl = (vel(xt + H, zt)[1] - vel(xt - H, zt)[1]) / (2 * H) - (vel(xt, zt + H)[0] - vel(xt, zt - H)[0]) / (2 * H)
    ome = S.reference("omega", g, xs, zs, xt, zt, vc)[0]
    dx, dz, f2, f3, f4 = _radial_derivatives(g, xs, zs, xt, zt, vc)
    tol = 10 * H**2 / 6 * (_d4(dx, f2, f3, f4).max() + _d4(dz, f2, f3, f4).max())
    assert 0 < tol < 1e-2 * np.abs(ome).max()
    assert np.abs(curl - ome).max() <= tol, (np.abs(curl - ome).max(), tol)


def test_without_a_core_the_reference_is_the_point_vortex():
    g, xs, zs, xt, zt, _ = _far_case(0.0)
    psi, bound = S.reference("psi", g, xs, zs, xt, zt, 0.0)
    r = np.hypot(xt[:, None] - xs[None, :], zt[:, None] - zs[None, :])
    point = (g[None, :] / (2 * np.pi) * np.log(r)).sum(axis=1)
    assert np.abs(psi - point).max() <= bound.max()
    ome, obound = S.reference("omega", g, xs, zs, xt, zt, 0.0)
    assert np.all(ome == 0) and np.all(obound == 0)


def test_a_point_on_a_source_is_finite_with_a_core():
    val, bound = S.reference("psi", [2.0], [0.25], [-0.5], [0.25], [-0.5], S.V_CORE)
    assert abs(val[0] - 2.0 / (4 * np.pi) * np.log(S.V_CORE**2 / 2)) <= bound[0]
    val, _ = S.reference("omega", [2.0], [0.25], [-0.5], [0.25], [-0.5], S.V_CORE)
    assert abs(val[0] + 2.0 / (np.pi * S.V_CORE**2)) <= 1e-12 * abs(val[0])


def test_the_float64_reference_sum_sits_inside_its_own_bound():
    """a sequential float64 sum of the float64 terms against the long double reference: inside the bound at every size of the
    GPU table (the bound is not one only a lucky order meets)"""
    tile = S.header_constant("kTileF64Few")
    for ns in (1, tile - 1, tile + 1, 4099):
        g, xs, zs = S.wake_strip(ns)
        xt, zt = S.targets(83)
        dx, dz = xt[:, None] - xs[None, :], zt[:, None] - zs[None, :]
        r2 = dx * dx + dz * dz
        s = np.sqrt(r2 * r2 + S.V_CORE**4)
        for kind, terms in (("psi", g / (4 * np.pi) * np.log((r2 + s) / 2)), ("omega", -g * S.V_CORE**4 / (np.pi * s**3))):
            val, bound = S.reference(kind, g, xs, zs, xt, zt, S.V_CORE)
            seq = np.zeros(len(xt))
            for j in range(ns):
                seq = seq + terms[:, j]
            assert np.all(np.abs(seq - val) <= bound), (kind, ns, (np.abs(seq - val) / bound).max())


# ---- the kernels, as the compiler builds them ------------------------------------------------------------------------------------
def test_scalar_kernels_compile_without_scratch():
    """pair_scalar_f64<PSI | OMEGA, 128 | 512> for gfx950 through tools/kernel_resources.py (no GPU needed): no scratch, no spill"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    K = {k: v for k, v in kr.resources(unit="flowfield.hip").items() if "pair_scalar_f64" in k}
    tiles = (S.header_constant("kTileF64Few"), S.header_constant("kTileF64"))
    assert sorted(K) == sorted("_ZN5ludvm15pair_scalar_f64ILi%dELi%dEEEvNS_8PairArgsE" % (kind, t) for kind in (0, 1) for t in tiles)
    for name, r in K.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) in (3 * 8 * tiles[0], 3 * 8 * tiles[1]), (name, r)


# ---- the class on an engine stub -----------------------------------------------------------------------------------------------
class ScalarStub(FakeEngine):
    """FakeEngine plus the two scalar methods: the reference helper's sums, every call recorded"""

    def __init__(self):
        super().__init__()
        self.scalar_calls = []

    def scalar_field(self, kind, circulation, xw, zw, xp, zp, v_core):
        self.scalar_calls.append(("points", kind, np.array(circulation, float), np.array(xw, float), np.array(zw, float), v_core))
        return S.reference(kind, circulation, xw, zw, xp, zp, v_core)[0]

    def flowfield_scalar(self, kind, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None):
        self.scalar_calls.append(("grid", kind, np.array(circulation, float), np.array(xw, float), np.array(zw, float), v_core,
                                  (xmin, zmin, dr, nx, nz, row_first, row_count)))
        x, z = S.grid_points(xmin, zmin, dr, nx, nz, row_first, row_count)
        return S.reference(kind, circulation, xw, zw, x, z, v_core)[0].reshape(-1, nz)


WINDOW = dict(xmin=-1.5, xmax=0.55, zmin=-0.5, zmax=0.5, dr=0.25)
TSTEPS = [0, 1, 9]


@pytest.fixture(scope="module")
def sims():
    kw = dict(CONFIG1, tf=0.6)
    return LUDVM(**kw, verbose=False, engine=ScalarStub()), LUDVM(**kw, verbose=False, engine=FakeEngine())


def test_flowfield_with_flags_hands_the_flowfield_sources_to_the_engine(sims):
    sim, plain = sims
    eng = sim.engine
    del eng.scalar_calls[:]
    sim.flowfield(**WINDOW, tsteps=TSTEPS, psi=True, omega=True)
    nx, nz = sim.x_ff.shape
    assert (nx, nz) == (len(np.arange(-1.5, 0.55, 0.25)), len(np.arange(-0.5, 0.5, 0.25)))
    assert sim.psi_ff.shape == sim.omega_ff.shape == sim.u_ff.shape == (len(TSTEPS), nx, nz)
    assert [c[1] for c in eng.scalar_calls] == ["psi", "omega"] * len(TSTEPS)
    for ii, s in enumerate(TSTEPS):
        g, xw, zw = sim._flowfield_sources(s)
        for call in eng.scalar_calls[2 * ii:2 * ii + 2]:
            assert call[0] == "grid" and call[5] == sim.v_core
            assert np.array_equal(call[2], np.asarray(g, float)) and np.array_equal(call[3], xw) and np.array_equal(call[4], zw)
            assert call[6] == (WINDOW["xmin"], WINDOW["zmin"], WINDOW["dr"], nx, nz, 0, None)
        # the mesh the engine generates is the class's x_ff, z_ff
        ref = S.reference("psi", g, xw, zw, sim.x_ff.ravel(), sim.z_ff.ravel(), sim.v_core)
        assert np.all(np.abs(sim.psi_ff[ii].ravel() - ref[0]) <= ref[1] + 1e-13)       # (arange's mesh against xmin + i dr)
    # the velocity fields and the stencil's vorticity are what they are without the flags
    plain.flowfield(**WINDOW, tsteps=TSTEPS)
    for name in ("x_ff", "z_ff", "u_ff", "w_ff", "ome_ff"):
        assert np.array_equal(getattr(sim, name), getattr(plain, name)), name


def test_one_flag_sets_one_attribute_and_the_default_call_sets_neither():
    kw = dict(CONFIG1, tf=0.6)
    sim = LUDVM(**kw, verbose=False, engine=ScalarStub())
    sim.flowfield(**WINDOW, tsteps=[1])
    assert not hasattr(sim, "psi_ff") and not hasattr(sim, "omega_ff") and sim.engine.scalar_calls == []
    sim.flowfield(**WINDOW, tsteps=[1], psi=True)
    assert hasattr(sim, "psi_ff") and not hasattr(sim, "omega_ff")
    assert [c[1] for c in sim.engine.scalar_calls] == ["psi"]
    sim.flowfield(**WINDOW, tsteps=[1], omega=True)
    assert sim.omega_ff.shape == sim.ome_ff.shape
    assert [c[1] for c in sim.engine.scalar_calls] == ["psi", "omega"]


def test_an_engine_without_the_methods_is_refused_by_name(sims):
    _, plain = sims
    with pytest.raises(RuntimeError, match="flowfield_scalar"):
        plain.flowfield(**WINDOW, tsteps=[1], psi=True)
    with pytest.raises(RuntimeError, match="scalar_field"):
        plain.stream_function([1.0], [0.0], [0.0], [1.0], [1.0])
    plain.flowfield(**WINDOW, tsteps=[1])              # ... and the plain call goes on working


def test_a_sharded_run_is_refused_before_any_engine_call():
    sim = LUDVM(**dict(CONFIG1, tf=0.6), verbose=False, engine=ScalarStub())
    calls = dict(sim.engine.calls)
    sim._shard = types.SimpleNamespace(world=2)          # what a `distributed` run and every replica of a `devices` run carry
    for kw in (dict(psi=True), dict(omega=True)):
        with pytest.raises(ValueError, match="one GPU"):
            sim.flowfield(**WINDOW, tsteps=[1], **kw)
    with pytest.raises(ValueError, match="one GPU"):
        sim.stream_function([1.0], [0.0], [0.0], [1.0], [1.0])
    with pytest.raises(ValueError, match="one GPU"):
        sim.vorticity([1.0], [0.0], [0.0], [1.0], [1.0])
    assert sim.engine.scalar_calls == [] and sim.engine.calls == calls


def test_point_methods_take_induced_velocitys_arguments(sims):
    sim, _ = sims
    del sim.engine.scalar_calls[:]
    g, xs, zs = S.wake_strip(5)
    xt, zt = S.targets(3)
    psi = sim.stream_function(g, xs, zs, xt, zt)
    ome = sim.vorticity(g, xs, zs, xt, zt, viscous=False)
    assert psi.shape == ome.shape == (3,) and np.all(ome == 0)
    assert [(c[1], c[5]) for c in sim.engine.scalar_calls] == [("psi", sim.v_core), ("omega", 0)]
    import inspect
    names = [list(inspect.signature(getattr(LUDVM, m)).parameters) for m in ("induced_velocity", "stream_function", "vorticity")]
    assert names[0] == names[1] == names[2]
