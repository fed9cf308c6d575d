"""CPU tier of the hi+lo fp32 route of the analytic vorticity and the velocity gradient (ludvm_scalar_f32x2,
ludvm_flowfield_scalar_rows_f32x2, ludvm_gradient_f32x2, ludvm_flowfield_gradient_rows_f32x2; Engine's precision='f32x2';
LUDVM.flowfield(field_precision='f32x2')).

What a GPU is not needed for: the scheme, restated in NumPy (tests/gradient_f32x2_common.py), meets the bound the GPU tier holds
the kernel to -- the bound can be met, with the margin DESIGN.md section 4.17 quotes; the kernels compile without scratch; the
symbols are declared, bound and exported; the engine refuses what has no fp32 route before it reaches the library; the class's
part on an engine stub."""
import fnmatch
import importlib.util
import os
import re
import types

import numpy as np
import pytest

import gradient_common as G
import gradient_f32x2_common as C
import scalar_field_common as S
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import LUDVM, Engine, _ffi

NAMES = ("ludvm_scalar_f32x2", "ludvm_flowfield_scalar_rows_f32x2", "ludvm_gradient_f32x2", "ludvm_flowfield_gradient_rows_f32x2")
TIER = 2e-6                     # direct_shapes_common.TOL["hilo"], the project's hi+lo tier


# ---- the scheme -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.host_cases()))
def test_the_restated_scheme_meets_the_bound_and_the_tier(name):
    inputs = C.host_cases()[name]
    ns = len(inputs[0])
    chunk, nsplit = C.plan(len(inputs[3]), ns)
    assert nsplit == (12 if ns == 3000 else 1)
    unit_of = lambda bound: bound / ((C.H + C.K32) + (ns + 16) * C.EPS64 / C.EPS32)       # noqa: E731  (eps32 mag)
    vals, bound = C.gradient_reference(*inputs)
    got = C.hilo_f32_gradient(*inputs, chunk=chunk)
    scale = max(np.abs(v).max() for v in vals)
    for comp, a, v in zip(G.NAMES, got, vals):
        err = np.abs(a - v)
        print(name, comp, "worst error: %.2f eps32 mag, %.2e of max|grad u|" % ((err / unit_of(bound)).max(), err.max() / scale))
        assert np.all(err <= bound), (name, comp)
        assert err.max() <= TIER * scale
        assert (err / unit_of(bound)).max() < 0.1 * (C.H + C.K32)         # the 15x margin the GPU tier's tier test leans on
    ome, obound = C.omega_reference(*inputs)
    got = C.hilo_f32_omega(*inputs, chunk=chunk)
    err = np.abs(got - ome)
    print(name, "omega worst error: %.2f eps32 mag, %.2e of max|omega|" % ((err / unit_of(obound)).max(), err.max() / np.abs(ome).max()))
    assert np.all(err <= obound) and err.max() <= TIER * np.abs(ome).max()


def test_the_bound_tells_a_wrong_term_and_the_scheme_needs_its_low_parts():
    """the bound is far below the field (a wrong sign or factor cannot hide in it), and without the lo parts -- plain fp32
    coordinates at x ~ -5000 -- the same arithmetic misses it: the cases can tell the scheme from its absence"""
    g, xs, zs, xt, zt, vc = C.host_cases()["at_-5000"]
    vals, bound = C.gradient_reference(g, xs, zs, xt, zt, vc)
    assert np.median(bound) < 1e-4 * max(np.abs(v).max() for v in vals)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                              # noqa: E731
    got = C.hilo_f32_gradient(g, f32(xs), f32(zs), f32(xt), f32(zt), vc)
    assert any(np.any(np.abs(a - v) > bound) for a, v in zip(got, vals))


def test_the_rule_is_a_function_of_the_two_counts_with_whole_tiles():
    for nt, ns in ((1, 1), (1, C.TILE + 1), (C.WORKGROUP + 1, 3000), (1 << 24, 200000), (5, 10**6)):
        chunk, nsplit = C.plan(nt, ns)
        assert chunk % C.TILE == 0 and (nsplit - 1) * chunk < ns <= nsplit * chunk and 1 <= nsplit <= 64, (nt, ns, chunk, nsplit)
    assert C.plan(1, C.TILE + 1) == (C.TILE, 2)              # the smallest launch that splits, its last split ragged


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def test_the_kernels_compile_without_scratch():
    """field_hilo_f32<omega | gradient, points per lane> for gfx950 through tools/kernel_resources.py (no GPU needed): both
    instantiations present, no scratch, no spill, five float planes of one tile in LDS"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    K = {k: v for k, v in kr.resources(unit="flowfield.hip").items() if "field_hilo_f32" in k}
    assert sorted(K) == sorted("_ZN5ludvm14field_hilo_f32ILb%dELi%dEEEvNS_8PairArgsE" % (grad, C.PER_LANE) for grad in (0, 1))
    for name, r in K.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) == 5 * 4 * C.TILE, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r)
        for other in ("pair_grad", "finish_grad", "pair_scalar_f64", "march_tracer_"):      # (what other tests select kernels by)
            assert other not in name


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return [p.strip() for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")]


def test_symbols_are_declared_like_their_twins_bound_exported_and_listed_as_additions():
    lib, exp = _ffi.load(), _ffi.load(_ffi.EXP_LIB_PATH)
    patterns = re.search(r"global:\s*([^;]*);", open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()).group(1).split()
    for name in NAMES:
        twin = name[:-len("f32x2")] + "f64"
        assert _prototype(name) == _prototype(twin), name                    # the same arguments, float64 in and out
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[twin]
        assert name in _ffi.ADDED_IN_ABI_7
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
        assert hasattr(lib, name) and hasattr(exp, name)
    assert _ffi.ABI_VERSION == 7


def test_a_null_context_is_refused():
    lib = _ffi.load()
    assert lib.ludvm_scalar_f32x2(None, 1, None, None, None, 0, None, None, 0, 0.1, None) == _ffi.E_ARG
    assert lib.ludvm_flowfield_scalar_rows_f32x2(None, 1, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None, 0, 0.1, None) == _ffi.E_ARG
    assert lib.ludvm_gradient_f32x2(None, None, None, None, 0, None, None, 0, 0.1, None, None, None) == _ffi.E_ARG
    assert lib.ludvm_flowfield_gradient_rows_f32x2(None, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None, 0, 0.1, None, None,
                                                   None) == _ffi.E_ARG


# ---- the engine: refusals that need no device -----------------------------------------------------------------------------------------
def test_the_engine_refuses_psi_and_unknown_precisions_before_the_library():
    eng = object.__new__(Engine)                         # no context: a call that got as far as the library would fail otherwise
    eng._lib = _ffi.load()
    one = [0.0]
    with pytest.raises(ValueError, match="no fp32 route"):
        eng.scalar_field("psi", one, one, one, one, one, 0.1, precision="f32x2")
    with pytest.raises(ValueError, match="no fp32 route"):
        eng.flowfield_scalar(_ffi.FIELD_KINDS["psi"], 0.0, 0.0, 0.5, 2, 2, one, one, one, 0.1, precision="f32x2")
    for call in (lambda p: eng.scalar_field("omega", one, one, one, one, one, 0.1, precision=p),
                 lambda p: eng.flowfield_scalar("omega", 0.0, 0.0, 0.5, 2, 2, one, one, one, 0.1, precision=p),
                 lambda p: eng.gradient_field(one, one, one, one, one, 0.1, precision=p),
                 lambda p: eng.flowfield_gradient(0.0, 0.0, 0.5, 2, 2, one, one, one, 0.1, precision=p)):
        for bad in ("f32", "auto", None, 64):
            with pytest.raises(ValueError, match="precision"):
                call(bad)


# ---- the class on an engine stub ---------------------------------------------------------------------------------------------------
class OldStub(FakeEngine):
    """FakeEngine plus the field methods with the signatures they had before the route: a `precision` keyword would be an error"""

    def __init__(self):
        super().__init__()
        self.field_calls = []

    def flowfield_scalar(self, kind, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None):
        self.field_calls.append((kind, None))
        return np.full((nx, nz), 1.0 if kind == "psi" else 2.0)

    def flowfield_gradient(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None):
        self.field_calls.append(("grad", None))
        return tuple(np.full((nx, nz), v) for v in (3.0, 4.0, 5.0))


class NewStub(FakeEngine):
    """... and with the keyword: every call recorded with the precision it asked for"""

    def __init__(self):
        super().__init__()
        self.field_calls = []

    def flowfield_scalar(self, kind, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None,
                         precision="f64"):
        self.field_calls.append((kind, precision))
        return np.full((nx, nz), (1.0 if kind == "psi" else 2.0) + (0.5 if precision == "f32x2" else 0.0))

    def flowfield_gradient(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None,
                           precision="f64"):
        self.field_calls.append(("grad", precision))
        return tuple(np.full((nx, nz), v + (0.5 if precision == "f32x2" else 0.0)) for v in (3.0, 4.0, 5.0))


WINDOW = dict(xmin=-1.5, xmax=0.55, zmin=-0.5, zmax=0.5, dr=0.25)


@pytest.fixture(scope="module")
def sims():
    kw = dict(CONFIG1, tf=0.6)
    return tuple(LUDVM(**kw, verbose=False, engine=e()) for e in (OldStub, NewStub, FakeEngine))


def test_the_default_calls_the_engine_as_before(sims):
    old, new, _ = sims
    for sim in (old, new):
        del sim.engine.field_calls[:]
    old.flowfield(**WINDOW, tsteps=[1], psi=True, omega=True, grad=True)          # (an engine of the old signatures: no keyword)
    old.flowfield(**WINDOW, tsteps=[1], psi=True, omega=True, grad=True, field_precision="f64")
    assert old.engine.field_calls == 2 * [("psi", None), ("omega", None), ("grad", None)]
    new.flowfield(**WINDOW, tsteps=[1], psi=True, omega=True, grad=True)
    assert new.engine.field_calls == [("psi", "f64"), ("omega", "f64"), ("grad", "f64")]


def test_f32x2_reaches_omega_and_the_gradient_and_leaves_psi_in_float64(sims):
    _, new, _ = sims
    del new.engine.field_calls[:]
    new.flowfield(**WINDOW, tsteps=[1], psi=True, omega=True, grad=True)
    before = {n: getattr(new, n).copy() for n in ("u_ff", "w_ff", "ome_ff", "psi_ff")}
    new.flowfield(**WINDOW, tsteps=[1], psi=True, omega=True, grad=True, field_precision="f32x2")
    assert new.engine.field_calls[3:] == [("psi", "f64"), ("omega", "f32x2"), ("grad", "f32x2")]
    for n, b in before.items():
        assert np.array_equal(getattr(new, n), b), n
    assert np.all(new.omega_ff == 2.5) and np.all(new.ux_ff == 3.5) and np.all(new.uz_ff == 4.5) and np.all(new.wx_ff == 5.5)
    assert np.array_equal(new.q_ff, -new.ux_ff * new.ux_ff - new.uz_ff * new.wx_ff)
    # alone, each flag takes the route too; without either the keyword governs nothing and nothing is asked of the engine
    del new.engine.field_calls[:]
    new.flowfield(**WINDOW, tsteps=[1], omega=True, field_precision="f32x2")
    new.flowfield(**WINDOW, tsteps=[1], grad=True, field_precision="f32x2")
    new.flowfield(**WINDOW, tsteps=[1], psi=True, field_precision="f32x2")
    assert new.engine.field_calls == [("omega", "f32x2"), ("grad", "f32x2"), ("psi", "f64")]


def test_refusals(sims):
    old, new, plain = sims
    del new.engine.field_calls[:]
    for bad in ("f32", "auto", None, True):
        with pytest.raises(ValueError, match="field_precision"):
            new.flowfield(**WINDOW, tsteps=[1], grad=True, field_precision=bad)
    # an engine whose methods do not know the keyword, or that has no such methods
    with pytest.raises(RuntimeError, match="f32x2"):
        old.flowfield(**WINDOW, tsteps=[1], grad=True, field_precision="f32x2")
    with pytest.raises(RuntimeError, match="f32x2"):
        old.flowfield(**WINDOW, tsteps=[1], omega=True, field_precision="f32x2")
    with pytest.raises(RuntimeError, match="flowfield_gradient"):
        plain.flowfield(**WINDOW, tsteps=[1], grad=True, field_precision="f32x2")
    # a sharded run, before any engine call
    sim = LUDVM(**dict(CONFIG1, tf=0.6), verbose=False, engine=NewStub())
    calls = dict(sim.engine.calls)
    sim._shard = types.SimpleNamespace(world=2)
    for flags in (dict(grad=True), dict(omega=True), {}):
        with pytest.raises(ValueError, match="one GPU"):
            sim.flowfield(**WINDOW, tsteps=[1], field_precision="f32x2", **flags)
    assert sim.engine.field_calls == [] and sim.engine.calls == calls and new.engine.field_calls == []
