"""CPU tier: the tracers' deformation gradient in hi+lo fp32 (LUDVM(..., tracers=, tracer_precision='f32x2',
tracer_gradient='f32x2')) -- the NumPy restatement of the fused walk against the two restatements it
fuses, twelve Euler steps of it against the float64 recursion within the derived tolerance, the keyword's refusals (from the
keywords alone), the errors of an engine that cannot serve it, what the object and a checkpoint carry, the C ABI of the new
entry and the compiler's report of the new kernel.  The kernel itself runs in tests/test_gpu_tracer_gradient_f32x2.py."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gradient_f32x2_common as GF
import tracer_gradient_common as TG
import tracer_gradient_f32x2_common as C
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from tracers_f32x2_common import hilo_f32_field

NAME = "ludvm_march_set_tracer_gradient_f32x2"


def _host_cases():
    cases = dict(GF.host_cases())
    cases["ns257"] = GF.case(257, 512, GF.V_CORE)          # one whole tile and one source
    return cases


@pytest.mark.parametrize("name", ["strip", "small_core", "at_-5000", "ns255", "ns257"])
def test_the_fusion_changes_neither_scheme(name):
    """One pass over the sources: with every float32 product and sum rounded, (u, w) of the fused walk ARE
    tracers_f32x2_common.hilo_f32_field's arrays; with the multiply-adds fused as the kernel has them, (A, B, C) ARE
    gradient_f32x2_common.hilo_f32_sums' arrays.  Under either rounding model all five sums come from one set of dx, dz, r2, y and
    G y, and the two models' own results differ by float32 roundings only."""
    g, xs, zs, xt, zt, v_core = _host_cases()[name]
    xt, zt = xt[:96], zt[:96]                                # (32 on top of sources, 32 at 0.3 v_core, 32 of the grid)
    u, w = hilo_f32_field(g, xs, zs, xt, zt, v_core)
    A, B, Cc = GF.hilo_f32_sums(g, xs, zs, xt, zt, v_core)
    plain = C.fused_hilo_f32(g, xs, zs, xt, zt, v_core, rounding="plain")
    fused = C.fused_hilo_f32(g, xs, zs, xt, zt, v_core, rounding="fused")
    assert np.array_equal(plain[0], u) and np.array_equal(plain[1], w)
    assert np.array_equal(fused[2], A) and np.array_equal(fused[3], B) and np.array_equal(fused[4], Cc)
    # the other model's arrays: the same sums up to float32 roundings of a term (the bound's float32 part, over the 2 pi where scaled)
    ns = len(g)
    mag = GF.gradient_reference(g, xs, zs, xt, zt, v_core)[1] / ((GF.H + GF.K32) * GF.EPS32 + (ns + 16) * GF.EPS64)
    for k, scale in ((2, np.pi), (3, 2 * np.pi), (4, 2 * np.pi / v_core ** 4)):
        assert (np.abs(plain[k] - fused[k]) <= 2 * GF.bound(ns, mag) * scale).all(), (name, k)
    vel = max(np.abs(u).max(), np.abs(w).max())
    assert max(np.abs(fused[0] - u).max(), np.abs(fused[1] - w).max()) <= 2e-6 * vel


def _synthetic(ns=300, M=37, seed=9):
    """a frozen wake-like source set of ns vortices (more than one 256-source tile) with 9 bound vortices, M seeds above and below
    it, released at 1, 4 and never in turn"""
    rng = np.random.default_rng(seed)
    src = (rng.normal(0, 0.3, ns), rng.uniform(-2.0, 0.0, ns), rng.normal(0, 0.3, ns), rng.normal(0, 0.1, 9), np.linspace(0, 1, 9),
           np.zeros(9))
    seeds = np.stack([rng.uniform(-2.0, 1.0, M), rng.uniform(0.5, 1.0, M) * np.where(np.arange(M) % 2, 1, -1)])
    rel = np.array([1, 4, 99], dtype=np.int64)[np.arange(M) % 3]
    return src, seeds, rel


def test_twelve_steps_stay_within_the_accumulated_tolerance_of_the_float64_recursion():
    """37 tracers through 12 steps of the restated route over 309 frozen sources.  Both recursions take every step from the
    restated path's start positions; the float64 one is tracer_gradient_common.step_F.  A step adds its own tolerance
    (tracer_gradient_f32x2_common.step_tolerance) to what the product carries over: err_i <= (I + dt (|G| + b)) err_{i-1} + tol_i,
    component by component.  The largest per-step tolerance is below 1e-2 of the largest single increment, which exceeds 1e-6.
    Held tracers keep the exact identity."""
    src, seeds, rel = _synthetic()
    M, dt, v_core = seeds.shape[1], 0.05, 0.0195
    F, F64, cur = TG.identity(M), TG.identity(M), None
    acc = np.zeros([4, M])
    tol_max, inc_max, worst = 0.0, 0.0, 0.0
    for i in range(1, 13):
        start = np.where(rel == i, seeds, seeds if cur is None else cur)
        tol, b = C.step_tolerance(F, start, rel, i, dt, v_core, src)
        free = rel <= i
        ux, uz, wx = (np.zeros(M) for _ in range(3))
        ux[free], uz[free], wx[free] = (np.abs(a) for a in TG.step_gradient(src, start[0][free], start[1][free], v_core))
        a11, a12, a21, a22 = acc
        acc = np.stack([a11 + dt * ((ux + b) * a11 + (uz + b) * a21), a12 + dt * ((ux + b) * a12 + (uz + b) * a22),
                        a21 + dt * ((wx + b) * a11 + (ux + b) * a21), a22 + dt * ((wx + b) * a12 + (ux + b) * a22)])
        acc += tol + np.where(free, C.ROUNDING * np.abs(F).max(), 0.0)
        cur, F = C.restated_step(F, seeds, cur, rel, i, dt, v_core, src)
        F64, inc = TG.step_F(F64, start, rel, i, dt, v_core, src)
        diff = np.abs(F - F64)
        assert (diff <= acc).all(), (i, float((diff / np.maximum(acc, 1e-300)).max()))
        worst = max(worst, float((diff[:, free] / acc[:, free]).max()))
        tol_max, inc_max = max(tol_max, float(tol.max())), max(inc_max, float(np.abs(inc).max()))
    held = rel > 12
    print(f"12 steps: worst {worst:.3f} of the accumulated tolerance; largest step tolerance {tol_max:.2e} = {tol_max / inc_max:.2e} of "
          f"the largest single increment ({inc_max:.3e}); |F - F64| <= {np.abs(F - F64).max():.2e}")
    assert inc_max > 1e-6 and tol_max < 1e-2 * inc_max
    assert held.any() and np.array_equal(F[:, held], TG.identity(int(held.sum()))) and np.array_equal(cur[:, held], seeds[:, held])
    assert np.abs(F[:, ~held] - TG.identity(int((~held).sum()))).max() > 1e-2
    assert not np.array_equal(F[:, ~held], F64[:, ~held])


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before tracer_gradient was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    import ludvm_amd.multi as multi
    monkeypatch.setattr(multi, "MultiDeviceLUDVM", NoEngine)
    ok = np.zeros([2, 3])
    f32 = dict(tracer_precision="f32x2", tracer_gradient="f32x2")
    with pytest.raises(ValueError, match="tracer_gradient needs `tracers`"):
        LUDVM(**CONFIG1, verbose=False, tracer_gradient="f32x2")
    with pytest.raises(ValueError, match="tracer_gradient='f32x2' needs tracer_precision='f32x2'.*'f64'"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient="f32x2")
    with pytest.raises(ValueError, match="tracer_gradient='f32x2' needs tracer_precision='f32x2'.*'f64'"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient="f32x2", tracer_precision="f64")
    # True with hi+lo tracers stays refused, and now names the way out; other values keep their message, extended
    with pytest.raises(ValueError, match="^tracer_gradient needs float64 tracers.*'f32x2'.*tracer_gradient='f32x2'"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, tracer_precision="f32x2")
    for bad in ("f32", "F32X2", "f64", 2, None):
        with pytest.raises(ValueError, match="^tracer_gradient must be True or False, or 'f32x2'"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_precision="f32x2", tracer_gradient=bad)
    for kw in (dict(march=False), dict(march=False, run=False)):
        with pytest.raises(ValueError, match="march=False"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, **f32, **kw)
    with pytest.raises(ValueError, match="tracer_gradient is evaluated inside the device-resident march: not with march=False"):
        M.LUDVM._check_tracer_gradient("f32x2", True, False, "f32x2")
    for dist in ("rccl", True):
        with pytest.raises(ValueError, match="one GPU"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, **f32, distributed=dist)
    with pytest.raises(ValueError, match="tracer_gradient runs on one GPU.*devices"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, **f32, devices=[0, 1])
    with pytest.raises(ValueError, match="tracer_gradient='f32x2' needs tracer_precision='f32x2'"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient="f32x2", devices=[0, 1])


def test_a_sweep_refuses_the_value():
    member = dict(CONFIG1, tf=1.0)
    ok = np.zeros([2, 3])
    with pytest.raises(ValueError, match=r"sweep: tracer_gradient='f32x2'.*LUDVM\(\.\.\., tracers="):
        LUDVM.sweep([member, member], particles=ok, tracer_gradient="f32x2")
    with pytest.raises(ValueError, match=r"sweep: member 1: tracer_gradient='f32x2'.*LUDVM\(\.\.\., tracers="):
        LUDVM.sweep([member, dict(member, tracer_gradient="f32x2")], particles=ok)


class Marcher(FakeEngine):
    def march_run(self, *a, **k):
        raise AssertionError("the march was entered")

    def march_setup(self, *a, **k):
        raise AssertionError("the march was set up")

    def march_set_tracers(self, *a, **k):
        raise AssertionError("the tracers were set")

    def march_set_tracer_precision(self, *a, **k):
        raise AssertionError("the precision was set")

    def march_set_tracer_gradient(self, *a, **k):
        raise AssertionError("the float64 gradient was set")


def test_a_run_that_cannot_take_the_march_raises():
    """tracer_gradient='f32x2' over an engine that does not march, over one that marches with both older setters but without the
    new entry, and in a run the march does not take: RuntimeError, no step run."""
    kw = dict(CONFIG1, tf=1.0)
    f32 = dict(tracers=[[1.0], [0.5]], tracer_precision="f32x2", tracer_gradient="f32x2")
    with pytest.raises(RuntimeError, match="tracer_gradient='f32x2'.*cannot take"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), **f32)
    with pytest.raises(RuntimeError, match="tracer_gradient='f32x2'.*march_set_tracer_gradient_f32x2"):
        LUDVM(**kw, verbose=False, engine=Marcher(), **f32)

    class Full(Marcher):
        def march_set_tracer_gradient_f32x2(self, *a, **k):
            raise AssertionError("the gradient was set")
    with pytest.raises(RuntimeError, match="tracer_gradient='f32x2'.*cannot take"):
        LUDVM(**dict(kw, Ncoeffs=70), verbose=False, engine=Full(), **f32)


def test_the_class_calls_the_one_setter_behind_the_tracers():
    """the new entry sets precision and gradient together: neither of the older setters is called"""
    seen = []

    class Stop(Exception):
        pass

    class Recorder(FakeEngine):
        def march_setup(self, *a, **k):
            seen.append("setup")

        def march_set_tracers(self, *a, **k):
            seen.append("tracers")

        def march_set_tracer_precision(self, precision):
            seen.append(("precision", precision))

        def march_set_tracer_gradient(self, on, F=None):
            seen.append(("gradient", on, F))

        def march_set_tracer_gradient_f32x2(self, F=None):
            seen.append(("gradient_f32x2", F))

        def march_anchor_steps(self, *a, **k):      # (the first thing a march call asks the engine)
            raise Stop

        def march_run(self, *a, **k):
            raise Stop
    common = dict(verbose=False, engine=Recorder(), history="sparse", tracers=[[1.0], [0.5]])
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), **common, tracer_precision="f32x2", tracer_gradient="f32x2")
    assert seen == ["setup", "tracers", ("gradient_f32x2", None)]
    del seen[:]
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), **common, tracer_precision="f32x2")
    assert seen == ["setup", "tracers", ("precision", "f32x2")]
    del seen[:]
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), **common, tracer_gradient=True)
    assert seen == ["setup", "tracers", ("gradient", True, None)]


class StateEngine(FakeEngine):
    """what `_write_checkpoint_file` asks of a marching engine"""

    def __init__(self, xz, F):
        super().__init__()
        self._xz, self._F = xz, F

    def march_tracer_state(self):
        return self._xz.copy()

    def march_tracer_gradient_state(self):
        return self._F.copy()


def test_the_object_and_a_checkpoint_carry_the_value(tmp_path):
    """`tracer_gradient` holds 'f32x2' (truthy), the constructor keywords store it, a checkpoint carries F as the float64 route's
    does and a second object built from the stored keywords is on the same route; 48 bytes per tracer and recorded row."""
    rng = np.random.default_rng(3)
    seeds = np.stack([np.linspace(0.0, 1.0, 5), np.full(5, 1.2)])
    cur, F_cur, F_3 = seeds + 0.1, rng.normal(1.0, 0.2, (4, 5)), rng.normal(1.0, 0.1, (4, 5))
    ck = str(tmp_path / "ck.npz")
    kw = dict(CONFIG1, tf=1.0)
    f32 = dict(tracer_precision="f32x2", tracer_gradient="f32x2")
    sim = LUDVM(**kw, verbose=False, engine=StateEngine(cur, F_cur), tracers=seeds, tracer_steps=[3, 8, 12], **f32, run=False,
                checkpoint_path=ck)
    assert sim.tracer_gradient == "f32x2" and sim.tracer_gradient and sim.tracer_precision == "f32x2"
    assert sim._ctor["tracer_gradient"] == "f32x2" and sim._ctor["tracer_precision"] == "f32x2"
    S = sim._loop_begin()
    sim._free_slot, sim.itev, sim.ilev = S.fslot, 0, 0     # (what time_loop has set by the time it writes a checkpoint)
    S.can_march = True
    assert np.array_equal(sim.tracer_F_path[0], TG.identity(5)) and S.tF is None
    sim.tracer_path.store(3, cur - 0.05)
    sim.tracer_F_path.store(3, F_3)
    sim._write_checkpoint_file(S, 6)
    R = np.load(ck, allow_pickle=False)
    assert np.array_equal(R["tracer_F_cur"], F_cur) and np.array_equal(R["tracer_cur"], cur)
    assert list(R["tracer_rows_steps"]) == [0, 3] and np.array_equal(R["tracer_F_rows"], np.stack([TG.identity(5), F_3]))
    ctor = json.loads(str(R["ctor"]))
    assert ctor["tracer_gradient"] == "f32x2" and ctor["tracer_precision"] == "f32x2"
    again = LUDVM(**ctor, verbose=False, engine=StateEngine(cur, F_cur), run=False)
    assert again.tracer_gradient == "f32x2"
    S2 = again._loop_begin()
    again._loop_restore(S2, R)
    assert np.array_equal(S2.tF, F_cur) and np.array_equal(S2.tcur, cur) and S2.first_step == 6
    assert again.tracer_F_path.steps() == [0, 3] and np.array_equal(again.tracer_F_path[3], F_3)
    T = sim.dt * 3.0
    assert np.array_equal(again.tracer_ftle(step=3), LUDVM.ftle_from_F(F_3, np.full(5, T)))

    class Capped(LUDVM):
        _tracer_call_bytes = 48 * 5 * 2
    c = Capped(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_steps=range(1, 21), **f32, run=False)
    Sc = c._loop_begin()
    Sc.can_march, Sc.dense_march, Sc.march_chunk = True, False, 32768
    c.history, c.snapshot_steps = "sparse", set()
    j, _ = c._march_extent(Sc, 1)
    assert j - 1 == 2, j


def test_header_exports_and_binding_agree_on_the_new_entry():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert NAME in _ffi.SIGNATURES and len(_ffi.SIGNATURES[NAME]) == 2 and NAME in _ffi.ADDED_IN_ABI_7
    assert hasattr(lib, NAME) and hasattr(_ffi.load(_ffi.EXP_LIB_PATH), NAME)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*ludvm_ctx\s*\*\s*ctx\s*,\s*const\s+double\s*\*\s*F\s*\)\s*;", code)
    assert re.search(r"\bT " + NAME + r"$", exported, flags=re.M)
    assert getattr(lib, NAME)(None, None) == _ffi.E_ARG
    from ludvm_amd.engine import Engine
    assert callable(getattr(Engine, "march_set_tracer_gradient_f32x2"))


def test_the_fused_kernel_uses_no_scratch_and_its_neighbours_are_compiled_as_before():
    """march_f32x2_grad_tracer_partial for gfx950 through tools/kernel_resources.py (no GPU needed): no scratch, no spills, the
    five float planes of one 256-source tile in LDS, four waves per SIMD as the plain hi+lo kernel has; the figures DESIGN.md
    section 4.18 quotes are printed.  The plain hi+lo kernel and the float64 gradient kernel beside it keep what they had."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.resources(unit="march.hip")
    (name, r), = {k: v for k, v in report.items() if "march_f32x2_grad_tracer_partial" in k}.items()
    print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == 5 * C.TILE * 4 and int(r["Occupancy [waves/SIMD]"]) >= 4, r
    before = {"march_f32x2_tracer_partial": (122, 5120, 0), "march_grad_tracer_partial": (68, 6144, 0),
              "march_grad_tracer_finish": (48, 0, 0)}
    for kernel, want in before.items():
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        assert (int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"])) == want, (name, r)
    kernels = open(os.path.join(ROOT, "ludvm_amd", "csrc", "march_kernels.hpp")).read()
    per_lane = int(re.search(r"constexpr int kTracerGradF32PerLane = (\d+);", kernels).group(1))
    assert _ffi.TRACER_F32X2_PER_LANE % per_lane == 0       # whole workgroups per tile of the plan
