"""CPU tier: the deformation gradient of the marched tracers (LUDVM(..., tracers=, tracer_gradient=True); DESIGN.md section
4.15) -- `ftle_from_F` against numpy's SVD, the NumPy recursion of tests/tracer_gradient_common.py against differences of
neighbouring paths, the keyword's refusals (from the keywords alone), the sweep's refusals, the errors of an engine that cannot
serve it, what the object and a checkpoint carry, the C ABI of the three entry points, and the compiler's report of the two
kernels.  The kernels themselves run in tests/test_gpu_tracer_gradient.py."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import tracer_gradient_common as TG
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from tracers_common import euler_step

NAMES = ("ludvm_march_set_tracer_gradient", "ludvm_march_read_tracer_gradient", "ludvm_march_tracer_gradient_state")


def test_ftle_from_F_is_numpys_largest_singular_value():
    rng = np.random.default_rng(5)
    F = rng.normal(0.0, 1.5, (4, 400))
    F[:, :50] = TG.identity(50) + 1e-9 * rng.normal(0.0, 1.0, (4, 50))      # close singular values
    F[:, 50] = [1.0, 0.0, 0.0, 1.0]
    c, s = np.cos(0.3), np.sin(0.3)
    F[:, 51] = [c, -s, s, c]                                                # a rotation: no stretching
    T = rng.uniform(0.05, 20.0, 400)
    T[60:70] = 0.0
    T[70:80] = -1.0
    sigma = np.linalg.svd(np.moveaxis(F.reshape(2, 2, -1), -1, 0), compute_uv=False)[:, 0]
    got = LUDVM.ftle_from_F(F, T)
    assert got.shape == (400,) and np.isnan(got[60:80]).all() and np.isfinite(np.delete(got, np.s_[60:80])).all()
    ok = T > 0
    # ln sigma to a few ulp of sigma
    assert np.abs(got[ok] * T[ok] - np.log(sigma[ok])).max() <= 1e-14 * max(1.0, np.abs(np.log(sigma)).max())
    assert got[50] == 0.0 and abs(got[51]) * T[51] <= 1e-15
    # one time for all, a mesh of tracers, one matrix
    assert np.array_equal(LUDVM.ftle_from_F(F, 2.0), LUDVM.ftle_from_F(F, np.full(400, 2.0)))
    assert LUDVM.ftle_from_F(F.reshape(4, 20, 20), T.reshape(20, 20)).shape == (20, 20)
    assert np.isclose(float(LUDVM.ftle_from_F([2.0, 0.0, 0.0, 0.5], 4.0)), np.log(2.0) / 4.0, rtol=1e-15)
    assert np.isnan(LUDVM.ftle_from_F([2.0, 0.0, 0.0, 0.5], 0.0))
    with pytest.raises(ValueError, match=r"\[4, \.\.\.\]"):
        LUDVM.ftle_from_F(np.zeros([2, 2, 5]), 1.0)


def test_the_recursion_is_the_derivative_of_the_discrete_map():
    """The NumPy recursion the GPU tier is checked against, against what it claims to be: centred differences of neighbouring
    Euler paths (tracers_common.euler_step, the oracle's sums) through 12 steps of a frozen wake-like source set, seeds moved by
    h = 1e-5 in X and in Z: 1e-8 of max|F| (truncation h^2, rounding eps / h)."""
    rng = np.random.default_rng(9)
    ns, M, dt, v_core, h = 120, 7, 0.05, 0.0195, 1e-5
    src = (rng.normal(0, 0.3, ns), rng.uniform(-2.0, 0.0, ns), rng.normal(0, 0.3, ns), rng.normal(0, 0.1, 9), np.linspace(0, 1, 9),
           np.zeros(9))
    seeds = np.stack([rng.uniform(-2.0, 1.0, M), rng.uniform(0.5, 1.0, M) * np.where(np.arange(M) % 2, 1, -1)])
    rel = np.array([1, 4, 99], dtype=np.int64)[np.arange(M) % 3]

    def paths(sd):
        cur, rows = None, [sd.copy()]
        for i in range(1, 13):
            cur = euler_step(sd, cur, rel, i, dt, v_core, src)
            rows.append(cur)
        return rows
    base = paths(seeds)
    F = TG.identity(M)
    for i in range(1, 13):
        start = np.where(rel == i, seeds, base[i - 1])
        F, _ = TG.step_F(F, start, rel, i, dt, v_core, src)
    ex, ez = np.array([[h], [0.0]]), np.array([[0.0], [h]])
    dX = (paths(seeds + ex)[12] - paths(seeds - ex)[12]) / (2 * h)
    dZ = (paths(seeds + ez)[12] - paths(seeds - ez)[12]) / (2 * h)
    fd = np.stack([dX[0], dZ[0], dX[1], dZ[1]])
    free = rel <= 12
    assert np.abs(F[:, free] - TG.identity(int(free.sum()))).max() > 1e-2
    assert np.abs(fd - F)[:, free].max() <= 1e-8 * np.abs(F).max(), np.abs(fd - F)[:, free].max()
    assert np.array_equal(F[:, ~free], TG.identity(int((~free).sum())))


def test_refusals_come_from_the_keywords_alone(monkeypatch):
    import ludvm_amd.ludvm as M

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before tracer_gradient was checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    import ludvm_amd.multi as multi
    monkeypatch.setattr(multi, "MultiDeviceLUDVM", NoEngine)
    ok = np.zeros([2, 3])
    with pytest.raises(ValueError, match="tracer_gradient needs `tracers`"):
        LUDVM(**CONFIG1, verbose=False, tracer_gradient=True)
    for bad in ("yes", 1, None, 1.0):
        with pytest.raises(ValueError, match="tracer_gradient must be True or False"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=bad)
    with pytest.raises(ValueError, match="tracer_gradient.*march=False"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, march=False)
    with pytest.raises(ValueError, match="tracer_gradient.*march=False"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, march=False, run=False)
    with pytest.raises(ValueError, match="tracer_gradient needs float64 tracers.*f32x2"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, tracer_precision="f32x2")
    for dist in ("rccl", True):
        with pytest.raises(ValueError, match="one GPU"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, distributed=dist)
    with pytest.raises(ValueError, match="tracer_gradient runs on one GPU.*devices"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_gradient=True, devices=[0, 1])
    with pytest.raises(ValueError, match="tracer_gradient needs `tracers`"):
        LUDVM(**CONFIG1, verbose=False, tracer_gradient=True, devices=2)


def test_a_sweep_refuses_the_keyword():
    member = dict(CONFIG1, tf=1.0)
    ok = np.zeros([2, 3])
    for value in (True, False):
        with pytest.raises(ValueError, match=r"sweep: tracer_gradient.*LUDVM\(\.\.\., tracers="):
            LUDVM.sweep([member, member], particles=ok, tracer_gradient=value)
        with pytest.raises(ValueError, match=r"sweep: member 1: tracer_gradient.*LUDVM\(\.\.\., tracers="):
            LUDVM.sweep([member, dict(member, tracer_gradient=value)], particles=ok)


class Marcher(FakeEngine):
    def march_run(self, *a, **k):
        raise AssertionError("the march was entered")

    def march_setup(self, *a, **k):
        raise AssertionError("the march was set up")

    def march_set_tracers(self, *a, **k):
        raise AssertionError("the tracers were set")


def test_a_run_that_cannot_take_the_march_raises():
    """tracer_gradient over an engine that does not march, over one that marches without the new entry, and in a run the march
    does not take: RuntimeError, no step run."""
    kw = dict(CONFIG1, tf=1.0)
    with pytest.raises(RuntimeError, match="tracer_gradient.*cannot take"):
        LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=[[1.0], [0.5]], tracer_gradient=True)
    with pytest.raises(RuntimeError, match="march_set_tracer_gradient"):
        LUDVM(**kw, verbose=False, engine=Marcher(), tracers=[[1.0], [0.5]], tracer_gradient=True)

    class Full(Marcher):
        def march_set_tracer_gradient(self, *a, **k):
            raise AssertionError("the gradient was set")
    with pytest.raises(RuntimeError, match="tracer_gradient.*cannot take"):
        LUDVM(**dict(kw, Ncoeffs=70), verbose=False, engine=Full(), tracers=[[1.0], [0.5]], tracer_gradient=True)


def test_the_class_sets_the_gradient_behind_the_tracers():
    seen = []

    class Stop(Exception):
        pass

    class Recorder(FakeEngine):
        def march_setup(self, *a, **k):
            seen.append("setup")

        def march_set_tracers(self, *a, **k):
            seen.append("tracers")

        def march_set_tracer_gradient(self, on, F=None):
            seen.append(("gradient", on, F))

        def march_anchor_steps(self, *a, **k):      # (the first thing a march call asks the engine)
            raise Stop

        def march_run(self, *a, **k):
            raise Stop
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Recorder(), history="sparse", tracers=[[1.0], [0.5]], tracer_gradient=True)
    assert seen == ["setup", "tracers", ("gradient", True, None)]
    del seen[:]
    with pytest.raises(Stop):
        LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=Recorder(), history="sparse", tracers=[[1.0], [0.5]])
    assert seen == ["setup", "tracers"]


def test_false_is_the_default_and_the_constructor_keywords_carry_only_true():
    kw = dict(CONFIG1, tf=1.0)
    seeds = [[1.0, 0.4], [0.5, 1.2]]
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_release=[1, 7])
    b = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_release=[1, 7], tracer_gradient=False)
    assert a.tracer_gradient is False and b.tracer_gradient is False
    assert a._ctor == b._ctor and "tracer_gradient" not in a._ctor
    assert not hasattr(a, "tracer_F_path") and not hasattr(a, "tracer_F_last")
    for s in a.tracer_path.steps():
        assert np.array_equal(a.tracer_path[s], b.tracer_path[s])
    with pytest.raises(ValueError, match="tracer_gradient=True"):
        a.tracer_ftle()
    plain = LUDVM(**kw, verbose=False, engine=FakeEngine())
    assert not any(k.startswith("tracer") for k in vars(plain)) and not any(k.startswith("tracer") for k in plain._ctor)
    c = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_gradient=True, run=False)
    assert c.tracer_gradient is True and c._ctor["tracer_gradient"] is True


class StateEngine(FakeEngine):
    """what `_write_checkpoint_file` asks of a marching engine"""

    def __init__(self, xz, F):
        super().__init__()
        self._xz, self._F = xz, F

    def march_tracer_state(self):
        return self._xz.copy()

    def march_tracer_gradient_state(self):
        return self._F.copy()


def test_the_checkpoint_carries_F_and_a_resume_restores_it(tmp_path):
    """The checkpoint dictionary of a gradient run: the current F, the F rows of the steps tracer_rows holds, the keyword among
    the constructor's; `_loop_restore` hands the current F to the loop and the rows to tracer_F_path.  The per-call record cap
    counts 48 bytes per tracer and row."""
    rng = np.random.default_rng(3)
    seeds = np.stack([np.linspace(0.0, 1.0, 5), np.full(5, 1.2)])
    cur, F_cur, F_3 = seeds + 0.1, rng.normal(1.0, 0.2, (4, 5)), rng.normal(1.0, 0.1, (4, 5))
    ck = str(tmp_path / "ck.npz")
    kw = dict(CONFIG1, tf=1.0)
    sim = LUDVM(**kw, verbose=False, engine=StateEngine(cur, F_cur), tracers=seeds, tracer_steps=[3, 8, 12], tracer_gradient=True,
                run=False, checkpoint_path=ck)
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
    import json
    assert json.loads(str(R["ctor"]))["tracer_gradient"] is True
    # ... and back: a second object built from the stored keywords, its loop restored from the file
    again = LUDVM(**json.loads(str(R["ctor"])), verbose=False, engine=StateEngine(cur, F_cur), run=False)
    assert again.tracer_gradient is True
    S2 = again._loop_begin()
    again._loop_restore(S2, R)
    assert np.array_equal(S2.tF, F_cur) and np.array_equal(S2.tcur, cur) and S2.first_step == 6
    assert again.tracer_F_path.steps() == [0, 3] and np.array_equal(again.tracer_F_path[3], F_3)
    # the cap on one call's recorded rows: 48 bytes per tracer and row with the gradient, 16 without
    for grad, row_bytes in ((True, 48), (False, 16)):
        class Capped(LUDVM):
            _tracer_call_bytes = 48 * 5 * 2
        c = Capped(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_steps=range(1, 21), tracer_gradient=grad, run=False)
        Sc = c._loop_begin()
        Sc.can_march, Sc.dense_march, Sc.march_chunk = True, False, 32768
        c.history, c.snapshot_steps = "sparse", set()
        j, _ = c._march_extent(Sc, 1)
        assert j - 1 == 48 * 5 * 2 // (row_bytes * 5), (grad, j)


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1)


def test_header_exports_and_binding_agree_on_the_new_entries():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # additions to ABI 7: detected by symbol
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        params = [p.strip() for p in _prototype(name).split(",")]
        assert len(params) == len(_ffi.SIGNATURES[name]) and params[0].startswith("ludvm_ctx*"), (name, params)
        assert name in _ffi.ADDED_IN_ABI_7 and hasattr(lib, name) and hasattr(_ffi.load(_ffi.EXP_LIB_PATH), name)
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M)
    assert lib.ludvm_march_set_tracer_gradient(None, 1, None) == _ffi.E_ARG
    assert lib.ludvm_march_read_tracer_gradient(None, None, 0, None, None) == _ffi.E_ARG
    assert lib.ludvm_march_tracer_gradient_state(None, None) == _ffi.E_ARG


def test_the_gradient_tracer_kernels_use_no_scratch_and_the_plain_ones_are_compiled_as_before():
    """march_grad_tracer_partial / march_grad_tracer_finish for gfx950 through tools/kernel_resources.py (no GPU needed): no
    scratch, no spills, the three float64 planes of one 256-source tile in LDS; march_tracer_partial / march_tracer_finish
    beside them keep the registers and LDS they had (52 VGPRs, 6144 bytes; 18 VGPRs, none)."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.resources(unit="march.hip")
    for kernel, lds in (("march_grad_tracer_partial", 3 * 256 * 8), ("march_grad_tracer_finish", 0)):
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) == lds, (name, r)
    for kernel, want in {"march_tracer_partial": (52, 6144, 0), "march_tracer_finish": (18, 0, 0)}.items():
        (name, r), = {k: v for k, v in report.items() if kernel in k}.items()
        assert (int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"])) == want, (name, r)
