"""CPU tier: passive tracers (LUDVM(..., tracers=...)) -- the definition against the reference's own zero-circulation free
vortices, the host logic of the drop-in class over the fake engine (per-step path: ludvm_amd/ludvm.py, `_roll_up`), passivity,
the refusals, checkpoint / resume, the C ABI of the three new entry points and the register budget of the two tracer kernels.
The marched path runs in tests/test_gpu_tracers.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from oracle import ludvm_oracle as O
from tracers_common import TracedOracle, euler_step, gust_cloud, path_error, releases_1_7_50, seeds37


def _quiet_rake():
    """37 seeds four chords above and below the line the foil travels along (it heaves within |z| <= 1 and goes from x = 0 to
    x = -5 in 100 steps), alternating.  The comparison below is between TWO oracle runs -- one with 37 more (zero-strength)
    entries in every pair sum -- whose NumPy sums group their terms differently: they are not the same run to the bit (Cl
    moves by 9e-11 by step 100 with G5's cloud, whose 61 vortices the foil runs into), and a particle that passes within a
    few core radii of the vortex sheet amplifies that difference of the runs, not of the definitions (seeds37(): 1.1e-10 of the
    largest displacement at step 100, 1.5e-14 at step 50).  Off the sheet the particles feel the whole field and not its fine
    structure."""
    return np.stack([np.linspace(-10.0, 6.0, 37), np.where(np.arange(37) % 2, 4.0, -4.0)])


def test_tracers_are_the_references_zero_circulation_free_vortices():
    """G5's gust cloud plus 37 appended zero-circulation free vortices, 100 steps of config 1 on the plain oracle: their
    path['FREE'] rows (convected by LUDVM.py:1120-1127) against TracedOracle with the same 37 seeds as tracers (release 1,
    lab frame) on the run WITHOUT them -- 1e-12 of the largest displacement over all 100 steps; and every TracedOracle row is,
    bit for bit, the Euler step recomputed from the sources it captured."""
    kw, gc, seeds = dict(CONFIG1, tf=5.0), gust_cloud(), _quiet_rake()
    nf = len(gc["circulation_freevort"])
    plain = O.OracleLUDVM(**kw, circulation_freevort=np.concatenate([gc["circulation_freevort"], np.zeros(37)]),
                          xy_freevort=np.concatenate([gc["xy_freevort"], seeds], axis=1))
    ref = TracedOracle(seeds, **kw, **gc)
    assert ref.nt == 101 and sorted(ref.rows) == list(range(1, 101))
    rows = ref.path_rows()
    free = plain.path["FREE"][:, :, nf:]
    disp = np.abs(free - seeds[None]).max()
    err = np.abs(free - rows).max() / disp
    print(f"tracers vs zero-circulation free vortices, steps 0-100: {err:.2e} of the largest displacement ({disp:.3f} chords)")
    assert np.array_equal(rows[0], seeds) and disp > 0.1
    assert err <= 1e-12, err
    cur = None
    rel = np.ones(37, dtype=np.int64)
    for i in range(1, 101):
        cur = euler_step(seeds, cur, rel, i, ref.dt, ref.v_core, ref.sources[i])
        assert np.array_equal(cur, ref.rows[i]), i


@pytest.mark.parametrize("method", ["Faure", "Ramesh"])
@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_class_on_the_per_step_path_matches_the_oracle(method, frame):
    """The class over the fake engine against TracedOracle: 37 seeds around the foil, released at steps 1, 7 and 50 in turn
    (the run has steps 1-49: the last third is never released), lab and tunnel frame, steps 1-49 at 1e-9 of the largest
    displacement; and with 50 steps, where the last third is released in the final one."""
    seeds = seeds37()
    rel = releases_1_7_50(37)
    shift = (lambda o: o.xpiv) if frame == "tunnel" else None
    for tf, last in ((2.45, 49), (2.5, 50)):
        kw = dict(CONFIG1, tf=tf, method=method)
        ref = TracedOracle(seeds, release=rel, shift=shift, **kw)
        assert ref.nt == last + 1
        sim = LUDVM(**kw, verbose=False, engine=FakeEngine(), tracers=seeds, tracer_release=rel, tracer_frame=frame)
        assert sim.tracer_path.steps() == list(range(last + 1))             # dense history: every step
        err = path_error(sim.tracer_path, ref, 1, last)
        print(f"{method} {frame} {last} steps: tracer paths vs oracle: {err:.2e} of the largest displacement")
        assert err <= 1e-9, err
        assert np.array_equal(sim.tracer_path[0], ref.seeds_at(0)) and np.array_equal(sim.tracer_last, sim.tracer_path[last])
        held = rel > last
        assert held.sum() == (12 if last == 49 else 0)
        for s in (1, 6, 7, last):
            assert np.array_equal(sim.tracer_released(s), rel <= s)
            still = rel > s                 # held: exactly the seed of that step
            assert np.array_equal(sim.tracer_path[s][:, still], ref.seeds_at(s)[:, still])
        assert np.array_equal(sim.tracer_xz, seeds) and np.array_equal(sim.tracer_release, rel) and sim.tracer_frame == frame
        moved = np.abs(sim.tracer_path[last] - ref.seeds_at(last))[:, rel <= last - 1]
        assert moved.max() > 0.05


def _result_arrays(sim):
    out = {k: getattr(sim, k) for k in ("Cl", "Cd", "Cm", "Fn", "Fs", "L", "D", "T", "M", "fourier", "LESP", "LESP_prev", "LEV_shed")}
    out.update({"circ_" + k: np.asarray(v) for k, v in sim.circulation.items()})
    for key in ("TEV", "LEV", "FREE"):
        P = sim.path[key]
        if isinstance(P, np.ndarray):
            out["path_" + key] = P
        else:
            for s in P.steps():
                out[f"path_{key}_{s}"] = P[s]
    return out


@pytest.mark.parametrize("history", ["full", "sparse"])
def test_tracers_are_passive_on_the_per_step_path(history):
    """Every other result array with and without tracers (and with probes set as well): bit-identical."""
    kw = dict(CONFIG1, tf=2.0, history=history, snapshot_steps=[5, 17])
    seeds, rel = seeds37(), releases_1_7_50(37)
    pts = np.array([[1.0, 2.0], [0.5, 1.0]])
    for extra in ({}, dict(probes=pts)):
        plain_eng, traced_eng = FakeEngine(), FakeEngine()
        plain = LUDVM(**kw, verbose=False, engine=plain_eng, **extra)
        traced = LUDVM(**kw, verbose=False, engine=traced_eng, tracers=seeds, tracer_release=rel, tracer_frame="tunnel", **extra)
        a, b = _result_arrays(plain), _result_arrays(traced)
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        for x, y in zip(plain_eng.wake_read(0, plain_eng.wake_size(), gamma=True), traced_eng.wake_read(0, traced_eng.wake_size(), gamma=True)):
            assert np.array_equal(x, y)
        if extra:
            assert np.array_equal(plain.probe_u, traced.probe_u) and np.array_equal(plain.probe_w, traced.probe_w)
        want = list(range(traced.nt)) if history == "full" else [0, 5, 17, traced.nt - 1]
        assert traced.tracer_path.steps() == want


def test_without_tracers_nothing_changes():
    eng = FakeEngine()
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng)
    for name in ("tracer_path", "tracer_xz", "tracer_release", "tracer_frame", "tracer_last"):
        assert not hasattr(sim, name), name
    assert not any(k.startswith("tracer") for k in sim._ctor)
    assert eng.calls["induce"] == 0 and eng.calls["points"] == 0
    traced = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=FakeEngine(), tracers=[[1.0], [0.5]], tracer_steps=[3, 20])
    assert traced._ctor["tracers"] == [[1.0], [0.5]] and traced._ctor["tracer_release"] == [1] and traced._ctor["tracer_frame"] == "lab"
    assert traced.tracer_path.steps() == [0, 3, 20]                 # (row 0 is always there)
    assert np.array_equal(traced.Cl, sim.Cl)
    # held tracers take part in no pair sum: none released, no engine call
    eng2 = FakeEngine()
    held = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng2, tracers=[[1.0], [0.5]], tracer_release=[21], tracer_frame="tunnel")
    assert eng2.calls["induce"] == 0 and eng2.calls["points"] == 0
    assert np.array_equal(held.tracer_last, [[1.0 + held.xpiv[20]], [0.5]])


@pytest.mark.parametrize("history,frame", [("full", "lab"), ("sparse", "tunnel")])
def test_checkpoint_between_two_releases_and_resume(tmp_path, history, frame):
    """Releases at steps 1, 7 and 50; checkpoint after step 23 and 46, resume from the last: the same tracer_path, bit for bit."""
    kw = dict(CONFIG1, tf=3.0)
    seeds, rel = seeds37(), releases_1_7_50(37)
    ck = str(tmp_path / "ck.npz")
    common = dict(verbose=False, history=history, snapshot_steps=[10, 40, 55], tracers=seeds, tracer_release=rel, tracer_frame=frame)
    a = LUDVM(**kw, engine=FakeEngine(), **common)
    LUDVM(**kw, engine=FakeEngine(), **common, checkpoint_every=23, checkpoint_path=ck)
    R = np.load(ck)
    assert int(R["next_step"]) == 47 and R["tracer_cur"].shape == (2, 37)
    assert list(R["tracer_rows_steps"]) == (list(range(47)) if history == "full" else [0, 10, 40])
    c = LUDVM.resume(ck, engine=FakeEngine(), verbose=False)
    assert c.tracer_frame == frame and np.array_equal(c.tracer_xz, seeds) and np.array_equal(c.tracer_release, rel)
    assert c.tracer_path.steps() == a.tracer_path.steps() == (list(range(61)) if history == "full" else [0, 10, 40, 55, 60])
    for s in a.tracer_path.steps():
        assert np.array_equal(c.tracer_path[s], a.tracer_path[s]), s
    assert np.array_equal(c.tracer_last, a.tracer_last) and np.array_equal(c.Cl, a.Cl)
    assert np.abs(a.tracer_path[60][:, rel == 50] - seeds[:, rel == 50]).min() > 0.0     # released after the checkpoint
    with pytest.raises(ValueError, match="one GPU"):
        LUDVM.resume(ck, devices=[0, 1], verbose=False)


def test_refusals_come_before_any_engine(monkeypatch):
    import ludvm_amd.ludvm as M
    import ludvm_amd.multi as MM

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the tracers were checked")

    def no_front(*a, **k):
        raise AssertionError("replica threads were created before the tracers were checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    monkeypatch.setattr(MM, "MultiDeviceLUDVM", no_front)
    ok = np.zeros([2, 3])
    bad = [np.zeros(3), np.zeros([3, 4]), np.zeros([2, 0]), np.zeros([2, 2, 2]), [[0.0, "a"], [1.0, 2.0]], [[0.0, np.nan], [1.0, 2.0]],
           [[0.0, np.inf], [1.0, 2.0]], np.zeros([2, 262145])]
    for t in bad:
        with pytest.raises(ValueError):
            LUDVM(**CONFIG1, verbose=False, tracers=t)
        with pytest.raises(ValueError):
            LUDVM(**CONFIG1, verbose=False, tracers=t, devices=[0, 1])
    for rel in ([1, 2], [1, 2, 0], [1, 2, -3], [1.0, 2.0, 3.0], [[1, 2, 3]], ["a", "b", "c"], 1):
        with pytest.raises(ValueError, match="tracer_release"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_release=rel)
    with pytest.raises(ValueError, match="tracer_frame"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_frame="body")
    with pytest.raises(ValueError, match="tracer_frame"):
        LUDVM(**CONFIG1, verbose=False, tracer_frame="body")
    for steps in ([-1], [401], [0, 5, 1000], [1.5], 3):               # config 1: nt = 401
        with pytest.raises(ValueError, match="tracer_steps"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, tracer_steps=steps)
    for dist in (True, "rccl", object()):
        with pytest.raises(ValueError, match="distributed"):
            LUDVM(**CONFIG1, verbose=False, tracers=ok, distributed=dist)
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, devices=[0, 1])
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, tracers=ok, devices=2)
    with pytest.raises(ValueError, match="tracers"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0), dict(CONFIG1, tf=1.0, tracers=ok)])
    with pytest.raises(ValueError, match="tracers"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0)], tracers=ok)
    # the limit itself, and the ends of the step range, are fine
    s = LUDVM(**CONFIG1, verbose=False, engine=FakeEngine(), tracers=np.zeros([2, 262144]), tracer_steps=[0, 400], run=False)
    assert s.tracer_xz.shape == (2, 262144) and s.tracer_release.dtype == np.int64 and (s.tracer_release == 1).all()


def test_header_exports_and_binding_agree_on_the_tracer_entry_points():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7         # an addition to ABI 7: detected by symbol
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ("ludvm_march_set_tracers", "ludvm_march_read_tracers", "ludvm_march_tracer_state"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M), name
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    assert re.search(r"#define\s+LUDVM_MARCH_MAX_TRACERS\s+262144", header) and _ffi.MARCH_MAX_TRACERS == 262144
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header)
    assert lib.ludvm_march_set_tracers(None, None, None, None, 0, None, 0, None, None, None, 0) == _ffi.E_ARG
    assert lib.ludvm_march_read_tracers(None, None, None, 0, None, None) == _ffi.E_ARG
    assert lib.ludvm_march_tracer_state(None, None, None) == _ffi.E_ARG


def test_tracer_kernels_use_no_scratch():
    """Register budget of the two tracer kernels as hipcc compiles them for gfx950 (no GPU needed): no scratch, no spills."""
    src = os.path.join(ROOT, "ludvm_amd", "csrc", "march.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull],
                         check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            kernels[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            kernels[cur][k.strip()] = v.strip()
    tracer = {k: v for k, v in kernels.items() if "march_tracer_" in k}
    assert len(tracer) == 2 and any("march_tracer_partial" in k for k in tracer) and any("march_tracer_finish" in k for k in tracer), sorted(kernels)
    for name, r in tracer.items():
        print(name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
