"""CPU tier: velocity probes (LUDVM(..., probes=...)) -- the host logic of the drop-in class over the fake engine (per-step
path: ludvm_amd/ludvm.py, `_roll_up`), the refusals, checkpoint / resume, the C ABI of the two new entry points and the
register budget of the two probe kernels.  The marched path runs in tests/test_gpu_probes.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CONFIG1, ROOT, load_golden
from fake_engine import FakeEngine
from ludvm_amd import _ffi
from ludvm_amd.ludvm import LUDVM
from probes_common import G3_STEPS, ProbedOracle, g3_errors, g3_probe_cases, g3_probe_points, probes32, series_error

# Step 100 against G3, measured with this file's own run (class on the fake engine, per-step path): 9.1e-11 of max|u|.  The
# wake is no longer bit-identical to the reference's there (the class solves with matrix products, the reference with loops:
# a rounding difference that grows about 10x per 12 steps); the bound is 10x the measured maximum and
# may never exceed 1e-7 of max|u|, the project's bound on loads over the first 200 steps.
STEP100_MEASURED = 9.1e-11
STEP100_BOUND = 10 * STEP100_MEASURED
assert STEP100_BOUND <= 1e-7


def test_probes_reproduce_the_references_own_rollup_fields():
    """tests/golden/g3_boundary_trace.npz holds the reference's roll-up calls of config 1 at steps 1-5 and 100: the targets
    of calls 3+4, 5+6, 7+8 are the TEV / LEV / FREE slices and u_wake + u_foil the field there -- 3, 4, 5, 6, 7 and 156
    points.  Config 1 with those 181 points as lab-frame probes: row s at step s's points equals the reference's numbers to
    1e-12 of max|u| at steps 1-5 (the float64 per-call tier; the wake is bit-identical there) and to STEP100_BOUND at step
    100 (measured 9.1e-11; bound 9.1e-10)."""
    cases = g3_probe_cases()
    pts, where = g3_probe_points(cases)
    assert pts.shape == (2, 181)
    sim = LUDVM(**CONFIG1, verbose=False, engine=FakeEngine(), probes=pts)
    assert sim.probe_u.shape == sim.probe_w.shape == (sim.nt, 181) and sim.probe_u.dtype == np.float64
    assert np.array_equal(sim.probe_xz, pts) and np.array_equal(sim.probe_positions(100), pts)
    err = g3_errors(sim, cases, where)
    print("G3 probe errors / max|u|:", {s: f"{e:.2e}" for s, e in err.items()})
    for s in G3_STEPS[:-1]:
        assert err[s] <= 1e-12, (s, err[s])
    assert err[100] <= STEP100_BOUND, err[100]


def _free_cloud():
    g = load_golden("g5_freevort.npz")
    return dict(circulation_freevort=g["gamma_freevort"], xy_freevort=g["xy_freevort"])


@pytest.mark.parametrize("case", ["config1", "ramesh", "freevort"])
def test_probe_series_matches_the_oracle_over_a_run(case):
    """The oracle's series at 32 points (near wake, far field, ahead of the foil), built from the sources of its own roll-up
    calls, against the class on the fake engine over steps 1-50: 1e-9 of max|u|; row 0 is the free-vortex field."""
    kw = dict(CONFIG1, tf=2.5)
    if case == "ramesh":
        kw["method"] = "Ramesh"
    if case == "freevort":
        kw.update(_free_cloud())
    pts = probes32()
    ref = ProbedOracle(pts, **kw)
    ou, ow = ref.series()
    assert sorted(ref.rows) == list(range(1, ref.nt)) and ref.nt == 51
    sim = LUDVM(**kw, verbose=False, engine=FakeEngine(), probes=pts)
    err = series_error(sim, ou, ow, 1, 50)
    print(f"{case}: probe series vs oracle, steps 1-50: {err:.2e} of max|u|")
    assert err <= 1e-9, err
    assert np.array_equal(sim.probe_u[0], ou[0]) and np.array_equal(sim.probe_w[0], ow[0])
    if case == "freevort":
        assert np.abs(ou[0]).max() > 0.0
    else:
        assert not ou[0].any() and not ow[0].any()       # (the default free vortex has zero strength)
    # passive: the run itself is the run without probes
    plain = LUDVM(**kw, verbose=False, engine=FakeEngine())
    assert np.array_equal(plain.Cl, sim.Cl) and np.array_equal(plain.path["TEV"][-1], sim.path["TEV"][-1])


def test_tunnel_frame_translates_with_the_pivot():
    """'tunnel': the lab position at step i is (x + xpiv[i], z).  Step by step, the series equals the row i of a lab-frame run
    whose probes sit at x + xpiv[i]."""
    kw = dict(CONFIG1, tf=0.4)
    pts = np.array([[0.5, 1.5, 3.0, -1.0], [1.0, 1.2, 0.5, 1.1]])
    tun = LUDVM(**kw, verbose=False, engine=FakeEngine(), probes=pts, probe_frame="tunnel")
    assert tun.nt == 9 and np.array_equal(tun.probe_xz, pts)
    for i in range(tun.nt):
        lab_pts = np.stack([pts[0] + tun.xpiv[i], pts[1]])
        assert np.array_equal(tun.probe_positions(i), lab_pts)
        lab = LUDVM(**kw, verbose=False, engine=FakeEngine(), probes=lab_pts)
        assert np.array_equal(lab.probe_positions(i), lab_pts)
        assert np.array_equal(lab.probe_u[i], tun.probe_u[i]) and np.array_equal(lab.probe_w[i], tun.probe_w[i]), i
    assert np.abs(tun.probe_w[1:]).min() > 0.0


def test_refusals_come_before_any_engine(monkeypatch):
    import ludvm_amd.ludvm as M
    import ludvm_amd.multi as MM

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the probes were checked")

    def no_front(*a, **k):
        raise AssertionError("replica threads were created before the probes were checked")
    monkeypatch.setattr(M, "Engine", NoEngine)
    monkeypatch.setattr(MM, "MultiDeviceLUDVM", no_front)
    ok = np.zeros([2, 3])
    bad = [np.zeros(3), np.zeros([3, 4]), np.zeros([2, 0]), np.zeros([2, 2, 2]), [[0.0, "a"], [1.0, 2.0]], [[0.0, np.nan], [1.0, 2.0]],
           [[0.0, np.inf], [1.0, 2.0]], np.zeros([2, 4097])]
    for p in bad:
        with pytest.raises(ValueError):
            LUDVM(**CONFIG1, verbose=False, probes=p)
        with pytest.raises(ValueError):
            LUDVM(**CONFIG1, verbose=False, probes=p, devices=[0, 1])
    with pytest.raises(ValueError, match="probe_frame"):
        LUDVM(**CONFIG1, verbose=False, probes=ok, probe_frame="body")
    with pytest.raises(ValueError, match="probe_frame"):
        LUDVM(**CONFIG1, verbose=False, probe_frame="body")
    for dist in (True, "rccl", object()):
        with pytest.raises(ValueError, match="distributed"):
            LUDVM(**CONFIG1, verbose=False, probes=ok, distributed=dist)
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, probes=ok, devices=[0, 1])
    with pytest.raises(ValueError, match="devices"):
        LUDVM(**CONFIG1, verbose=False, probes=ok, devices=2)
    with pytest.raises(ValueError, match="probes"):
        LUDVM.sweep([dict(CONFIG1, tf=1.0), dict(CONFIG1, tf=1.0, probes=ok)])
    # the limit itself is fine
    s = LUDVM(**CONFIG1, verbose=False, engine=FakeEngine(), probes=np.zeros([2, 4096]), run=False)
    assert s.probe_xz.shape == (2, 4096)


def test_without_probes_nothing_changes():
    eng = FakeEngine()
    sim = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=eng)
    for name in ("probe_u", "probe_w", "probe_xz", "probe_frame"):
        assert not hasattr(sim, name), name
    assert "probes" not in sim._ctor and "probe_frame" not in sim._ctor
    assert eng.calls["induce"] == 0 and eng.calls["points"] == 0        # (the per-step path's chord sums are 'chord' calls)
    probed = LUDVM(**dict(CONFIG1, tf=1.0), verbose=False, engine=FakeEngine(), probes=np.array([[1.0], [0.5]]))
    assert probed._ctor["probes"] == [[1.0], [0.5]] and probed._ctor["probe_frame"] == "lab"
    assert np.array_equal(probed.Cl, sim.Cl)


@pytest.mark.parametrize("history,frame", [("full", "lab"), ("sparse", "tunnel")])
def test_checkpoint_resume_continues_the_series(tmp_path, history, frame):
    kw = dict(CONFIG1, tf=3.0)
    pts = probes32()[:, :8]
    ck = str(tmp_path / "ck.npz")
    a = LUDVM(**kw, verbose=False, engine=FakeEngine(), history=history, probes=pts, probe_frame=frame)
    LUDVM(**kw, verbose=False, engine=FakeEngine(), history=history, probes=pts, probe_frame=frame, checkpoint_every=23,
          checkpoint_path=ck)
    R = np.load(ck)
    assert int(R["next_step"]) == 47 and R["probe_u"].shape == (47, 8)
    c = LUDVM.resume(ck, engine=FakeEngine(), verbose=False)
    assert c.probe_frame == frame and np.array_equal(c.probe_xz, pts)
    assert np.array_equal(c.probe_u, a.probe_u) and np.array_equal(c.probe_w, a.probe_w)
    assert np.array_equal(c.Cl, a.Cl)
    assert np.abs(a.probe_u[47:]).min() > 0.0
    with pytest.raises(ValueError, match="one GPU"):
        LUDVM.resume(ck, devices=[0, 1], verbose=False)


def test_abi_7_declares_and_exports_the_probe_entry_points():
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    for name in ("ludvm_march_set_probes", "ludvm_march_read_probes"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert re.search(r"#define\s+LUDVM_MARCH_MAX_PROBES\s+4096", header) and _ffi.MARCH_MAX_PROBES == 4096
    assert lib.ludvm_march_set_probes(None, None, None, 0, None, 0) == _ffi.E_ARG
    assert lib.ludvm_march_read_probes(None, None, None, 0) == _ffi.E_ARG


def test_probe_kernels_use_no_scratch():
    """Register budget of the two probe kernels as hipcc compiles them for gfx950 (no GPU needed): no scratch, no spills."""
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
    probe = {k: v for k, v in kernels.items() if "march_probe_" in k}
    assert len(probe) == 2 and any("march_probe_partial" in k for k in probe) and any("march_probe_finish" in k for k in probe), sorted(kernels)
    for name, r in probe.items():
        print(name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
