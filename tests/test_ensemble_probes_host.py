"""CPU tier of velocity probes in a sweep (`sweep(cases, probes=..., probe_frame=...)`): the host side over a test-side engine
that answers `ensemble_run_probed` with solo probed runs in the device layout (include/ludvm_hip.h,
ludvm_ensemble_run_probed), every refusal, the C ABI of the new entry point and the resources of the two instantiations of
the ensemble kernel as hipcc compiles them for gfx950.  The kernel itself runs in tests/test_gpu_ensemble_probes.py."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from probes_common import probes32
from test_ensemble_host import Counting, EnsembleFake, SetupRecorder, mixed_cases

SNAPS = (1, 2, 10)


class ProbedEnsembleFake(EnsembleFake):
    """EnsembleFake whose solo runs carry the sweep's probes: `ensemble_run_probed` checks and answers the packed inputs as
    `ensemble_run` does and adds the solo runs' probe rows as [kin_rows, P], a member's time level i at row kin_off + i."""

    def __init__(self, cases, snapshot_steps, probes, frame):
        FakeEngine.__init__(self)
        from ludvm_amd import LUDVM
        self.snaps = sorted(int(s) for s in snapshot_steps if s >= 1)
        self.solos, self.setups = [], []
        self.ensemble_calls = self.plain_calls = self.probed_calls = 0
        self.handed = None
        for kw in cases:
            self.solos.append(LUDVM(**kw, verbose=False, engine=FakeEngine(), precision="f64", history="full", march=False,
                                    probes=probes, probe_frame=frame))
            rec = SetupRecorder()
            obj = LUDVM(**kw, verbose=False, engine=rec, precision="f64", history="sparse", run=False)
            S = obj._loop_begin()
            obj._free_slot, S.fsl = None, slice(0, S.nf)
            obj._loop_prepare_engine(S)
            self.setups.append(rec.setup)

    def ensemble_run(self, *packed):
        self.plain_calls += 1
        return EnsembleFake.ensemble_run(self, *packed)

    def ensemble_run_probed(self, *packed, probe_x, probe_z, shift_x=None):
        self.probed_calls += 1
        rows, wakes, wake_n = EnsembleFake.ensemble_run(self, *packed)
        self.handed = (np.array(probe_x), np.array(probe_z), None if shift_x is None else np.array(shift_x))
        kin_rows = sum(s.nt for s in self.solos)
        assert np.asarray(packed[4]).shape[0] == kin_rows and (shift_x is None or len(shift_x) == kin_rows)
        pu = np.concatenate([s.probe_u for s in self.solos])
        pw = np.concatenate([s.probe_w for s in self.solos])
        assert pu.shape == (kin_rows, len(probe_x))
        return rows, wakes, wake_n, pu, pw


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_sweep_hands_the_probes_over_and_stores_every_members_series(frame):
    from ludvm_amd import LUDVM
    pts = probes32()[:, :8]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fake = ProbedEnsembleFake(mixed_cases(), SNAPS, pts, frame)
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS, probes=pts, probe_frame=frame)
    assert (fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 1)
    px, pz, shift = fake.handed
    assert np.array_equal(px, pts[0]) and np.array_equal(pz, pts[1])
    if frame == "lab":
        assert shift is None
    else:
        assert np.array_equal(shift, np.concatenate([s.xpiv for s in fake.solos]))
        assert len({float(s.xpiv[-1]) for s in fake.solos}) >= 3          # (the members' pivots travel differently)
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert sim.probe_u.shape == sim.probe_w.shape == (solo.nt, 8) and sim.probe_u.dtype == np.float64, m
        assert np.array_equal(sim.probe_u, solo.probe_u) and np.array_equal(sim.probe_w, solo.probe_w), m
        assert np.array_equal(sim.probe_xz, pts) and sim.probe_frame == frame
        for step in (0, 1, solo.nt - 1):
            assert np.array_equal(sim.probe_positions(step), solo.probe_positions(step)), (m, step)
        assert np.abs(sim.Cl - solo.Cl).max() <= 1e-13 and np.array_equal(sim.LEV_shed, solo.LEV_shed), m
    assert np.abs(sims[3].probe_u[0]).max() > 0.0            # (member 3 has the free-vortex cloud: row 0 is its field)
    # without probes: the calls a sweep made before there were any
    plain = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS)
    assert (fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 1, 2)
    for sim in plain:
        for name in ("probe_u", "probe_w", "probe_xz", "probe_frame"):
            assert not hasattr(sim, name), name


class CountingProbed(Counting):
    def __init__(self):
        super().__init__()
        self.ensemble_run_probed = lambda *a, **k: (_ for _ in ()).throw(AssertionError("ensemble_run_probed reached"))


OK = np.zeros([2, 3])


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([dict(tf=1), dict(tf=1, probes=OK)], {}, CountingProbed, "`probes` belongs to the sweep"),
    ([dict(tf=1), dict(tf=1, probes=OK)], dict(probes=OK), CountingProbed, "member 1"),
    ([dict(tf=1, probe_frame="tunnel")], dict(probes=OK), CountingProbed, "`probe_frame` belongs to the sweep"),
    ([dict(tf=1)], dict(probes=np.zeros([2, 1025])), CountingProbed, "at most 1024"),
    ([dict(tf=1)], dict(probes=[[0.0, np.nan], [1.0, 2.0]]), CountingProbed, "finite"),
    ([dict(tf=1)], dict(probes=[[0.0, np.inf], [1.0, 2.0]]), CountingProbed, "finite"),
    ([dict(tf=1)], dict(probes=np.zeros([3, 4])), CountingProbed, "probes"),
    ([dict(tf=1)], dict(probes=OK, probe_frame="body"), CountingProbed, "probe_frame"),
    ([dict(tf=1)], dict(probe_frame="body"), CountingProbed, "probe_frame"),
    ([dict(tf=1)], dict(probes=OK), Counting, "ensemble_run_probed"),
    # 40 members of 1985 time levels (dt = 1 / 64: exact) x 1024 probes: 2 x 8 x 79400 x 1024 bytes = 1.21 GiB
    ([dict(tf=31, dt=2.0 ** -6)] * 40, dict(probes=np.zeros([2, 1024])), CountingProbed, "split the case list"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word) as e:
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []
    if word == "split the case list":
        assert str(2 * 8 * 79400 * 1024) in str(e.value) and "1.21 GiB" in str(e.value)


def test_the_limits_themselves_are_fine():
    """1024 probes, and a case list exactly at the byte cap (32 members x 2048 time levels x 1024 probes x 16 bytes = 1 GiB), pass
    the checks: the engine is reached."""
    from ludvm_amd import sweep

    class Reached(Exception):
        pass

    class Stop(FakeEngine):
        def ensemble_run(self, *a, **k):
            raise AssertionError("not called")

        def ensemble_run_probed(self, *a, probe_x, probe_z, shift_x=None):
            raise Reached(f"{np.asarray(a[4]).shape[0]} rows, {len(probe_x)} probes")
    with pytest.raises(Reached, match="21 rows, 1024 probes"):
        sweep([dict(CONFIG1, tf=1)], engine=Stop(), probes=np.zeros([2, 1024]))
    from ludvm_amd import ensemble
    merged = [dict(t0=0, tf=2047 / 64, dt=1 / 64)] * 32              # (dt = 1 / 64: exact, 2048 time levels)
    assert ensemble._check_sweep_probes(np.zeros([2, 1024]), "lab", merged).shape == (2, 1024)
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_probes(np.zeros([2, 1024]), "lab", merged + [dict(t0=0, tf=1 / 64, dt=1 / 64)])


def test_abi_7_declares_and_exports_the_probed_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header) and re.search(r"#define\s+LUDVM_ENSEMBLE_DESC\s+6\b", header)
    limit = re.search(r"#define\s+LUDVM_ENSEMBLE_MAX_PROBES\s+(\d+)", header)
    assert limit and int(limit.group(1)) == _ffi.ENSEMBLE_MAX_PROBES == 1024 and 4 * _ffi.ENSEMBLE_MAX_PROBES == _ffi.MARCH_MAX_PROBES
    assert _ffi.ENSEMBLE_PROBE_BYTES == 1 << 30
    name = "ludvm_ensemble_run_probed"
    assert re.search(r"\bint\s+" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert name in _ffi.SIGNATURES and hasattr(lib, name)
    # ludvm_ensemble_run's arguments, then probe_x, probe_z, nprobe, shift_x, shift_rows, probe_u, probe_w
    extra = [_ffi._pd, _ffi._pd, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t, _ffi._pd, _ffi._pd]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run"] + extra
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    assert getattr(lib, name)(*([None] + [0 if t in (_ffi.c_int, _ffi.c_size_t) else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG


def test_both_instantiations_of_the_ensemble_kernel_fit_and_the_unprobed_one_is_as_before():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_march<false> and ensemble_march<true> exist; <false>
    reports the (SGPRs, VGPRs, scratch, occupancy, SGPR spill, VGPR spill, LDS) of the ensemble_march of the commit before the
    probes, read there with this very command; both use no scratch, spill no vector register, keep at least two waves per
    SIMD and the static LDS of before; the kernels of the solo march report what tests/test_ensemble_host.py lists."""
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

    def tup(r):
        return tuple(int(r[k]) for k in ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
                                         "VGPRs Spill", "LDS Size [bytes/block]"))
    ens = {k: v for k, v in kernels.items() if "ensemble_march" in k}
    assert len(ens) == 2, sorted(kernels)
    plain = [v for k, v in ens.items() if "ensemble_marchILb0E" in k]
    probed = [v for k, v in ens.items() if "ensemble_marchILb1E" in k]
    assert len(plain) == 1 and len(probed) == 1, sorted(ens)
    print("ensemble_march<false>:", tup(plain[0]), " ensemble_march<true>:", tup(probed[0]))
    before = (106, 219, 0, 2, 92, 0, 16272)          # ensemble_march of the parent commit
    assert tup(plain[0]) == before, tup(plain[0])
    for r in (plain[0], probed[0]):
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) == before[6], r
    march = {"march_begin": (28, 20, 0, 8, 0, 0, 32), "march_chord_finish": (19, 20, 0, 8, 0, 0, 0),
             "march_solve": (94, 150, 0, 3, 0, 0, 3328), "march_finish_sym": (102, 57, 0, 7, 0, 0, 3088)}
    for short, want in march.items():
        hits = [v for k, v in kernels.items() if re.search(r"\d" + short + "E", k)]
        assert len(hits) == 1 and tup(hits[0]) == want, (short, hits)
