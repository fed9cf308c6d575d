"""CPU tier of passive tracers in a sweep (`sweep(cases, particles=..., particle_release=..., particle_frame=...,
particle_steps=...)`): the host side over a test-side engine that answers `ensemble_run_traced` with solo per-step runs in
the device layout (include/ludvm_hip.h, ludvm_ensemble_run_traced), every refusal, the C ABI of the new entry point and the
resources of the two instantiations of the traced kernel as hipcc compiles them for gfx950.  The kernel itself runs in
tests/test_gpu_ensemble_tracers.py."""
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
from tracers_common import seeds37

SNAPS = (1, 2, 10, 70)          # (70 lies beyond the last step of the shorter members)
RELEASE = np.array([1, 7, 50, 10 ** 6], dtype=np.int64)[np.arange(37) % 4]


class TracedEnsembleFake(EnsembleFake):
    """EnsembleFake whose solo runs carry the sweep's tracers (and probes, when given): `ensemble_run_traced` checks and
    answers the packed inputs as `ensemble_run` does and adds the solo runs' tracer rows as [members, ntrec + 1, 2, M] -- the
    recorded steps a member has, zeros for those it has not, its last step in the final record."""

    def __init__(self, cases, snapshot_steps, seeds, release, frame, probes=None, probe_frame="lab"):
        FakeEngine.__init__(self)
        from ludvm_amd import LUDVM
        self.snaps = sorted(int(s) for s in snapshot_steps if s >= 1)
        self.solos, self.setups = [], []
        self.ensemble_calls = self.plain_calls = self.probed_calls = self.traced_calls = 0
        self.handed = None
        extra = {} if probes is None else dict(probes=probes, probe_frame=probe_frame)
        for kw in cases:
            self.solos.append(LUDVM(**kw, verbose=False, engine=FakeEngine(), precision="f64", history="full", march=False,
                                    tracers=seeds, tracer_release=release, tracer_frame=frame, **extra))
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
        raise AssertionError("ensemble_run_probed reached")

    def ensemble_run_traced(self, *packed, seed_x, seed_z, release, shift_x=None, record_steps=(), probe_x=None, probe_z=None,
                            probe_shift_x=None):
        self.traced_calls += 1
        rows, wakes, wake_n = EnsembleFake.ensemble_run(self, *packed)
        opt = lambda a: None if a is None else np.array(a)
        self.handed = dict(seed_x=np.array(seed_x), seed_z=np.array(seed_z), release=np.array(release), shift_x=opt(shift_x),
                           record_steps=list(record_steps), probe_x=opt(probe_x), probe_z=opt(probe_z), probe_shift_x=opt(probe_shift_x))
        kin_rows = sum(s.nt for s in self.solos)
        assert np.asarray(packed[4]).shape[0] == kin_rows and (shift_x is None or len(shift_x) == kin_rows)
        rec = list(record_steps)
        assert all(a < b for a, b in zip(rec, rec[1:])) and (not rec or rec[0] >= 1)
        M = len(seed_x)
        trows = np.zeros([len(self.solos), len(rec) + 1, 2, M])
        for m, solo in enumerate(self.solos):
            for r, step in enumerate(rec):
                if step <= solo.nt - 1:
                    trows[m, r] = solo.tracer_path[step]
            trows[m, len(rec)] = solo.tracer_path[solo.nt - 1]
        if probe_x is None:
            return rows, wakes, wake_n, trows
        pu = np.concatenate([s.probe_u for s in self.solos])
        pw = np.concatenate([s.probe_w for s in self.solos])
        return rows, wakes, wake_n, trows, pu, pw


def _fake(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return TracedEnsembleFake(*a, **k)


@pytest.mark.parametrize("frame", ["lab", "tunnel"])
def test_sweep_hands_the_tracers_over_and_stores_every_members_paths(frame):
    from ludvm_amd import LUDVM, SparseHistory
    seeds = seeds37()
    fake = _fake(mixed_cases(), SNAPS, seeds, RELEASE, frame)
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS, particles=seeds, particle_release=RELEASE,
                       particle_frame=frame)
    assert (fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 0, 1)
    h = fake.handed
    assert np.array_equal(h["seed_x"], seeds[0]) and np.array_equal(h["seed_z"], seeds[1]) and np.array_equal(h["release"], RELEASE)
    assert h["record_steps"] == [1, 2, 10, 70] and h["probe_x"] is None and h["probe_z"] is None and h["probe_shift_x"] is None
    if frame == "lab":
        assert h["shift_x"] is None
    else:
        assert np.array_equal(h["shift_x"], np.concatenate([s.xpiv for s in fake.solos]))
        assert len({float(s.xpiv[-1]) for s in fake.solos}) >= 3          # (the members' pivots travel differently)
    assert {s.nt - 1 < 70 for s in fake.solos} == {True, False}          # (members shorter than a recorded step, and longer)
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        nt = solo.nt
        assert isinstance(sim.tracer_path, SparseHistory)
        assert sim.tracer_path.steps() == sorted({0, nt - 1} | {s for s in SNAPS if s <= nt - 1}), m
        for s in sim.tracer_path.steps():
            assert sim.tracer_path[s].shape == (2, 37) and sim.tracer_path[s].dtype == np.float64
            assert np.array_equal(sim.tracer_path[s], solo.tracer_path[s]), (m, s)
        assert np.array_equal(sim.tracer_last, solo.tracer_last) and np.array_equal(sim.tracer_last, sim.tracer_path[nt - 1]), m
        assert np.array_equal(sim.tracer_xz, seeds) and np.array_equal(sim.tracer_release, RELEASE) and sim.tracer_frame == frame
        assert sim.tracer_release.dtype == np.int64
        for step in (0, 6, 7, nt - 1):
            assert np.array_equal(sim.tracer_released(step), solo.tracer_released(step)), (m, step)
            assert np.array_equal(sim._tracer_seeds(step), solo._tracer_seeds(step)), (m, step)
        assert np.abs(sim.Cl - solo.Cl).max() <= 1e-13 and np.array_equal(sim.LEV_shed, solo.LEV_shed), m
        moved = np.abs(sim.tracer_last - sim._tracer_seeds(nt - 1))
        assert moved[:, RELEASE == 1].min(axis=0).max() > 0.0 and not moved[:, RELEASE > nt - 1].any(), m
    # without particles: the calls a sweep made before there were any, and no tracer attribute
    plain = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS)
    assert (fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 1, 2)
    for sim in plain:
        for name in ("tracer_path", "tracer_last", "tracer_xz", "tracer_release", "tracer_frame"):
            assert not hasattr(sim, name), name


def test_listed_steps_are_the_rows_and_the_default_release_is_step_1():
    """particle_steps given: exactly those rows (and row 0) for the members that have the step; a member's last step is
    `tracer_last` whether listed or not.  particle_release=None: every tracer free from step 1."""
    from ludvm_amd import LUDVM
    seeds = seeds37()[:, :5]
    fake = _fake(mixed_cases(), (), seeds, None, "tunnel")
    sims = LUDVM.sweep(mixed_cases(), engine=fake, particles=seeds, particle_frame="tunnel", particle_steps=[100, 3, 40, 3])
    assert fake.handed["record_steps"] == [3, 40, 100] and np.array_equal(fake.handed["release"], np.ones(5, dtype=np.int64))
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert sim.tracer_path.steps() == [0] + [s for s in (3, 40, 100) if s <= solo.nt - 1], m
        for s in sim.tracer_path.steps():
            assert np.array_equal(sim.tracer_path[s], solo.tracer_path[s]), (m, s)
        assert np.array_equal(sim.tracer_last, solo.tracer_last), m
    assert [s.nt - 1 for s in fake.solos] == [60, 40, 100, 100, 80]


def test_probes_and_particles_compose_in_one_call():
    from ludvm_amd import LUDVM
    seeds, pts = seeds37()[:, :9], probes32()[:, :8]
    rel = RELEASE[:9]
    fake = _fake(mixed_cases(), SNAPS, seeds, rel, "lab", probes=pts, probe_frame="tunnel")
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS, particles=seeds, particle_release=rel, probes=pts,
                       probe_frame="tunnel")
    assert (fake.traced_calls, fake.probed_calls, fake.plain_calls, fake.ensemble_calls) == (1, 0, 0, 1)
    h = fake.handed
    assert h["shift_x"] is None and np.array_equal(h["probe_shift_x"], np.concatenate([s.xpiv for s in fake.solos]))
    assert np.array_equal(h["probe_x"], pts[0]) and np.array_equal(h["probe_z"], pts[1])
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert np.array_equal(sim.probe_u, solo.probe_u) and np.array_equal(sim.probe_w, solo.probe_w), m
        assert sim.probe_frame == "tunnel" and sim.tracer_frame == "lab"
        for s in sim.tracer_path.steps():
            assert np.array_equal(sim.tracer_path[s], solo.tracer_path[s]), (m, s)


class CountingTraced(Counting):
    def __init__(self):
        super().__init__()
        self.ensemble_run_probed = lambda *a, **k: (_ for _ in ()).throw(AssertionError("ensemble_run_probed reached"))
        self.ensemble_run_traced = lambda *a, **k: (_ for _ in ()).throw(AssertionError("ensemble_run_traced reached"))


class CountingProbedOnly(Counting):
    def __init__(self):
        super().__init__()
        self.ensemble_run_probed = lambda *a, **k: (_ for _ in ()).throw(AssertionError("ensemble_run_probed reached"))


OK = np.zeros([2, 3])


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([dict(tf=1), dict(tf=1, particles=OK)], {}, CountingTraced, "`particles` belongs to the sweep"),
    ([dict(tf=1), dict(tf=1, particles=OK)], dict(particles=OK), CountingTraced, "member 1"),
    ([dict(tf=1, particle_release=[1, 1, 1])], dict(particles=OK), CountingTraced, "`particle_release` belongs to the sweep"),
    ([dict(tf=1, particle_frame="tunnel")], dict(particles=OK), CountingTraced, "`particle_frame` belongs to the sweep"),
    ([dict(tf=1, particle_steps=[1])], dict(particles=OK), CountingTraced, "`particle_steps` belongs to the sweep"),
    ([dict(tf=1), dict(tf=1, tracers=OK)], {}, CountingTraced, "tracers"),
    ([dict(tf=1), dict(tf=1, tracers=OK)], {}, CountingTraced, "particles="),
    ([dict(tf=1)], dict(tracers=OK), CountingTraced, "tracers"),
    ([dict(tf=1)], dict(particles=np.zeros([2, 4097])), CountingTraced, "at most 4096"),
    ([dict(tf=1)], dict(particles=[[0.0, np.nan], [1.0, 2.0]]), CountingTraced, "finite"),
    ([dict(tf=1)], dict(particles=[[0.0, np.inf], [1.0, 2.0]]), CountingTraced, "finite"),
    ([dict(tf=1)], dict(particles=np.zeros([3, 4])), CountingTraced, "particles"),
    ([dict(tf=1)], dict(particles=np.zeros([2, 0])), CountingTraced, "particles"),
    ([dict(tf=1)], dict(particles=OK, particle_release=[1, 2]), CountingTraced, "particle_release"),
    ([dict(tf=1)], dict(particles=OK, particle_release=[1, 2, 0]), CountingTraced, "particle_release"),
    ([dict(tf=1)], dict(particles=OK, particle_release=[1.0, 2.0, 3.0]), CountingTraced, "particle_release"),
    ([dict(tf=1)], dict(particle_release=[1, 2, 3]), CountingTraced, "need `particles`"),
    ([dict(tf=1)], dict(particle_steps=[1]), CountingTraced, "need `particles`"),
    ([dict(tf=1)], dict(particles=OK, particle_frame="body"), CountingTraced, "particle_frame"),
    ([dict(tf=1)], dict(particle_frame="body"), CountingTraced, "particle_frame"),
    ([dict(tf=1)], dict(particles=OK, particle_steps=[0]), CountingTraced, "particle_steps"),
    ([dict(tf=1, dt=5e-2), dict(tf=2, dt=5e-2)], dict(particles=OK, particle_steps=[41]), CountingTraced, "particle_steps"),   # (40 steps)
    ([dict(tf=1)], dict(particles=OK, particle_steps=[1.5]), CountingTraced, "particle_steps"),
    ([dict(tf=1)], dict(particles=OK, particle_steps=3), CountingTraced, "particle_steps"),
    ([dict(tf=1)], dict(particles=OK), CountingProbedOnly, "ensemble_run_traced"),
    # 40 members x (410 steps + the last) records x 4096 tracers x 16 bytes = 1.00 GiB and a little
    ([dict(tf=20.5, dt=5e-2)] * 40, dict(particles=np.zeros([2, 4096]), particle_steps=range(1, 411)), CountingTraced,
     "split the case list"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word) as e:
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []
    if word == "split the case list":
        assert str(40 * 411 * 16 * 4096) in str(e.value) and "1.00 GiB" in str(e.value)


def test_the_limits_themselves_are_fine():
    """4096 tracers, the ends of the step range, and a case list exactly at the byte cap (32 members x 512 records x 4096
    tracers x 16 bytes = 1 GiB) pass the checks: the engine is reached."""
    from ludvm_amd import ensemble, sweep

    class Reached(Exception):
        pass

    class Stop(FakeEngine):
        def ensemble_run(self, *a, **k):
            raise AssertionError("not called")

        def ensemble_run_traced(self, *a, seed_x, record_steps, **k):
            raise Reached(f"{np.asarray(a[4]).shape[0]} rows, {len(seed_x)} tracers, steps {list(record_steps)}")
    with pytest.raises(Reached, match=r"21 rows, 4096 tracers, steps \[1, 20\]"):
        sweep([dict(CONFIG1, tf=1)], engine=Stop(), particles=np.zeros([2, 4096]), particle_steps=[20, 1])
    merged = [dict(t0=0, tf=2047 / 64, dt=1 / 64)] * 32              # (dt = 1 / 64: exact, 2048 time levels)
    xz, rel, rec = ensemble._check_sweep_particles(np.zeros([2, 4096]), None, "lab", range(1, 512), (), merged)
    assert xz.shape == (2, 4096) and (rel == 1).all() and rec == list(range(1, 512))
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_particles(np.zeros([2, 4096]), None, "lab", range(1, 513), (), merged)
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_particles(np.zeros([2, 4096]), None, "lab", range(1, 512), (), merged + merged[:1])
    # the default records snapshot_steps (those a member can have) and the last step
    assert ensemble._check_sweep_particles(np.zeros([2, 4096]), None, "lab", None, range(0, 5000), merged[:8])[2] is None
    with pytest.raises(ValueError, match="split the case list"):
        ensemble._check_sweep_particles(np.zeros([2, 4096]), None, "lab", None, range(0, 5000), merged[:9])


def test_abi_7_declares_and_exports_the_traced_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert re.search(r"#define\s+LUDVM_ABI_VERSION\s+7\b", header) and re.search(r"#define\s+LUDVM_ENSEMBLE_DESC\s+6\b", header)
    limit = re.search(r"#define\s+LUDVM_ENSEMBLE_MAX_TRACERS\s+(\d+)", header)
    assert limit and int(limit.group(1)) == _ffi.ENSEMBLE_MAX_TRACERS == 4096 and _ffi.ENSEMBLE_TRACER_BYTES == 1 << 30
    name = "ludvm_ensemble_run_traced"
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert decl and name in _ffi.SIGNATURES and hasattr(lib, name) and name in _ffi.ADDED_IN_ABI_7
    # ludvm_ensemble_run_probed's arguments, then seed_x, seed_z, release, ntracer, tshift_x, tshift_rows, trec_steps, ntrec,
    # tracer_rows, tracer_doubles
    pll = _ffi.POINTER(_ffi.c_longlong)
    extra = [_ffi._pd, _ffi._pd, pll, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t, pll, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run_probed"] + extra
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    probed = re.search(r"\bint\s+ludvm_ensemble_run_probed\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert params[:-10] == [" ".join(p.split()) for p in probed.group(1).split(",")]
    assert params[-10:] == ["const double* seed_x", "const double* seed_z", "const long long* release", "size_t ntracer",
                            "const double* tshift_x", "size_t tshift_rows", "const long long* trec_steps", "size_t ntrec",
                            "double* tracer_rows", "size_t tracer_doubles"]
    assert len(params) == len(_ffi.SIGNATURES[name])
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    assert getattr(lib, name)(*([None] + [0 if t in (_ffi.c_int, _ffi.c_size_t) else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG


def test_both_instantiations_of_the_traced_kernel_fit():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_traced<false> and ensemble_traced<true> exist beside
    the two ensemble_march kernels; they use no scratch, spill no vector register, keep at least two waves per SIMD and no
    more static LDS than ensemble_march's 16272 bytes.  (SGPRs, VGPRs, scratch, occupancy, SGPR spill, VGPR spill, LDS) as
    DESIGN.md section 4.10 records them: <false> (106, 218, 0, 2, 133, 0, 16272), <true> (106, 218, 0, 2, 156, 0, 16272)."""
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
    traced = {k: v for k, v in kernels.items() if "ensemble_traced" in k}
    assert len(traced) == 2 and len([k for k in kernels if "ensemble_march" in k]) == 2, sorted(kernels)
    plain = [v for k, v in traced.items() if "ensemble_tracedILb0E" in k]
    probed = [v for k, v in traced.items() if "ensemble_tracedILb1E" in k]
    assert len(plain) == 1 and len(probed) == 1, sorted(traced)
    print("ensemble_traced<false>:", tup(plain[0]), " ensemble_traced<true>:", tup(probed[0]))
    for r in (plain[0], probed[0]):
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= 16272, r
