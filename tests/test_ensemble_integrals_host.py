"""CPU tier of the wake integrals in a sweep (`sweep(cases, integrals=True, energy_steps=...)`): the host
side over a test-side engine that answers `ensemble_run_integrals` with the long-double sums over the sources of solo per-step
runs (tests/wake_integrals_common.py's reference) in the device layout (include/ludvm_hip.h, ludvm_ensemble_run_integrals),
every refusal, the C ABI of the new entry point and the resources of the sixteen instantiations of the new kernel family as
hipcc compiles them for gfx950.  The kernels themselves run in tests/test_gpu_ensemble_integrals.py."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import ensemble_integrals_common as EI
import wake_integrals_common as WI
from conftest import CONFIG1, ROOT
from fake_engine import FakeEngine
from probes_common import probes32
from test_ensemble_host import Counting, EnsembleFake
from tracers_common import seeds37

WINDOW = (1, 380, 19)           # (380 lies beyond the last step of the shorter members: clipped for them)


def three_cases():
    return [dict(CONFIG1), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=1.5, **WI.mixed_cloud(60))]


class IntegralsEnsembleFake(EnsembleFake):
    """EnsembleFake with `ensemble_run_integrals`: checks and answers the packed inputs as `ensemble_run` does and adds the
    reference's rows over the sources of its solo runs (dense history), [rows of kin, 4, 2, 6] with row 0 of a member left 0, and
    the reference's W at the sampled steps, NaN elsewhere."""

    def __init__(self, cases, snapshot_steps):
        super().__init__(cases, snapshot_steps)
        self.plain_calls = self.integral_calls = 0
        self.handed = None

    def ensemble_run(self, *packed):
        self.plain_calls += 1
        return EnsembleFake.ensemble_run(self, *packed)

    def ensemble_run_integrals(self, *packed, energy_steps=None, **others):
        self.integral_calls += 1
        self.handed = dict(others, energy_steps=energy_steps)
        assert not others, sorted(others)               # (this fake carries no other observer)
        rows, wakes, wake_n = EnsembleFake.ensemble_run(self, *packed)
        kin_rows = sum(s.nt for s in self.solos)
        assert np.asarray(packed[4]).shape[0] == kin_rows
        isums = np.zeros([kin_rows, 4, 2, 6])
        energy = None if energy_steps is None else np.full(kin_rows, np.nan)
        off = 0
        for solo in self.solos:
            sampled = set() if energy_steps is None else set(WI.window_steps(energy_steps, solo.nt))
            for i in range(1, solo.nt):
                ref = WI.reference(solo, i, energy=i in sampled)
                isums[off + i] = ref["sums"]
                if i in sampled:
                    energy[off + i] = ref["W"]
            off += solo.nt
        self.isums, self.energy = isums, energy
        return rows, wakes, wake_n, np.zeros([len(self.solos), 1, 2, 0]), None, None, None, None, isums, energy


@pytest.fixture(scope="module")
def fake():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return IntegralsEnsembleFake(three_cases(), (2, 50))


def carrying(sim, kw):
    """the solo class's host formulas over the member's rows: a LUDVM that never runs, carrying them"""
    from ludvm_amd import LUDVM
    s = LUDVM(**kw, verbose=False, engine=FakeEngine(), wake_integrals=True, run=False)
    s.integral_sums, s.wake_energy = sim.integral_sums.copy(), sim.wake_energy.copy()
    return s


def test_every_member_gets_the_solo_attributes_from_the_integrals_call(fake):
    from ludvm_amd import LUDVM
    before = (fake.integral_calls, fake.plain_calls)
    sims = LUDVM.sweep(three_cases(), engine=fake, snapshot_steps=(2, 50), integrals=True, energy_steps=WINDOW)
    assert (fake.integral_calls, fake.plain_calls) == (before[0] + 1, before[1]) and fake.handed == dict(energy_steps=WINDOW)
    off = 0
    for m, (sim, solo, kw) in enumerate(zip(sims, fake.solos, three_cases())):
        nt = sim.nt
        assert sim.wake_integrals is True and sim.wake_energy_steps == (1, min(380, nt), 19)
        assert sim.integral_sums.shape == (nt, 4, 2, 6) and sim.integral_sums.dtype == np.float64 and sim.wake_energy.shape == (nt,)
        assert np.array_equal(sim.integral_sums[1:], fake.isums[off + 1:off + nt])
        # row 0: the member's free vortices, as a solo run sets it
        nf = sim.n_freevort
        xy = np.array(sim.xy_freevort, dtype=float).reshape(2, nf)
        row0 = LUDVM._integral_row(np.zeros(nf, dtype=np.int64), np.asarray(sim.circulation_freevort, float).reshape(-1), xy[0], xy[1])
        assert np.array_equal(sim.integral_sums[0], row0) and sim.integral_sums[0, WI.FREE, :, 0].sum() == nf
        assert not sim.integral_sums[0, 1:].any()
        # the NaN pattern: row 0 and every step off the window
        sampled = WI.window_steps(WINDOW, nt)
        on = np.zeros(nt, bool)
        on[sampled] = True
        assert len(sampled) >= 2 and np.isnan(sim.wake_energy[~on]).all() and np.isfinite(sim.wake_energy[on]).all()
        assert np.array_equal(sim.wake_energy[on], fake.energy[off:off + nt][on])
        # the host properties are the solo class's over the same rows
        solo_like = carrying(sim, kw)
        for name in EI.PROPERTIES:
            assert np.array_equal(getattr(sim, name), getattr(solo_like, name), equal_nan=True), (m, name)
        for cls in WI.CLASSES:
            for sign in ("+", "-", None):
                assert np.array_equal(sim.wake_circulation(cls, sign), solo_like.wake_circulation(cls, sign)), (m, cls, sign)
        assert np.array_equal(sim.wake_centroid("TEV", "+"), solo_like.wake_centroid("TEV", "+"), equal_nan=True)
        i = nt - 1
        tot = fake.isums[off + i].sum(axis=(0, 1))
        assert np.allclose(sim.wake_impulse[i], sim.rho * np.array([-tot[3], tot[2]]), rtol=1e-12)
        assert np.allclose(sim.wake_circulation("LEV")[i], fake.isums[off + i, WI.LEV, :, 1].sum(), rtol=0, atol=1e-13)
        assert np.isnan(sim.impulse_force[:2]).all() and np.isfinite(sim.impulse_force[2:]).all()
        # everything else is the sweep's without integrals
        assert np.abs(sim.Cl - solo.Cl).max() <= 1e-13 and sim.path["TEV"].steps() == sorted({0, 2, nt - 1} | ({50} if nt > 50 else set()))
        off += nt
    # config 1: the impulse's lift follows the loads'
    corr = np.corrcoef(sims[0].impulse_Cl[2:], sims[0].Cl[2:])[0, 1]
    print(f"member 0 (config 1): corr(impulse_Cl, Cl) = {corr:.4f}")
    assert sims[0].nt == 401 and corr > 0.9
    assert (WI.class_census(fake.solos[2], range(1, 20))[WI.FREE] > 10).all()


def test_without_energy_steps_there_is_no_sample_and_without_integrals_the_calls_are_the_ones_made_before(fake):
    from ludvm_amd import LUDVM
    cases = three_cases()
    n_i, n_p = fake.integral_calls, fake.plain_calls
    sims = LUDVM.sweep(cases, engine=fake, snapshot_steps=(2, 50), integrals=True)
    assert (fake.integral_calls, fake.plain_calls) == (n_i + 1, n_p) and fake.handed == dict(energy_steps=None)
    for sim in sims:
        assert sim.wake_integrals is True and sim.wake_energy_steps is None and np.isnan(sim.wake_energy).all()
        assert sim.integral_sums[1:, WI.BOUND, :, 0].sum(axis=1).min() == sim.Npoints - 1
        assert np.isnan(sim.wake_energy_interaction).all()
    for kw in (dict(), dict(integrals=False), dict(integrals=False, energy_steps=None)):
        n_p = fake.plain_calls
        sims = LUDVM.sweep(cases, engine=fake, snapshot_steps=(2, 50), **kw)
        assert (fake.integral_calls, fake.plain_calls) == (n_i + 1, n_p + 1), kw
        for sim in sims:
            assert sim.wake_integrals is False and not hasattr(sim, "integral_sums") and not hasattr(sim, "wake_energy")
            with pytest.raises(ValueError, match="wake_integrals=True"):
                sim.wake_impulse
    # an engine from before the entry point serves every sweep it served, and refuses this one before any call
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        old = EnsembleFake(cases[1:2], ())
    assert not hasattr(old, "ensemble_run_integrals")
    LUDVM.sweep(cases[1:2], engine=old)
    assert old.ensemble_calls == 1
    with pytest.raises(ValueError, match="sweep: integrals: this engine has no ensemble_run_integrals"):
        LUDVM.sweep(cases[1:2], engine=old, integrals=True)
    assert old.ensemble_calls == 1


def test_a_member_with_every_step_recorded_serves_the_reference_as_a_dense_run_does():
    """The construction the GPU tier relies on: under snapshot_steps=range(1, nt) a member's own `path` gives the sources of every
    step (SparseHistory takes the dense arrays' indexing), so the reference over the MEMBER reproduces the rows the fake formed
    from its solo runs -- the fake hands the solo wakes over bit for bit."""
    from ludvm_amd import LUDVM
    cases = [dict(CONFIG1, tf=2, method="Ramesh", LESPcrit=0.05), dict(CONFIG1, tf=1.5, **WI.mixed_cloud(60))]
    snaps = EI.dense_snapshots(41)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = IntegralsEnsembleFake(cases, snaps)
    win = (2, 40, 7)
    sims = LUDVM.sweep(cases, engine=eng, snapshot_steps=snaps, integrals=True, energy_steps=win)
    assert [s.nt for s in sims] == [41, 31]
    for m, sim in enumerate(sims):
        assert sim.path["TEV"].steps() == list(range(sim.nt))
        worst = EI.check_member(sim, WI.window_steps(win, sim.nt), f"fake sweep, member {m}, its own sources")
        assert max(worst) <= 1e-3
        lag_m, lag_w = EI.lagged_misses(sim, range(2, sim.nt), WI.window_steps(win, sim.nt))
        assert lag_m > 10 and lag_w > 10, (lag_m, lag_w)
    assert EI.class_census(sims[0], range(1, 41))[WI.LEV].sum() > 0


class Handed(Exception):
    pass


class Recording(FakeEngine):
    """every ensemble entry; the new one keeps its keywords and ends the sweep"""

    def __init__(self):
        super().__init__()
        for name in ("ensemble_run", "ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
                     "ensemble_run_surveyed_graded"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))

    def ensemble_run_integrals(self, *packed, **kw):
        self.kw = kw
        raise Handed()


def test_every_other_observer_goes_through_the_one_call():
    from ludvm_amd import sweep
    pts, rake, seeds = probes32()[:, 8:13], probes32()[:, :4], seeds37()[:, :6]
    cases = [dict(CONFIG1, tf=2), dict(CONFIG1, tf=1.5)]
    eng = Recording()
    with pytest.raises(Handed):
        sweep(cases, engine=eng, integrals=True, energy_steps=(2, 30, 3), probes=rake, probe_frame="tunnel", particles=seeds,
              survey=pts, survey_frame="tunnel", survey_steps=(2, 35, 1), survey_phases=5, survey_grad=True)
    kw = eng.kw
    assert kw["energy_steps"] == (2, 30, 3) and kw["grad"] is True and kw["nbins"] == 5 and len(kw["bin_of_step"]) == 41 + 31
    assert np.array_equal(kw["survey_x"], pts[0]) and kw["survey_steps"] == (2, 35, 1) and len(kw["survey_shift_x"]) == 72
    assert np.array_equal(kw["probe_x"], rake[0]) and len(kw["probe_shift_x"]) == 72 and np.array_equal(kw["seed_x"], seeds[0])
    with pytest.raises(Handed):
        sweep(cases, engine=eng, integrals=True, survey=pts)
    assert eng.kw["energy_steps"] is None and eng.kw["grad"] is False and "nbins" not in eng.kw and "probe_x" not in eng.kw
    with pytest.raises(Handed):
        sweep(cases, engine=eng, integrals=True, probes=rake)
    assert "survey_x" not in eng.kw and np.array_equal(eng.kw["probe_z"], rake[1]) and eng.kw["probe_shift_x"] is None


class CountingIntegrals(Counting):
    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
                     "ensemble_run_surveyed_graded", "ensemble_run_integrals"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


class CountingOlder(Counting):
    """every older entry, not the new one"""

    def __init__(self):
        super().__init__()
        for name in ("ensemble_run_probed", "ensemble_run_traced", "ensemble_run_surveyed", "ensemble_run_surveyed_binned",
                     "ensemble_run_surveyed_graded"):
            setattr(self, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(_n + " reached")))


S1 = dict(tf=1, dt=5e-2)            # 21 time levels
S2 = dict(tf=0.5, dt=5e-2)          # 11


@pytest.mark.parametrize("cases,kwargs,engine,word", [
    ([S1], dict(integrals=1), CountingIntegrals, "integrals=1: integrals must be True or False"),
    ([S1], dict(integrals=None), CountingIntegrals, "integrals must be True or False"),
    ([S1], dict(integrals="yes"), CountingIntegrals, "integrals must be True or False"),
    ([S1], dict(energy_steps=(1, 5, 1)), CountingIntegrals, "sweep: energy_steps needs integrals=True"),
    ([S1], dict(integrals=False, energy_steps=(1, 5, 1)), CountingIntegrals, "sweep: energy_steps needs integrals=True"),
    ([S1], dict(integrals=True, energy_steps=(0, 5, 1)), CountingIntegrals, "sweep: energy_steps: first >= 1 and every >= 1"),
    ([S1], dict(integrals=True, energy_steps=(1, 5, 0)), CountingIntegrals, "sweep: energy_steps: first >= 1 and every >= 1"),
    ([S1], dict(integrals=True, energy_steps=(1, 5)), CountingIntegrals, "sweep: energy_steps must be three integers"),
    ([S1], dict(integrals=True, energy_steps=(1, 5.5, 1)), CountingIntegrals, "sweep: energy_steps must be three integers"),
    ([S1], dict(integrals=True, energy_steps=(5, 5, 1)), CountingIntegrals, r"energy_steps: the window \[5, 5\) holds no time step"),
    ([S1, S2], dict(integrals=True, energy_steps=(11, 20, 1)), CountingIntegrals,
     r"sweep: member 1: energy_steps: the window \[11, 11\) holds no time step of its 10"),
    ([S1, dict(S1, integrals=True)], {}, CountingIntegrals, "member 1: `integrals` belongs to the sweep"),
    ([S1, dict(S1, integrals=False)], dict(integrals=True), CountingIntegrals, "member 1: `integrals` belongs to the sweep"),
    ([dict(S1, energy_steps=(1, 5, 1)), S1], dict(integrals=True), CountingIntegrals, "member 0: `energy_steps` belongs to the sweep"),
    # the solo keywords stay refused, with the words they had
    ([S1], dict(wake_integrals=True), CountingIntegrals, "sweep: wake_integrals=True: .*solo keyword.*integrals=True"),
    ([S1], dict(integrals=True, wake_energy_steps=(1, 5, 1)), CountingIntegrals, "sweep: wake_energy_steps=.*solo keyword"),
    ([S1, dict(S1, wake_integrals=True)], dict(integrals=True), CountingIntegrals, "sweep: member 1: wake_integrals=True: .*solo keyword"),
    ([S1, dict(S1, wake_energy_steps=(1, 5, 1))], {}, CountingIntegrals, "sweep: member 1: wake_energy_steps=.*solo keyword"),
    ([S1], dict(integrals=True), CountingOlder, "sweep: integrals: this engine has no ensemble_run_integrals"),
    ([S1], dict(integrals=True, energy_steps=(1, 5, 1), survey=np.zeros([2, 3]), survey_grad=True), CountingOlder,
     "sweep: integrals: this engine has no ensemble_run_integrals"),
])
def test_refusals_make_no_engine_call(cases, kwargs, engine, word):
    from ludvm_amd import sweep
    eng = engine()
    with pytest.raises(ValueError, match=word):
        sweep(cases, engine=eng, **kwargs)
    assert eng.ncalls == []


def test_abi_7_declares_and_exports_the_integrals_ensemble_entry_point():
    from ludvm_amd import _ffi
    lib = _ffi.load()
    assert _ffi.ABI_VERSION == 7 and lib.ludvm_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    name = "ludvm_ensemble_run_integrals"
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert decl and name in _ffi.SIGNATURES and hasattr(lib, name) and name in _ffi.ADDED_IN_ABI_7
    # ludvm_ensemble_run_surveyed_graded's arguments, then the seven of the integrals
    extra = [_ffi._pd, _ffi.c_size_t, _ffi._pd, _ffi.c_size_t, _ffi.c_longlong, _ffi.c_longlong, _ffi.c_longlong]
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["ludvm_ensemble_run_surveyed_graded"] + extra
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    graded = re.search(r"\bint\s+ludvm_ensemble_run_surveyed_graded\s*\((.*?)\)\s*;", plain, flags=re.S)
    assert params[:-7] == [" ".join(p.split()) for p in graded.group(1).split(",")]
    assert params[-7:] == ["double* integral_sums", "size_t integral_doubles", "double* energy", "size_t energy_doubles",
                           "long long energy_first", "long long energy_stop", "long long energy_every"]
    assert len(params) == len(_ffi.SIGNATURES[name])
    assert "global: ludvm_*;" in open(os.path.join(ROOT, "ludvm_amd", "csrc", "exports.map")).read()
    for lib_path in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT " + name + r"$", out, re.M), lib_path
    ints = (_ffi.c_int, _ffi.c_size_t, _ffi.c_longlong)
    assert getattr(lib, name)(*([None] + [0 if t in ints else None for t in _ffi.SIGNATURES[name][1:]])) == _ffi.E_ARG
    from ludvm_amd import Engine
    assert hasattr(Engine, "ensemble_run_integrals")


FAMILIES = {"ensemble_march": 2, "ensemble_traced": 2, "ensemble_surveyed": 4, "ensemble_binned": 4, "ensemble_graded": 4}
BINNED_TUPLES = {"ILb0ELb0E": (106, 218, 0, 2, 129, 0, 16272), "ILb1ELb0E": (106, 218, 0, 2, 158, 0, 16272),
                 "ILb0ELb1E": (106, 219, 0, 2, 173, 0, 16272), "ILb1ELb1E": (106, 219, 0, 2, 172, 0, 16272)}


def test_the_sixteen_instantiations_of_the_integrals_kernel_fit_and_the_other_families_are_compiled_as_before():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): ensemble_integrals<PROBES, TRACERS, SURVEY> exists sixteen times;
    they use no scratch, spill no vector register, have no dynamic stack, use no AGPRs, keep two waves per SIMD and no more static
    LDS than the family's 16272 bytes.  The name holds none of the substrings the older tests count their kernels by; those
    families have the counts they had, and the four ensemble_binned kernels the tuples they had.  The tuples of the sixteen are
    printed, as DESIGN.md section 4.23 records them."""
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
    mine = {k: v for k, v in kernels.items() if "ensemble_integrals" in k}
    assert len(mine) == 16, sorted(kernels)
    assert not [k for k in mine for old in FAMILIES if old in k]
    for probes in (0, 1):
        for tracers in (0, 1):
            for survey in range(4):
                flags = f"ensemble_integralsILb{probes}ELb{tracers}ELi{survey}E"
                found = [v for k, v in mine.items() if flags in k]
                assert len(found) == 1, (flags, sorted(mine))
                r = found[0]
                print(f"ensemble_integrals<{bool(probes)}, {bool(tracers)}, {survey}>:".lower(), tup(r))
                assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
                assert int(r["Occupancy [waves/SIMD]"]) >= 2 and int(r["AGPRs"]) == 0, r
                assert int(r["LDS Size [bytes/block]"]) <= 16272, r
    for family, count in FAMILIES.items():
        assert len([k for k in kernels if family in k]) == count, family
    for flags, expect in BINNED_TUPLES.items():
        found = [v for k, v in kernels.items() if "ensemble_binned" + flags in k]
        assert len(found) == 1 and tup(found[0]) == expect, (flags, [tup(v) for v in found])
