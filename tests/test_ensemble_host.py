"""CPU tier of `sweep` (many small simulations in one device launch): the host side -- packing of every member's inputs,
per-member offsets, ragged step counts, storing of the returned rows, LEV_shed / slot bookkeeping, the phantom LEV slot --
against solo runs, with a test-side engine that checks what it is handed and answers with those solo runs' results in
the device layout (include/ludvm_hip.h, ludvm_ensemble_run).  No second implementation of the step mathematics.
Plus: every refusal, and the resources of the new kernel as hipcc compiles it for gfx950."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from conftest import CONFIG1, ROOT, load_golden
from fake_engine import FakeEngine

H = 12      # head of a march row (ludvm_march_run)


def mixed_cases():
    g = load_golden("g5_freevort.npz")
    return [dict(CONFIG1, tf=3),
            dict(CONFIG1, tf=2, method="Ramesh"),
            dict(CONFIG1, tf=5, alpha_m=5, alpha_max=15),
            dict(CONFIG1, tf=5, circulation_freevort=g["gamma_freevort"], xy_freevort=g["xy_freevort"]),
            dict(CONFIG1, tf=2, dt=2.5e-2)]


class SetupRecorder(FakeEngine):
    """Looks like an engine with the march to LUDVM._loop_prepare_engine and keeps what it hands march_setup."""

    def march_setup(self, npan, ncoef, scalars, tables, kin):
        self.setup = (npan, ncoef, np.asarray(scalars, dtype=float), np.asarray(tables), np.asarray(kin))

    def march_run(self, *a, **k):
        raise AssertionError("not called")


def wake_order(solo, s):
    """(kind, index) of the wake's vortices after step s, in shedding order: FREE first, then each step's TEV (and LEV)."""
    nf = solo.n_freevort
    order = [("FREE", k) for k in range(nf)]
    for q in range(1, s + 1):
        order.append(("TEV", q - 1))
        if solo.LEV_shed[q] != -1:
            order.append(("LEV", int(solo.LEV_shed[q])))
    return order


class EnsembleFake(FakeEngine):
    """Holds a solo per-step run per case; `ensemble_run` (a) asserts the packed inputs are, member by member, what
    _loop_prepare_engine hands march_setup for that solo object and (b) returns the solo results in the device layout."""
    MARCH_ROW_HEAD = H

    def __init__(self, cases, snapshot_steps):
        super().__init__()
        from ludvm_amd import LUDVM
        self.snaps = sorted(int(s) for s in snapshot_steps if s >= 1)
        self.solos, self.setups = [], []
        self.ensemble_calls = 0
        for kw in cases:
            self.solos.append(LUDVM(**kw, verbose=False, engine=FakeEngine(), precision="f64", history="full", march=False))
            rec = SetupRecorder()
            obj = LUDVM(**kw, verbose=False, engine=rec, precision="f64", history="sparse", run=False)
            S = obj._loop_begin()
            obj._free_slot, S.fsl = None, slice(0, S.nf)
            obj._loop_prepare_engine(S)
            self.setups.append(rec.setup)

    def ensemble_run(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=()):
        self.ensemble_calls += 1
        members = len(self.solos)
        scalars, tables, init = np.asarray(scalars), np.asarray(tables), np.asarray(init)
        kin, free_xzg, desc = np.asarray(kin), np.asarray(free_xzg), np.asarray(desc)
        assert list(snap_steps) == self.snaps
        assert desc.shape == (members, 6) and scalars.shape == (members, 12) and init.shape == (members, 8 + ncoef)
        nrec = len(self.snaps) + 1
        row_doubles = H + 2 * ncoef + 2 * npan
        rows = np.full([int((desc[:, 0] - 1).sum()), row_doubles], np.nan)
        wakes = np.full(int((nrec * 3 * (desc[:, 2] + 2 * (desc[:, 0] - 1))).sum()), np.nan)
        wake_n = np.full([members, nrec], -7, dtype=np.int64)
        kin_off = free_off = row_off = wake_off = 0
        for m, (solo, setup) in enumerate(zip(self.solos, self.setups)):
            nt, nf = solo.nt, solo.n_freevort
            cap = nf + 2 * (nt - 1)
            # (a) the inputs
            assert list(desc[m]) == [nt, kin_off, nf, free_off, row_off, wake_off], (m, desc[m])
            assert (npan, ncoef) == setup[:2]
            assert np.abs(scalars[m] - setup[2]).max() <= 1e-15
            assert tables[m].shape == setup[3].shape and np.abs(tables[m] - setup[3]).max() <= 1e-15
            assert np.abs(kin[kin_off:kin_off + nt] - setup[4]).max() <= 1e-15
            foil = solo.path["airfoil"]
            place = [foil[0, 0, -1] + 0.5 * solo.Uinf * solo.dt, foil[1, 0, 0], foil[0, 1, -1], foil[1, 1, 0]]
            assert np.abs(init[m, :4] - place).max() <= 1e-15
            assert init[m, 4] == solo.LESPcrit and np.all(init[m, 5:8] == 0)
            assert np.abs(init[m, 8:] - solo.fourier[0, 0]).max() <= 1e-15
            fr = free_xzg[3 * free_off:3 * (free_off + nf)]
            xy = np.array(solo.xy_freevort, dtype=float).reshape(2, nf)
            assert np.abs(fr - np.concatenate([xy[0], xy[1], np.asarray(solo.circulation_freevort, float)])).max() <= 1e-15
            # (b) the solo run's results in the device layout
            C, P = solo.circulation, solo.path
            shed_before = 0
            for s in range(1, nt):
                r = rows[row_off + s - 1]
                shed = solo.LEV_shed[s] != -1
                r[0], r[3], r[4], r[5] = C["TEV"][s - 1], C["bound"][s - 1], solo.LESP_prev[s - 1], solo.LESP[s - 1]
                r[1] = C["LEV"][int(solo.LEV_shed[s])] if shed else 0.0
                r[2] = float(shed)
                r[6], r[7], r[8] = solo.Fn[s], solo.Fs[s], solo.M[s]
                r[9] = nf + (s - 1) + shed_before
                r[10:12] = 0.0 if shed else P["LEV"][s][:, shed_before] / solo.dt
                r[H:H + ncoef], r[H + ncoef:H + 2 * ncoef] = solo.fourier[s, 0], solo.fourier[s, 1]
                r[H + 2 * ncoef:H + 2 * ncoef + npan] = C["gamma_airfoil"][s - 1]
                r[H + 2 * ncoef + npan:] = C["airfoil"][s - 1]
                shed_before += int(shed)
            gam = {"FREE": np.asarray(C["FREE"], float), "TEV": C["TEV"], "LEV": C["LEV"]}
            for k, s in enumerate(self.snaps + [nt - 1]):
                if k < len(self.snaps) and s > nt - 1:
                    wake_n[m, k] = -1
                    continue
                order = wake_order(solo, s)
                rec = wakes[wake_off + k * 3 * cap:wake_off + (k + 1) * 3 * cap]
                for i, (kind, idx) in enumerate(order):
                    rec[i], rec[cap + i], rec[2 * cap + i] = P[kind][s][0, idx], P[kind][s][1, idx], gam[kind][idx]
                wake_n[m, k] = len(order)
            kin_off, free_off, row_off, wake_off = kin_off + nt, free_off + nf, row_off + nt - 1, wake_off + nrec * 3 * cap
        assert kin.shape[0] == kin_off and len(free_xzg) == 3 * free_off
        return rows, wakes, wake_n


SNAPS = (1, 2, 10, 50, 70)        # (70 lies beyond the last step of the shorter members: skipped for them)


@pytest.fixture(scope="module")
def fake():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return EnsembleFake(mixed_cases(), SNAPS)


def test_sweep_packs_members_and_stores_their_rows_like_solo_runs(fake):
    import ludvm_amd
    from ludvm_amd import LUDVM, SparseHistory
    assert hasattr(ludvm_amd, "sweep") and hasattr(LUDVM, "sweep")
    sims = LUDVM.sweep(mixed_cases(), engine=fake, snapshot_steps=SNAPS)
    assert fake.ensemble_calls == 1 and len(sims) == len(fake.solos)
    assert len({s.nt for s in sims}) >= 3                    # ragged step counts
    for m, (sim, solo) in enumerate(zip(sims, fake.solos)):
        assert isinstance(sim, LUDVM) and sim.precision == "f64" and sim.history == "sparse"
        assert (sim.nt, sim.itev, sim.ilev) == (solo.nt, solo.itev, solo.ilev), m
        assert np.array_equal(sim.LEV_shed, solo.LEV_shed), m
        for name in ("Cl", "Cd", "Cm", "Cn", "Cs", "Ct", "Fn", "Fs", "L", "D", "T", "M", "LESP", "LESP_prev", "fourier"):
            assert np.abs(getattr(sim, name) - getattr(solo, name)).max() <= 1e-13, (m, name)
        assert set(sim.circulation) == set(solo.circulation)
        for key in solo.circulation:
            assert np.abs(np.asarray(sim.circulation[key], float) - np.asarray(solo.circulation[key], float)).max() <= 1e-13, (m, key)
        nt = sim.nt
        stored = sorted({0} | {s for s in SNAPS if s <= nt - 1} | {nt - 1})
        for key in ("TEV", "LEV", "FREE"):
            assert isinstance(sim.path[key], SparseHistory) and sim.path[key].steps() == stored, (m, key)
        for s in stored[1:]:
            shed_so_far = int((solo.LEV_shed[:s + 1] != -1).sum())
            n_lev = shed_so_far + (0 if solo.LEV_shed[s] != -1 else 1)      # the phantom slot of a non-shedding step
            for key, ncol in (("TEV", s), ("LEV", n_lev), ("FREE", solo.n_freevort)):
                row = sim.path[key][s]
                assert row.shape == (2, ncol), (m, key, s, row.shape)
                assert np.abs(row - solo.path[key][s][:, :ncol]).max() <= 1e-13, (m, key, s)
    # both kinds of recorded step occur: one that sheds a LEV, and one that does not (the phantom slot)
    kinds = {bool(sol.LEV_shed[s] != -1) for sol in fake.solos for s in SNAPS + (sol.nt - 1,) if s <= sol.nt - 1}
    assert kinds == {True, False}
    # flowfield works on a member for a stored step
    sims[0].flowfield(xmin=-1, xmax=0, zmin=-0.5, zmax=0.5, dr=0.25, tsteps=[2])
    fake.solos[0].flowfield(xmin=-1, xmax=0, zmin=-0.5, zmax=0.5, dr=0.25, tsteps=[2])
    assert np.abs(sims[0].u_ff - fake.solos[0].u_ff).max() <= 1e-12


class Counting(FakeEngine):
    """Counts every method call made on the engine."""

    def __init__(self, with_ensemble=True):
        super().__init__()
        self.ncalls = []
        if with_ensemble:
            self.ensemble_run = lambda *a, **k: (_ for _ in ()).throw(AssertionError("ensemble_run reached"))

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if callable(v) and not name.startswith("_"):
            log = object.__getattribute__(self, "ncalls")

            def counted(*a, **k):
                log.append(name)
                return v(*a, **k)
            return counted
        return v


@pytest.mark.parametrize("cases,common,word", [
    ([dict(tf=1), dict(tf=1, Npoints=61)], {}, "member 1"),
    ([dict(tf=1), dict(tf=1, Ncoeffs=20)], {}, "member 1"),
    ([dict(tf=1), dict(tf=1), dict(tf=40, dt=1e-2)], {}, "member 2"),                 # 4000 steps
    ([dict(tf=1, circulation_freevort=np.zeros(9000), xy_freevort=np.zeros([2, 9000]))], {}, "on its own"),
    ([dict(tf=1, precision="f32")], {}, "member 0"),
    ([dict(tf=1), dict(tf=1, precision="f32x2")], {}, "member 1"),
    ([dict(tf=1)], dict(history="full"), "member 0"),
    ([dict(tf=1, checkpoint_every=10, checkpoint_path="x.npz")], {}, "member 0"),
    ([dict(tf=1, checkpoint_path="x.npz")], {}, "member 0"),
    ([dict(tf=1, distributed="rccl")], {}, "member 0"),
    ([dict(tf=1, devices=[0, 1])], {}, "member 0"),
    ([dict(tf=1)], dict(march=False), "member 0"),
    ([dict(tf=1, run=False)], {}, "member 0"),
])
def test_sweep_refusals_make_no_engine_call(cases, common, word):
    from ludvm_amd import sweep
    eng = Counting()
    with pytest.raises(ValueError, match=word):
        sweep(cases, engine=eng, **common)
    assert eng.ncalls == []


@pytest.mark.parametrize("kw,word", [(dict(Npoints=2), "Npoints=2"), (dict(Npoints=1), "Npoints=1"), (dict(Npoints=258), "Npoints=258"),
                                     (dict(Ncoeffs=3), "Ncoeffs=3"), (dict(Ncoeffs=65), "Ncoeffs=65")])
def test_sweep_refuses_sections_and_coefficient_counts_it_cannot_run_by_name(kw, word):
    """Npoints = 2 (one panel) used to pass the keyword check and fail in the constructor with a bare IndexError; the smallest
    and largest shapes a sweep takes pass it (Npoints = 3 / 257, Ncoeffs = 4 / 64)."""
    from ludvm_amd import sweep
    from ludvm_amd.ensemble import _check_case
    eng = Counting()
    with pytest.raises(ValueError, match="member 1.*" + word):
        sweep([dict(tf=1, **{k: 30 if k == "Ncoeffs" else 81 for k in kw}), dict(tf=1, **kw)], engine=eng)
    assert eng.ncalls == []
    assert _check_case(0, dict(CONFIG1, tf=1, Npoints=3, Ncoeffs=4), None) == (3, 4)
    assert _check_case(0, dict(CONFIG1, tf=1, Npoints=257, Ncoeffs=64), None) == (257, 64)


def test_sweep_refuses_an_engine_without_ensemble_run_and_returns_nothing_for_no_cases():
    from ludvm_amd import LUDVM, sweep
    eng = Counting(with_ensemble=False)
    with pytest.raises(ValueError, match="ensemble_run"):
        sweep([dict(tf=1)], engine=eng)
    assert eng.ncalls == []
    assert sweep([], engine=eng) == [] and LUDVM.sweep([], engine=eng) == [] and eng.ncalls == []


def test_python_mirrors_the_header_limits():
    from ludvm_amd import _ffi
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    defs = dict(re.findall(r"#define (LUDVM_ENSEMBLE_\w+) (\d+)", text))
    assert int(defs["LUDVM_ENSEMBLE_MAX_STEPS"]) == _ffi.ENSEMBLE_MAX_STEPS
    assert int(defs["LUDVM_ENSEMBLE_MAX_WAKE"]) == _ffi.ENSEMBLE_MAX_WAKE
    assert int(defs["LUDVM_ENSEMBLE_MAX_SNAPSHOTS"]) == _ffi.ENSEMBLE_MAX_SNAPSHOTS
    assert int(defs["LUDVM_ENSEMBLE_INIT_HEAD"]) == _ffi.ENSEMBLE_INIT_HEAD
    assert int(defs["LUDVM_ENSEMBLE_DESC"]) == _ffi.ENSEMBLE_DESC
    # config 1 and the G5 cases are inside
    assert 400 <= _ffi.ENSEMBLE_MAX_STEPS and 1 + 2 * 400 <= _ffi.ENSEMBLE_MAX_WAKE


def test_ensemble_kernel_resources_and_the_march_kernels_are_as_before():
    """As hipcc compiles march.hip for gfx950 (no GPU needed): the ensemble kernel uses no scratch, spills no vector
    register and keeps its static LDS small enough for at least two workgroups per CU (<= 80 KiB of 160 KiB); the kernels of
    the solo march report what they reported before the ensemble was added to their translation unit."""
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
    ens = {k: v for k, v in kernels.items() if "ensemble_march" in k}
    assert len(ens) >= 1, sorted(kernels)
    for name, r in ens.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 80 * 1024, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r)            # 256 threads = one wave per SIMD per workgroup
    # (SGPRs, VGPRs, scratch, occupancy, SGPR spill, VGPR spill, LDS) of the solo march's kernels on the parent commit
    before = {"march_begin": (28, 20, 0, 8, 0, 0, 32), "march_chord_finish": (19, 20, 0, 8, 0, 0, 0),
              "march_solve": (94, 150, 0, 3, 0, 0, 3328), "march_finish_sym": (102, 57, 0, 7, 0, 0, 3088)}
    for short, want in before.items():
        hits = [v for k, v in kernels.items() if re.search(r"\d" + short + "E", k)]
        assert len(hits) == 1, (short, sorted(kernels))
        r = hits[0]
        got = tuple(int(r[k]) for k in ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
                                        "VGPRs Spill", "LDS Size [bytes/block]"))
        assert got == want and int(r["AGPRs"]) == 0, (short, got, want)
