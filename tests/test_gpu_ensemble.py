"""GPU tier of `sweep`: many small simulations in ONE device launch (ludvm_ensemble_run, csrc/ensemble_kernels.hpp) --
against the reference's golden runs, against solo runs on the same engine, bitwise independence of a member from its batch,
the context left alone, device-side refusals, and that the members really run side by side.  Tolerances are the ones
tests/test_gpu_wake.py uses for the same comparisons (tier T3, the G5 tests)."""
import time
import warnings

import numpy as np
import pytest

from conftest import CONFIG1, load_golden

pytestmark = pytest.mark.gpu

SNAPS = (1, 2, 10, 50)


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def golden_batch():
    g = load_golden("g5_freevort.npz")
    return [dict(CONFIG1), dict(CONFIG1, tf=2, method="Ramesh"), dict(CONFIG1, tf=5, alpha_m=5, alpha_max=15),
            dict(CONFIG1, tf=5, circulation_freevort=g["gamma_freevort"], xy_freevort=g["xy_freevort"])]


def test_mixed_batch_against_the_reference_golden_runs(eng):
    """One mixed batch: config 1 (tier T3 bounds, all of them), 'Ramesh', alpha_m, free vortices (the G5 bounds)."""
    from ludvm_amd import sweep
    g2 = load_golden("g2_config1.npz")
    sims = sweep(golden_batch(), engine=eng, snapshot_steps=SNAPS)
    sim = sims[0]
    assert (sim.nt, sim.itev, sim.ilev) == (401, 399, 202)
    assert np.array_equal(sim.LEV_shed, g2["LEV_shed"])
    for name in ("Cl", "Cd", "Cm"):
        d = np.abs(getattr(sim, name) - g2[name])
        print(f"member 0 {name}: max|d| [:100] {d[:100].max():.3e} [:200] {d[:200].max():.3e} all {d.max():.3e}; "
              f"mean[200:] diff {abs(getattr(sim, name)[200:].mean() - g2[name][200:].mean()):.3e}")
        assert d[:100].max() <= 1e-9 and d[:200].max() <= 1e-7 and d.max() <= 1e-3, name
        assert abs(getattr(sim, name)[200:].mean() - g2[name][200:].mean()) <= 1e-4, name
    np.testing.assert_allclose(sim.circulation["TEV"][:200], g2["circ_TEV"][:200], rtol=0, atol=1e-7)
    np.testing.assert_allclose(sim.fourier[:200], g2["fourier"][:200], rtol=0, atol=1e-6)
    for s in SNAPS:      # the stored sparse row against the leading columns of the golden dense row
        for key in ("TEV", "LEV", "FREE"):
            row = sim.path[key][s]
            assert row.shape[1] >= 1, (key, s)
            np.testing.assert_allclose(row, g2[f"{key}_{s}"][:, :row.shape[1]], rtol=0, atol=1e-9, err_msg=f"{key}@{s}")
        assert sim.path["TEV"][s].shape[1] == s
    c = sim.circulation
    assert abs(c["bound"][399] + c["TEV"].sum() + c["LEV"].sum() - c["IC"]) < 1e-9      # Kelvin
    assert np.abs(sim.LESP).max() <= 0.2 + 1e-9
    for m, fixture in ((1, "g5_ramesh.npz"), (2, "g5_alpham.npz")):
        g = load_golden(fixture)
        assert np.array_equal(sims[m].LEV_shed, g["LEV_shed"]), m
        for name in ("Cl", "Cd", "Cm", "LESP"):
            d = np.abs(getattr(sims[m], name) - g[name]).max()
            print(f"member {m} {name}: max|d| {d:.3e}")
            assert d <= 1e-7, (m, name)
    g = load_golden("g5_freevort.npz")
    assert np.array_equal(sims[3].LEV_shed, g["LEV_shed"])
    for name in ("Cl", "Cd", "Cm"):
        d = np.abs(getattr(sims[3], name) - g[name]).max()
        print(f"member 3 {name}: max|d| {d:.3e}")
        assert d <= 1e-6, name
    np.testing.assert_allclose(sims[3].path["FREE"][10], g["FREE_10"], rtol=0, atol=1e-9)


def grid_cases():
    cases = [dict(LESPcrit=l, alpha_max=a) for l in (0.1, 0.2, 0.3, 10) for a in (10, 20)]
    cases += [dict(dt=2.5e-2), dict(k=0.4 * np.pi), dict(Naca="2412"), dict(method="Ramesh")]
    return cases


def test_members_against_solo_runs_on_the_same_engine(eng):
    """The 12-member grid: a member and its solo precision='f64' run differ by summation order only -- the T3 windows
    (1e-9 over the first 100 steps, 1e-7 over the first 200).  tf = 10: 200 steps (400 for the dt = 2.5e-2 member), which is
    all the windows cover."""
    from ludvm_amd import LUDVM, sweep
    common = dict(CONFIG1, tf=10)
    cases = grid_cases()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the cambered section's "parity unpinned" warning
        sims = sweep(cases, engine=eng, **common)
        solos = [LUDVM(**dict(common, **kw), verbose=False, engine=eng, precision="f64", history="sparse") for kw in cases]
    assert len(sims) == 12
    for m, (sim, solo) in enumerate(zip(sims, solos)):
        if not np.array_equal(sim.LEV_shed, solo.LEV_shed):
            s = int(np.argmax(sim.LEV_shed != solo.LEV_shed))
            pytest.fail(f"member {m} {cases[m]}: LEV_shed differs first at step {s}: |A0| sweep {abs(sim.LESP_prev[s - 1])!r}, "
                        f"solo {abs(solo.LESP_prev[s - 1])!r}, LESPcrit {sim.LESPcrit}")
        assert (sim.nt, sim.itev, sim.ilev) == (solo.nt, solo.itev, solo.ilev), m
        for name in ("Cl", "Cd", "Cm"):
            d = np.abs(getattr(sim, name) - getattr(solo, name))
            print(f"member {m} {name}: max|d| [:100] {d[:100].max():.3e} [:200] {d[:200].max():.3e}")
            assert d[:100].max() <= 1e-9 and d[:200].max() <= 1e-7, (m, name)
    for m in (6, 7):
        assert cases[m]["LESPcrit"] == 10 and sims[m].ilev == 0 and np.all(sims[m].LEV_shed == -1)
    assert sims[8].nt == 401 and sims[0].nt == 201


def _bits(sim):
    last = sim.nt - 1
    return [sim.Cl, sim.fourier, sim.circulation["TEV"], sim.circulation["LEV"], sim.circulation["bound"], sim.circulation["airfoil"],
            sim.path["TEV"][last], sim.path["LEV"][last], sim.path["FREE"][last]]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def test_member_bits_do_not_depend_on_the_batch_and_repeat(eng):
    from ludvm_amd import sweep
    X = dict(CONFIG1)
    others = [dict(CONFIG1, tf=3 + (q % 5), LESPcrit=0.1 + 0.01 * (q % 17), alpha_max=5 + (q % 11),
                   method="Ramesh" if q % 7 == 0 else "Faure") for q in range(298)]
    alone = sweep([X], engine=eng)[0]
    batch = [X] + others + [X]
    assert len(batch) == 300
    first = sweep(batch, engine=eng)
    again = sweep(batch, engine=eng)
    assert _same_bits(alone, first[0]) and _same_bits(alone, first[299])
    for a, b in zip(first, again):
        assert _same_bits(a, b)
    assert not np.array_equal(first[1].Cl, first[2].Cl)          # (the other members are different cases)


def test_the_context_is_left_alone(eng):
    from ludvm_amd import LUDVM, sweep
    cases = golden_batch()[1:]

    def solo():
        s = LUDVM(**CONFIG1, verbose=False, engine=eng, precision="f32", history="sparse")
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.path["LEV"][s.nt - 1]]
    before = solo()
    sweep(cases, engine=eng)
    after = solo()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))

    # a hand-placed resident wake
    rng = np.random.default_rng(3)
    x, z, g = rng.uniform(-3, 0, 500), rng.uniform(-1, 1, 500), rng.standard_normal(500)
    eng.wake_clear()
    eng.wake_append(x, z, g)
    sweep(cases, engine=eng, snapshot_steps=(3,))
    assert eng.wake_size() == 500
    xr, zr, gr = eng.wake_read(0, 500, gamma=True)
    assert np.array_equal(xr, x) and np.array_equal(zr, z) and np.array_equal(gr, g)

    # a sweep between two march_run calls of a chunked solo run
    class Chunked(LUDVM):
        _march_chunk = 96
        between = None

        def _march_call(self, S, i, j, rec_i, print_dt):
            super()._march_call(S, i, j, rec_i, print_dt)
            if self.between is not None and j < self.nt:
                self.between()

    def chunked(between):
        Chunked.between = staticmethod(between) if between else None
        s = Chunked(**CONFIG1, verbose=False, engine=eng, precision="f32", history="sparse")
        return [s.Cl, s.fourier, s.circulation["TEV"], s.path["TEV"][s.nt - 1], s.path["LEV"][s.nt - 1]]
    count = []
    plain = chunked(None)
    mixed = chunked(lambda: count.append(len(sweep(cases, engine=eng))))
    assert len(count) >= 3
    assert all(np.array_equal(a, b) for a, b in zip(plain, mixed))


def _arrays(members, npan=80, ncoef=30, nt=3, per_scalar=12):
    T = 8 * npan + ncoef * npan + (ncoef - 1) * npan
    scalars = np.ones([members, per_scalar])
    scalars[:, 8:] = 0.0
    desc = np.array([[nt, m * nt, 1, m, m * (nt - 1), m * 3 * (1 + 2 * (nt - 1))] for m in range(members)], dtype=np.int64)
    return dict(scalars=scalars, tables=np.zeros([members, T]), kin=np.zeros([members * nt, 7 + 2 * npan]),
                init=np.zeros([members, 8 + ncoef]), free_xzg=np.zeros(3 * members), desc=desc)


def test_device_side_refusals_launch_nothing(eng):
    from ludvm_amd import LUDVM, LudvmHipError, _ffi, sweep
    over = _arrays(2)
    over["desc"][1, 0] = _ffi.ENSEMBLE_MAX_STEPS + 2                 # a member over the cap (checked before its ranges)
    bad = [("member 1", dict(npan=80, ncoef=30, **over)),
           ("Npanels", dict(npan=257, ncoef=30, **_arrays(1, npan=257))),
           ("12 values", dict(npan=80, ncoef=30, **_arrays(2, per_scalar=11)))]
    for word, kw in bad:
        with pytest.raises(LudvmHipError) as e:
            eng.ensemble_run(kw.pop("npan"), kw.pop("ncoef"), kw["scalars"], kw["tables"], kw["kin"], kw["init"], kw["free_xzg"],
                             kw["desc"])
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (word, str(e.value))
    assert eng.ensemble_limits() == (_ffi.ENSEMBLE_MAX_STEPS, _ffi.ENSEMBLE_MAX_WAKE, _ffi.ENSEMBLE_MAX_SNAPSHOTS)
    assert sweep([], engine=eng) == []
    sim = sweep([dict(CONFIG1, tf=1)], engine=eng)[0]                # a following sweep works
    solo = LUDVM(**dict(CONFIG1, tf=1), verbose=False, engine=eng, precision="f64")
    assert np.abs(sim.Cl - solo.Cl).max() <= 1e-9


def test_members_run_side_by_side(eng):
    """The one timing assertion, deliberately loose: the device call for 256 copies of config 1 takes less than 32 x one solo
    config-1 time_loop (march, fp64, sparse history; set-up excluded on both sides) -- a speed-up of at least 8 over running
    them in turn.  Both measured here, best of 3 after a warm-up each."""
    from ludvm_amd import LUDVM, sweep
    spent = []
    inner = eng.ensemble_run

    def timed(*a, **k):
        t0 = time.perf_counter()
        out = inner(*a, **k)
        spent.append(time.perf_counter() - t0)
        return out
    eng.ensemble_run = timed
    try:
        batch = [dict(CONFIG1)] * 256
        for _ in range(4):
            sims = sweep(batch, engine=eng)
    finally:
        del eng.ensemble_run
    t_batch = min(spent[1:])
    t_solo = []
    for _ in range(4):
        s = LUDVM(**CONFIG1, verbose=False, engine=eng, precision="f64", history="sparse", run=False)
        t0 = time.perf_counter()
        s.time_loop()
        t_solo.append(time.perf_counter() - t0)
    t_solo = min(t_solo[1:])
    print(f"256 members: device call {t_batch * 1e3:.2f} ms; one solo time_loop {t_solo * 1e3:.2f} ms; "
          f"ratio {t_batch / t_solo:.2f} (bound 32), speed-up over running in turn {256 * t_solo / t_batch:.1f}x")
    assert np.array_equal(sims[0].Cl, sims[255].Cl)
    assert t_batch < 32 * t_solo
