"""GPU tier: the resident roll-up through the engine (wake_advect, wake_step_into) against the float64 oracle at the wake and
foil counts where its bookkeeping changes branch: an origin class less than half full, a block that holds one vortex, wakes
on both sides of every block and tile edge up to 1024, foil counts on both sides of the finisher's 256-source chunk, bound
vortices that open a block, and a call inside which the wake arrays grow.

The layout is where plain fp32 coordinates would lose three digits (|x| ~ 50, neighbours 1e-3 apart, v_core = 1.3e-3): a
sheet in shedding order whose newest vortex, the last one, sits next to the foil."""
import numpy as np
import pytest

from observer_sources_common import fast_iv

pytestmark = pytest.mark.gpu

VC, DT = 1.3e-3, 1e-3
TOL = {"f32": 1e-5, "f32x2": 3e-6, "f64": 1e-12}       # of max|u|: include/ludvm_hip.h; test_wake_advect_is_one_reference_roll_up_step
EULER = 2e-14                                          # the float64 update of the masters at |x| ~ 50 (fma or not)
N_WAKE = (1, 2, 3, 127, 128, 129, 130, 255, 256, 257, 258, 383, 384, 385, 386, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025)
N_FOIL = (0, 1, 2, 80, 255, 256, 257, 513)
KERNELS = {"direct": 0, "symmetric": 2}                # set_symmetric: never / from two vortices


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


def sheet(n, seed=0):
    """n vortices in shedding order: index k at x = -50 - 1e-3 (n - 1 - k)."""
    rng = np.random.default_rng(1000 + seed)
    x = -50.0 - 1e-3 * (n - 1 - np.arange(n, dtype=float))
    z = 0.3 * np.sin(0.7 * x) + 1e-3 * rng.standard_normal(n)
    g = 1e-3 * rng.standard_normal(n)
    return x, z, g


def foil(nfoil, seed=0):
    """Bound vortices on x in [-50 + 1e-3, -49], strengths a hundredth of the wake's."""
    rng = np.random.default_rng(2000 + seed)
    x = np.linspace(-50.0 + 1e-3, -49.0, nfoil)
    z = 0.3 * np.sin(0.7 * x)
    return x, z, 1e-5 * rng.standard_normal(nfoil)


def velocity(iv, wake, bound, x, z):
    """(u, w) of wake + bound vortices at (x, z), float64."""
    u, w = iv(wake[2], wake[0], wake[1], x, z, VC)
    if len(bound[0]):
        uf, wf = iv(bound[2], bound[0], bound[1], x, z, VC)
        u, w = u + uf, w + wf
    return u, w


def check_advect(eng, iv, n, nfoil, precision, label):
    x, z, g = sheet(n)
    fx, fz, fg = foil(nfoil)
    tol = TOL[precision]
    eng.wake_clear()
    eng.wake_append(x, z, g)
    ur, wr = velocity(iv, (x, z, g), (fx, fz, fg), x, z)
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    u, w = eng.wake_advect(DT, fx, fz, fg, VC, precision=precision, return_velocity=True)
    err = max(np.abs(u - ur).max(), np.abs(w - wr).max())
    assert err <= tol * scale, (label, "first step", err / max(scale, 1e-300))
    assert eng.wake_size() == n, label
    xn, zn, gn = eng.wake_read(0, n, gamma=True)
    assert np.array_equal(gn, g), label
    assert np.abs(xn - (x + DT * u)).max() <= EULER and np.abs(zn - (z + DT * w)).max() <= EULER, label
    # the second step reads the origins and mirrors the first one's finisher republished
    u2r, w2r = velocity(iv, (xn, zn, g), (fx, fz, fg), xn, zn)
    scale2 = max(np.abs(u2r).max(), np.abs(w2r).max())
    u2, w2 = eng.wake_advect(DT, fx, fz, fg, VC, precision=precision, return_velocity=True)
    err2 = max(np.abs(u2 - u2r).max(), np.abs(w2 - w2r).max())
    assert err2 <= tol * scale2, (label, "second step", err2 / max(scale2, 1e-300))
    x2, z2 = eng.wake_read(0, n)
    assert eng.wake_size() == n, label
    assert np.abs(x2 - (xn + DT * u2)).max() <= EULER and np.abs(z2 - (zn + DT * w2)).max() <= EULER, label
    return max(err / scale, err2 / scale2) if scale > 0 and scale2 > 0 else 0.0


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n", N_WAKE)
def test_wake_advect_at_block_tile_and_chunk_edges(eng, iv, n, kernel):
    worst = {}
    try:
        eng.set_symmetric(KERNELS[kernel])
        for precision in TOL:
            for nfoil in N_FOIL:
                e = check_advect(eng, iv, n, nfoil, precision, (n, nfoil, precision, kernel))
                worst[precision] = max(worst.get(precision, 0.0), e)
    finally:
        eng.set_symmetric(1)
    print(f"wake_advect n = {n} {kernel}: worst error / max|u| over nfoil in {N_FOIL}: "
          + ", ".join(f"{p} {v:.2e}" for p, v in worst.items()))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n", [2, 3, 129, 130, 255, 256, 257, 258, 300, 383, 384, 512, 513])
def test_wake_advect_with_the_zero_strength_slot_behind_the_wake(eng, iv, n, kernel):
    """What the per-step path of a time loop rolls up on a recorded step that sheds no leading-edge vortex: the wake, then
    a vortex of zero strength at the origin of the plane -- 50 chords from this wake -- as its last entry, then 80 bound
    vortices.  The slot is a target like any other and moves with the flow; as the newest vortex of its index parity it must
    not cost its origin class the local offsets."""
    xs, zs, gs = sheet(n)
    x, z, g = np.r_[xs, 0.0], np.r_[zs, 0.0], np.r_[gs, 0.0]
    fx, fz, fg = foil(80)
    ur, wr = velocity(iv, (x, z, g), (fx, fz, fg), x, z)
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    worst = {}
    try:
        eng.set_symmetric(KERNELS[kernel])
        for precision in TOL:
            for together in (True, False):       # appended with the shed vortices, or after them
                eng.wake_clear()
                if together:
                    eng.wake_append(x, z, g)
                else:
                    eng.wake_append(xs, zs, gs)
                    eng.wake_append([0.0], [0.0], [0.0])
                u, w = eng.wake_advect(DT, fx, fz, fg, VC, precision=precision, return_velocity=True)
                err = max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale
                worst[precision] = max(worst.get(precision, 0.0), err)
                assert err <= TOL[precision], (n, precision, kernel, together, err)
                xn, zn = eng.wake_read(0, n + 1)
                assert np.abs(xn - (x + DT * u)).max() <= EULER and np.abs(zn - (z + DT * w)).max() <= EULER
    finally:
        eng.set_symmetric(1)
    print(f"wake_advect n = {n} + zero-strength slot + 80 {kernel}: " + ", ".join(f"{p} {v:.2e}" for p, v in worst.items()))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n", [4016, 4017])
def test_wake_advect_when_the_arrays_grow_inside_the_call(iv, n, kernel):
    """A fresh engine holds 4096 entries after the first append: with 80 bound vortices n = 4016 fills them exactly and
    n = 4017 makes the call itself move the wake to larger arrays."""
    from ludvm_amd import Engine
    for precision in TOL:
        e = Engine(0)
        try:
            e.set_symmetric(KERNELS[kernel])
            err = check_advect(e, iv, n, 80, precision, (n, 80, precision, kernel))
            print(f"wake_advect n = {n} + 80 {kernel} {precision}: {err:.2e}")
        finally:
            e.close()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n0", [254, 255, 256, 510, 511, 512, 174, 175, 176])
def test_wake_step_appends_across_block_edges(eng, iv, n0, kernel):
    """The one-round-trip step: one or two vortices staged on, across and behind a block edge (254 .. 256, 510 .. 512) and,
    with 80 bound vortices behind them, a foil tail that opens a block (174 .. 176).  Positions against the oracle's Euler
    step of the staged state; tail, placement and chord sums against the separate calls on the state the step left."""
    from ludvm_amd.engine import PRECISIONS
    nfoil = 80
    fx, fz, fg = foil(nfoil)
    xt, zt = fx + 5e-4, fz + 1e-3
    te, le = np.array([fx[0] - 5e-4, fz[0]]), np.array([fx[-1], fz[-1]])
    b = eng.step_buffers(nfoil)
    try:
        eng.set_symmetric(KERNELS[kernel])
        for precision in ("f32", "f32x2"):
            for n_new in (1, 2):
                label = (n0, n_new, precision, kernel)
                xa, za, ga = sheet(n0 + n_new, seed=n_new)            # the newest n_new are the staged ones
                eng.wake_clear()
                eng.wake_append(xa[:n0], za[:n0], ga[:n0])
                # one earlier roll-up, so that the old wake's origins are a finisher's, as in a time loop
                eng.wake_advect(DT, fx, fz, fg, VC, precision=precision)
                xo, zo = eng.wake_read(0, n0)
                x, z = np.r_[xo, xa[n0:]], np.r_[zo, za[n0:]]
                eng.wake_step_into(b, np.ascontiguousarray(xa[n0:]), np.ascontiguousarray(za[n0:]), np.ascontiguousarray(ga[n0:]),
                                   DT, fx, fz, fg, VC, PRECISIONS[precision], te, le, n_new == 2, n_new, xt, zt)
                n = n0 + n_new
                assert eng.wake_size() == n, label
                ur, wr = velocity(iv, (x, z, ga), (fx, fz, fg), x, z)
                scale = max(np.abs(ur).max(), np.abs(wr).max())
                xn, zn, gn = eng.wake_read(0, n, gamma=True)
                assert np.array_equal(gn, ga), label
                err = max(np.abs(xn - (x + DT * ur)).max(), np.abs(zn - (z + DT * wr)).max()) / DT
                assert err <= TOL[precision] * scale + EULER / DT, (label, err / scale)
                # tail and placement: the newest vortices as the masters hold them, a third of the way from the edges
                assert np.array_equal(b.tail[0, :n_new], xn[-n_new:]) and np.array_equal(b.tail[1, :n_new], zn[-n_new:]), label
                tev = te + (np.array([xn[-n_new], zn[-n_new]]) - te) / 3
                lev = le + (np.array([xn[-1], zn[-1]]) - le) / 3 if n_new == 2 else le
                assert np.array_equal(b.unit[0], [tev[0], lev[0]]) and np.array_equal(b.unit[1], [tev[1], lev[1]]), label
                # chord sums: the separate call on the same state (another, equally fixed, order of the source splits)
                u, w, uu, wu = eng.wake_chord_sums(0, n, xt, zt, b.unit[0], b.unit[1], VC)
                assert np.abs(b.u - u).max() <= 1e-13 * np.abs(u).max() and np.abs(b.w - w).max() <= 1e-13 * np.abs(w).max(), label
                assert np.array_equal(b.uu, uu) and np.array_equal(b.wu, wu), label
                cu, cw = iv(ga, xn, zn, xt, zt, VC)
                assert np.abs(b.u - cu).max() <= 1e-11 * np.abs(cu).max() and np.abs(b.w - cw).max() <= 1e-11 * np.abs(cw).max(), label
                # the next roll-up reads what the step's staging and finisher left
                u2r, w2r = velocity(iv, (xn, zn, ga), (fx, fz, fg), xn, zn)
                u2, w2 = eng.wake_advect(DT, fx, fz, fg, VC, precision=precision, return_velocity=True)
                s2 = max(np.abs(u2r).max(), np.abs(w2r).max())
                err2 = max(np.abs(u2 - u2r).max(), np.abs(w2 - w2r).max())
                assert err2 <= TOL[precision] * s2, (label, "next step", err2 / s2)
                print(f"wake_step n0 = {n0} + {n_new} {kernel} {precision}: {err / scale:.2e}, next step {err2 / s2:.2e}")
    finally:
        eng.set_symmetric(1)
