"""GPU tier of the symmetric-kernel shape table (tests/sym_shapes_common.py): every variant of pair_sym_f32<T, HILO, R> and
pair_sym_quad_f32<8> by value against the float64 reference at ALL targets, on rings of 1 .. 25 tiles, where items run several
rounds, workgroups hold idle waves, owners hold nothing or one ragged quad -- shapes the size rule never gives the kernels in
production, forced by set_sym_tuning / set_tuning and, for the mixed form, the quad variant and the XCD placement, by engines of
the measurement build.  tests/test_sym_shapes_host.py proves the partition of every shape sent here, on the CPU.

Besides the values: a launch repeats bit for bit; LUDVM_XCD_RUN changes no bit; the owners' integer sums add up to the single
owner's; Morton order changes values within the tolerance only; the advect entry is x + dt u of the induce entry; a non-finite
input poisons the result; marched runs read their counts on the device.  Tolerances are imported, none is new."""
import contextlib
import os

import numpy as np
import pytest

import sym_shapes_common as S
import test_gpu_rollup_edges as E
from observer_sources_common import fast_iv
from oracle import g8_cases as G8
from rollup_common import CLOUDS, case_keywords
from test_gpu_direct_shapes import Guarded
from test_gpu_rollup_steps import check_run

pytestmark = pytest.mark.gpu

TOL = G8.TOL                               # the induce entries: plain 1e-5 (local 1e-5, hilo 2e-6)
WAKE_TOL = E.TOL                           # wake_advect: f32 1e-5, f32x2 3e-6
PRECISION = {"local": "f32", "hilo": "f32x2"}
ADVECT_DT, ADVECT_BOUND = 0.05, 1e-6       # tests/test_gpu_self_order.py::test_advect_step_in_morton_order


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


@pytest.fixture(scope="module")
def exp():
    """engines of the measurement build, by key of S.EXP, made when first asked for and closed with the module; the environment is
    set for the constructor only (tests/test_gpu_direct_shapes.py::exp)"""
    from ludvm_amd import Engine, _ffi
    made = {}

    def get(build):
        if build not in made:
            env = S.EXP[build]
            assert not any(k in os.environ for k in env)
            os.environ.update(env)
            try:
                made[build] = Engine(0, lib_path=_ffi.EXP_LIB_PATH)
            finally:
                for k in env:
                    del os.environ[k]
        return made[build]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def iv():
    return fast_iv()


@contextlib.contextmanager
def restored(*engines):
    try:
        yield
    finally:
        for e in engines:
            e.set_tuning(0, 0)
            e.set_sym_tuning(0, 0)
            e.set_symmetric(1)
            e.set_self_order(1)
            e.set_stream(None)
            e.wake_clear()


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _cases(family, **kw):
    return [c for c in S.table() if c.family == family and all(getattr(c, k) == v for k, v in kw.items())]


def _by_size(cases):
    out = {}
    for c in cases:
        out.setdefault(c.n, []).append(c)
    return out


class Ring:
    """one input of the plain form on the device, in guarded buffers, with its reference"""

    def __init__(self, torch, iv, n):
        self.torch, self.n = torch, n
        self.g, self.x, self.z, self.vc = S.cloud(n)
        self.src = [Guarded(torch, n, a) for a in (self.x, self.z, self.g)]
        self.out = [Guarded(torch, n), Guarded(torch, n)]
        self.ref = S.reference(iv, ("plain", n, 0), self.g, self.x, self.z, self.vc)

    def induce(self, e, what):
        for o in self.out:
            o.arm()
        s = self.src
        e.induce_dev(s[0].ptr(), s[1].ptr(), s[2].ptr(), self.n, s[0].ptr(), s[1].ptr(), self.n, self.vc, self.out[0].ptr(), self.out[1].ptr())
        self.torch.cuda.synchronize()
        return self.out[0].read(what), self.out[1].read(what)

    def advect(self, e, what):
        for o in self.out:
            o.arm()
        s = self.src
        e.advect_dev(s[0].ptr(), s[1].ptr(), s[2].ptr(), self.n, 0, self.n, self.vc, ADVECT_DT, self.out[0].ptr(), self.out[1].ptr())
        self.torch.cuda.synchronize()
        return self.out[0].read(what), self.out[1].read(what)


def _tune(e, c):
    e.set_sym_tuning(c.T, c.code)
    e.set_tuning(0, c.split)


def _check_plain(e, ring, c, worst):
    """the case by value at all targets, and again: the same bits"""
    _tune(e, c)
    got = ring.induce(e, c)
    err = S.rel_err(got[0], got[1], *ring.ref)
    worst[c.family] = max(worst.get(c.family, 0.0), err)
    assert err <= TOL["plain"], (c, err, TOL["plain"])
    assert _same_bits(got, ring.induce(e, c)), ("a launch repeats", c)
    return got


def _check_wake(e, iv, c, nfoil, worst, second=False):
    """wake_advect of the case's sheet (tests/test_gpu_rollup_edges.py::check_advect): velocities at all wake vortices against the
    float64 sums of wake + bound vortices; second: also the next step, which reads the origins the first one's finisher republished"""
    precision = PRECISION[c.form]
    g, x, z, vc = S.sheet(c.n)
    fx, fz, fg = S.foil(nfoil)
    _tune(e, c)
    e.wake_clear()
    e.wake_append(x, z, g)
    ur, wr = S.reference(iv, ("sheet", c.n, nfoil), g, x, z, vc, nfoil)
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    u, w = e.wake_advect(S.DT, fx, fz, fg, vc, precision=precision, return_velocity=True)
    err = max(np.abs(u - ur).max(), np.abs(w - wr).max()) / scale
    key = c.family + " " + c.form
    worst[key] = max(worst.get(key, 0.0), err)
    assert err <= WAKE_TOL[precision], (c, nfoil, "first step", err, WAKE_TOL[precision])
    assert e.wake_size() == c.n
    xn, zn = e.wake_read(0, c.n)
    assert np.abs(xn - (x + S.DT * u)).max() <= E.EULER and np.abs(zn - (z + S.DT * w)).max() <= E.EULER, c
    if second:
        u2r, w2r = E.velocity(iv, (xn, zn, g), (fx, fz, fg), xn, zn)
        s2 = max(np.abs(u2r).max(), np.abs(w2r).max())
        u2, w2 = e.wake_advect(S.DT, fx, fz, fg, vc, precision=precision, return_velocity=True)
        err2 = max(np.abs(u2 - u2r).max(), np.abs(w2 - w2r).max()) / s2
        worst[key] = max(worst[key], err2)
        assert err2 <= WAKE_TOL[precision], (c, nfoil, "second step", err2, WAKE_TOL[precision])
    return u, w


def _wake_family(e, iv, cases, worst):
    """every case with 0 and 80 bound vortices; per size one case (another one from size to size) also takes the second step"""
    for k, (n, group) in enumerate(sorted(_by_size(cases).items())):
        for j, c in enumerate(group):
            for nfoil in S.N_FOIL:
                _check_wake(e, iv, c, nfoil, worst, second=(nfoil == 80 and j == k % len(group)))


# ---- pair_sym_f32<T, false, R>, plain positions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", S.TS)
def test_plain_positions_every_tile_and_split_by_value_with_guards(eng, iv, T):
    """induce_dev on one array (guarded buffers) for R in {1, 2, 4} x d-chunks {0, 1, 2, 3} on rings of 1 .. 17 tiles with last tiles of
    1, 63, 64, 65, W - 1 and W members; per ring also advect_dev over the whole array (x + dt u of the induce entry) and the launch
    in Morton order (set_self_order(2): within the tolerance)"""
    import torch
    worst = {}
    with restored(eng):
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.set_symmetric(2)
        eng.set_self_order(0)
        for k, (n, group) in enumerate(sorted(_by_size(_cases("plain", T=T)).items())):
            ring = Ring(torch, iv, n)
            for j, c in enumerate(group):
                u, w = _check_plain(eng, ring, c, worst)
                if j == k % len(group):
                    xo, zo = ring.advect(eng, ("advect_dev", c))
                    assert np.abs(xo - (ring.x + ADVECT_DT * u)).max() <= ADVECT_BOUND, ("advect_dev", c)
                    assert np.abs(zo - (ring.z + ADVECT_DT * w)).max() <= ADVECT_BOUND, ("advect_dev", c)
                    eng.set_self_order(2)
                    try:
                        mo = ring.induce(eng, ("Morton order", c))
                        xm, zm = ring.advect(eng, ("advect_dev, Morton order", c))
                    finally:
                        eng.set_self_order(0)
                    err = S.rel_err(mo[0], mo[1], *ring.ref)
                    worst["morton"] = max(worst.get("morton", 0.0), err)
                    assert err <= TOL["plain"], ("Morton order", c, err)
                    assert np.abs(xm - (ring.x + ADVECT_DT * mo[0])).max() <= ADVECT_BOUND, ("advect_dev, Morton order", c)
                    assert np.abs(zm - (ring.z + ADVECT_DT * mo[1])).max() <= ADVECT_BOUND, ("advect_dev, Morton order", c)
    print(f"plain positions, T = {T}: worst error / max|u| = {worst['plain']:.2e}, in Morton order {worst['morton']:.2e} (bound {TOL['plain']:.0e})")


# ---- pair_sym_f32<T, false, R> with local origins, pair_sym_f32<4, true, R> ----------------------------------------------------------
@pytest.mark.parametrize("form,T", [("local", 4), ("local", 8), ("hilo", 4)])
def test_resident_wake_local_origins_and_hilo_by_value(eng, iv, form, T):
    """wake_advect(..., 'f32' | 'f32x2') on the sheet at |x| ~ 50, with 0 and 80 bound vortices, same rings, R and d-chunks; a second
    step per ring reads the republished origins"""
    worst = {}
    with restored(eng):
        eng.set_symmetric(2)
        _wake_family(eng, iv, _cases(form, T=T), worst)
    p = PRECISION[form]
    print(f"resident wake, {form}, T = {T}: worst error / max|u| = {worst[form + ' ' + form]:.2e} (bound {WAKE_TOL[p]:.0e})")


# ---- pair_sym_f32<T, false, 0>: the mixed form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", S.TS)
def test_mixed_granularity_by_value(exp, iv, T):
    """code -1 of the measurement build with LUDVM_SYM_TAIL_ITEMS = 17: a bulk of four-wave items in front of a tail of four-wave
    items (0 < ytail < ysplit), or the tail alone; plain and local"""
    import torch
    e = exp("mixed")
    worst = {}
    with restored(e):
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.set_symmetric(2)
        e.set_self_order(0)
        for n, group in sorted(_by_size(_cases("mixed", T=T, form="plain")).items()):
            ring = Ring(torch, iv, n)
            for c in group:
                _check_plain(e, ring, c, worst)
        e.set_stream(None)
        _wake_family(e, iv, _cases("mixed", T=T, form="local"), worst)
    print(f"mixed form, T = {T}: worst error / max|u| = plain {worst['mixed']:.2e} (bound {TOL['plain']:.0e}), "
          f"local {worst['mixed local']:.2e} (bound {WAKE_TOL['f32']:.0e})")


@pytest.mark.parametrize("rbulk", [2, 1])
def test_mixed_granularity_with_a_bulk_of_two_wave_and_of_one_wave_items(exp, iv, rbulk):
    """the smallest rings at which the rule gives the mixed form a bulk of 2 waves and of 1 wave per item (103 and 146 tiles of 256:
    the one shape of this table above 12 800 vortices), last tile of 65 members, 0 < ytail < ysplit; plain and local"""
    import torch
    e = exp("mixed")
    tiles = dict((rb, t) for rb, t, _ in S.mixed_big_rings())[rbulk]
    cases = [c for c in _cases("mixed_big") if -(-c.n // 256) == tiles]
    assert len(cases) == 2 and all(S.geometry(c).rbulk == rbulk for c in cases)
    worst = {}
    with restored(e):
        e.set_symmetric(2)
        e.set_self_order(0)
        for c in cases:
            if c.form == "plain":
                e.set_stream(torch.cuda.current_stream().cuda_stream)
                _check_plain(e, Ring(torch, iv, c.n), c, worst)
                e.set_stream(None)
            else:
                _check_wake(e, iv, c, 80, worst, second=True)
    print(f"mixed form, bulk of {rbulk}-wave items ({tiles} tiles): worst error / max|u| = plain {worst['mixed_big']:.2e}, "
          f"local {worst['mixed_big local']:.2e}")


# ---- pair_sym_quad_f32<8> and its diag_only companion ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "local"])
def test_quad_variant_by_value(exp, iv, form):
    """code -4 of the measurement build on rings of 16 .. 25 tiles: last quads of 1, 2, 3 and 4 tiles, a last tile of 1 member and a
    full one, the tapered chunk table (split 0) and 1, 2, 3, 5 uniform chunks, the partly empty rounds at both ends of the D range"""
    import torch
    e = exp("exp")
    worst = {}
    with restored(e):
        e.set_symmetric(2)
        e.set_self_order(0)
        if form == "plain":
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            for n, group in sorted(_by_size(_cases("quad", form="plain")).items()):
                ring = Ring(torch, iv, n)
                for c in group:
                    _check_plain(e, ring, c, worst)
        else:
            _wake_family(e, iv, _cases("quad", form="local"), worst)
    print(f"quad variant, {form}: worst error / max|u| = {max(worst.values()):.2e} (bound 1e-05)")


# ---- the placement on the XCDs ----------------------------------------------------------------------------------------------------
def test_the_xcd_placement_changes_no_bit(exp, iv):
    """LUDVM_XCD_RUN = 1 and 3 (chunks per run of the XCD rotation) against the default placement: the same items, the same partial
    sums, the same bits -- every R, the mixed form, the quad variant"""
    import torch
    base, others = exp("exp"), {b: exp(b) for b in S.XCD_RUN}
    worst = {}
    n_cases = 0
    with restored(base, *others.values()):
        for e in (base, *others.values()):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            e.set_symmetric(2)
            e.set_self_order(0)
        for n, group in sorted(_by_size(_cases("xcd", build="xcd1")).items()):
            ring = Ring(torch, iv, n)
            for c in group:
                ref_bits = _check_plain(base, ring, c._replace(build="exp"), worst)
                for b, e in others.items():
                    _tune(e, c)
                    assert _same_bits(ref_bits, ring.induce(e, (b, c))), (b, c)
                    n_cases += 1
    assert n_cases == len(_cases("xcd"))
    print(f"XCD placement: {n_cases} launches bit for bit the default's; worst error / max|u| = {worst['xcd']:.2e}")


# ---- owners of a sharded ring -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(S.OWNER_TILES))
def test_owner_blocks_add_up_to_the_single_owner_bit_for_bit(eng, exp, iv, kind):
    """sym_scale_dev / sym_accumulate_dev over the blocks shard_block gives for 2, 3, 5 and 7 owners (some own nothing, some one ragged
    quad): the integer sums add up to the single owner's, the NaN counter stays 0, and the single owner's sums are the reference's"""
    import torch
    e = eng if kind == "plain" else exp("exp")
    dev = torch.device("cuda", 0)
    worst = 0.0
    with restored(e):
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        for code in (S.RS if kind == "plain" else (S.QUAD,)):
            for _, n, world, split in [c for c in S.owner_cases() if c[0] == kind]:
                e.set_sym_tuning(8, code)
                e.set_tuning(0, split)
                g, x, z, vc = S.cloud(n)
                ur, wr = S.reference(iv, ("plain", n, 0), g, x, z, vc)
                src = [Guarded(torch, n, a) for a in (x, z, g)]
                scale = torch.zeros([32], dtype=torch.uint8, device=dev)
                e.sym_scale_dev(src[2].ptr(), n, vc, scale.data_ptr())

                def accumulate(first, count):
                    acc = torch.zeros([2 * n + 1], dtype=torch.int64, device=dev)
                    b = acc.data_ptr()
                    e.sym_accumulate_dev(src[0].ptr(), src[1].ptr(), src[2].ptr(), n, first, count, vc, scale.data_ptr(), b, b + 8 * n, b + 16 * n)
                    return acc
                blocks = S.sym_rule.shard_blocks(-(-n // 512), world)
                total = sum(accumulate(f, cnt) for f, cnt in blocks)
                one = accumulate(0, -(-n // 512))
                torch.cuda.synchronize()
                what = (kind, code, n, world, split)
                assert torch.equal(total, one), what
                assert int(one[-1]) == 0, what
                rec = scale.cpu().numpy()
                inv = float(rec[8:16].view(np.float64)[0])
                acc = one.cpu().numpy()
                u, w = acc[:n].astype(np.float64) * inv / (2 * np.pi), -acc[n:2 * n].astype(np.float64) * inv / (2 * np.pi)
                err = S.rel_err(u, w, ur, wr)
                worst = max(worst, err)
                assert err <= TOL["plain"], (what, err)
    print(f"owners, {kind}: worst error / max|u| of the single owner's sums = {worst:.2e} (bound {TOL['plain']:.0e})")


# ---- a non-finite input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "local", "hilo", "quad"])
def test_a_non_finite_last_member_of_a_ragged_tile_poisons_the_result(eng, exp, form):
    """as test_symmetric_kernel_propagates_nan_like_the_reference at large n: the launch returns, every velocity is NaN, and a
    clean launch afterwards is clean"""
    import torch
    e = exp("exp") if form == "quad" else eng
    T, code, n = (8, S.QUAD, S.size(17, 8, 65)) if form == "quad" else (4 if form == "hilo" else 8, 2, S.size(5, 4 if form == "hilo" else 8, 65))
    with restored(e):
        e.set_symmetric(2)
        e.set_self_order(0)
        e.set_sym_tuning(T, code)
        e.set_tuning(0, 2)
        if form in ("plain", "quad"):
            g, x, z, vc = S.cloud(n)
            bad = x.copy()
            bad[n - 1] = np.nan
            dev = torch.device("cuda", 0)
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            dx, dz, dg, dbad = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (x, z, g, bad))
            du, dw = torch.zeros_like(dx), torch.zeros_like(dx)
            e.induce_dev(dbad.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dbad.data_ptr(), dz.data_ptr(), n, vc, du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            assert torch.isnan(du).all() and torch.isnan(dw).all()
            e.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, vc, du.data_ptr(), dw.data_ptr())
            torch.cuda.synchronize()
            assert torch.isfinite(du).all() and torch.isfinite(dw).all()
        else:
            g, x, z, vc = S.sheet(n)
            fx, fz, fg = S.foil(80)
            bad = x.copy()
            bad[n - 1] = np.nan
            for xs, finite in ((bad, False), (x, True)):
                e.wake_clear()
                e.wake_append(xs, z, g)
                u, w = e.wake_advect(S.DT, fx, fz, fg, vc, precision=PRECISION[form], return_velocity=True)
                assert (np.isfinite(u).all() and np.isfinite(w).all()) if finite else (np.isnan(u).all() and np.isnan(w).all()), (form, finite)


# ---- marched runs: counts read on the device, surplus workgroups, sym_grid_bound --------------------------------------------------------
@pytest.fixture(scope="module")
def f64_last_rows():
    made = {}

    def get(name):
        if name not in made:
            sim = _run(name, "f64", 0, 0, 0)
            made[name] = sim.path["TEV"][sim.nt - 1].copy()
        return made[name]
    return get


def _run(name, precision, tile, R, split):
    from ludvm_amd import Engine, LUDVM
    e = Engine(0)
    try:
        e.set_symmetric(8)
        e.set_sym_tuning(tile, R)
        e.set_tuning(0, split)
        return LUDVM(**case_keywords(name), verbose=False, engine=e, precision=precision, history="full", march=True)
    finally:
        try:
            e.set_symmetric(1)
            e.set_sym_tuning(0, 0)
            e.set_tuning(0, 0)
        finally:
            e.close()


@pytest.mark.parametrize("tile", S.TS)
@pytest.mark.parametrize("precision", ["f32", "f32x2"])
@pytest.mark.parametrize("name", CLOUDS)
def test_marched_clouds_with_forced_variants_every_step(name, precision, tile, iv, f64_last_rows):
    """the four free-vortex clouds of tests/rollup_common.py (100 overlapped march steps, the symmetric kernel from 8 vortices) with
    R in {1, 2} x d-chunks {1, 2}: every step to the step-local residuals of tests/test_gpu_rollup_steps.py, unchanged"""
    for R in (1, 2):
        for split in (1, 2):
            sim = _run(name, precision, tile, R, split)
            assert sim.nt == 101
            check_run(f"{name} {precision} tile={tile} R={R} split={split}", name, sim, precision, True, iv, f64_last_rows(name))
