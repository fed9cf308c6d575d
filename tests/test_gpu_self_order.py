"""GPU tier: symmetric launches on device arrays evaluated in Morton order (ludvm_set_self_order; csrc/order.hip self_order_f32,
the scatter fused into finish_sym / finish_sym_advect).  Every output is compared at its own caller index, so a wrong
permutation fails.  Mode 2 forces the path at sizes far below the rule's threshold; the threshold itself is read from the
rule's header through tools/sym_rule.py, the way Python asks the launch rule anything.  The checker is oracle/c_oracle
on sampled targets (the first 300, the last 300, 100 random), relative to max|u| of the sample."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import c_oracle

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sym_rule  # noqa: E402

pytestmark = pytest.mark.gpu

V_CORE = 0.065
TOL = 1e-5          # of max|u|: the bound the fp32 kernels are held to everywhere in this suite


@pytest.fixture(scope="module")
def eng():
    import torch
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    e.close()


def cloud(n, seed=20260101):
    """bench.py's synthetic wake"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 0, n)
    z = rng.uniform(-2, 2, n)
    g = rng.standard_normal(n) / n
    return x.astype(np.float32), z.astype(np.float32), g.astype(np.float32)


def induce(e, mode, x, z, g):
    """Engine.induce_dev of the array on itself in self-order mode `mode` -> (u, w) on the host"""
    import torch
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, z, g))
    du, dw = torch.full_like(dx, 7.0), torch.full_like(dx, 7.0)
    n = len(x)
    e.set_self_order(mode)
    try:
        e.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, V_CORE, du.data_ptr(), dw.data_ptr())
        torch.cuda.synchronize()
    finally:
        e.set_self_order(1)
    return du.cpu().numpy(), dw.cpu().numpy()


def sample(n):
    rnd = np.random.default_rng(n).choice(n, size=min(100, n), replace=False)
    return np.unique(np.r_[np.arange(min(300, n)), np.arange(max(0, n - 300), n), rnd])


def oracle_err(x, z, g, u, w):
    idx = sample(len(x))
    xs, zs, gs = (a.astype(np.float64) for a in (x, z, g))
    uo, wo = c_oracle.induced_velocity(gs, xs, zs, xs[idx], zs[idx], V_CORE)
    scale = max(np.abs(uo).max(), np.abs(wo).max())
    return max(np.abs(u[idx] - uo).max(), np.abs(w[idx] - wo).max()) / scale


def same_bits(a, b):
    return all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))


# 16 384: T = 4, whole tiles; 20 001: ragged; 45 001: T = 8, ragged; 327 681: the first quad size plus one
@pytest.mark.parametrize("n", [16384, 20001, 45001, 327681])
def test_cloud_in_morton_order_against_the_oracle_and_the_given_order(eng, n):
    x, z, g = cloud(n)
    u2, w2 = induce(eng, 2, x, z, g)
    err = oracle_err(x, z, g, u2, w2)
    u0, w0 = induce(eng, 0, x, z, g)
    scale = max(np.abs(u0).max(), np.abs(w0).max())
    diff = max(np.abs(u2 - u0).max(), np.abs(w2 - w0).max()) / scale
    print(f"n={n}: mode 2 vs oracle {err:.3e}, mode 2 vs mode 0 {diff:.3e} of max|u|")
    assert err <= TOL
    assert diff <= TOL


N_DEG = 20001


def test_identical_points_keep_the_given_order_bit_for_bit(eng):
    """no extent in either axis: every key is equal, the stable sort returns the identity"""
    _, _, g = cloud(N_DEG)
    x, z = np.full(N_DEG, -3.25, np.float32), np.full(N_DEG, 0.5, np.float32)
    assert same_bits(induce(eng, 2, x, z, g), induce(eng, 0, x, z, g))


def degenerate(kind):
    x, z, g = cloud(N_DEG)
    if kind == "line":                      # zero extent in z
        z[:] = 0.75
    elif kind == "ties":                    # only n / 4 distinct positions: key ties, kept in the caller's order
        k = np.arange(N_DEG) % (N_DEG // 4)
        x, z = x[k], z[k]
    elif kind == "outlier":                 # one zero-strength vortex at 1e6 (the padding of test_symmetric_tile_ring_partition)
        x[-1] = z[-1] = 1e6
        g[-1] = 0.0
    return x, z, g


@pytest.mark.parametrize("kind", ["line", "ties", "outlier"])
def test_degenerate_sets_against_the_oracle(eng, kind):
    x, z, g = degenerate(kind)
    u, w = induce(eng, 2, x, z, g)
    err = oracle_err(x, z, g, u, w)
    print(f"{kind}: mode 2 vs oracle {err:.3e} of max|u|")
    assert err <= TOL


def test_non_finite_positions_return_and_poison_what_they_poison_unordered(eng):
    x, z, g = cloud(N_DEG)
    x[5] = np.nan
    z[777] = np.inf
    u2, w2 = induce(eng, 2, x, z, g)        # (returns)
    u0, w0 = induce(eng, 0, x, z, g)
    assert np.array_equal(np.isfinite(u2), np.isfinite(u0)) and np.array_equal(np.isfinite(w2), np.isfinite(w0))


def test_the_same_call_gives_the_same_bits(eng):
    from ludvm_amd import Engine
    import torch
    x, z, g = cloud(45001)
    first = induce(eng, 2, x, z, g)
    assert same_bits(first, induce(eng, 2, x, z, g))
    with Engine(0) as other:
        other.set_stream(torch.cuda.current_stream().cuda_stream)
        assert same_bits(first, induce(other, 2, x, z, g))


def test_the_rule_orders_from_its_threshold_and_nothing_below(eng):
    n_min = sym_rule.constants()["kSelfOrderMin"]
    assert n_min > 45001
    x, z, g = cloud(45001)
    assert same_bits(induce(eng, 1, x, z, g), induce(eng, 0, x, z, g))
    x, z, g = cloud(n_min)
    by_rule, forced, given = induce(eng, 1, x, z, g), induce(eng, 2, x, z, g), induce(eng, 0, x, z, g)
    assert same_bits(by_rule, forced)
    assert not same_bits(by_rule, given)        # (the quad variant adds a quad's partial sums in fp32: another order, other bits)


def test_advect_step_in_morton_order(eng):
    """the self path of advect_dev in mode 2 against x + dt u of induce_dev in mode 2 (fma against mul + add: 1e-6, as the tile
    ring test has it)"""
    import torch
    dt = 0.05
    x, z, g = cloud(N_DEG)
    u, w = induce(eng, 2, x, z, g)
    dev = torch.device("cuda", 0)
    dx, dz, dg = (torch.from_numpy(a).to(dev) for a in (x, z, g))
    xo, zo = torch.empty_like(dx), torch.empty_like(dx)
    eng.set_self_order(2)
    try:
        eng.advect_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), N_DEG, 0, N_DEG, V_CORE, dt, xo.data_ptr(), zo.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.set_self_order(1)
    assert np.abs(xo.cpu().numpy() - (x + dt * u)).max() <= 1e-6
    assert np.abs(zo.cpu().numpy() - (z + dt * w)).max() <= 1e-6
