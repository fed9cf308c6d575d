"""GPU tier of G8: every fp32 pair-kernel route at the library's routing thresholds against the reference's own numbers.

Each case of oracle/g8_cases.py runs through a production entry point with the default rule (no forcing switch), on its
full inputs, and its sampled targets are compared with tests/golden/g8_fp32_routes.npz (the reference's induced_velocity,
LUDVM.py:549-570, on those targets).  The tolerances are the contract's (include/ludvm_hip.h), relative to
max(|u_ref|, |w_ref|) over the sampled targets: float64 1e-11, fp32 on local origins and the plain-fp32 device entry 1e-5,
hi+lo positions 2e-6.  tests/test_g8_fixture.py (CPU) ties each pair of cases to the threshold it straddles."""
import numpy as np
import pytest

from conftest import grouped, load_golden
from oracle import g8_cases as G8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from ludvm_amd import Engine
    e = Engine(0)
    assert "gfx950" in e.device_info()["name"]
    yield e
    e.close()


@pytest.fixture(scope="module")
def g8():
    return grouped(load_golden("g8_fp32_routes.npz"))


def _run(eng, c, entry, inp):
    """(u, w) float64 over all targets of the case, through `entry`."""
    vc = c["v_core"]
    g, xs, zs = inp["g"], inp["xs"], inp["zs"]
    if entry in ("induce_f32", "induce_f32x2"):
        prec = entry.split("_")[1]
        if "xt" in inp:
            return eng.induce(g, xs, zs, inp["xt"], inp["zt"], vc, precision=prec)
        return eng.induce(g, xs, zs, xs, zs, vc, precision=prec)          # the same objects: self-interaction
    if entry == "induce_dev":
        import torch
        dev = torch.device("cuda", 0)
        n = len(xs)
        dx, dz, dg = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (xs, zs, g))
        du, dw = torch.full_like(dx, float("nan")), torch.full_like(dx, float("nan"))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.induce_dev(dx.data_ptr(), dz.data_ptr(), dg.data_ptr(), n, dx.data_ptr(), dz.data_ptr(), n, vc, du.data_ptr(),
                           dw.data_ptr())
            torch.cuda.synchronize()
        finally:
            eng.set_stream(None)
        return du.cpu().numpy().astype(np.float64), dw.cpu().numpy().astype(np.float64)
    if entry in ("wake_f32", "wake_f32x2"):
        eng.wake_clear()
        try:
            eng.wake_append(xs, zs, g)
            return eng.wake_advect(1e-3, inp["foil_x"], inp["foil_z"], inp["foil_g"], vc, precision=entry.split("_")[1],
                                   return_velocity=True)
        finally:
            eng.wake_clear()
    if entry == "flowfield":
        u, w = eng.flowfield(c["xmin"], c["zmin"], c["dr"], c["nx"], c["nz"], g, xs, zs, vc)
        return u.reshape(-1).astype(np.float64), w.reshape(-1).astype(np.float64)
    raise ValueError(entry)


CASES = [pytest.param(c["name"], e, id=f"{c['name']}-{e}") for c in G8.CASES for e in c["entries"]]


@pytest.mark.parametrize("name,entry", CASES)
def test_g8_route_against_the_reference(eng, g8, name, entry):
    c = G8.BY_NAME[name]
    ref = g8[name]
    assert np.array_equal(ref["params"], G8.params(c)), "the case table changed: regenerate G8 (oracle/gen_golden.py g8)"
    inp = G8.inputs(c)
    assert np.array_equal(G8.digest(inp), ref["sha256"]), "the inputs do not regenerate as the fixture's"
    idx = ref["idx"]
    assert np.array_equal(idx, G8.sample(c))
    ur, wr = ref["u"], ref["w"]
    if entry.startswith("wake_"):          # LUDVM.py:1105-1106: the wake's and the bound vortices' calls, summed
        ur, wr = ur + ref["u_foil"], wr + ref["w_foil"]
    if c["extent_side"] is not None:       # the route's precondition, as the device sees it
        order, reordered, extent = eng.spatial_order(inp["xs"], inp["zs"], with_extent=True)
        assert reordered == c["reordered"], (name, reordered)
        bound = 150.0 if reordered else 300.0
        ratio = extent / c["v_core"]
        assert (ratio > bound) if c["extent_side"] == "above" else (ratio < bound), (name, ratio, bound)
    eng.set_symmetric(1)
    eng.set_tuning(0, 0)
    eng.set_sym_tuning(0, 0)
    try:
        u, w = _run(eng, c, entry, inp)
    finally:
        eng.set_symmetric(1)
        eng.set_tuning(0, 0)
        eng.set_sym_tuning(0, 0)
    assert u.shape == (c["nt"],) and w.shape == (c["nt"],)
    us, ws = u[idx], w[idx]
    assert np.isfinite(us).all() and np.isfinite(ws).all(), name
    scale = max(np.abs(ur).max(), np.abs(wr).max())
    err = max(np.abs(us - ur).max(), np.abs(ws - wr).max()) / scale
    tol = G8.tolerance(c, entry)
    print(f"G8 {name} {entry} route={c['entries'][entry]} err={err:.3e} tol={tol:.0e}")
    assert err <= tol, (name, entry, err, tol)
