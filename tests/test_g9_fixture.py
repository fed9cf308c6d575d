"""CPU tier of G9 (tests/golden/g9_edge_runs.npz, oracle/g9_cases.py): the inputs regenerate, the oracle and the product's host
loop reproduce the reference's runs at the edge panel, coefficient and wake counts, and every pair of neighbouring panel counts
still straddles the kernel constant it is named after.  A constant that moves fails here: move the case pair with it and
regenerate G9 (python oracle/gen_golden.py g9).  The GPU tier runs the same cases through `sweep` and the solo march
(tests/test_gpu_g9.py)."""
import os
import re
import sys

import numpy as np
import pytest

from g9_common import RUNS, compare_dense, fixture, oracle_run
from oracle import g9_cases as G9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ludvm_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_rule  # noqa: E402
REGEN = "regenerate G9 with the case pair at the new value (oracle/g9_cases.py, python oracle/gen_golden.py g9)"
HOST_NPAN = (2, 64, 256)


@pytest.fixture(scope="module")
def g9():
    return fixture()


def test_g9_inputs_regenerate_and_the_fixture_is_the_table(g9):
    assert sorted(g9) == sorted(G9.key(c, m) for c, m in RUNS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g9_edge_runs.npz")) < 1 << 20
    for c, m in RUNS:
        ref = g9[G9.key(c, m)]
        assert np.array_equal(ref["sha256"], G9.digest(c)), c["name"]
        assert np.array_equal(ref["params"], G9.params(c)), c["name"]
        steps = {"A": 100, "B": 30, "C": 1}[c["group"]]
        assert ref["nt"] == steps + 1 and ref["itev"] == steps - 1 and len(ref["Cl"]) == steps + 1 and len(ref["circ_TEV"]) == steps
        assert ref["TEV"].shape == (2, c["snap"]) and ref["FREE"].shape == (2, max(c["nfree"], 1)), c["name"]
        assert all(np.isfinite(v).all() for v in ref.values() if isinstance(v, np.ndarray)), c["name"]
    # the table is what the issue lists
    assert [c["npan"] for c in G9.GROUP_A] == list(G9.A_NPAN) + [256, 2]
    assert [c["ncoef"] for c in G9.GROUP_A] == [4, 5, 30, 63, 64, 4, 5, 30, 63, 64, 4, 5, 30, 63, 64, 4, 5, 64, 64]
    assert all(c["methods"] == ("Faure", "Ramesh") and c["seed"] == 9000 + c["npan"] and c["nfree"] == 120 for c in G9.GROUP_A)
    assert [c["nfree"] for c in G9.GROUP_B] == list(G9.B_NFREE) + [0]
    # every group-A run sheds LEVs except the two-panel ones; the wake passes 128 and 256 vortices
    for c, m in RUNS:
        if c["group"] == "A":
            ref = g9[G9.key(c, m)]
            nlev = int((ref["LEV_shed"] != -1).sum())
            assert (nlev == 0) == (c["npan"] == 2), (c["name"], m)
            assert c["nfree"] < 128 and (c["nfree"] + 100 + nlev > 256 or c["npan"] == 2), (c["name"], m)


@pytest.mark.parametrize("group", ["A", "B", "C"])
def test_g9_python_oracle_reproduces_the_reference(g9, group):
    """OracleLUDVM on every stored run: every series and wake row to 1e-10 of its maximum (tests/test_oracle_golden.py's
    bound; measured 0: the same float64 operations in the same order), identical LEV_shed."""
    worst = 0.0
    for c, m in RUNS:
        if c["group"] == group:
            worst = max(worst, compare_dense(oracle_run(c, m), g9[G9.key(c, m)], 1e-10, G9.key(c, m)))
    print(f"G9 group {group}: oracle vs reference, worst relative difference {worst:.2e}")


@pytest.mark.parametrize("name,method", [(c["name"], m) for c, m in RUNS if c["group"] == "A" and c["npan"] in HOST_NPAN])
def test_g9_host_loop_reproduces_the_fixture_on_the_fake_engine(g9, name, method):
    """The product's per-step host loop (pair sums by the CPU oracle) at 2, 64 and 256 panels, 4 .. 64 coefficients: the
    oracle's bound, 1e-10 of each series' maximum (measured 2.5e-14 against the oracle at these panel counts)."""
    from fake_engine import FakeEngine
    from ludvm_amd import LUDVM
    c = G9.BY_NAME[name]
    sim = LUDVM(**G9.kwargs(c, method), verbose=False, engine=FakeEngine())
    worst = compare_dense(G9.unpack(G9.pack(sim, c)), g9[G9.key(c, method)], 1e-10, (name, method))
    print(f"G9 {name} {method}: host loop vs reference, worst relative difference {worst:.2e}")


def _constants():
    def one(pattern, path, conv=int):
        m = re.findall(pattern, open(path).read())
        assert len(m) == 1, (pattern, m)
        return conv(m[0])
    plan = plan_rule.constants()        # the direct kernels' plan constants, from the plan itself (tools/plan_rule.py)
    k = {
        "kBlock": one(r"constexpr int kBlock = (\d+);", os.path.join(CSRC, "pair_kernels.hpp")),
        "kFewGroupsMax": plan["kFewGroupsMax"],
        "kTileF64Few": plan["kTileF64Few"],
        "kFewTargets": plan["kFewTargets"],
        "kEnsSlicesMax": one(r"constexpr int kEnsSlicesMax = (\d+);", os.path.join(CSRC, "ensemble_kernels.hpp")),
        "kEnsGroup": one(r"constexpr int kEnsGroup = (\d+);", os.path.join(CSRC, "ensemble_kernels.hpp")),
        "ENSEMBLE_MAX_WAKE": one(r"#define LUDVM_ENSEMBLE_MAX_WAKE (\d+)", os.path.join(ROOT, "include", "ludvm_hip.h")),
    }
    tile = one(r"constexpr int kEnsTile = (\w+);", os.path.join(CSRC, "ensemble_kernels.hpp"), str)
    k["kEnsTile"] = k[tile] if tile in k else int(tile)
    return k


def test_g9_pairs_straddle_the_kernels_constants():
    """Each pair of neighbouring panel counts is (t - 1, t) at an edge of the lane arithmetic as the sources state it now:
    the sweep's chord sums (ensemble_kernels.hpp: ntt = npan + 1 targets, slices = min(kBlock / ntt, kEnsSlicesMax), a second
    pass from ntt > kBlock) and the march's (plan_rule.hpp: nt = npan + 3 targets; pair_f64_few with groups = min(kBlock / nt,
    kFewGroupsMax) while 2 nt <= kBlock; the short-tile plan up to kFewTargets targets); the wake counts sit on both sides of
    the source tiles and a member's slab is filled exactly."""
    from ludvm_amd import _ffi
    k = _constants()
    launch = open(os.path.join(CSRC, "plan_rule.hpp")).read()
    ens = open(os.path.join(CSRC, "ensemble_kernels.hpp")).read()
    # the rules themselves, as the sources state them
    assert re.search(r"\bntt = npan \+ 1\b", ens), REGEN
    assert re.search(r"int slices = kBlock / cnt;\s*if \(slices > kEnsSlicesMax\) slices = kEnsSlicesMax;", ens), REGEN
    assert k["kBlock"] == plan_rule.constants()["kPlanBlock"]
    assert "2 * nt_few <= kPlanBlock" in launch and "plan_min(kPlanBlock / nt_few, kFewGroupsMax)" in launch, REGEN
    assert "nt <= kFewTargets" in launch, REGEN

    def slices(npan):
        return min(k["kBlock"] // min(npan + 1, k["kBlock"]), k["kEnsSlicesMax"])

    def passes(npan):
        return -(-(npan + 1) // k["kBlock"])

    def groups(npan):          # 0: not pair_f64_few
        nt = npan + 3
        return min(k["kBlock"] // nt, k["kFewGroupsMax"]) if 2 * nt <= k["kBlock"] else 0
    # ... and as the plan itself answers for the march's chord launch, with that launch's own arguments (march.hip,
    # march_chord_launch: fp64, results in the slab, the SOURCE count on the device -- planned from the host's bound --, the npan + 3
    # targets on the host): pair_f64_few wherever the lane arithmetic above says so.  A launch whose TARGET count is completed on
    # the device (the march's roll-up) never is.
    with open(os.path.join(CSRC, "march.hip")) as f:
        chord = re.search(r"int march_chord_launch\(.*?\n}\n", f.read(), re.S).group(0)
    assert "a.ns_dev = 1; a.nt_dev = 0;" in chord and "a.nt = (long long)NT;" in chord, REGEN
    assert "launch_pair(c, a, p, LUDVM_PREC_F64, nullptr, nullptr)" in chord, REGEN
    with open(os.path.join(CSRC, "launch.hip")) as f:
        assert re.search(r"direct_variant\([^;]*a\.part != nullptr,\s*a\.nt_dev != 0\);", f.read()), REGEN
    for npan in G9.A_NPAN:
        for ns_bound in (300, 5000, 70000):
            got, dev = plan_rule.plan([dict(precision="f64", ns=ns_bound, nt=npan + 3, slab=True),
                                       dict(precision="f64", ns=ns_bound, nt=npan + 3, slab=True, nt_on_device=True)])
            assert (got.groups, got.family == "f64_few") == (groups(npan), groups(npan) > 0), (npan, ns_bound)
            assert dev.family == "f64" and dev.groups == 0, (npan, ns_bound)
    want = {"sweep slices 4|3": lambda a, b: (slices(a), slices(b)) == (4, 3) and passes(b) == 1,
            "sweep slices 3|2": lambda a, b: (slices(a), slices(b)) == (3, 2) and passes(b) == 1,
            "sweep slices 2|1": lambda a, b: (slices(a), slices(b)) == (2, 1) and passes(b) == 1,
            "sweep second pass": lambda a, b: (passes(a), passes(b)) == (1, 2) and (b + 1) % k["kBlock"] == 1,
            "march groups 4|3": lambda a, b: (groups(a), groups(b)) == (4, 3),
            "march groups 3|2": lambda a, b: (groups(a), groups(b)) == (3, 2),
            "march few|plain": lambda a, b: (groups(a), groups(b)) == (2, 0),
            "march kFewTargets": lambda a, b: a + 3 == k["kFewTargets"] and b + 3 == k["kFewTargets"] + 1}
    assert sorted(w for _, _, w in G9.PAIRS) == sorted(want)
    for lo, hi, what in G9.PAIRS:
        assert hi == lo + 1 and lo in G9.A_NPAN and hi in G9.A_NPAN, what
        assert want[what](lo, hi), f"{what}: {lo} | {hi} no longer straddles it ({k}); {REGEN}"
    assert max(G9.A_NPAN) == k["kBlock"] == 256                   # the most panels a sweep or a march takes (kMarchMaxPan)
    # wake counts: group A starts under the march's short source tile and ends over the sweep's tile (checked on the fixture's
    # own counts above); group B has the counts around 1, 2 and 4 tiles of either kind
    assert G9.A_NFREE < k["kTileF64Few"] and G9.A_NFREE + 100 > k["kTileF64Few"], REGEN
    for t in (k["kTileF64Few"], k["kEnsTile"], 2 * k["kEnsTile"]):
        assert {t - 1, t, t + 1} <= set(G9.B_NFREE), f"{t}; {REGEN}"
    assert {4 * k["kEnsTile"] - 1, 4 * k["kEnsTile"] + 1} <= set(G9.B_NFREE), REGEN
    # the roll-up's source count n + npan takes every residue of its group of kEnsGroup within one group-A run, at any npan:
    # a step adds one or two vortices
    assert k["kEnsGroup"] == 4
    # the capacity edge
    assert k["ENSEMBLE_MAX_WAKE"] == _ffi.ENSEMBLE_MAX_WAKE
    assert G9.C_NFREE + 2 * 1 == k["ENSEMBLE_MAX_WAKE"] and G9.C_OVER + 2 * 1 == k["ENSEMBLE_MAX_WAKE"] + 1, REGEN
