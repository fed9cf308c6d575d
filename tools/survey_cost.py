#!/usr/bin/env python3
"""What a wake survey costs (profiles/survey_cost.txt): a marched run with `survey=None` against the parent build, the added
time per sampled step with K points in both precisions of the survey (survey_precision 'f64' | 'f32', runs alternated in one
process), and -- from rocprofv3 kernel statistics -- the pairs/s of march_survey_partial and march_f32_survey_partial beside
pair_f64's and pair_f32's on the same points and wake.

    python tools/survey_cost.py ab     --parent-lib LIB [--repeats R]        survey=None: this build and the parent's library
                                                                              loaded in ONE process, runs alternated
    python tools/survey_cost.py time   --survey K [--repeats R] [--every E] [--first F] [--lib LIB]
                                                                              wall time, added time per sampled step and pair
                                                                              count: a float64 and an fp32 column, and their ratio
                                                                              (--lib: another build of the library, also with
                                                                              --bins; A/B of two libraries: one process each)
    python tools/survey_cost.py time   --survey K --bins B [--repeats R] [--every E] [--first F] [--precision f64|f32]
                                                                              the same run with the survey alone and with B phase
                                                                              bins (survey_bins=B), alternated: the added time
                                                                              per sampled step of each, side by side
    python tools/survey_cost.py once   --survey K [--induce] [--every E] [--first F]
                                                                              one run per precision (under rocprofv3); --induce:
                                                                              also 5 Engine.induce calls in f64 and 5 in f32, K
                                                                              points x final wake
    python tools/survey_cost.py stats  kernel_stats.csv [--pairs N] [--induce-pairs N]
                                                                              the survey and pair kernels' time and pairs/s
                                                                              (--pairs: of ONE run; each precision runs once)

The run: 5000 steps of config 1's foil at dt = 1e-3, history='sparse', precision='f32' (DESIGN 4.7's 'long' case).  The
survey: K points of a box behind the trailing edge in the tunnel frame, sampled in every `--every`-th step from step `--first`
(--steps 17000 --first 16000: every sample sees at least 16 000 sources).  --lespcrit 10 sheds no leading-edge vortex: the wake is
one trailing-edge sheet, whose origin classes are compact (the fp32 kernel evaluates none of them in float64)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["ab", "time", "once", "stats"])
ap.add_argument("files", nargs="*")
ap.add_argument("--survey", type=int, default=0)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--bins", type=int, default=0, help="time: B phase bins against the survey alone")
ap.add_argument("--precision", default="f64", choices=["f64", "f32"], help="the survey's precision of the --bins comparison")
ap.add_argument("--first", type=int, default=1)
ap.add_argument("--lespcrit", type=float, default=0.2, help="10: no leading-edge vortex is shed, the wake is one sheet")
ap.add_argument("--induce", action="store_true")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=5000)
ap.add_argument("--lib", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--pairs", type=float, default=0)
ap.add_argument("--induce-pairs", type=float, default=0)
args = ap.parse_args()

if args.mode == "stats":
    with open(args.files[0]) as f:
        rows = {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}
    for k, (calls, ns) in rows.items():
        pairs = {"march_survey_partial": args.pairs, "march_f32_survey_partial": args.pairs, "pair_f64<": args.induce_pairs,
                 "pair_f32<": args.induce_pairs}
        hit = [p for name, p in pairs.items() if name in k]
        if "march_survey" in k or (hit and "pair_f64_few" not in k):
            rate = f", {hit[0] / (ns * 1e-9):.3g} pairs/s" if hit and hit[0] else ""
            print(f"  {k.split('(')[0]}: {calls} dispatches, {ns / 1e6:.2f} ms total, {ns / calls / 1e3:.2f} us each{rate}")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

kw = dict(t0=0, tf=args.steps * 1e-3, dt=1e-3, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=args.lespcrit, Naca="0012",
          history="sparse", precision="f32")


def box(K):
    rng = np.random.default_rng(1)
    return np.stack([rng.uniform(0.75, 4.75, K), rng.uniform(-2.0, 2.0, K)])


def extras(K, precision="f64"):
    return dict(survey=box(K), survey_frame="tunnel", survey_steps=(args.first, 10 ** 9, args.every),
                survey_precision=precision) if K else {}


def run(eng, **extra):
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)        # (ends in the read of the device's rows: synchronised)
    return time.perf_counter() - t0, sim


def sources_per_step(sim):
    """Sources of step i's field: the wake after the step's solve plus the bound vortices."""
    shed = np.cumsum(sim.LEV_shed != -1)
    return sim.n_freevort + np.arange(sim.nt) + shed + sim.Npoints - 1


def guarded_classes(eng, v_core, limit=300.0):
    """(classes of the resident wake wider than limit x v_core, classes, median width / v_core): the fp32 kernel's origin classes
    -- tiles of 256 slots, even and odd slots, width = largest |offset| from the middle member -- as NumPy restates them."""
    n = eng.wake_size()
    x, z = eng.wake_read(0, n)[:2]
    ext = []
    for base in range(0, n, 256):
        for par in (0, 1):
            idx = np.arange(base + par, min(base + 256, n), 2)
            if len(idx):
                mid = idx[len(idx) // 2]
                ext.append(max(np.abs(x[idx] - x[mid]).max(), np.abs(z[idx] - z[mid]).max()) / v_core)
    ext = np.array(ext)
    return int((ext > limit).sum()), len(ext), float(np.median(ext))


def spread(ts):
    return f"min {min(ts):.4f} median {sorted(ts)[len(ts) // 2]:.4f} max {max(ts):.4f} s over {len(ts)} runs"


if args.mode == "ab":
    here, parent = Engine(0), Engine(0, lib_path=args.parent_lib)
    run(here)
    run(parent)
    ta, tb = [], []
    for _ in range(args.repeats):
        tb.append(run(parent)[0])
        ta.append(run(here)[0])
    print(f"survey=None, {args.steps} steps, builds alternated in one process:")
    print(f"  parent build: {spread(tb)}")
    print(f"  this build:   {spread(ta)}")
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    print(f"  ratio of medians this / parent: {ma / mb:.4f}; this build's median inside the parent's window "
          f"[{min(tb):.4f}, {max(tb):.4f}]: {min(tb) <= ma <= max(tb)}")
    sys.exit(0)

eng = Engine(0, lib_path=args.lib)
if args.lib:
    print(f"library: {args.lib}")
if args.mode == "once":
    run(eng)
    for prec in ("f64", "f32"):
        t, sim = run(eng, **extras(args.survey, prec))
        ns = sources_per_step(sim)
        sampled = np.arange(args.first, sim.nt, args.every)
        pairs = float(args.survey) * float(ns[sampled].sum())
        print(f"K={args.survey} every={args.every} first={args.first} {prec}: {t:.4f} s, {sim.nt - 1} steps, {len(sampled)} sampled, "
              f"sources {ns[sampled].min()} .. {ns[sampled].max()}, final wake {eng.wake_size()}; {pairs:.6g} survey pairs in this run")
    if args.induce:
        n = eng.wake_size()
        x, z, g = eng.wake_read(0, n, gamma=True)
        px, pz = box(args.survey)
        for prec in ("f64", "f32"):
            for _ in range(5):
                eng.induce(g, x, z, px + sim.xpiv[-1], pz, sim.v_core, precision=prec)
        print(f"Engine.induce: 5 calls in f64 and 5 in f32 of {args.survey} points x {n} sources = {5.0 * args.survey * n:.6g} pairs each")
elif args.bins:
    base = extras(args.survey, args.precision)
    binned = dict(base, survey_bins=args.bins)
    for extra in ({}, base, binned):
        run(eng, **extra)
    ts = {"plain": [], "survey": [], "binned": []}
    for _ in range(args.repeats):
        ts["plain"].append(run(eng)[0])
        ts["survey"].append(run(eng, **base)[0])
        t, sim = run(eng, **binned)
        ts["binned"].append(t)
    nb = int(sim.survey_bin_count.sum())
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    print(f"{sim.nt - 1} steps, K={args.survey}, survey_precision={args.precision}, {sim.survey_count} sampled steps (first {args.first}, "
          f"every {args.every}), {args.bins} bins holding {nb} of them ({sim.survey_bin_count.min()} .. {sim.survey_bin_count.max()} per bin)")
    print(f"plain:            {spread(ts['plain'])}")
    for name, label in (("survey", "survey alone:    "), ("binned", f"survey, {args.bins:2d} bins: ")):
        add = med[name] - med["plain"]
        print(f"{label} {spread(ts[name])}; added {add:.4f} s = {add / sim.survey_count * 1e6:.2f} us per sampled step")
    print(f"the bins add {(med['binned'] - med['survey']) / max(nb, 1) * 1e6:.2f} us per binned step (one finisher per sampled step "
          "either way; the binned one also updates the bin's five sums)")
else:
    run(eng)
    for prec in ("f64", "f32"):
        run(eng, **extras(args.survey, prec))
    ts = {"plain": [], "f64": [], "f32": []}
    for _ in range(args.repeats):
        ts["plain"].append(run(eng)[0])
        for prec in ("f64", "f32"):
            t, sim = run(eng, **extras(args.survey, prec))
            ts[prec].append(t)
    ns = sources_per_step(sim)
    sampled = np.arange(args.first, sim.nt, args.every)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    pairs = float(args.survey) * float(ns[sampled].sum())
    print(f"{sim.nt - 1} steps, K={args.survey}, {len(sampled)} sampled steps (first {args.first}, every {args.every}), sources "
          f"{ns[sampled].min()} .. {ns[sampled].max()}, {pairs:.6g} survey pairs")
    print(f"plain:       {spread(ts['plain'])}")
    for prec in ("f64", "f32"):
        add = med[prec] - med["plain"]
        print(f"survey {prec}:  {spread(ts[prec])}; added {add:.4f} s = {add / len(sampled) * 1e6:.2f} us per sampled step, "
              f"{pairs / max(add, 1e-9):.3g} pairs/s of the added time")
    wide, classes, median = guarded_classes(eng, sim.v_core)
    print(f"origin classes of the final wake wider than 300 v_core (evaluated in float64 by the fp32 kernel): {wide} of {classes}; "
          f"median width {median:.0f} v_core")
    print(f"added time per sampled step, f32 / f64: {(med['f32'] - med['plain']) / max(med['f64'] - med['plain'], 1e-9):.3f}")
