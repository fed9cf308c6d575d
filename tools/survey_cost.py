#!/usr/bin/env python3
"""What a wake survey costs (profiles/survey_cost.txt): a marched run with `survey=None` against the parent build, the added
time per sampled step with K points, and -- from rocprofv3 kernel statistics -- march_survey_partial's pairs/s beside pair_f64's
on the same shape.

    python tools/survey_cost.py ab     --parent-lib LIB [--repeats R]        survey=None: this build and the parent's library
                                                                              loaded in ONE process, runs alternated
    python tools/survey_cost.py time   --survey K [--repeats R] [--every E]   wall time, added time per sampled step, pair count
    python tools/survey_cost.py once   --survey K [--induce] [--every E]      one warm-up + one run (under rocprofv3); --induce:
                                                                              also 5 Engine.induce f64 calls, K points x final wake
    python tools/survey_cost.py stats  kernel_stats.csv [--pairs N] [--induce-pairs N]
                                                                              the survey and pair_f64 kernels' time and pairs/s

The run: 5000 steps of config 1's foil at dt = 1e-3, history='sparse', precision='f32' (DESIGN 4.7's 'long' case).  The
survey: K points of a box behind the trailing edge in the tunnel frame, sampled in every `--every`-th step from step 1."""
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
ap.add_argument("--induce", action="store_true")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=5000)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--pairs", type=float, default=0)
ap.add_argument("--induce-pairs", type=float, default=0)
args = ap.parse_args()

if args.mode == "stats":
    with open(args.files[0]) as f:
        rows = {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}
    for k, (calls, ns) in rows.items():
        pairs = {"march_survey_partial": args.pairs, "pair_f64<": args.induce_pairs}
        hit = [p for name, p in pairs.items() if name in k]
        if "march_survey" in k or (hit and "pair_f64_few" not in k):
            rate = f", {hit[0] / (ns * 1e-9):.3g} pairs/s" if hit and hit[0] else ""
            print(f"  {k.split('(')[0]}: {calls} dispatches, {ns / 1e6:.2f} ms total, {ns / calls / 1e3:.2f} us each{rate}")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

kw = dict(t0=0, tf=args.steps * 1e-3, dt=1e-3, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
          history="sparse", precision="f32")


def box(K):
    rng = np.random.default_rng(1)
    return np.stack([rng.uniform(0.75, 4.75, K), rng.uniform(-2.0, 2.0, K)])


def extras(K):
    return dict(survey=box(K), survey_frame="tunnel", survey_steps=(1, 10 ** 9, args.every)) if K else {}


def run(eng, **extra):
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)        # (ends in the read of the device's rows: synchronised)
    return time.perf_counter() - t0, sim


def sources_per_step(sim):
    """Sources of step i's field: the wake after the step's solve plus the bound vortices."""
    shed = np.cumsum(sim.LEV_shed != -1)
    return sim.n_freevort + np.arange(sim.nt) + shed + sim.Npoints - 1


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

eng = Engine(0)
extra = extras(args.survey)
if args.mode == "once":
    run(eng, **extra)
    t, sim = run(eng, **extra)
    ns = sources_per_step(sim)
    sampled = np.arange(1, sim.nt, args.every)
    pairs = float(args.survey) * float(ns[sampled].sum())
    print(f"K={args.survey} every={args.every}: {t:.4f} s, {sim.nt - 1} steps, {len(sampled)} sampled, final wake {eng.wake_size()}; "
          f"{pairs:.6g} survey pairs per run, {2 * pairs:.6g} for the two runs of this process")
    if args.induce:
        n = eng.wake_size()
        x, z, g = eng.wake_read(0, n, gamma=True)
        px, pz = box(args.survey)
        for _ in range(5):
            eng.induce(g, x, z, px + sim.xpiv[-1], pz, sim.v_core, precision="f64")
        print(f"Engine.induce f64: 5 calls of {args.survey} points x {n} sources = {5.0 * args.survey * n:.6g} pairs")
else:
    run(eng)
    run(eng, **extra)
    t0s, t1s = [], []
    for _ in range(args.repeats):
        t0s.append(run(eng)[0])
        t, sim = run(eng, **extra)
        t1s.append(t)
    ns = sources_per_step(sim)
    sampled = np.arange(1, sim.nt, args.every)
    m0, m1 = sorted(t0s)[len(t0s) // 2], sorted(t1s)[len(t1s) // 2]
    pairs = float(args.survey) * float(ns[sampled].sum())
    print(f"plain:            {spread(t0s)}")
    print(f"K={args.survey} every={args.every}: {spread(t1s)}")
    print(f"added: {m1 - m0:.4f} s = {(m1 - m0) / len(sampled) * 1e6:.2f} us per sampled step ({len(sampled)} of {sim.nt - 1} steps); "
          f"{pairs:.6g} survey pairs, {pairs / max(m1 - m0, 1e-9):.3g} pairs/s of the added time")
