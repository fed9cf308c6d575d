#!/usr/bin/env python3
"""What passive tracers cost (profiles/tracers_cost.txt): a marched run with `tracers=None` against the parent build, the
added time per step with M tracers, the same in both precisions of the tracers (tracer_precision 'f64' | 'f32x2', runs
alternated in one process), and -- from rocprofv3 kernel statistics -- the tracer kernels' pairs/s beside pair_f64's and the
probe kernel's on the same run.

    python tools/tracers_cost.py ab     --parent-lib LIB [--repeats R]       tracers=None: this build and the parent's library
                                                                              loaded in ONE process, runs alternated
    python tools/tracers_cost.py time   [--tracers M] [--probes P] [--repeats R]   wall time, added time per step, pair count
    python tools/tracers_cost.py precision --tracers M [--steps N] [--release R] [--repeats R]
                                                                              plain / 'f64' / 'f32x2' runs alternated: added time
                                                                              per free step of each precision, and their ratio
    python tools/tracers_cost.py once   [--tracers M] [--probes P] [--induce M] [--lib LIB] [--precision f64|f32x2|both]
                                                                              one warm-up + one run (under rocprofv3); --induce:
                                                                              also 5 Engine.induce f64 calls, M points x final wake
    python tools/tracers_cost.py stats  A_kernel_stats.csv [B_kernel_stats.csv] [--pairs N] [--induce-pairs N] [--probe-pairs N]
                                                                              kernel names and counts (equal?); the tracer, probe
                                                                              and pair_f64 kernels' time and pairs/s
    python tools/tracers_cost.py trace  kernel_trace.csv --free N --pairs P   the N longest dispatches of each tracer kernel (the
                                                                              free steps: a dispatch whose tiles are all held
                                                                              returns at once): mean time, pairs/s at P pairs

The run: 5000 steps of config 1's foil at dt = 1e-3, history='sparse', precision='f32' (DESIGN 4.7's 'long' case).  Tracers: a
box of M seeds around the foil's path in the tunnel frame, a quarter released at step 1, 1250, 2500 and 3750 each -- or, with
--release R, all of them at step R (--steps 17000 --release 16000: every free step sees at least 16 000 sources, the run of
tools/survey_cost.py)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["ab", "time", "precision", "once", "stats", "trace"])
ap.add_argument("files", nargs="*")
ap.add_argument("--tracers", type=int, default=0)
ap.add_argument("--probes", type=int, default=0)
ap.add_argument("--induce", type=int, default=0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=5000)
ap.add_argument("--release", type=int, default=0, help="release every tracer at this step (default: a quarter at four steps)")
ap.add_argument("--precision", default="f64", choices=["f64", "f32x2", "both"], help="tracer_precision of `time` and `once`")
ap.add_argument("--lib", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--pairs", type=float, default=0)
ap.add_argument("--free", type=int, default=0, help="trace: the number of dispatches with free tracers")
ap.add_argument("--induce-pairs", type=float, default=0)
ap.add_argument("--probe-pairs", type=float, default=0)
args = ap.parse_args()


def stats(path):
    with open(path) as f:
        return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}


if args.mode == "trace":
    took = {}
    with open(args.files[0]) as f:
        for r in csv.DictReader(f):
            if "tracer_partial" in r["Kernel_Name"]:
                took.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for k, ns in took.items():
        ns.sort()
        rest, free = ns[:len(ns) - args.free], ns[len(ns) - args.free:]
        line = f"  {k}: {len(ns)} dispatches; the {len(free)} longest: {np.mean(free) / 1e3:.2f} us each (min {free[0] / 1e3:.2f})"
        if args.pairs:
            line += f", {args.pairs / (sum(free) * 1e-9):.3g} pairs/s"
        if rest:
            line += f"; the other {len(rest)}: {np.mean(rest) / 1e3:.2f} us each (max {rest[-1] / 1e3:.2f})"
        print(line)
    sys.exit(0)

if args.mode == "stats":
    a = stats(args.files[0])
    if len(args.files) > 1:
        b = stats(args.files[1])
        same = {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
        print(f"kernel names and counts identical: {same}  ({len(a)} kernels, {sum(v[0] for v in a.values())} / "
              f"{sum(v[0] for v in b.values())} dispatches)")
        if not same:
            for k in sorted(set(a) | set(b)):
                if a.get(k, (0,))[0] != b.get(k, (0,))[0]:
                    print("  differs:", k[:90], a.get(k, (0,))[0], b.get(k, (0,))[0])
    for k, (calls, ns) in a.items():
        pairs = {"march_tracer_partial": args.pairs, "march_f32x2_tracer_partial": args.pairs, "march_probe_partial": args.probe_pairs,
                 "pair_f64<": args.induce_pairs}
        hit = [p for name, p in pairs.items() if name in k]
        if "march_tracer" in k or "march_f32x2_tracer" in k or "march_probe" in k or (hit and "pair_f64_few" not in k):
            rate = f", {hit[0] / (ns * 1e-9):.3g} pairs/s" if hit and hit[0] else ""
            print(f"  {k.split('(')[0]}: {calls} dispatches, {ns / 1e6:.2f} ms total, {ns / calls / 1e3:.2f} us each{rate}")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

kw = dict(t0=0, tf=args.steps * 1e-3, dt=1e-3, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
          history="sparse", precision="f32")


def extras(M, P, precision="f64"):
    e = {}
    if M:
        rng = np.random.default_rng(1)
        quarters = np.array([1, args.steps // 4, args.steps // 2, 3 * args.steps // 4], dtype=np.int64)[np.arange(M) % 4]
        e.update(tracers=np.stack([rng.uniform(-1.0, 3.0, M), rng.uniform(-2.0, 2.0, M)]), tracer_frame="tunnel",
                 tracer_release=np.full(M, args.release, dtype=np.int64) if args.release else quarters)
        if precision != "f64":          # (the keyword only where it is needed: --lib may name a build without it)
            e.update(tracer_precision=precision)
    if P:
        e.update(probes=np.stack([np.full(P, 2.0), np.linspace(-2.0, 2.0, P)]), probe_frame="tunnel")
    return e


def run(eng, **extra):
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)
    return time.perf_counter() - t0, sim


def sources_per_step(sim):
    """Sources of step i's roll-up field: the wake after the step's solve plus the bound vortices."""
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
    print(f"tracers=None, {args.steps} steps, builds alternated in one process:")
    print(f"  parent build: {spread(tb)}")
    print(f"  this build:   {spread(ta)}")
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    print(f"  ratio of medians this / parent: {ma / mb:.4f}; this build's median inside the parent's window "
          f"[{min(tb):.4f}, {max(tb):.4f}]: {min(tb) <= ma <= max(tb)}")
    sys.exit(0)

def tracer_pairs(sim):
    free = (sim.tracer_release[None, :] <= np.arange(1, sim.nt)[:, None]).sum(axis=1)
    return float((free * sources_per_step(sim)[1:]).sum()), int((free > 0).sum())


eng = Engine(0, lib_path=args.lib) if args.lib else Engine(0)
if args.mode == "precision":
    run(eng)
    for prec in ("f64", "f32x2"):
        run(eng, **extras(args.tracers, 0, prec))
    ts = {"plain": [], "f64": [], "f32x2": []}
    for _ in range(args.repeats):
        ts["plain"].append(run(eng)[0])
        for prec in ("f64", "f32x2"):
            t, sim = run(eng, **extras(args.tracers, 0, prec))
            ts[prec].append(t)
    pairs, free_steps = tracer_pairs(sim)
    ns = sources_per_step(sim)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    print(f"{sim.nt - 1} steps, M={args.tracers}, {free_steps} steps with free tracers, sources {ns[sim.nt - free_steps]} .. {ns[-1]}, "
          f"{pairs:.6g} tracer pairs")
    print(f"plain:          {spread(ts['plain'])}")
    for prec in ("f64", "f32x2"):
        add = med[prec] - med["plain"]
        print(f"tracers {prec}:  {spread(ts[prec])}; added {add:.4f} s = {add / free_steps * 1e6:.2f} us per free step, "
              f"{pairs / max(add, 1e-9):.3g} pairs/s of the added time")
    print(f"added time per free step, f32x2 / f64: {(med['f32x2'] - med['plain']) / max(med['f64'] - med['plain'], 1e-9):.3f}")
    sys.exit(0)

if args.mode == "once" and args.precision == "both":
    run(eng)
    for prec in ("f64", "f32x2"):
        t, sim = run(eng, **extras(args.tracers, args.probes, prec))
        pairs, free_steps = tracer_pairs(sim)
        print(f"M={args.tracers} {prec}: {t:.4f} s, {sim.nt - 1} steps, {free_steps} with free tracers, final wake {eng.wake_size()}; "
              f"{pairs:.6g} tracer pairs in this run")
    sys.exit(0)

extra = extras(args.tracers, args.probes, args.precision)
if args.mode == "once":
    run(eng, **extra)
    t, sim = run(eng, **extra)
    print(f"M={args.tracers} P={args.probes}: {t:.4f} s, {sim.nt - 1} steps, final wake {eng.wake_size()} (two runs in this process)")
    if args.induce:
        n = eng.wake_size()
        x, z, g = eng.wake_read(0, n, gamma=True)
        rng = np.random.default_rng(2)
        px, pz = sim.xpiv[-1] + rng.uniform(-1.0, 3.0, args.induce), rng.uniform(-2.0, 2.0, args.induce)
        for _ in range(5):
            eng.induce(g, x, z, px, pz, sim.v_core, precision="f64")
        print(f"Engine.induce f64: 5 calls of {args.induce} points x {n} sources = {5 * args.induce * n:.6g} pairs")
else:
    run(eng)
    run(eng, **extra)
    t0s, t1s = [], []
    for _ in range(args.repeats):
        t0s.append(run(eng)[0])
        t1s.append(run(eng, **extra)[0])
    sim = run(eng, **extra)[1]
    ns = sources_per_step(sim)
    steps = np.arange(sim.nt)
    m0, m1 = sorted(t0s)[len(t0s) // 2], sorted(t1s)[len(t1s) // 2]
    print(f"plain:            {spread(t0s)}")
    print(f"M={args.tracers} P={args.probes}: {spread(t1s)}")
    line = f"added: {m1 - m0:.4f} s = {(m1 - m0) / (sim.nt - 1) * 1e6:.2f} us per step"
    if args.tracers:
        free = (sim.tracer_release[None, :] <= steps[1:, None]).sum(axis=1)
        pairs = float((free * ns[1:]).sum())
        line += f"; {pairs:.6g} tracer pairs ({2 * pairs:.6g} for two runs), {pairs / max(m1 - m0, 1e-9):.3g} pairs/s of the added time"
    if args.probes:
        pp = float(args.probes * ns[1:].sum())
        line += f"; {pp:.6g} probe pairs ({2 * pp:.6g} for two runs)"
    print(line)
