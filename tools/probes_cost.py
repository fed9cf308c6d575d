#!/usr/bin/env python3
"""What velocity probes cost (profiles/probes_cost.txt): wall time of a marched run with P probes, and the parent's only way
to one probe row -- Engine.induce(precision='f64') against the final wake -- beside it.

    python tools/probes_cost.py time   [--case config1|long] [--probes P] [--repeats R] [--root DIR] [--lib LIB]
    python tools/probes_cost.py once   [--case ...] [--probes P] [--root DIR]      one run, no warm-up (under rocprofv3)
    python tools/probes_cost.py induce [--probes P]                                 Engine.induce f64, P points x final wake
    python tools/probes_cost.py stats  A_kernel_stats.csv [B_kernel_stats.csv]      kernel names and counts (equal?), probe kernels

--root DIR imports ludvm_amd from another checkout (A/B against another build; probes need this one); --lib LIB loads another
build of the library into this checkout's package (A/B of two libraries: one process each, processes alternated).
'long' = 5000 steps at dt = 1e-3, history='sparse', precision='f32'; 'config1' = the README case."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["time", "once", "induce", "stats"])
ap.add_argument("files", nargs="*")
ap.add_argument("--case", default="long", choices=["config1", "long"])
ap.add_argument("--probes", type=int, default=0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--lib", default=None)
args = ap.parse_args()

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")
LONG = dict(CONFIG1, tf=5.0, dt=1e-3)


def stats(path):
    with open(path) as f:
        return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}


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
        if "march_probe" in k:
            print(f"  {k.split('(')[0]}: {calls} dispatches, {ns / 1e6:.2f} ms total, {ns / calls / 1e3:.2f} us each")
    sys.exit(0)

sys.path.insert(0, args.root)
from ludvm_amd import LUDVM, Engine  # noqa: E402

kw = dict(CONFIG1) if args.case == "config1" else dict(LONG, history="sparse", precision="f32")
extra = {}
if args.probes:
    # a rake behind the foil in the frame of the pivot, P points over z in [-2, 2]
    extra = dict(probes=np.stack([np.full(args.probes, 2.0), np.linspace(-2.0, 2.0, args.probes)]), probe_frame="tunnel")
eng = Engine(0, lib_path=args.lib)


def run():
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)
    return time.perf_counter() - t0, sim


if args.mode == "once":
    t, sim = run()
    print(f"{args.case} P={args.probes}: {t:.4f} s (no warm-up), {sim.nt - 1} steps")
elif args.mode == "time":
    run()
    ts = [run()[0] for _ in range(args.repeats)]
    sim = run()[1]
    pairs = 0
    if args.probes:
        n_src = eng.wake_size() / 2 + sim.Npoints - 1           # mean number of sources over the run, roughly
        pairs = args.probes * n_src * (sim.nt - 1)
    print(f"{args.case} P={args.probes} root={os.path.basename(os.path.abspath(args.root))} lib={args.lib or 'own'}: "
          f"min {min(ts):.4f} median {sorted(ts)[len(ts) // 2]:.4f} max {max(ts):.4f} s over {len(ts)} runs, {sim.nt - 1} steps, "
          f"final wake {eng.wake_size()}" + (f", ~{pairs:.3g} probe pairs" if pairs else ""))
else:
    _, sim = run()
    n = eng.wake_size()
    x, z, g = eng.wake_read(0, n, gamma=True)
    P = args.probes or 1024
    px, pz = sim.xpiv[-1] + np.full(P, 2.0), np.linspace(-2.0, 2.0, P)
    for _ in range(5):
        eng.induce(g, x, z, px, pz, sim.v_core, precision="f64")
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        eng.induce(g, x, z, px, pz, sim.v_core, precision="f64")
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    print(f"Engine.induce f64, {P} points x {n} wake vortices (host arrays in and out): median {t * 1e6:.1f} us per call, "
          f"{P * n / t:.3g} pairs/s; one call per step over {sim.nt - 1} steps would be {t * (sim.nt - 1):.3f} s "
          "(and needs the wake of every step on the host)")
