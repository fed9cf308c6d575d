#!/usr/bin/env python3
"""Throughput of `sweep` (many small simulations in one device launch) on one MI355X, against running the members in turn:
    python tools/ensemble_throughput.py [--sizes 1 16 64 256 1024 4096] [--mixed 1024] > profiles/ensemble_throughput.txt
For B copies of config 1 (the README case: 400 steps) and for a mixed sweep (the 12-member grid of tests/test_gpu_ensemble.py
repeated): wall time of `sweep` split into host packing / device call (host clock around the synchronous ludvm_ensemble_run:
uploads, ONE kernel, downloads) / host unpacking; member-steps and pairs per second of the device call; and B x the solo
`time_loop` time (march, float64, sparse history; geometry and kinematics excluded) measured in the same command, the two
alternated.  Every shape is warmed up first; a small B is repeated inside a timed window until the window is about a second;
min and median over the repetitions.  The profiler is off (kernel time: tools/profile_cmd.sh on this script with --sizes 256)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[1, 16, 64, 256, 1024, 4096])
ap.add_argument("--mixed", type=int, default=1024, help="members of the mixed sweep (0: skip)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window should last")
a = ap.parse_args()

from ludvm_amd import LUDVM, Engine, sweep  # noqa: E402

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")
GRID = [dict(LESPcrit=l, alpha_max=am) for l in (0.1, 0.2, 0.3, 10) for am in (10, 20)] \
    + [dict(dt=2.5e-2), dict(k=0.4 * np.pi), dict(Naca="2412"), dict(method="Ramesh")]

eng = Engine(0)
info = eng.device_info()
print(f"# device: {info['name']}, {info['cu_count']} CUs, nominal clock {info['clock_khz'] / 1e3:.0f} MHz (the device's own figure; "
      "the clock held during the run was not read)")
print("# times in ms; min / median over the repetitions; 'in turn' = B x one solo time_loop measured beside it")

marks = {}
inner = eng.ensemble_run


def timed(*args, **kw):
    marks["enter"] = time.perf_counter()
    out = inner(*args, **kw)
    marks["exit"] = time.perf_counter()
    return out


eng.ensemble_run = timed


def pairs_of(sim):
    """Pairs a member evaluates: per step (npan + 1) targets x the wake before the solve, then the wake after it x (itself +
    the npan bound vortices)."""
    npan, nf = sim.Npoints - 1, sim.n_freevort
    shed = (sim.LEV_shed[1:] != -1).astype(np.int64)
    before = nf + np.arange(sim.nt - 1) + np.concatenate([[0], np.cumsum(shed)[:-1]])
    after = before + 1 + shed
    return int(((npan + 1) * before + after * (after + npan)).sum())


def one_sweep(cases):
    t0 = time.perf_counter()
    sims = sweep(cases, engine=eng)
    t1 = time.perf_counter()
    return sims, (marks["enter"] - t0, marks["exit"] - marks["enter"], t1 - marks["exit"])


def solo_time_loop(kw):
    s = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", run=False)
    t0 = time.perf_counter()
    s.time_loop()
    return time.perf_counter() - t0


def measure(label, cases, solo_cases):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sims, first = one_sweep(cases)                    # warm-up of this shape (buffers grow here)
        for kw in solo_cases:
            solo_time_loop(kw)
        inner_reps = max(1, int(a.window / max(sum(first), 1e-4)))
        steps = sum(s.nt - 1 for s in sims)
        pairs = sum(pairs_of(s) for s in sims)
        T, solo = [], []
        for _ in range(a.reps):                           # sweep and solo runs alternated
            acc = np.zeros(3)
            for _ in range(inner_reps):
                acc += one_sweep(cases)[1]
            T.append(acc / inner_reps)
            solo.append(sum(solo_time_loop(kw) for kw in solo_cases) * (len(cases) / len(solo_cases)))
    T, solo = np.array(T) * 1e3, np.array(solo) * 1e3
    wall = T.sum(axis=1)
    dev = T[:, 1]
    print(f"{label:<22} members {len(cases):5d}  steps {steps:8d}  pairs {pairs:.3e}  windows of {inner_reps} sweep(s)\n"
          f"    pack   {T[:, 0].min():10.2f} / {np.median(T[:, 0]):10.2f}\n"
          f"    device {dev.min():10.2f} / {np.median(dev):10.2f}   {steps / dev.min() * 1e3:.3e} member-steps/s  "
          f"{pairs / dev.min() * 1e3:.3e} pairs/s\n"
          f"    unpack {T[:, 2].min():10.2f} / {np.median(T[:, 2]):10.2f}\n"
          f"    sweep  {wall.min():10.2f} / {np.median(wall):10.2f}\n"
          f"    in turn {solo.min():9.2f} / {np.median(solo):10.2f}   device call {solo.min() / dev.min():.1f}x faster, "
          f"whole sweep {solo.min() / wall.min():.1f}x", flush=True)


for B in a.sizes:
    measure(f"config 1 x {B}", [dict(CONFIG1)] * B, [dict(CONFIG1)])
if a.mixed:
    cases = [dict(CONFIG1, **GRID[q % len(GRID)]) for q in range(a.mixed)]
    measure(f"mixed grid x {a.mixed}", cases, [dict(CONFIG1, **g) for g in GRID])
