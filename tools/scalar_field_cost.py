#!/usr/bin/env python3
"""Kernel time of one stream-function grid and one analytic-vorticity grid (Engine.flowfield_scalar) next to the float64
velocity grid (Engine.flowfield_rows, precision 'f64', vorticity off) at the same shape, on one MI355X in one process:
    python tools/scalar_field_cost.py [--n 1024] [--sources 20000] [--rounds 7] [--out FILE]
Times are the library's own (ludvm_kernel_timing: HIP events around the main pair kernel, not the split finisher or the
copies).  Every shape is warmed up once; the timed launches alternate velocity, psi, omega, velocity ... so that a drift of the
box shows in all three columns.  Report only: the velocity grid is the yardstick because a psi pair is a velocity pair plus one
logarithm (profiles/scalar_field.txt)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="grid points per side")
ap.add_argument("--sources", type=int, default=20000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

rng = np.random.default_rng(5)
ns = args.sources
g, xs, zs = rng.normal(0, 0.02, ns), rng.uniform(-60, 0, ns), rng.normal(0, 0.5, ns)      # a wake-like strip
dr, vc = 0.02, 0.0195
grid = (-dr * args.n, -dr * args.n / 2, dr)
eng = Engine(0)
info = eng.device_info()
eng.kernel_timing(True)


def run(what):
    eng.kernel_time_ms(reset=True)
    if what == "velocity":
        eng.flowfield_rows(*grid, args.n, args.n, 0, args.n, g, xs, zs, vc, vorticity=False, precision="f64")
    else:
        eng.flowfield_scalar(what, *grid, args.n, args.n, g, xs, zs, vc)
    ms, launches = eng.kernel_time_ms(reset=True)
    assert launches == 1, launches
    return ms


kinds = ("velocity", "psi", "omega")
for k in kinds:
    run(k)
times = {k: [] for k in kinds}
for _ in range(args.rounds):
    for k in kinds:
        times[k].append(run(k))
pairs = args.n * args.n * ns
med = {k: statistics.median(times[k]) for k in kinds}
lines = [f"# python tools/scalar_field_cost.py --n {args.n} --sources {ns} --rounds {args.rounds}",
         f"# {info['name']}, {info['cu_count']} CUs; {args.n} x {args.n} grid points x {ns} sources = {pairs:.3e} pairs per launch,",
         f"# v_core {vc}, float64; main pair kernel only (HIP events), one warm-up per shape, {args.rounds} alternating rounds",
         "kernel       median ms     min ms     max ms    pairs/s"]
for k in kinds:
    t = times[k]
    lines.append(f"{k:9s}   {med[k]:10.3f} {min(t):10.3f} {max(t):10.3f}   {pairs / (med[k] * 1e-3):.3e}")
lines.append(f"psi / velocity   = {med['psi'] / med['velocity']:.2f}")
lines.append(f"omega / velocity = {med['omega'] / med['velocity']:.2f}")
report = "\n".join(lines) + "\n"
print(report, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(report)
eng.close()
