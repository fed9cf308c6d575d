#!/usr/bin/env python3
"""Streaklines: dye released every `k` steps from a small rake that rides ahead of the leading edge (tracer_frame='tunnel':
a held tracer translates with the pivot; staggered tracer_release: one particle per rake point every k steps).  At the end
of the run the particles of one rake point, in release order, are that point's streakline.

    python examples/streaklines.py [--tf 10] [--dt 1e-2] [--every 5] [--rake 7] [--plot streaklines.png] [--f32x2]

--f32x2: the tracers' pair sums in fp32 on hi+lo positions (tracer_precision='f32x2': velocities within 2e-6 of max|u| of the
float64 ones, every other result of the run unchanged) -- the choice for many particles over a long run.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tf", type=float, default=10.0)
ap.add_argument("--dt", type=float, default=1e-2)
ap.add_argument("--every", type=int, default=5, help="release a particle from every rake point each so many steps")
ap.add_argument("--rake", type=int, default=7, help="points of the rake")
ap.add_argument("--plot", default=None, help="write the picture here (needs matplotlib)")
ap.add_argument("--f32x2", action="store_true", help="advect the tracers with hi+lo fp32 pair sums (tracer_precision='f32x2')")
args = ap.parse_args()

nt = len(np.arange(0, args.tf + args.dt, args.dt))
releases = np.arange(1, nt, args.every)                          # release steps of one rake point
# the rake: half a chord ahead of the leading edge (the pivot is a quarter chord behind it; the foil moves towards -x),
# across the heave amplitude
rake_z = np.linspace(-1.2, 1.2, args.rake)
seeds = np.stack([np.full(args.rake * len(releases), -0.75), np.repeat(rake_z, len(releases))])
release = np.tile(releases, args.rake)                           # tracer p * len(releases) + q: rake point p, q-th release

t0 = time.perf_counter()
sim = LUDVM(t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            verbose=False, history="sparse", tracers=seeds, tracer_release=release, tracer_frame="tunnel",
            tracer_precision="f32x2" if args.f32x2 else "f64")
last = sim.nt - 1
print(f"{last} steps, {seeds.shape[1]} tracers ({args.rake} rake points x {len(releases)} releases) in {sim.tracer_precision}, "
      f"{time.perf_counter() - t0:.2f} s; tracer rows kept: {sim.tracer_path.steps()}")

end = sim.tracer_path[last].reshape(2, args.rake, len(releases))   # [x | z, rake point, release]
out = sim.tracer_released(last).reshape(args.rake, len(releases))
for p in range(args.rake):
    x, z = end[0, p, out[p]] - sim.xpiv[last], end[1, p, out[p]]
    length = np.hypot(np.diff(x), np.diff(z)).sum()
    print(f"streakline from z = {rake_z[p]:+.2f}: {out[p].sum()} particles, x - xpiv from {x.min():+.2f} to {x.max():+.2f}, "
          f"z from {z.min():+.2f} to {z.max():+.2f}, length {length:.2f} chords")

if args.plot:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not installed: no picture")
    else:
        fig, ax = plt.subplots(figsize=(10, 4))
        for p in range(args.rake):
            ax.plot(end[0, p, out[p]], end[1, p, out[p]], "-", lw=0.8)
        foil = sim.path["airfoil"][last]
        ax.plot(foil[0], foil[1], "k-", lw=2)
        ax.set_aspect("equal")
        ax.set_xlabel("x")
        ax.set_ylabel("z")
        fig.savefig(args.plot, dpi=150, bbox_inches="tight")
        print("wrote", args.plot)
