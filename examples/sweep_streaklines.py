#!/usr/bin/env python3
"""Streaklines for every member of a sweep over the reduced frequency k: ONE rake ahead of the leading edge, dye released
every few steps (particle_frame='tunnel': a held particle rides with each member's own pivot), all members advected inside
ONE device launch.  A member carries the attributes of a solo run with tracers, so the post-processing is that of
examples/streaklines.py.

    python examples/sweep_streaklines.py [--k 0.2 0.4 0.6 0.8] [--tf 10] [--dt 2e-2] [--every 5] [--rake 7] [--plot sweep_streaklines.png]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=float, nargs="*", default=[0.2, 0.4, 0.6, 0.8], help="reduced frequencies, in units of pi")
ap.add_argument("--tf", type=float, default=10.0)
ap.add_argument("--dt", type=float, default=2e-2)
ap.add_argument("--every", type=int, default=5, help="release a particle from every rake point each so many steps")
ap.add_argument("--rake", type=int, default=7, help="points of the rake")
ap.add_argument("--plot", default=None, help="write the picture here (needs matplotlib)")
args = ap.parse_args()

nt = len(np.arange(0, args.tf + args.dt, args.dt))
releases = np.arange(1, nt, args.every)                          # release steps of one rake point
rake_z = np.linspace(-1.2, 1.2, args.rake)
seeds = np.stack([np.full(args.rake * len(releases), -0.75), np.repeat(rake_z, len(releases))])
release = np.tile(releases, args.rake)                           # tracer p * len(releases) + q: rake point p, q-th release

t0 = time.perf_counter()
sims = sweep([dict(k=k * np.pi) for k in args.k], t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30,
             LESPcrit=0.2, Naca="0012", particles=seeds, particle_release=release, particle_frame="tunnel")
print(f"{len(sims)} members x {nt - 1} steps, {seeds.shape[1]} tracers each ({args.rake} rake points x {len(releases)} releases), one "
      f"launch: {time.perf_counter() - t0:.2f} s")

ends = []
for k, sim in zip(args.k, sims):
    last = sim.nt - 1
    end = sim.tracer_path[last].reshape(2, args.rake, len(releases))   # [x | z, rake point, release]
    out = sim.tracer_released(last).reshape(args.rake, len(releases))
    ends.append((end, out))
    p = args.rake // 2
    x, z = end[0, p, out[p]] - sim.xpiv[last], end[1, p, out[p]]
    print(f"k = {k:.2f} pi: mean Cl {sim.Cl.mean():+.4f}; streakline from z = {rake_z[p]:+.2f}: {out[p].sum()} particles, z from "
          f"{z.min():+.2f} to {z.max():+.2f}, length {np.hypot(np.diff(x), np.diff(z)).sum():.2f} chords")

if args.plot:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not installed: no picture")
    else:
        fig, axes = plt.subplots(len(sims), 1, figsize=(10, 3 * len(sims)), squeeze=False)
        for ax, k, sim, (end, out) in zip(axes[:, 0], args.k, sims, ends):
            for p in range(args.rake):
                ax.plot(end[0, p, out[p]], end[1, p, out[p]], "-", lw=0.8)
            foil = sim.path["airfoil"][sim.nt - 1]
            ax.plot(foil[0], foil[1], "k-", lw=2)
            ax.set_aspect("equal")
            ax.set_title(f"k = {k:.2f} pi")
        fig.savefig(args.plot, dpi=150, bbox_inches="tight")
        print("wrote", args.plot)
