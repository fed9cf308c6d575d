#!/usr/bin/env python3
"""The mean vorticity of the wake behind a plunging foil as a function of the reduced frequency k: examples/wake_vorticity.py
for a whole Strouhal sweep in ONE device launch (`sweep(cases, survey=..., survey_phases=8, survey_grad=True)`).  In every
sampled step of every member the closed-form velocity gradient at the survey points is added to five more sums per point inside
the launch, and every member carries the attributes of a solo run with survey_gradient=True.  Printed per member: the sign and
the peak of the mean vorticity in the upper and in the lower row of the wake -- a von Karman street (drag) has clockwise
vorticity, omega < 0, in the upper row, a reverse von Karman street (thrust) has it in the lower one, and the switch between
them is what a Strouhal study looks for -- and the coherent (phase-locked) share of <omega'^2> at 8 phases of the stroke.

    python examples/sweep_wake_vorticity.py [--k 0.5 1.0 2.0 3.0] [--periods 3] [--steps-per-period 200] [--bins 8] [--h 0.25]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=float, nargs="*", default=[0.5, 1.0, 2.0, 3.0], help="reduced frequencies omega c / U")
ap.add_argument("--periods", type=int, default=3, help="averaged periods (one more is run first and left out)")
ap.add_argument("--steps-per-period", type=int, default=200, help="a member may run 2048 steps at most")
ap.add_argument("--bins", type=int, default=8, help="phase bins of the stroke")
ap.add_argument("--h", type=float, default=0.25, help="plunge amplitude in chords")
ap.add_argument("--dr", type=float, default=0.1)
args = ap.parse_args()

spp = args.steps_per_period
steps = (args.periods + 1) * spp
window = (spp + 1, steps + 1, 1)                                 # the start-up period is left out; common to the sweep
grid = dict(xmin=1.0, xmax=4.0, zmin=-1.5, zmax=1.5, dr=args.dr)
# every member runs the same number of steps per period, so its dt follows its k (chord = Uinf = 1: the period is 2 pi / k)
cases = [dict(k=k, dt=2 * np.pi / k / spp, tf=(steps - 0.5) * 2 * np.pi / k / spp) for k in args.k]

t0 = time.perf_counter()
sims = sweep(cases, survey=grid, survey_frame="tunnel", survey_steps=window, survey_phases=args.bins, survey_grad=True, t0=0, chord=1,
             rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012", alpha_max=0, h_max=args.h)
print(f"{len(sims)} members x {steps} steps ({spp} per period), a survey of {sims[0].survey_x.size} points with gradient sums in "
      f"{args.bins} phase bins over {args.periods} periods each, one launch: {time.perf_counter() - t0:.2f} s")

for k, sim in zip(args.k, sims):
    om, z = sim.survey_mean_omega, sim.survey_z
    zc = (z * sim.survey_omega2).sum() / sim.survey_omega2.sum()   # the wake's centre line: the centroid of the enstrophy
    rows = {"upper": z > zc, "lower": z < zc}
    line = f"k = {k:4.2f} (St = {k * args.h / np.pi:.3f}):"
    sign = {}
    for name, mask in rows.items():
        vals = np.where(mask, om, 0.0)
        j = np.unravel_index(np.argmax(np.abs(vals)), vals.shape)
        sign[name] = np.sign(vals[j])
        line += f"  {name} row: mean omega peak {vals[j]:+.3f} at (x - xpiv, z) = ({sim.survey_x[j]:.2f}, {z[j]:+.2f})"
    kind = "reverse von Karman (thrust)" if sign["upper"] > 0 > sign["lower"] else \
        "von Karman (drag)" if sign["upper"] < 0 < sign["lower"] else "neither"
    print(line + f"  -> {kind}")
    total = sim.survey_coherent_omega2 + sim.survey_random_omega2
    print(f"    {sim.survey_bin_count.min()} .. {sim.survey_bin_count.max()} samples per bin; mean enstrophy <omega^2> over the grid "
          f"{sim.survey_omega2.mean():.4f}; vortex cores (mean Q > 0) at {int((sim.survey_mean_q > 0).sum())} of {om.size} points; coherent "
          f"share of <omega'^2> at {sim.survey_nbins} phases: {sim.survey_coherent_omega2.sum() / total.sum():.1%}")
