#!/usr/bin/env python3
"""The time-averaged wake behind a plunging foil as a function of the reduced frequency k: a sweep over k with ONE survey mesh
in the frame that translates with each member's pivot, the five raw sums of every member accumulated inside the one device
launch (`sweep(cases, survey=..., survey_frame='tunnel', survey_steps=...)`) -- no per-step rows come back.  A member carries
the attributes of a solo run with a survey, so the post-processing is that of examples/wake_survey.py: the mean-jet peak (the
largest excess of the mean streamwise velocity), its height and half-width at one station, and the largest Reynolds stress.

    python examples/sweep_wake_survey.py [--k 0.2 0.4 0.6 0.8] [--tf 15] [--dt 2e-2] [--station 2.0] [--skip 0.5]
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
ap.add_argument("--tf", type=float, default=15.0)
ap.add_argument("--dt", type=float, default=2e-2, help="a member may run 2048 steps at most")
ap.add_argument("--station", type=float, default=2.0, help="where the jet is measured, chords behind the pivot")
ap.add_argument("--skip", type=float, default=0.5, help="fraction of the run left out of the average (the starting vortex)")
args = ap.parse_args()

nt = len(np.arange(0, args.tf + args.dt, args.dt))
first = max(1, int(args.skip * nt))
# behind the pivot (the foil moves towards -x: behind it is +x), across the wake: about 1300 points of a sweep's 4096
mesh = dict(xmin=0.5, xmax=max(3.55, args.station + 0.05), zmin=-2.0, zmax=2.05, dr=0.1)
t0 = time.perf_counter()
sims = sweep([dict(k=k * np.pi) for k in args.k], survey=mesh, survey_frame="tunnel", survey_steps=(first, nt, 1),
             t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012", alpha_max=0,
             h_max=0.25)
print(f"{len(sims)} members x {nt - 1} steps, a survey of {sims[0].survey_x.size} points over steps {first} .. {nt - 1} each, one launch: "
      f"{time.perf_counter() - t0:.2f} s")

for k, sim in zip(args.k, sims):
    col = int(np.argmin(np.abs(sim.survey_x[:, 0] - args.station)))
    z, u = sim.survey_z[col], sim.survey_mean_u[col]
    # the induced field has no freestream term: u is the excess over the flow past the foil, and a jet behind a foil that
    # moves towards -x points towards +x
    top = int(np.argmax(u))
    above = z[u >= 0.5 * u[top]]
    print(f"k = {k:.2f} pi: mean Cl {sim.Cl.mean():+.4f}; mean jet at x = {sim.survey_x[col, 0]:.2f} behind the pivot over "
          f"{sim.survey_count} steps: peak {u[top]:+.4f} U at z = {z[top]:+.2f}, half-width {above.max() - above.min():.2f} chords; largest "
          f"|<u'w'>| on the mesh {np.abs(sim.survey_uw).max():.4f}")
