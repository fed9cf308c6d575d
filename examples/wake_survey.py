#!/usr/bin/env python3
"""Time-averaged wake of a plunging foil: a survey grid behind the trailing edge that rides with the pivot
(survey_frame='tunnel'), averaged over whole periods of the motion after a start-up period (survey_steps).  The mean
streamwise velocity across one station is the picture of the reverse Karman street: a jet on the wake's centre line when
the foil produces thrust.  (The field is the induced one: no freestream term.)

    python examples/wake_survey.py [--periods 3] [--steps-per-period 400] [--k 1.5] [--h 0.25] [--station 2.0] [--plot wake.png]
                                   [--f32]

--f32: the survey's pair sums in fp32 on local origins (survey_precision='f32': means within 1e-5 of max|u| of the float64
survey, every other result of the run unchanged) -- the choice for a fine grid over a long run.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--periods", type=int, default=3, help="averaged periods (one more is run first and left out)")
ap.add_argument("--steps-per-period", type=int, default=400)
ap.add_argument("--k", type=float, default=1.5, help="reduced frequency omega c / U")
ap.add_argument("--h", type=float, default=0.25, help="plunge amplitude in chords")
ap.add_argument("--station", type=float, default=2.0, help="x - xpiv of the printed profile")
ap.add_argument("--dr", type=float, default=0.05)
ap.add_argument("--plot", default=None, help="write the picture here (needs matplotlib)")
ap.add_argument("--f32", action="store_true", help="evaluate the survey's field in fp32 (survey_precision='f32')")
args = ap.parse_args()

period = 2 * np.pi / args.k                                      # chord = Uinf = 1
dt = period / args.steps_per_period
steps = (args.periods + 1) * args.steps_per_period
first = args.steps_per_period + 1                                # the start-up period is left out
window = (first, first + args.periods * args.steps_per_period, 1)
# the grid: from a quarter chord behind the trailing edge (the pivot is three quarters of a chord ahead of it) downstream
grid = dict(xmin=1.0, xmax=4.0, zmin=-1.5, zmax=1.5, dr=args.dr)

t0 = time.perf_counter()
sim = LUDVM(t0=0, tf=(steps - 0.5) * dt, dt=dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            alpha_max=0, h_max=args.h, k=args.k, verbose=False, history="sparse", survey=grid, survey_frame="tunnel",
            survey_steps=window, survey_precision="f32" if args.f32 else "f64")
nx, nz = sim.survey_x.shape
print(f"{sim.nt - 1} steps of dt = {dt:.4g} ({args.steps_per_period} per period), {nx} x {nz} survey points in {sim.survey_precision}, "
      f"{sim.survey_count} sampled steps = {sim.survey_count / args.steps_per_period:g} periods, {time.perf_counter() - t0:.2f} s")

ix = int(np.argmin(np.abs(sim.survey_x[:, 0] - args.station)))
z, u = sim.survey_z[ix], sim.survey_mean_u[ix]
print(f"mean induced u at x - xpiv = {sim.survey_x[ix, 0]:.2f} (urms = sqrt(<u'u'>), -<u'w'> the Reynolds shear stress):")
for j in range(0, nz, max(1, nz // 20)):
    print(f"  z = {z[j]:+.2f}   <u> = {u[j]:+.4f}   urms = {np.sqrt(max(sim.survey_uu[ix, j], 0.0)):.4f}   "
          f"-<u'w'> = {-sim.survey_uw[ix, j]:+.5f}")
jmax = int(np.argmax(u))
print(f"peak <u> = {u[jmax]:+.4f} at z = {z[jmax]:+.2f}; integral of <u> across the station: "
      f"{float((u[1:] + u[:-1]) @ np.diff(z)) / 2:+.4f} (positive: a jet, the foil pushes fluid back)")

if args.plot:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not installed: no picture")
    else:
        fig, ax = plt.subplots(figsize=(9, 4))
        im = ax.pcolormesh(sim.survey_x, sim.survey_z, sim.survey_mean_u, shading="auto", cmap="RdBu_r")
        fig.colorbar(im, ax=ax, label="<u> (induced)")
        ax.axvline(sim.survey_x[ix, 0], color="k", lw=0.6)
        ax.set_aspect("equal")
        ax.set_xlabel("x - xpiv")
        ax.set_ylabel("z")
        fig.savefig(args.plot, dpi=150, bbox_inches="tight")
        print("wrote", args.plot)
