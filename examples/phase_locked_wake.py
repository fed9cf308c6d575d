#!/usr/bin/env python3
"""Phase-locked wake of a plunging foil: the survey of examples/wake_survey.py with the stroke divided into 8 phase bins
(survey_bins=8).  Every sampled step adds its field to the sums of its bin as well, inside the device-resident march, so one
run gives the phase-averaged field at 8 phases of the stroke -- what a phase-locked PIV measurement shows -- and the split of
the fluctuation about the time average into a coherent part (the phase averages about the mean) and a random part (the
cycle-to-cycle scatter within a phase).  (The field is the induced one: no freestream term.)

    python examples/phase_locked_wake.py [--periods 3] [--steps-per-period 400] [--bins 8] [--k 1.5] [--h 0.25] [--station 2.0]
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
ap.add_argument("--bins", type=int, default=8, help="phase bins of the stroke")
ap.add_argument("--k", type=float, default=1.5, help="reduced frequency omega c / U")
ap.add_argument("--h", type=float, default=0.25, help="plunge amplitude in chords")
ap.add_argument("--station", type=float, default=2.0, help="x - xpiv of the printed profiles")
ap.add_argument("--dr", type=float, default=0.05)
args = ap.parse_args()

period = 2 * np.pi / args.k                                      # chord = Uinf = 1
dt = period / args.steps_per_period
steps = (args.periods + 1) * args.steps_per_period
first = args.steps_per_period + 1                                # the start-up period is left out
window = (first, first + args.periods * args.steps_per_period, 1)
grid = dict(xmin=1.0, xmax=4.0, zmin=-1.5, zmax=1.5, dr=args.dr)

t0 = time.perf_counter()
sim = LUDVM(t0=0, tf=(steps - 0.5) * dt, dt=dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            alpha_max=0, h_max=args.h, k=args.k, verbose=False, history="sparse", survey=grid, survey_frame="tunnel",
            survey_steps=window, survey_bins=args.bins)          # (survey_period defaults to the motion's, survey_phase0 to t0)
nx, nz = sim.survey_x.shape
print(f"{sim.nt - 1} steps of dt = {dt:.4g} ({args.steps_per_period} per period), {nx} x {nz} survey points, {sim.survey_count} sampled "
      f"steps in {sim.survey_nbins} phase bins of {sim.survey_bin_count.min()} .. {sim.survey_bin_count.max()} samples, "
      f"{time.perf_counter() - t0:.2f} s")

ix = int(np.argmin(np.abs(sim.survey_x[:, 0] - args.station)))
z = sim.survey_z[ix]
rows = range(0, nz, max(1, nz // 12))
print(f"phase-averaged induced u at x - xpiv = {sim.survey_x[ix, 0]:.2f} (columns: phase of the stroke, last: the time average):")
print("  z       " + "".join(f"{p:8.3f}" for p in sim.survey_phase) + "    mean")
for j in rows:
    print(f"  {z[j]:+.2f}   " + "".join(f"{sim.survey_bin_mean_u[b, ix, j]:+8.4f}" for b in range(sim.survey_nbins))
          + f"  {sim.survey_mean_u[ix, j]:+8.4f}")
peak = [int(np.argmax(sim.survey_bin_mean_u[b, ix])) for b in range(sim.survey_nbins)]
print("the jet's peak by phase: " + ", ".join(f"z = {z[j]:+.2f}" for j in peak))

coh, ran, tot = sim.survey_coherent_uu[ix], sim.survey_random_uu[ix], sim.survey_uu[ix]
print("<u'u'> across the station and its coherent (phase-locked) and random (cycle-to-cycle) shares:")
for j in rows:
    share = f"{coh[j] / tot[j]:6.1%} coherent, {ran[j] / tot[j]:6.1%} random" if tot[j] > 0 else "-"
    print(f"  z = {z[j]:+.2f}   <u'u'> = {tot[j]:.5f}   {share}")
print(f"over the whole grid: coherent {sim.survey_coherent_uu.sum() / sim.survey_uu.sum():.1%}, random "
      f"{sim.survey_random_uu.sum() / sim.survey_uu.sum():.1%} of the sum of <u'u'>")
