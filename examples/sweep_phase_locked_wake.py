#!/usr/bin/env python3
"""The phase-locked wake behind a plunging foil as a function of the reduced frequency k: examples/phase_locked_wake.py for a
whole Strouhal sweep in ONE device launch (`sweep(cases, survey=..., survey_phases=8)`).  Every member is binned by its own
stroke -- its period is 1 / f, phase 0 at its t0 -- so one B serves members of different k and dt; the bin sums of every member
are accumulated inside the launch beside its time-averaged sums, and a member carries the attributes of a solo run with
survey_bins.  Printed per member: the peak of the phase-averaged jet at one station for each phase of the stroke (what a
phase-locked PIV measurement shows), and the coherent (phase-locked) share of <u'u'>.  (The field is the induced one: no
freestream term.)

    python examples/sweep_phase_locked_wake.py [--k 1.0 1.5 2.0 2.5] [--periods 3] [--steps-per-period 200] [--bins 8] [--h 0.25]
                                               [--station 2.0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=float, nargs="*", default=[1.0, 1.5, 2.0, 2.5], help="reduced frequencies omega c / U")
ap.add_argument("--periods", type=int, default=3, help="averaged periods (one more is run first and left out)")
ap.add_argument("--steps-per-period", type=int, default=200, help="a member may run 2048 steps at most")
ap.add_argument("--bins", type=int, default=8, help="phase bins of the stroke")
ap.add_argument("--h", type=float, default=0.25, help="plunge amplitude in chords")
ap.add_argument("--station", type=float, default=2.0, help="x - xpiv of the printed profiles")
ap.add_argument("--dr", type=float, default=0.1)
args = ap.parse_args()

spp = args.steps_per_period
steps = (args.periods + 1) * spp
window = (spp + 1, steps + 1, 1)                                 # the start-up period is left out; common to the sweep
grid = dict(xmin=1.0, xmax=4.0, zmin=-1.5, zmax=1.5, dr=args.dr)
# every member runs the same number of steps per period, so its dt follows its k (chord = Uinf = 1: the period is 2 pi / k)
cases = [dict(k=k, dt=2 * np.pi / k / spp, tf=(steps - 0.5) * 2 * np.pi / k / spp) for k in args.k]

t0 = time.perf_counter()
sims = sweep(cases, survey=grid, survey_frame="tunnel", survey_steps=window, survey_phases=args.bins, t0=0, chord=1, rho=1.225, Uinf=1,
             Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012", alpha_max=0, h_max=args.h)
print(f"{len(sims)} members x {steps} steps ({spp} per period), a survey of {sims[0].survey_x.size} points in {args.bins} phase bins "
      f"over {args.periods} periods each, one launch: {time.perf_counter() - t0:.2f} s")

print("phase of the stroke:          " + "".join(f"{p:16.3f}" for p in sims[0].survey_phase))
for k, sim in zip(args.k, sims):
    ix = int(np.argmin(np.abs(sim.survey_x[:, 0] - args.station)))
    z = sim.survey_z[ix]
    peaks = [int(np.argmax(sim.survey_bin_mean_u[b, ix])) for b in range(sim.survey_nbins)]
    print(f"k = {k:4.2f} (St = {k * args.h / np.pi:.3f}): jet peak  "
          + "".join(f"  {sim.survey_bin_mean_u[b, ix, j]:+.3f} @ {z[j]:+.2f}" for b, j in enumerate(peaks)))
    total = sim.survey_coherent_uu + sim.survey_random_uu
    print(f"    {sim.survey_bin_count.min()} .. {sim.survey_bin_count.max()} samples per bin; mean jet peak at the station "
          f"{sim.survey_mean_u[ix].max():+.4f} U; coherent share of <u'u'>: {sim.survey_coherent_uu[ix].sum() / total[ix].sum():.1%} at the "
          f"station, {sim.survey_coherent_uu.sum() / total.sum():.1%} over the grid")
