#!/usr/bin/env python3
"""Phase-averaged vorticity and Q of a plunging foil's wake, without a stored wake.

A wake survey rides with the pivot (tunnel frame) and, with survey_gradient=True, every sampled step adds the closed-form
gradient of the field at the survey points to running sums inside the device-resident march: ux, the strain e, the vorticity
omega, omega^2 and Q = omega^2 / 4 - ux^2 - e^2.  Eight phase bins of the motion's period give the phase-locked maps; printed per
phase are the extremes of the mean vorticity and the place of the largest mean Q -- where the vortex cores sit at that phase --
and, over all samples, the enstrophy split into its coherent and random parts and the integral of the production of
fluctuation energy -<u_i' u_j'> dU_i/dx_j, from the survey's own Reynolds stresses and mean gradient.

--f32x2 takes the same ten sums from one walk per sampled step in packed fp32 on hi+lo positions (survey_gradient='f32x2'): the
same attributes from the same code, the pair sums -- the velocity's too -- at the hi+lo tier instead of float64.

    python examples/wake_vorticity.py [--tf 20] [--dt 5e-2] [--skip 0.25] [--dr 0.05] [--f32x2] [--plot out.png]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tf", type=float, default=20.0)
ap.add_argument("--dt", type=float, default=5e-2)
ap.add_argument("--skip", type=float, default=0.25, help="fraction of the run left out of the averages (the starting vortex)")
ap.add_argument("--dr", type=float, default=0.05, help="spacing of the survey mesh")
ap.add_argument("--f32x2", action="store_true", help="the pair sums of the survey in hi+lo fp32 (survey_gradient='f32x2')")
ap.add_argument("--plot", default=None, help="write the eight vorticity maps with their Q = 0 contours to this PNG")
args = ap.parse_args()

nt = len(np.arange(0, args.tf + args.dt, args.dt))
first = max(1, int(args.skip * (nt - 1)))
B = 8
# the mesh, x measured from the pivot: from the trailing edge to five chords behind it
mesh = dict(xmin=0.8, xmax=5.8, zmin=-2.0, zmax=2.0, dr=args.dr)
sim = LUDVM(t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            verbose=False, survey=mesh, survey_frame="tunnel", survey_steps=(first, nt, 1), survey_bins=B,
            survey_gradient="f32x2" if args.f32x2 else True)
x, z = sim.survey_x, sim.survey_z
print(f"{x.size} survey points ({x.shape[0]} x {x.shape[1]}), steps {first} .. {nt - 1}: {sim.survey_count} samples, "
      f"{sim.survey_bin_count.tolist()} per phase bin")
print("phase   mean omega in            largest mean Q   at (x behind the pivot, z)")
for b in range(B):
    om, q = sim.survey_bin_mean_omega[b], sim.survey_bin_mean_q[b]
    if not np.isfinite(q).all():
        print(f"{sim.survey_phase[b]:5.3f}   (no sample)")
        continue
    i, j = np.unravel_index(int(np.argmax(q)), q.shape)
    print(f"{sim.survey_phase[b]:5.3f}   [{om.min():+8.3f}, {om.max():+8.3f}]   {q[i, j]:12.3f}     ({x[i, j]:5.2f}, {z[i, j]:+5.2f})")

cell = args.dr * args.dr
print(f"time-averaged: omega in [{sim.survey_mean_omega.min():+.3f}, {sim.survey_mean_omega.max():+.3f}], "
      f"{100 * (sim.survey_mean_q > 0).mean():.1f} % of the window rotation-dominated in the mean")
print(f"enstrophy integral (sum omega^2 / 2 n) = {0.5 * sim.survey_omega2.sum() * cell:.4f}; of the variance of omega, "
      f"coherent {sim.survey_coherent_omega2.sum() * cell:.4f} and random {sim.survey_random_omega2.sum() * cell:.4f}")
print(f"production integral -<u_i' u_j'> dU_i/dx_j = {sim.survey_production.sum() * cell:+.5f}")

if args.plot:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(4, 2, figsize=(12, 14))
    lim = np.nanmax(np.abs(sim.survey_bin_mean_omega))
    for b, a in enumerate(ax.ravel()):
        a.pcolormesh(x, z, sim.survey_bin_mean_omega[b], shading="auto", cmap="RdBu_r", vmin=-lim, vmax=lim)
        a.contour(x, z, sim.survey_bin_mean_q[b], levels=[0.0], colors="k", linewidths=0.5)
        a.set_title(f"phase {sim.survey_phase[b]:.3f}: mean omega, Q = 0")
        a.set_aspect("equal")
    fig.tight_layout()
    fig.savefig(args.plot, dpi=120)
    print("wrote", args.plot)
