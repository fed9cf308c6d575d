#!/usr/bin/env python3
"""Streamlines of the README case: contours of the stream function `psi_ff` at three time steps, in the frame of the fluid at
rest and -- `psi_ff + Uinf * z_ff` -- in the frame that translates with the foil (a wind tunnel's); and the core model's
vorticity `omega_ff` next to the finite-difference `ome_ff` on the reference's dr = 0.02 mesh, where the stencil cannot
resolve a core of radius v_core = 1.3 dt.

    python examples/streamlines.py [--tf 20] [--dt 5e-2] [--plot out.png]
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
ap.add_argument("--plot", default=None, help="write the streamlines of the three steps (both frames) to this PNG")
args = ap.parse_args()

sim = LUDVM(t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            verbose=False)
last = sim.nt - 2          # (flowfield's gather takes TEV circulations [:s + 1]: the history holds them up to this step)
tsteps = [last // 4, last // 2, last]
# the window follows nothing: the foil starts at x in [0, 1] and moves towards -x, the wake stays where it was shed
window = dict(xmin=-sim.Uinf * args.tf - 1.0, xmax=2.0, zmin=-3.0, zmax=3.0)
sim.flowfield(**window, dr=0.1, tsteps=tsteps, psi=True)
psi_tunnel = sim.psi_ff + sim.Uinf * sim.z_ff
for ii, s in enumerate(tsteps):
    print(f"step {s}: psi in [{sim.psi_ff[ii].min():+.4f}, {sim.psi_ff[ii].max():+.4f}], "
          f"tunnel frame in [{psi_tunnel[ii].min():+.4f}, {psi_tunnel[ii].max():+.4f}]")
psi, x_ff, z_ff = sim.psi_ff, sim.x_ff, sim.z_ff

# the vorticity itself against the stencil, on the reference's mesh around the newest wake
near = dict(xmin=sim.xpiv[last] - 0.5, xmax=sim.xpiv[last] + 2.5, zmin=-1.0, zmax=1.0)
sim.flowfield(**near, dr=0.02, tsteps=[last], omega=True)
for name, f in (("omega_ff", sim.omega_ff[0]), ("ome_ff", sim.ome_ff[0])):
    print(f"dr = 0.02, step {last}: {name:8s} in [{f.min():+9.2f}, {f.max():+9.2f}]")
print(f"(v_core = {sim.v_core:.4f}: a core's peak vorticity is |Gamma| / (pi v_core^2) = {1 / (np.pi * sim.v_core**2):.1f} per unit "
      "circulation; the stencil spreads it over 2 dr)")

if args.plot:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(len(tsteps), 2, figsize=(12, 3 * len(tsteps)), squeeze=False)
    for ii, s in enumerate(tsteps):
        for col, (f, frame) in enumerate(((psi[ii], "fluid at rest"), (psi_tunnel[ii], "tunnel frame"))):
            ax[ii, col].contour(x_ff, z_ff, f, levels=40, linewidths=0.6)
            ax[ii, col].set_aspect("equal")
            ax[ii, col].set_title(f"step {s}, {frame}")
    fig.tight_layout()
    fig.savefig(args.plot, dpi=120)
    print("wrote", args.plot)
