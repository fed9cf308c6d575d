#!/usr/bin/env python3
"""A calibration sweep over LESPcrit of config 1 with the wake integrals of every member: how much circulation the leading-edge
vortices of each sign carry at the end, how well the lift the impulse of the vortex system implies follows the
unsteady-Bernoulli `Cl`, and the kinetic energy in the wake at the sampled steps -- examples/wake_impulse.py for a whole sweep in
ONE device launch (`sweep(cases, integrals=True, energy_steps=...)`).

    python examples/sweep_wake_impulse.py [--lesp 0.1 0.15 0.2 0.25 0.3] [--energy-every 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lesp", type=float, nargs="*", default=[0.1, 0.15, 0.2, 0.25, 0.3], help="critical LESP of each member")
ap.add_argument("--energy-every", type=int, default=50, help="steps between energy samples (each is a pair sum over all sources)")
args = ap.parse_args()

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, Naca="0012")
every = args.energy_every
t0 = time.perf_counter()
sims = sweep([dict(LESPcrit=l) for l in args.lesp], integrals=True, energy_steps=(every, 1 << 30, every), **CONFIG1)
print(f"{len(sims)} members x {sims[0].nt - 1} steps with wake integrals, the energy every {every} steps, one launch: "
      f"{time.perf_counter() - t0:.2f} s")

for lesp, sim in zip(args.lesp, sims):
    period = int(round(1.0 / sim.f / sim.dt))                    # steps of the first period, left out of the comparison
    levs = sim.integral_sums[-1, 2, :, 0]
    d = (sim.impulse_Cl - sim.Cl)[period:]
    print(f"LESPcrit = {lesp:4.2f}: LEVs at the last step: {int(levs[0]):3d} with Gamma >= 0 carrying "
          f"{sim.wake_circulation('LEV', '+')[-1]:+.3f}, {int(levs[1]):3d} with Gamma < 0 carrying "
          f"{sim.wake_circulation('LEV', '-')[-1]:+.3f}; rms(impulse_Cl - Cl) after the first period = {np.sqrt((d * d).mean()):.3f} "
          f"(max |Cl| = {np.abs(sim.Cl[period:]).max():.3f})")
    # Gamma is clockwise-positive, so the kinetic energy per unit span is -rho W (examples/wake_impulse.py)
    steps = np.flatnonzero(np.isfinite(sim.wake_energy))
    E = -sim.rho * sim.wake_energy[steps]
    print("    -rho W at steps " + ", ".join(f"{i}: {e:+.3f}" for i, e in zip(steps, E)))
