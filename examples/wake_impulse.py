#!/usr/bin/env python3
"""Wake integrals of a plunging foil: the lift the impulse of the vortex system implies next to the unsteady-Bernoulli `Cl`, the
shares of the TEVs, the LEVs and the bound vortices in the lift impulse, and the kinetic energy the run puts into the wake per
period -- from a run that keeps no dense history (`wake_integrals=True`).

    python examples/wake_impulse.py [--periods 4] [--steps-per-period 200] [--k 1.5] [--h 0.25] [--energy-every 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--periods", type=int, default=4)
ap.add_argument("--steps-per-period", type=int, default=200)
ap.add_argument("--k", type=float, default=1.5, help="reduced frequency omega c / U")
ap.add_argument("--h", type=float, default=0.25, help="plunge amplitude in chords")
ap.add_argument("--energy-every", type=int, default=20, help="steps between energy samples")
args = ap.parse_args()

P = args.steps_per_period
period = 2 * np.pi / args.k                                      # chord = Uinf = 1
dt = period / P
steps = args.periods * P
t0 = time.perf_counter()
sim = LUDVM(t0=0, tf=(steps - 0.5) * dt, dt=dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            alpha_max=0, h_max=args.h, k=args.k, verbose=False, history="sparse", wake_integrals=True,
            wake_energy_steps=(args.energy_every, steps + 1, args.energy_every))
print(f"{sim.nt - 1} steps of dt = {dt:.4g} ({P} per period), {int(sim.integral_sums[-1, :3, :, 0].sum())} wake vortices, "
      f"{time.perf_counter() - t0:.2f} s")

# the lift by two routes, after the first period
cl, icl = sim.Cl[P:], sim.impulse_Cl[P:]
d = icl - cl
print(f"Cl (unsteady Bernoulli) against impulse_Cl (-dI/dt of the vortex system), steps {P} .. {sim.nt - 1}:")
print(f"  max |Cl| = {np.abs(cl).max():.3f}   correlation = {np.corrcoef(cl, icl)[0, 1]:.4f}   max |difference| = {np.abs(d).max():.3f}   "
      f"rms = {np.sqrt((d * d).mean()):.3f}")

# who carries the lift impulse I_z = rho sum G x: its change over the last period, class by class
Iz = sim.rho * sim.integral_sums[:, :, :, 2].sum(axis=2)         # [nt, class]
last = Iz[-1] - Iz[-1 - P]
print("change of the lift impulse rho sum G x over the last period, by class (their sum over the period is -integral of the lift):")
for name, v in zip(sim.integral_classes, last):
    print(f"  {name:<5} {v:+.4f}")
print(f"  all   {last.sum():+.4f}   (-integral of L dt over the period from Cl: {-0.5 * sim.rho * np.sum(sim.Cl[-P:]) * dt:+.4f})")
levs = sim.integral_sums[-1, 2, :, 0]
print(f"LEVs in the system at the end: {int(levs[0])} with Gamma >= 0 carrying {sim.wake_circulation('LEV', '+')[-1]:+.3f}, "
      f"{int(levs[1])} with Gamma < 0 carrying {sim.wake_circulation('LEV', '-')[-1]:+.3f}")

# the energy the run has put into the fluid, period by period.  W = 1/2 sum G psi is formed with the clockwise-positive Gamma of
# the project, whose vorticity is -Gamma: the kinetic energy per unit span (finite because Kelvin keeps the total circulation
# at its initial value, 0 here) is -rho W; the cores' self part is left out (it only counts the vortices)
W = -sim.rho * sim.wake_energy_interaction
print("kinetic energy -rho W (interaction part) of the vortex system at the end of each period, and what the period added:")
prev = None
for p in range(1, args.periods + 1):
    i = p * P // args.energy_every * args.energy_every           # the last sample of the period
    if np.isfinite(W[i]):
        print(f"  period {p}: E = {W[i]:+.4f}" + ("" if prev is None else f"   added {W[i] - prev:+.4f}"))
        prev = W[i]
