#!/usr/bin/env python3
"""A 64-member LESPcrit x alpha_max sweep of the README case as ONE device launch (ludvm_amd.sweep), mean Cl per member.

    python examples/sweep_lespcrit.py [--tf 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tf", type=float, default=20.0)
args = ap.parse_args()

lesp = np.linspace(0.05, 0.40, 8)
amax = np.linspace(5.0, 22.5, 8)
cases = [dict(LESPcrit=float(l), alpha_max=float(a)) for l in lesp for a in amax]
t0 = time.perf_counter()
sims = sweep(cases, t0=0, tf=args.tf, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, Naca="0012")
print(f"{len(sims)} members, {sims[0].nt - 1} steps each, {time.perf_counter() - t0:.2f} s")
print("mean Cl; rows LESPcrit, columns alpha_max =", " ".join(f"{a:7.2f}" for a in amax))
for i, l in enumerate(lesp):
    print(f"LESPcrit {l:5.2f}: " + " ".join(f"{sims[i * len(amax) + j].Cl.mean():7.4f}" for j in range(len(amax)))
          + "   LEVs " + " ".join(f"{sims[i * len(amax) + j].ilev:3d}" for j in range(len(amax))))
