#!/usr/bin/env python3
"""Shedding frequency behind the foil as a function of the reduced frequency k: a sweep over k with ONE 64-point rake in
the frame that translates with each member's pivot, the probe series of every member evaluated inside the one device launch
(`sweep(cases, probes=..., probe_frame='tunnel')`), and the spectrum of examples/wake_rake.py per member.

    python examples/sweep_strouhal.py [--tf 20] [--dt 1e-2] [--x 2.0] [--k 0.2 0.4 0.6 0.8 1.0]
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
ap.add_argument("--dt", type=float, default=1e-2, help="a member may run 2048 steps at most")
ap.add_argument("--x", type=float, default=2.0, help="rake position, chords behind the pivot")
ap.add_argument("--k", type=float, nargs="*", default=[0.2, 0.4, 0.6, 0.8, 1.0], help="reduced frequencies, in units of pi")
args = ap.parse_args()

# 64 points across the wake, `x` behind the pivot (the foil moves towards -x: behind it is +x)
rake = np.stack([np.full(64, args.x), np.linspace(-2.0, 2.0, 64)])
t0 = time.perf_counter()
sims = sweep([dict(k=k * np.pi) for k in args.k], probes=rake, probe_frame="tunnel",
             t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")
print(f"{len(sims)} members x {sims[0].nt - 1} steps in one launch, {time.perf_counter() - t0:.2f} s")

for k, sim in zip(args.k, sims):
    # spectrum of w over the second half of the run (the starting vortex has left the rake by then)
    half = sim.nt // 2
    w = sim.probe_w[half:] - sim.probe_w[half:].mean(axis=0)
    spec = np.abs(np.fft.rfft(w * np.hanning(len(w))[:, None], axis=0)) ** 2
    freq = np.fft.rfftfreq(len(w), d=sim.dt)
    peak = freq[1:][np.argmax(spec[1:].sum(axis=1))]
    print(f"k = {k:.2f} pi: dominant frequency of probe_w at the rake {peak:.4f}  (motion: f = {sim.f:.4f}; "
          f"St = f c / U = {peak * sim.chord / sim.Uinf:.4f}); rms of w over the rake {w.std():.3f}; mean Cl {sim.Cl.mean():.4f}")
