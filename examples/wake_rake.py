#!/usr/bin/env python3
"""A rake of velocity probes behind the foil, in the frame that translates with the pivot, on a run that keeps no dense
history: the dominant frequency of the wake signal `probe_w`, next to the motion's own frequency.

    python examples/wake_rake.py [--tf 40] [--dt 5e-3] [--x 2.0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tf", type=float, default=40.0)
ap.add_argument("--dt", type=float, default=5e-3)
ap.add_argument("--x", type=float, default=2.0, help="rake position, chords behind the pivot")
args = ap.parse_args()

# 17 points across the wake, `x` behind the pivot (the foil moves towards -x: behind it is +x)
rake = np.stack([np.full(17, args.x), np.linspace(-2.0, 2.0, 17)])
t0 = time.perf_counter()
sim = LUDVM(t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            verbose=False, history="sparse", probes=rake, probe_frame="tunnel")
print(f"{sim.nt - 1} steps, {sim.itev + sim.ilev + 2} wake vortices, {time.perf_counter() - t0:.2f} s; "
      f"history rows kept: {len(sim.path['TEV'].steps())}")

# spectrum of w over the second half of the run (the starting vortex has left the rake by then)
half = sim.nt // 2
w = sim.probe_w[half:] - sim.probe_w[half:].mean(axis=0)
spec = np.abs(np.fft.rfft(w * np.hanning(len(w))[:, None], axis=0)) ** 2
freq = np.fft.rfftfreq(len(w), d=sim.dt)
peak = freq[1:][np.argmax(spec[1:].sum(axis=1))]
print(f"dominant frequency of probe_w at the rake: {peak:.4f}  (motion: f = {sim.f:.4f}; St = f c / U = {peak * sim.chord / sim.Uinf:.4f})")
print("rms of w along the rake (z from -2 to 2):", " ".join(f"{v:.3f}" for v in w.std(axis=0)))
