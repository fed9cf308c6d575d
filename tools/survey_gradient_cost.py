#!/usr/bin/env python3
"""What the survey's gradient sums cost, on one MI355X in one process (profiles/survey_gradient_cost.txt):
    python tools/survey_gradient_cost.py [--points 65536] [--steps 17000] [--first 16000] [--repeats 3] [--out FILE]

A sampled step of a gradient survey against a sampled step of the plain float64 survey: the run of tools/tracer_gradient_cost.py
(config 1's foil at dt = 1e-3, fp32 roll-up, sparse history), --points survey points in the tunnel frame, every step from --first
on sampled, so that every sampled step sees the wake of that many steps: about 22 000 vortices at the defaults.  Plain run /
survey / survey with survey_gradient=True / survey with survey_gradient='f32x2' alternated; the added wall time per sampled step of
each, medians of --repeats runs, and their ratios.  The plain survey kernels and the float64 gradient pair are the parent
build's, instruction for instruction: the gradient pair takes the plain pair's place only when the flag is set, the hi+lo fp32
walk only with 'f32x2'.

Report only: no ratio is promised.  The float64 body costs 1.48 on the tracers, the fused hi+lo walk 0.34 of the float64
gradient-tracer step (profiles/tracer_gradient_cost.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--steps", type=int, default=17000)
ap.add_argument("--first", type=int, default=16000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

eng = Engine(0)
info = eng.device_info()
lines = [f"# python tools/survey_gradient_cost.py --points {args.points} --steps {args.steps} --first {args.first} --repeats {args.repeats}",
         f"# {info['name']}, {info['cu_count']} CUs"]

kw = dict(t0=0, tf=args.steps * 1e-3, dt=1e-3, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
          history="sparse", precision="f32")
K = args.points
rng = np.random.default_rng(1)
surveyed = dict(survey=np.stack([rng.uniform(-1.0, 3.0, K), rng.uniform(-2.0, 2.0, K)]), survey_frame="tunnel",
                survey_steps=(args.first, args.steps + 1, 1))
variants = {"plain": {}, "survey": surveyed, "gradient": dict(surveyed, survey_gradient=True),
            "gradient_f32x2": dict(surveyed, survey_gradient="f32x2")}


def run(extra):
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)
    return time.perf_counter() - t0, sim


for extra in variants.values():
    run(extra)
ts = {k: [] for k in variants}
for _ in range(args.repeats):
    for k, extra in variants.items():
        t, sim = run(extra)
        ts[k].append(t)
sampled = sim.survey_count
ns = sim.n_freevort + np.arange(sim.nt) + np.cumsum(sim.LEV_shed != -1) + sim.Npoints - 1
pairs = float(K) * float(ns[args.first:args.first + sampled].sum())
med = {k: statistics.median(v) for k, v in ts.items()}
lines += [f"# {sim.nt - 1} steps at dt = 1e-3 (config 1's foil, precision f32, sparse history), {K} survey points, every step from {args.first} "
          f"sampled: {sampled} sampled steps,",
          f"# sources {ns[args.first]} .. {ns[-1]}, {pairs:.4g} point pairs; runs alternated, medians of {args.repeats}"]
for k in variants:
    line = f"{k:14s} min {min(ts[k]):.4f} median {med[k]:.4f} max {max(ts[k]):.4f} s"
    if k != "plain":
        add = med[k] - med["plain"]
        line += f"; added {add:.4f} s = {add / sampled * 1e6:.2f} us per sampled step, {pairs / max(add, 1e-9):.3g} pairs/s of the added time"
    lines.append(line)
lines.append(f"gradient-survey step / plain float64 survey step (added time per sampled step) = "
             f"{(med['gradient'] - med['plain']) / max(med['survey'] - med['plain'], 1e-9):.2f}")
# (the denominator: the float64 gradient-survey step, survey_gradient=True -- the code path of the build before the route -- in the
# same process and rounds)
lines.append(f"'f32x2' gradient-survey step / float64 gradient-survey step (added time per sampled step) = "
             f"{(med['gradient_f32x2'] - med['plain']) / max(med['gradient'] - med['plain'], 1e-9):.2f}")
lines.append(f"'f32x2' gradient-survey step / plain float64 survey step (added time per sampled step) = "
             f"{(med['gradient_f32x2'] - med['plain']) / max(med['survey'] - med['plain'], 1e-9):.2f}")
report = "\n".join(lines) + "\n"
print(report, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(report)
eng.close()
