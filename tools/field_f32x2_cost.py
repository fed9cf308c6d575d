#!/usr/bin/env python3
"""What the hi+lo fp32 route of the analytic vorticity and the velocity gradient costs against the float64 route, on one MI355X
in one process (profiles/field_f32x2_cost.txt):
    python tools/field_f32x2_cost.py [--shapes 1024x20000,2048x200000] [--rounds 7] [--out FILE]

Per shape (n x n grid points, that many sources): Engine.flowfield_gradient and Engine.flowfield_scalar('omega') in precision
'f64' and 'f32x2', with the fp32 velocity grid (Engine.flowfield_rows, vorticity off) beside them -- tools/scalar_field_cost.py's
measurement: the library's own kernel time (HIP events around the main pair kernel, not the uploads, the finisher or the
downloads), one warm-up per kernel and shape, alternating rounds; median, min and max.  The float64 kernels are the
denominators: they are the kernels of the build before the route (tests/test_gradient_f32x2_host.py and the resource table in
DESIGN.md show their code unchanged), measured here in the same process and the same rounds as the new ones.  The outputs of
the two routes are compared at the timed size (largest difference over the field's maximum).

Report only: no ratio is promised.  By instruction count the gradient's fp32 pair is 20 packed operations and 2 v_rsq_f32 per
two pairs against about 30 float64-rate operations per pair: about 0.4 to 0.5 of the float64 kernel's time was expected."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1024x20000,2048x200000", help="comma-separated: grid points per side x sources")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

eng = Engine(0)
info = eng.device_info()
lines = [f"# python tools/field_f32x2_cost.py --shapes {args.shapes} --rounds {args.rounds}",
         f"# {info['name']}, {info['cu_count']} CUs",
         "# main pair kernel only (HIP events), one warm-up per kernel and shape, alternating rounds; float64 kernels: the code of the",
         "# build before the route, measured in the same rounds"]
eng.kernel_timing(True)
dr, vc = 0.02, 0.0195
KINDS = ("velocity f32", "gradient f64", "gradient f32x2", "omega f64", "omega f32x2")

for n, nsrc in shapes:
    rng = np.random.default_rng(5)
    g, xs, zs = rng.normal(0, 0.02, nsrc), rng.uniform(-60, 0, nsrc), rng.normal(0, 0.5, nsrc)      # a wake-like strip
    grid = (-dr * n, -dr * n / 2, dr)
    keep = {}

    def launch(what):
        name, prec = what.split()
        eng.kernel_time_ms(reset=True)
        if name == "velocity":
            eng.flowfield_rows(*grid, n, n, 0, n, g, xs, zs, vc, vorticity=False, precision=prec)
        elif name == "gradient":
            keep[what] = eng.flowfield_gradient(*grid, n, n, g, xs, zs, vc, precision=prec)
        else:
            keep[what] = (eng.flowfield_scalar("omega", *grid, n, n, g, xs, zs, vc, precision=prec),)
        ms, launches = eng.kernel_time_ms(reset=True)
        assert launches >= 1, launches
        return ms * launches

    for k in KINDS:
        launch(k)
    times = {k: [] for k in KINDS}
    for _ in range(args.rounds):
        for k in KINDS:
            times[k].append(launch(k))
    pairs = float(n) * n * nsrc
    med = {k: statistics.median(times[k]) for k in KINDS}
    lines += [f"# {n} x {n} points x {nsrc} sources = {pairs:.3e} pairs per launch, v_core {vc}, {args.rounds} rounds",
              "kernel             median ms     min ms     max ms    pairs/s"]
    for k in KINDS:
        t = times[k]
        lines.append(f"{k:15s}   {med[k]:10.3f} {min(t):10.3f} {max(t):10.3f}   {pairs / (med[k] * 1e-3):.3e}")
    for name in ("gradient", "omega"):
        a, b = keep[f"{name} f32x2"], keep[f"{name} f64"]
        diff = max(np.abs(x - y).max() for x, y in zip(a, b)) / max(np.abs(y).max() for y in b)
        lines.append(f"{name} f32x2 / {name} f64 = {med[name + ' f32x2'] / med[name + ' f64']:.2f} of the kernel time (expected 0.4 to 0.5);"
                     f" largest difference of the outputs = {diff:.2e} of the field's maximum")
    lines.append(f"gradient f32x2 / velocity f32 = {med['gradient f32x2'] / med['velocity f32']:.2f}")
    keep.clear()
report = "\n".join(lines) + "\n"
print(report, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(report)
eng.close()
