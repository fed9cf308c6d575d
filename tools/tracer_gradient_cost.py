#!/usr/bin/env python3
"""What the velocity gradient costs, on one MI355X in one process (profiles/tracer_gradient_cost.txt):
    python tools/tracer_gradient_cost.py [--tracers 65536,262144] [--steps 17000] [--release 16000] [--repeats 3]
                                         [--n 1024] [--sources 20000] [--rounds 7] [--out FILE]

1. A gradient-tracer step against a plain float64 tracer step: the run of tools/tracers_cost.py `precision` (config 1's foil at
   dt = 1e-3, fp32 roll-up, sparse history, every tracer released at step --release, so that every free step sees the wake of
   that many steps: about 22 000 vortices at the defaults).  Plain run / tracers / tracers with tracer_gradient=True / tracers
   with tracer_precision='f32x2' / those with tracer_gradient='f32x2'  alternated, for each tracer count;
   the added wall time per free step of each, min / median / max of --repeats runs after one warm-up run each, and their ratios.
   The plain tracer kernels are the parent build's, instruction for instruction: the gradient kernels take their place only when
   the flag is set.
2. A gradient grid (Engine.flowfield_gradient) against the float64 velocity grid (Engine.flowfield_rows, vorticity off) at the
   same shape: tools/scalar_field_cost.py's measurement -- the library's own kernel time (HIP events around the main pair
   kernel), one warm-up per shape, alternating rounds.

Report only: no ratio is promised.  By operation count a gradient pair adds about 9 float64 operations to about 15."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tracers", type=lambda v: [int(m) for m in v.split(",")], default=[65536, 262144],
                help="tracer counts, comma separated: part 1 is run for each")
ap.add_argument("--steps", type=int, default=17000)
ap.add_argument("--release", type=int, default=16000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--n", type=int, default=1024, help="grid points per side")
ap.add_argument("--sources", type=int, default=20000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

eng = Engine(0)
info = eng.device_info()
lines = [f"# python tools/tracer_gradient_cost.py --tracers {','.join(str(m) for m in args.tracers)} --steps {args.steps} --release {args.release} "
         f"--repeats {args.repeats} --n {args.n} --sources {args.sources} --rounds {args.rounds}",
         f"# {info['name']}, {info['cu_count']} CUs"]

# ---- 1. the marched tracers ---------------------------------------------------------------------------------------------------
kw = dict(t0=0, tf=args.steps * 1e-3, dt=1e-3, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
          history="sparse", precision="f32")


def run(extra):
    t0 = time.perf_counter()
    sim = LUDVM(**kw, verbose=False, engine=eng, **extra)
    return time.perf_counter() - t0, sim


for M in args.tracers:
    rng = np.random.default_rng(1)
    traced = dict(tracers=np.stack([rng.uniform(-1.0, 3.0, M), rng.uniform(-2.0, 2.0, M)]), tracer_frame="tunnel",
                  tracer_release=np.full(M, args.release, dtype=np.int64))
    variants = {"plain": {}, "tracers": traced, "gradient": dict(traced, tracer_gradient=True),
                "f32x2": dict(traced, tracer_precision="f32x2"),
                "grad_f32x2": dict(traced, tracer_precision="f32x2", tracer_gradient="f32x2")}
    for extra in variants.values():
        run(extra)
    ts = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, extra in variants.items():
            t, sim = run(extra)
            ts[k].append(t)
    free = (sim.tracer_release[None, :] <= np.arange(1, sim.nt)[:, None]).sum(axis=1)
    ns = sim.n_freevort + np.arange(sim.nt) + np.cumsum(sim.LEV_shed != -1) + sim.Npoints - 1
    pairs, free_steps = float((free * ns[1:]).sum()), int((free > 0).sum())
    med = {k: statistics.median(v) for k, v in ts.items()}
    lines += [f"# 1. marched tracers: {sim.nt - 1} steps at dt = 1e-3 (config 1's foil, precision f32, sparse history), {M} tracers released at step "
              f"{args.release}: {free_steps} free steps,",
              f"#    sources {ns[sim.nt - free_steps]} .. {ns[-1]}, {pairs:.4g} tracer pairs; runs alternated, medians of {args.repeats}"]
    for k in variants:
        line = f"{k:10s} min {min(ts[k]):.4f} median {med[k]:.4f} max {max(ts[k]):.4f} s"
        if k != "plain":
            add = med[k] - med["plain"]
            line += f"; added {add:.4f} s = {add / free_steps * 1e6:.2f} us per free step, {pairs / max(add, 1e-9):.3g} pairs/s of the added time"
        lines.append(line)
    added = {k: med[k] - med["plain"] for k in variants if k != "plain"}
    lines.append(f"gradient-tracer step / plain float64 tracer step (added time per free step) = "
                 f"{added['gradient'] / max(added['tracers'], 1e-9):.2f}")
    lines.append(f"plain f32x2 tracer step / plain float64 tracer step = {added['f32x2'] / max(added['tracers'], 1e-9):.2f}")
    lines.append(f"f32x2 gradient-tracer step / float64 gradient-tracer step = {added['grad_f32x2'] / max(added['gradient'], 1e-9):.2f}")
    lines.append(f"f32x2 gradient-tracer step / plain float64 tracer step = {added['grad_f32x2'] / max(added['tracers'], 1e-9):.2f}")
    lines.append(f"f32x2 gradient-tracer step / plain f32x2 tracer step = {added['grad_f32x2'] / max(added['f32x2'], 1e-9):.2f}")

# ---- 2. the grid ----------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(5)
nsrc = args.sources
g, xs, zs = rng.normal(0, 0.02, nsrc), rng.uniform(-60, 0, nsrc), rng.normal(0, 0.5, nsrc)      # a wake-like strip
dr, vc = 0.02, 0.0195
grid = (-dr * args.n, -dr * args.n / 2, dr)
eng.kernel_timing(True)


def launch(what):
    eng.kernel_time_ms(reset=True)
    if what == "velocity":
        eng.flowfield_rows(*grid, args.n, args.n, 0, args.n, g, xs, zs, vc, vorticity=False, precision="f64")
    else:
        eng.flowfield_gradient(*grid, args.n, args.n, g, xs, zs, vc)
    ms, launches = eng.kernel_time_ms(reset=True)
    assert launches == 1, launches
    return ms


kinds = ("velocity", "gradient")
for k in kinds:
    launch(k)
times = {k: [] for k in kinds}
for _ in range(args.rounds):
    for k in kinds:
        times[k].append(launch(k))
gp = args.n * args.n * nsrc
gmed = {k: statistics.median(times[k]) for k in kinds}
lines += [f"# 2. grids: {args.n} x {args.n} points x {nsrc} sources = {gp:.3e} pairs per launch, v_core {vc}, float64; main pair kernel only",
          f"#    (HIP events), one warm-up per shape, {args.rounds} alternating rounds",
          "kernel       median ms     min ms     max ms    pairs/s"]
for k in kinds:
    t = times[k]
    lines.append(f"{k:9s}   {gmed[k]:10.3f} {min(t):10.3f} {max(t):10.3f}   {gp / (gmed[k] * 1e-3):.3e}")
lines.append(f"gradient grid / velocity grid = {gmed['gradient'] / gmed['velocity']:.2f}")
report = "\n".join(lines) + "\n"
print(report, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(report)
eng.close()
