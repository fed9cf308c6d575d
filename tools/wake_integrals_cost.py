#!/usr/bin/env python3
"""What the wake integrals cost, and how far impulse_Cl is from Cl (profiles/wake_integrals_cost.txt), on one MI355X in one process:

    python tools/wake_integrals_cost.py [--wake 22000] [--steps 200] [--rounds 3] [--cfg2-rounds 1] [--out FILE]

cost      a marched run of `--steps` steps behind `--wake` free vortices ('f32', sparse history), alternating WITHOUT the keyword,
          with wake_integrals=True (the moments alone) and with an energy sample at every step: added wall time per step of the
          moments, wall time per energy sample, and that sample's pair rate against the float64 psi grid kernel's
          (profiles/scalar_field.txt: the same pair body).  Then config 2's full run (50 000 steps), alternating without and
          with the moments (--cfg2-rounds 0 skips it).  Wall times end in the device synchronise of the read-back.
agreement impulse_Cl against Cl on config 1 and on the plunging foil of examples/wake_impulse.py, at the case's dt and at dt / 2:
          maximum and rms difference after the first period.  A reported figure: the difference is the discretisation error of
          an explicit scheme, not a test bound."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ludvm_amd import LUDVM, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--wake", type=int, default=22000)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cfg2-rounds", type=int, default=1)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

PSI_GRID_PAIRS_PER_S = 5.33e11        # profiles/scalar_field.txt: pair_scalar_f64<psi>, 1024 x 1024 points x 20 000 sources
CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")
eng = Engine(0)
info = eng.device_info()
lines = [f"# python tools/wake_integrals_cost.py --wake {args.wake} --steps {args.steps} --rounds {args.rounds} --cfg2-rounds {args.cfg2_rounds}",
         f"# {info['name']}, {info['cu_count']} CUs; wall times (perf_counter around LUDVM(...), which ends in the read-back's synchronise)"]


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def timed(kw, **extra):
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sim = LUDVM(**kw, verbose=False, engine=eng, **extra)
    return time.perf_counter() - t0, sim


# ---- cost behind a large wake ---------------------------------------------------------------------------------------------------
rng = np.random.default_rng(5)
n, dt = args.wake, 1e-3
cloud = dict(circulation_freevort=rng.normal(0.0, 0.02, n),
             xy_freevort=np.stack([rng.uniform(2.0, 62.0, n), rng.normal(0.0, 0.5, n)]))        # a wake-like strip behind the foil
kw = dict(CONFIG1, dt=dt, tf=(args.steps - 0.5) * dt, precision="f32", history="sparse", **cloud)
variants = {"off": {}, "moments": dict(wake_integrals=True),
            "moments + energy": dict(wake_integrals=True, wake_energy_steps=(1, args.steps + 1, 1))}
for v in variants.values():
    timed(kw, **v)                      # warm-up of every shape
times = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, v in variants.items():
        times[k].append(timed(kw, **v)[0])
med = {k: statistics.median(t) for k, t in times.items()}
say(f"\n## {args.steps} marched steps behind {n} free vortices ('f32', sparse history), {args.rounds} alternating rounds")
say("variant               median s      min s      max s")
for k, t in times.items():
    say(f"{k:<20} {med[k]:9.4f}  {min(t):9.4f}  {max(t):9.4f}")
ns = n + args.steps / 2 + 80
per_step = (med["moments"] - med["off"]) / args.steps
per_sample = (med["moments + energy"] - med["moments"]) / args.steps
say(f"moments alone: {per_step * 1e6:+.1f} us per step ({100 * (med['moments'] / med['off'] - 1):+.2f} % of the run)")
say(f"energy: {per_sample * 1e3:.3f} ms per sample at about {ns:.0f} sources = {ns * ns / per_sample:.3e} pairs/s "
    f"(float64 psi grid kernel: {PSI_GRID_PAIRS_PER_S:.3e}; ratio {ns * ns / per_sample / PSI_GRID_PAIRS_PER_S:.2f})")

# ---- config 2's full run ----------------------------------------------------------------------------------------------------------
if args.cfg2_rounds:
    kw2 = dict(CONFIG1, dt=1e-3, tf=50, precision="f32", history="sparse", snapshot_steps=[])
    t2 = {"off": [], "moments": []}
    sims = {}
    for _ in range(args.cfg2_rounds):
        for k in t2:
            t, sims[k] = timed(kw2, **variants[k])
            t2[k].append(t)
    say(f"\n## config 2's full run ({sims['off'].nt - 1} steps, final wake {sims['off'].itev + sims['off'].ilev + 1}), {args.cfg2_rounds} alternating round(s), no warm-up run")
    for k, t in t2.items():
        say(f"{k:<20} " + "  ".join(f"{v:8.3f} s" for v in t))
    m_off, m_on = statistics.median(t2["off"]), statistics.median(t2["moments"])
    say(f"moments alone: {(m_on - m_off) / (sims['off'].nt - 1) * 1e6:+.2f} us per step ({100 * (m_on / m_off - 1):+.2f} % of the run); "
        f"Cl bit-identical: {np.array_equal(sims['off'].Cl, sims['moments'].Cl)}")

# ---- agreement of impulse_Cl with Cl ------------------------------------------------------------------------------------------------
say("\n## impulse_Cl against Cl after the first period ('f64'; a reported figure, not a bound)")
say("case                 dt          steps   max |Cl|   max |diff|   rms diff")
period_c1 = 2 * np.pi / (0.2 * np.pi)                              # f = k U / (2 pi c) with k = 0.2 pi: T = 10
k_pl, h_pl = 1.5, 0.25
period_pl = 2 * np.pi / k_pl
for name, base, period in (("config 1", dict(CONFIG1), period_c1),
                           ("plunging k=1.5 h=0.25", dict(CONFIG1, alpha_max=0, h_max=h_pl, k=k_pl, dt=period_pl / 200, tf=4 * period_pl - 0.5 * period_pl / 200),
                            period_pl)):
    for div in (1, 2):
        kwc = dict(base, dt=base["dt"] / div, precision="f64", history="sparse")
        sim = timed(kwc, wake_integrals=True)[1]
        first = int(round(period / kwc["dt"]))
        d = (sim.impulse_Cl - sim.Cl)[first:]
        say(f"{name:<20} {kwc['dt']:<10.5g}  {sim.nt - 1:<6d}  {np.abs(sim.Cl[first:]).max():8.3f}   {np.abs(d).max():9.4f}   {np.sqrt((d * d).mean()):9.4f}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
