#!/usr/bin/env python3
"""Forward-time FTLE field of the README case's wake, and a Q snapshot beside it.

A mesh of passive tracers is released behind the plunging foil (tunnel frame: the mesh rides with the pivot until its release)
and every tracer carries the deformation gradient F of its own path through the device-resident march (tracer_gradient=True; --f32x2: 'f32x2'):
no neighbouring paths are differenced, so the field does not saturate once neighbours separate.  The finite-time Lyapunov
exponent ln sigma_max(F) / T over the rest of the run is printed as its ridge -- for every mesh column the height of the largest
exponent: the material lines that bound the wake vortices -- and the Q / Okubo-Weiss field `q_ff` = -ux^2 - uz wx of the same
window at the release step shows the cores (Q > 0) and the shear layers (Q < 0) the Eulerian way.

    python examples/ftle_field.py [--tf 20] [--dt 5e-2] [--release-at 0.5] [--dr 0.05] [--plot out.png]
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
ap.add_argument("--release-at", type=float, default=0.5, help="fraction of the run after which the mesh is released")
ap.add_argument("--dr", type=float, default=0.05, help="spacing of the tracer mesh")
ap.add_argument("--f32x2", action="store_true", help="hi+lo fp32 pair sums: the marched tracer mesh on tracer_precision='f32x2', tracer_gradient='f32x2', "
                "and the Q snapshot's gradient sums with field_precision='f32x2'")
ap.add_argument("--plot", default=None, help="write the FTLE field and the Q snapshot to this PNG")
args = ap.parse_args()

nt = len(np.arange(0, args.tf + args.dt, args.dt))
release = max(2, int(args.release_at * (nt - 1)))
# the mesh, x measured from the pivot: from the trailing edge to five chords behind it
x1, z1 = np.arange(0.8, 5.8, args.dr), np.arange(-2.0, 2.0, args.dr)
X, Z = np.meshgrid(x1, z1, indexing="ij")
M = X.size
sim = LUDVM(t0=0, tf=args.tf, dt=args.dt, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012",
            verbose=False, tracers=np.stack([X.ravel(), Z.ravel()]), tracer_release=np.full(M, release), tracer_frame="tunnel",
            **(dict(tracer_precision="f32x2", tracer_gradient="f32x2") if args.f32x2 else dict(tracer_gradient=True)))
last = sim.nt - 1
T = sim.dt * (last - release + 1)
ftle = sim.tracer_ftle().reshape(X.shape)
print(f"{M} tracers ({len(x1)} x {len(z1)}) released at step {release} of {last}; forward time T = {T:.2f}")
print(f"FTLE in [{ftle.min():+.3f}, {ftle.max():+.3f}]")
print("ridge (x behind the pivot at release, z of the largest exponent, its value):")
for i in range(0, len(x1), max(1, len(x1) // 20)):
    j = int(np.argmax(ftle[i]))
    print(f"  x = {x1[i]:5.2f}   z = {z1[j]:+5.2f}   FTLE = {ftle[i, j]:.3f}")

# the Eulerian reading of the same window at the release step
x0 = sim.xpiv[release]
window = dict(xmin=x0 + x1[0], xmax=x0 + x1[-1] + args.dr / 2, zmin=z1[0], zmax=z1[-1] + args.dr / 2)
sim.flowfield(**window, dr=args.dr, tsteps=[release], grad=True, field_precision="f32x2" if args.f32x2 else "f64")
q = sim.q_ff[0]
print(f"Q at step {release}: in [{q.min():+.2f}, {q.max():+.2f}]; {100 * (q > 0).mean():.1f} % of the window rotation-dominated")

if args.plot:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(2, 1, figsize=(10, 7))
    ax[0].pcolormesh(X, Z, ftle, shading="auto")
    ax[0].set_title(f"forward FTLE over T = {T:.2f} (seeds, pivot frame at release)")
    ax[1].pcolormesh(sim.x_ff - x0, sim.z_ff, np.sign(q) * np.sqrt(np.abs(q)), shading="auto", cmap="RdBu_r")
    ax[1].set_title(f"sign(Q) sqrt|Q| at step {release}")
    for a in ax:
        a.set_aspect("equal")
    fig.tight_layout()
    fig.savefig(args.plot, dpi=120)
    print("wrote", args.plot)
