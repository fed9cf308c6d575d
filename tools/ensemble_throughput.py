#!/usr/bin/env python3
"""Throughput of `sweep` (many small simulations in one device launch) on one MI355X, against running the members in turn:
    python tools/ensemble_throughput.py [--sizes 1 16 64 256 1024 4096] [--mixed 1024] > profiles/ensemble_throughput.txt
For B copies of config 1 (the README case: 400 steps) and for a mixed sweep (the 12-member grid of tests/test_gpu_ensemble.py
repeated): wall time of `sweep` split into host packing / device call (host clock around the synchronous ludvm_ensemble_run:
uploads, ONE kernel, downloads) / host unpacking; member-steps and pairs per second of the device call; and B x the solo
`time_loop` time (march, float64, sparse history; geometry and kinematics excluded) measured in the same command, the two
alternated.  Every shape is warmed up first; a small B is repeated inside a timed window until the window is about a second;
min and median over the repetitions.  The profiler is off (kernel time: tools/profile_cmd.sh on this script with --sizes 256).

    python tools/ensemble_throughput.py --probes-leg [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_probes_cost.txt
What velocity probes in a sweep cost: the device call of 256 copies of config 1, packed once, without probes on
this build and -- with --parent-lib, a build of the commit before the probes (tools/build_variant.sh) -- on that one, the
two alternated in one process; then with a rake of P = 64 and of P = 1024 points in the tunnel frame (P = 1024: 128 copies,
and 128 copies without probes beside them -- the probe rows of 256 would be over the 1 GiB one call returns).  Kernel time is
not in this output: rocprofv3 --kernel-trace --stats on this command with --reps 2 --window 0.1 names the two
instantiations (and the parent's kernel) apart.

    python tools/ensemble_throughput.py --particles-leg [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_tracers_cost.txt
What passive tracers in a sweep cost: the same device call of 256 copies of config 1 without tracers on this
build and on the parent build, alternated; then with M = 256 and M = 4096 tracers (a rake in the tunnel frame, all released
at step 1, the last step recorded).

    python tools/ensemble_throughput.py --survey-leg [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_survey_cost.txt
What a wake survey in a sweep costs: the same device call of 256 copies of config 1 without a survey on this
build and on the parent build, alternated; then with K = 256 and K = 4096 survey points (a rake in the tunnel frame, every
step sampled), and the probe phase on the K = 256 rake beside them.

    python tools/ensemble_throughput.py --survey-leg --bins 8 [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_survey_bins_cost.txt
What the bins of a survey in a sweep cost: the surveyed device call of 256 copies of config 1 at K = 256 and K =
4096 (every step sampled) on the parent build and on this one, alternated -- the same kernels -- and, on this build, the same
call with every step in one of B phase bins of the stroke (ludvm_ensemble_run_surveyed_binned): the added time per sampled step,
and beside it the call with ONE bin -- the same updates in the kernel, B times less to clear and to copy back.

    python tools/ensemble_throughput.py --survey-leg --grad [--bins 8] [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_survey_grad_cost.txt
What the gradient sums of a survey in a sweep cost: the unsurveyed and the surveyed device call of 256 copies of
config 1 at K = 256 and K = 4096 (every step sampled) on the parent build and on this one, alternated -- the same kernels --
and, on this build, the same call with the gradient sums (ludvm_ensemble_run_surveyed_graded): per call, per sampled step, and
the survey phase alone (the call less the unsurveyed call) against the plain survey phase.  With --bins B also the binned call
and the graded call with every step in one of B phase bins.

    python tools/ensemble_throughput.py --integrals-leg [--parent-lib _ab/libludvm_hip_parent.so] > profiles/ensemble_integrals_cost.txt
What the wake integrals of a sweep cost: the device call of 256 copies of config 1, packed once, (a) without
integrals on the parent build and on this one, alternated -- the same kernel --, (b) with the moments of every step
(ludvm_ensemble_run_integrals): the added time per member-step, and (c) with the energy sampled every 10th step beside them: the
added time per sample, and pairs per second of the one-workgroup psi walk against the solo march_energy_partial figure of DESIGN
4.22 (3.8e11 pairs/s)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[1, 16, 64, 256, 1024, 4096])
ap.add_argument("--mixed", type=int, default=1024, help="members of the mixed sweep (0: skip)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window should last")
ap.add_argument("--probes-leg", action="store_true", help="the cost of probes in a sweep instead of the size ladder")
ap.add_argument("--particles-leg", action="store_true", help="the cost of passive tracers in a sweep instead of the size ladder")
ap.add_argument("--survey-leg", action="store_true", help="the cost of a wake survey in a sweep instead of the size ladder")
ap.add_argument("--bins", type=int, default=0, help="survey leg: the cost of B phase bins over the plain survey instead (0: the plain leg)")
ap.add_argument("--grad", action="store_true", help="survey leg: the cost of the gradient sums over the plain (and, with --bins, the binned) survey instead")
ap.add_argument("--integrals-leg", action="store_true", help="the cost of the wake integrals in a sweep instead of the size ladder")
ap.add_argument("--parent-lib", default="", help="probes / particles / survey leg: a build of the parent commit, timed beside this one")
a = ap.parse_args()

from ludvm_amd import LUDVM, Engine, sweep  # noqa: E402

CONFIG1 = dict(t0=0, tf=20, dt=5e-2, chord=1, rho=1.225, Uinf=1, Npoints=81, Ncoeffs=30, LESPcrit=0.2, Naca="0012")
GRID = [dict(LESPcrit=l, alpha_max=am) for l in (0.1, 0.2, 0.3, 10) for am in (10, 20)] \
    + [dict(dt=2.5e-2), dict(k=0.4 * np.pi), dict(Naca="2412"), dict(method="Ramesh")]

eng = Engine(0)
info = eng.device_info()
print(f"# device: {info['name']}, {info['cu_count']} CUs, nominal clock {info['clock_khz'] / 1e3:.0f} MHz (the device's own figure; "
      "the clock held during the run was not read)")
print("# times in ms; min / median over the repetitions; 'in turn' = B x one solo time_loop measured beside it")

marks = {}
inner = eng.ensemble_run


def timed(*args, **kw):
    marks["enter"] = time.perf_counter()
    out = inner(*args, **kw)
    marks["exit"] = time.perf_counter()
    return out


eng.ensemble_run = timed


def pairs_of(sim):
    """Pairs a member evaluates: per step (npan + 1) targets x the wake before the solve, then the wake after it x (itself +
    the npan bound vortices)."""
    npan, nf = sim.Npoints - 1, sim.n_freevort
    shed = (sim.LEV_shed[1:] != -1).astype(np.int64)
    before = nf + np.arange(sim.nt - 1) + np.concatenate([[0], np.cumsum(shed)[:-1]])
    after = before + 1 + shed
    return int(((npan + 1) * before + after * (after + npan)).sum())


def one_sweep(cases):
    t0 = time.perf_counter()
    sims = sweep(cases, engine=eng)
    t1 = time.perf_counter()
    return sims, (marks["enter"] - t0, marks["exit"] - marks["enter"], t1 - marks["exit"])


def solo_time_loop(kw):
    s = LUDVM(**kw, verbose=False, engine=eng, precision="f64", history="sparse", run=False)
    t0 = time.perf_counter()
    s.time_loop()
    return time.perf_counter() - t0


def measure(label, cases, solo_cases):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sims, first = one_sweep(cases)                    # warm-up of this shape (buffers grow here)
        for kw in solo_cases:
            solo_time_loop(kw)
        inner_reps = max(1, int(a.window / max(sum(first), 1e-4)))
        steps = sum(s.nt - 1 for s in sims)
        pairs = sum(pairs_of(s) for s in sims)
        T, solo = [], []
        for _ in range(a.reps):                           # sweep and solo runs alternated
            acc = np.zeros(3)
            for _ in range(inner_reps):
                acc += one_sweep(cases)[1]
            T.append(acc / inner_reps)
            solo.append(sum(solo_time_loop(kw) for kw in solo_cases) * (len(cases) / len(solo_cases)))
    T, solo = np.array(T) * 1e3, np.array(solo) * 1e3
    wall = T.sum(axis=1)
    dev = T[:, 1]
    print(f"{label:<22} members {len(cases):5d}  steps {steps:8d}  pairs {pairs:.3e}  windows of {inner_reps} sweep(s)\n"
          f"    pack   {T[:, 0].min():10.2f} / {np.median(T[:, 0]):10.2f}\n"
          f"    device {dev.min():10.2f} / {np.median(dev):10.2f}   {steps / dev.min() * 1e3:.3e} member-steps/s  "
          f"{pairs / dev.min() * 1e3:.3e} pairs/s\n"
          f"    unpack {T[:, 2].min():10.2f} / {np.median(T[:, 2]):10.2f}\n"
          f"    sweep  {wall.min():10.2f} / {np.median(wall):10.2f}\n"
          f"    in turn {solo.min():9.2f} / {np.median(solo):10.2f}   device call {solo.min() / dev.min():.1f}x faster, "
          f"whole sweep {solo.min() / wall.min():.1f}x", flush=True)


def probes_leg():
    """Device call only: the members are packed once (what `sweep` hands the engine is kept) and the call is repeated."""
    import torch
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = {B: sweep([dict(CONFIG1)] * B, engine=eng) for B in (256, 128)}
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))

    def variant(which, B, P):
        e, packed = engines[which], kept[B]
        if P == 0:
            return lambda: e.ensemble_run(*packed)
        # a rake behind the foil in the frame of the pivot, P points over z in [-2, 2]
        px, pz = np.full(P, 2.0), np.linspace(-2.0, 2.0, P)
        shift = np.concatenate([s.xpiv for s in sims[B]])
        return lambda: e.ensemble_run_probed(*packed, probe_x=px, probe_z=pz, shift_x=shift)
    order = ([("parent build", 256, 0)] if a.parent_lib else []) + [("this build", 256, 0), ("this build", 256, 64),
                                                                    ("this build", 128, 0), ("this build", 128, 1024)]
    calls = {v: variant(*v) for v in order}
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print("# probes leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of B copies\n"
          "# of config 1 packed once; ms per call, min / median / max over the windows and the build's own spread (max - min) / min")
    base = {}
    for v in order:
        which, B, P = v
        t = np.array(T[v])
        s1 = sims[B][0]
        steps = B * (s1.nt - 1)
        line = (f"{which:<13} B {B:4d}  P {P:5d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if P == 0:
            base[(which, B)] = t
        else:
            # sources a probe sees in step s: the wake after the solve + the bound vortices
            shed = (s1.LEV_shed[1:] != -1).astype(np.int64)
            nsrc = s1.n_freevort + np.arange(1, s1.nt) + np.cumsum(shed) + s1.Npoints - 1
            pairs = B * P * int(nsrc.sum() + s1.n_freevort)
            added = np.median(t) - np.median(base[(which, B)])
            line += (f"\n{'':13} added {added:9.3f} ms per call = {added / (s1.nt - 1) * 1e3:8.3f} us per step (of every member, side by "
                     f"side); {pairs:.3e} probe pairs, {pairs / (added * 1e-3):.3e} pairs/s of the added time; roll-up pairs of the "
                     f"call {B * pairs_of(s1):.3e}: P / mean wake size = {P / (nsrc.mean() - s1.Npoints + 1):.2f}")
            # the return copy alone: two arrays of [rows of kin, P] doubles, device -> pageable host memory
            n = B * s1.nt * P
            d = torch.empty(n, dtype=torch.float64, device="cuda")
            h = [np.empty(n), np.empty(n)]
            cp = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(2):
                    torch.from_numpy(h[k]).copy_(d)
                torch.cuda.synchronize()
                cp.append((time.perf_counter() - t0) * 1e3)
            line += f"\n{'':13} return copy of the probe rows alone ({2 * n * 8 / 2**20:.1f} MiB, device -> pageable host): {min(cp[1:]):9.3f} ms"
        print(line, flush=True)
    if a.parent_lib:
        p, n = base[("parent build", 256)], base[("this build", 256)]
        print(f"unprobed device call, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the parent's own windows "
              f"span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
              f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")


def particles_leg():
    """Device call only, like the probes leg: B = 256 copies of config 1 packed once, the call repeated."""
    B = 256
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = sweep([dict(CONFIG1)] * B, engine=eng)
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))
    packed, s1 = kept[B], sims[0]
    shift = np.concatenate([s.xpiv for s in sims])

    def variant(which, M):
        e = engines[which]
        if M == 0:
            return lambda: e.ensemble_run(*packed)
        # a rake behind the foil in the frame of the pivot, M seeds over z in [-2, 2], free from step 1
        sx, sz = np.full(M, 2.0), np.linspace(-2.0, 2.0, M)
        return lambda: e.ensemble_run_traced(*packed, seed_x=sx, seed_z=sz, release=np.ones(M, dtype=np.int64), shift_x=shift)
    order = ([("parent build", 0)] if a.parent_lib else []) + [("this build", 0), ("this build", 256), ("this build", 4096)]
    calls = {v: variant(*v) for v in order}
    # beside them, in the same windows: the probe phase on the same rake (P = 256: 420 MB of probe rows)
    px, pz = np.full(256, 2.0), np.linspace(-2.0, 2.0, 256)
    order.append(("probes", 256))
    calls[("probes", 256)] = lambda: eng.ensemble_run_probed(*packed, probe_x=px, probe_z=pz, shift_x=shift)
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print("# particles leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of 256 copies\n"
          "# of config 1 packed once; ms per call, min / median / max over the windows and the build's own spread (max - min) / min")
    base = {}
    for v in order:
        which, M = v
        t = np.array(T[v])
        if which == "probes":
            nsrc = s1.n_freevort + np.arange(1, s1.nt) + np.cumsum((s1.LEV_shed[1:] != -1).astype(np.int64)) + s1.Npoints - 1
            pairs = B * M * int(nsrc.sum() + s1.n_freevort)
            added = np.median(t) - np.median(base["this build"])
            print(f"{'this build':<13} B {B:4d}  P {M:5d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                  f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %\n{'':13} the probe phase on the same rake: added "
                  f"{added:9.3f} ms per call = {added / (s1.nt - 1) * 1e3:8.3f} us per step; {pairs:.3e} probe pairs, "
                  f"{pairs / (added * 1e-3):.3e} pairs/s of the added time, which holds the clearing and the return copy of "
                  f"{2 * B * s1.nt * M * 8 / 2**20:.1f} MiB of probe rows (tracers return {B * 2 * M * 8 / 2**20:.1f} MiB)", flush=True)
            continue
        line = (f"{which:<13} B {B:4d}  M {M:5d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if M == 0:
            base[which] = t
        else:
            # sources a tracer sees in step s: the wake after the solve + the bound vortices
            shed = (s1.LEV_shed[1:] != -1).astype(np.int64)
            nsrc = s1.n_freevort + np.arange(1, s1.nt) + np.cumsum(shed) + s1.Npoints - 1
            pairs = B * M * int(nsrc.sum())
            added = np.median(t) - np.median(base[which])
            line += (f"\n{'':13} added {added:9.3f} ms per call = {added / (s1.nt - 1) * 1e3:8.3f} us per step (of every member, side by "
                     f"side); {pairs:.3e} tracer pairs, {pairs / (added * 1e-3):.3e} pairs/s of the added time (the probe phase: 1.65-1.7e11); "
                     f"roll-up pairs of the call {B * pairs_of(s1):.3e}: M / mean wake size = {M / (nsrc.mean() - s1.Npoints + 1):.2f}")
        print(line, flush=True)
    if a.parent_lib:
        p, n = base["parent build"], base["this build"]
        print(f"untraced device call, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the parent's own windows "
              f"span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
              f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")
    else:
        print("untraced device call against the parent build: NOT MEASURED (no --parent-lib given)")


def survey_leg():
    """Device call only, like the probes leg: B = 256 copies of config 1 packed once, the call repeated."""
    B = 256
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = sweep([dict(CONFIG1)] * B, engine=eng)
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))
    packed, s1 = kept[B], sims[0]
    shift = np.concatenate([s.xpiv for s in sims])

    def variant(which, K):
        e = engines[which]
        if K == 0:
            return lambda: e.ensemble_run(*packed)
        # a rake behind the foil in the frame of the pivot, K points over z in [-2, 2], every step sampled
        vx, vz = np.full(K, 2.0), np.linspace(-2.0, 2.0, K)
        return lambda: e.ensemble_run_surveyed(*packed, survey_x=vx, survey_z=vz, survey_steps=(1, 1 << 62, 1), survey_shift_x=shift)
    order = ([("parent build", 0)] if a.parent_lib else []) + [("this build", 0), ("this build", 256), ("this build", 4096)]
    calls = {v: variant(*v) for v in order}
    # beside them, in the same windows: the probe phase on the same rake (P = 256: 420 MB of probe rows)
    px, pz = np.full(256, 2.0), np.linspace(-2.0, 2.0, 256)
    order.append(("probes", 256))
    calls[("probes", 256)] = lambda: eng.ensemble_run_probed(*packed, probe_x=px, probe_z=pz, shift_x=shift)
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print("# survey leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of 256 copies\n"
          "# of config 1 packed once; ms per call, min / median / max over the windows and the build's own spread (max - min) / min")
    base = {}
    # sources a point sees in step s: the wake after the solve + the bound vortices
    nsrc = s1.n_freevort + np.arange(1, s1.nt) + np.cumsum((s1.LEV_shed[1:] != -1).astype(np.int64)) + s1.Npoints - 1
    for v in order:
        which, K = v
        t = np.array(T[v])
        if which == "probes":
            pairs = B * K * int(nsrc.sum() + s1.n_freevort)
            added = np.median(t) - np.median(base["this build"])
            print(f"{'this build':<13} B {B:4d}  P {K:5d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                  f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %\n{'':13} the probe phase on the same rake: added "
                  f"{added:9.3f} ms per call = {added / (s1.nt - 1) * 1e3:8.3f} us per step; {pairs:.3e} probe pairs, "
                  f"{pairs / (added * 1e-3):.3e} pairs/s of the added time, which holds the clearing and the return copy of "
                  f"{2 * B * s1.nt * K * 8 / 2**20:.1f} MiB of probe rows (the survey returns {B * 5 * K * 8 / 2**20:.1f} MiB)", flush=True)
            continue
        line = (f"{which:<13} B {B:4d}  K {K:5d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if K == 0:
            base[which] = t
        else:
            pairs = B * K * int(nsrc.sum())
            added = np.median(t) - np.median(base[which])
            line += (f"\n{'':13} added {added:9.3f} ms per call = {added / (s1.nt - 1) * 1e3:8.3f} us per sampled step (of every member, "
                     f"side by side); {pairs:.3e} survey pairs, {pairs / (added * 1e-3):.3e} pairs/s of the added time (the probe phase: "
                     f"1.65-1.7e11); sums returned {B * 5 * K * 8 / 2**20:.1f} MiB; roll-up pairs of the call {B * pairs_of(s1):.3e}: "
                     f"K / mean wake size = {K / (nsrc.mean() - s1.Npoints + 1):.2f}")
        print(line, flush=True)
    if a.parent_lib:
        p, n = base["parent build"], base["this build"]
        print(f"unsurveyed device call, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the parent's own "
              f"windows span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
              f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")
    else:
        print("unsurveyed device call against the parent build: NOT MEASURED (no --parent-lib given)")


def survey_bins_leg(nbins):
    """Device call only, like the survey leg: B = 256 copies of config 1 packed once; the surveyed call with and without bins."""
    B = 256
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = sweep([dict(CONFIG1)] * B, engine=eng)
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))
    packed, s1 = kept[B], sims[0]
    shift = np.concatenate([s.xpiv for s in sims])
    # the phase bin of every step of config 1 (200 steps per period), the table `sweep(..., survey_phases=nbins)` builds
    steps_per_period = int(round(1.0 / s1.f / s1.dt))
    table = np.tile((np.arange(s1.nt) % steps_per_period) * nbins // steps_per_period, B)

    def variant(which, K, bins):
        e = engines[which]
        vx, vz = np.full(K, 2.0), np.linspace(-2.0, 2.0, K)
        kw = dict(survey_x=vx, survey_z=vz, survey_steps=(1, 1 << 62, 1), survey_shift_x=shift)
        if bins:
            # (one bin: the same ten memory operations per point and step, an eighth of the sums cleared and returned)
            tb = table if bins > 1 else np.zeros_like(table)
            return lambda: e.ensemble_run_surveyed_binned(*packed, **kw, bin_of_step=tb, nbins=bins)
        return lambda: e.ensemble_run_surveyed(*packed, **kw)
    order = []
    for K in (256, 4096):
        order += ([("parent build", K, 0)] if a.parent_lib else []) + [("this build", K, 0), ("this build", K, nbins)]
        if nbins > 1:
            order.append(("this build", K, 1))
    calls = {v: variant(*v) for v in order}
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print(f"# survey bins leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of 256 copies\n"
          f"# of config 1 packed once, a survey of K points with every step sampled, without bins and with every step in one of {nbins} bins;\n"
          "# ms per call, min / median / max over the windows and the build's own spread (max - min) / min")
    nsrc = s1.n_freevort + np.arange(1, s1.nt) + np.cumsum((s1.LEV_shed[1:] != -1).astype(np.int64)) + s1.Npoints - 1
    for v in order:
        which, K, bins = v
        t = np.array(T[v])
        line = (f"{which:<13} B {B:4d}  K {K:5d}  bins {bins:2d}  windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / "
                f"{t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if bins:
            base = np.array(T[(which, K, 0)])
            added = np.median(t) - np.median(base)
            line += (f"\n{'':13} added over the plain survey {added:9.3f} ms per call ({added / np.median(base) * 100:+.2f} % of it; the plain "
                     f"survey's own windows span {(base.max() - base.min()) / base.min() * 100:.2f} %) = {added / (s1.nt - 1) * 1e3:8.3f} us per "
                     f"sampled step (of every member, side by side); {B * K * (s1.nt - 1) * 10:.3e} more memory operations against "
                     f"{B * K * int(nsrc.sum()):.3e} survey pairs; bin sums returned {B * bins * 5 * K * 8 / 2**20:.1f} MiB beside "
                     f"{B * 5 * K * 8 / 2**20:.1f} MiB of plain sums")
        print(line, flush=True)
    for K in (256, 4096):
        if a.parent_lib:
            p, n = np.array(T[("parent build", K, 0)]), np.array(T[("this build", K, 0)])
            print(f"plain surveyed device call at K = {K}, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the "
                  f"parent's own windows span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
                  f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")
        else:
            print(f"plain surveyed device call at K = {K} against the parent build: NOT MEASURED (no --parent-lib given)")


def survey_grad_leg(nbins):
    """Device call only, like the survey leg: B = 256 copies of config 1 packed once; unsurveyed, surveyed (binned) and graded."""
    B = 256
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = sweep([dict(CONFIG1)] * B, engine=eng)
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))
    packed, s1 = kept[B], sims[0]
    shift = np.concatenate([s.xpiv for s in sims])
    steps_per_period = int(round(1.0 / s1.f / s1.dt))
    table = np.tile((np.arange(s1.nt) % steps_per_period) * max(nbins, 1) // steps_per_period, B)

    def variant(which, K, bins, grad):
        e = engines[which]
        if K == 0:
            return lambda: e.ensemble_run(*packed)
        vx, vz = np.full(K, 2.0), np.linspace(-2.0, 2.0, K)
        kw = dict(survey_x=vx, survey_z=vz, survey_steps=(1, 1 << 62, 1), survey_shift_x=shift)
        if bins:
            kw.update(bin_of_step=table, nbins=bins)
        if grad:
            return lambda: e.ensemble_run_surveyed_graded(*packed, **kw)
        if bins:
            return lambda: e.ensemble_run_surveyed_binned(*packed, **kw)
        return lambda: e.ensemble_run_surveyed(*packed, **kw)
    builds = (["parent build"] if a.parent_lib else []) + ["this build"]
    order = [(w, 0, 0, False) for w in builds]
    for K in (256, 4096):
        for bins in ([0, nbins] if nbins else [0]):
            order += [(w, K, bins, False) for w in builds] + [("this build", K, bins, True)]
    calls = {v: variant(*v) for v in order}
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print("# survey gradient leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of 256\n"
          "# copies of config 1 packed once, a survey of K points with every step sampled: without a survey (K 0), plain, and with the\n"
          "# gradient sums (grad); ms per call, min / median / max over the windows and the build's own spread (max - min) / min")
    none = np.median(T[("this build", 0, 0, False)])
    for v in order:
        which, K, bins, grad = v
        t = np.array(T[v])
        line = (f"{which:<13} B {B:4d}  K {K:5d}  bins {bins:2d}  {'grad ' if grad else 'plain'}  windows of {reps_in[v]:3d}  device call "
                f"{t.min():9.3f} / {np.median(t):9.3f} / {t.max():9.3f}  spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if grad:
            base = np.array(T[(which, K, bins, False)])
            added = np.median(t) - np.median(base)
            line += (f"\n{'':13} over the {'binned' if bins else 'plain'} survey call of this build: {np.median(t) / np.median(base):.4f} x per call, "
                     f"added {added:9.3f} ms = {added / (s1.nt - 1) * 1e3:8.3f} us per sampled step (of every member, side by side); the survey "
                     f"phase alone (call less the unsurveyed call, {none:.3f} ms): {(np.median(t) - none) / (np.median(base) - none):.4f} x "
                     f"(expected from the solo route's pair phase: 1.59-1.63); sums returned "
                     f"{B * (bins + 1) * 10 * K * 8 / 2**20:.1f} MiB against {B * (bins + 1) * 5 * K * 8 / 2**20:.1f} MiB")
        print(line, flush=True)
    for v in order:
        which, K, bins, grad = v
        if which != "this build" or grad:
            continue
        name = "unsurveyed" if K == 0 else f"{'binned' if bins else 'plain'} surveyed (K = {K})"
        if a.parent_lib:
            p, n = np.array(T[("parent build", K, bins, False)]), np.array(T[v])
            print(f"{name} device call, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the parent's own "
                  f"windows span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
                  f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")
        else:
            print(f"{name} device call against the parent build: NOT MEASURED (no --parent-lib given)")


def integrals_leg():
    """Device call only: B = 256 copies of config 1 packed once; plain (both builds), with the moments, with moments and energy."""
    B = 256
    kept = {}
    plain_call = inner

    def keep(*args, **kw):
        kept[len(args[7])] = args
        return plain_call(*args, **kw)
    eng.ensemble_run = keep
    sims = sweep([dict(CONFIG1)] * B, engine=eng)
    del eng.ensemble_run
    engines = {"this build": eng}
    if a.parent_lib:
        engines["parent build"] = Engine(0, lib_path=os.path.abspath(a.parent_lib))
    packed, s1 = kept[B], sims[0]
    win = (1, s1.nt, 10)
    sampled = np.arange(win[0], s1.nt, win[2])
    ns = s1.n_freevort + np.arange(s1.nt) + np.cumsum(s1.LEV_shed != -1) + (s1.Npoints - 1)       # sources behind step i's solve
    pairs = int((ns[sampled].astype(np.int64) ** 2).sum())

    def variant(which, kind):
        e = engines[which]
        if kind == "plain":
            return lambda: e.ensemble_run(*packed)
        return lambda: e.ensemble_run_integrals(*packed, energy_steps=win if kind == "energy" else None)
    builds = (["parent build"] if a.parent_lib else []) + ["this build"]
    order = [(w, "plain") for w in builds] + [("this build", "moments"), ("this build", "energy")]
    calls = {v: variant(*v) for v in order}
    reps_in = {}
    for v, f in calls.items():                        # warm-up of every shape (buffers grow here)
        f()
        t0 = time.perf_counter()
        f()
        reps_in[v] = max(1, int(a.window / (time.perf_counter() - t0)))
    T = {v: [] for v in order}
    for _ in range(a.reps):                           # the variants alternated
        for v, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps_in[v]):
                f()
            T[v].append((time.perf_counter() - t0) / reps_in[v] * 1e3)
    print("# integrals leg: device call (host clock around the synchronous entry point: uploads, ONE kernel, downloads) of 256 copies\n"
          "# of config 1 packed once: plain, with the moments of every step, and with the energy every 10th step as well; ms per call,\n"
          "# min / median / max over the windows and the build's own spread (max - min) / min")
    base = np.median(T[("this build", "plain")])
    mom = np.median(T[("this build", "moments")])
    for v in order:
        which, kind = v
        t = np.array(T[v])
        line = (f"{which:<13} B {B:4d}  {kind:<8} windows of {reps_in[v]:3d}  device call {t.min():9.3f} / {np.median(t):9.3f} / {t.max():9.3f}  "
                f"spread {(t.max() - t.min()) / t.min() * 100:5.2f} %")
        if kind == "moments":
            added = np.median(t) - base
            line += (f"\n{'':13} over the plain call of this build: {np.median(t) / base:.4f} x per call, added {added:9.3f} ms = "
                     f"{added / (s1.nt - 1) * 1e3:8.3f} us per step (of every member, side by side) = "
                     f"{added / (B * (s1.nt - 1)) * 1e6:8.3f} ns per member-step; rows returned {B * s1.nt * 48 * 8 / 2**20:.1f} MiB")
        if kind == "energy":
            added = np.median(t) - mom
            line += (f"\n{'':13} over the call with the moments: {np.median(t) / mom:.4f} x per call, added {added:9.3f} ms for {len(sampled)} "
                     f"samples of every member (sources {ns[sampled].min()} .. {ns[sampled].max()}) = {added / len(sampled) * 1e3:8.3f} us per "
                     f"sample (of every member, side by side); {pairs} pairs per member, {B * pairs / (added * 1e-3):.3e} pairs/s over "
                     f"{B} workgroups on {info['cu_count']} CUs, against 3.8e11 of the solo march_energy_partial (DESIGN 4.22): "
                     f"{B * pairs / (added * 1e-3) / 3.8e11:.3f} x")
        print(line, flush=True)
    if a.parent_lib:
        p, n = np.array(T[("parent build", "plain")]), np.array(T[("this build", "plain")])
        print(f"plain device call, this build against the parent build: median {np.median(n) / np.median(p):.4f} x; the parent's own windows "
              f"span {p.min():.3f} .. {p.max():.3f} ms, this build's {n.min():.3f} .. {n.max():.3f} ms: "
              f"{'inside' if p.min() <= np.median(n) <= p.max() else 'OUTSIDE'} the parent's run-to-run spread")
    else:
        print("plain device call against the parent build: NOT MEASURED (no --parent-lib given)")


if a.integrals_leg:
    eng.ensemble_run = inner
    integrals_leg()
    sys.exit(0)
if a.survey_leg:
    eng.ensemble_run = inner
    if a.grad:
        survey_grad_leg(a.bins)
    elif a.bins:
        survey_bins_leg(a.bins)
    else:
        survey_leg()
    sys.exit(0)
if a.particles_leg:
    eng.ensemble_run = inner
    particles_leg()
    sys.exit(0)
if a.probes_leg:
    eng.ensemble_run = inner
    probes_leg()
    sys.exit(0)
for B in a.sizes:
    measure(f"config 1 x {B}", [dict(CONFIG1)] * B, [dict(CONFIG1)])
if a.mixed:
    cases = [dict(CONFIG1, **GRID[q % len(GRID)]) for q in range(a.mixed)]
    measure(f"mixed grid x {a.mixed}", cases, [dict(CONFIG1, **g) for g in GRID])
