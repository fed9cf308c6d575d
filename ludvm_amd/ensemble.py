"""`sweep`: many small LUDVM simulations in ONE device launch (Engine.ensemble_run / ludvm_ensemble_run; with velocity probes
Engine.ensemble_run_probed / ludvm_ensemble_run_probed; with passive tracers Engine.ensemble_run_traced /
ludvm_ensemble_run_traced; with a wake survey Engine.ensemble_run_surveyed / ludvm_ensemble_run_surveyed; with a phase-locked
one Engine.ensemble_run_surveyed_binned / ludvm_ensemble_run_surveyed_binned; with the survey's gradient sums
Engine.ensemble_run_surveyed_graded / ludvm_ensemble_run_surveyed_graded; with wake integrals Engine.ensemble_run_integrals /
ludvm_ensemble_run_integrals).

A reduced-order model is run many times -- calibrate LESPcrit, sweep k, alpha_max, phi, dt, move a gust vortex, switch
'Faure' / 'Ramesh'.  Each such run on its own is a chain of tiny dependent launches that leaves the GPU idle; the members of
a sweep are independent, so the engine gives each a workgroup of its own and runs its whole time loop inside one kernel
(ludvm_amd/csrc/ensemble_kernels.hpp).

    from ludvm_amd import sweep
    sims = sweep([dict(LESPcrit=l, alpha_max=a) for l in (0.1, 0.2, 0.3) for a in (10, 20)], tf=6, verbose=False)
    print([s.Cl.mean() for s in sims])

Geometry and kinematics of every member come from the ordinary constructor (run=False); the tables a member hands the device
are the ones a solo march uploads (LUDVM._march_inputs) and its results are stored by the routine that stores a solo march's
(LUDVM._store_march_results).
"""
import numpy as np

from . import _ffi
from .ludvm import LUDVM, SparseHistory

__all__ = ["sweep"]

_BINS_SOLO = ("the bins of a sweep are common to it: sweep(cases, survey=..., survey_phases=...) -- survey_bins / survey_period / "
              "survey_phase0 belong to a solo run, LUDVM(..., survey=..., survey_bins=...)")

_INTEGRALS_SOLO = ("the wake integrals are a solo keyword: the integrals of a sweep are common to it -- sweep(cases, integrals=True, "
                   "energy_steps=...) (or run the member on its own, LUDVM(..., wake_integrals=True))")

_REFUSED = {
    # keyword -> (value that is fine, why not otherwise)
    "checkpoint_every": (0, "a sweep has no checkpoint / resume"),
    "checkpoint_path": (None, "a sweep has no checkpoint / resume"),
    "distributed": (None, "a sweep runs on one GPU (members are independent: split the list per device)"),
    "devices": (None, "a sweep runs on one GPU (members are independent: split the list per device)"),
    "march": (True, "the members of a sweep are marched on the device"),
    "run": (True, "the members of a sweep are run"),
    "tracers": (None, "the tracers of a sweep are common to it: sweep(cases, particles=[2, M], particle_release=..., "
                      "particle_frame=..., particle_steps=...) (or run the member on its own: LUDVM(..., tracers=...))"),
    "tracer_release": (None, "the tracers of a sweep are common to it: sweep(cases, particles=..., particle_release=...)"),
    "tracer_steps": (None, "the tracers of a sweep are common to it: sweep(cases, particles=..., particle_steps=...)"),
    "tracer_frame": ("lab", "the tracers of a sweep are common to it: sweep(cases, particles=..., particle_frame=...)"),
    "survey": (None, "the survey of a sweep is common to it: sweep(cases, survey=...)"),
    "survey_steps": (None, "the survey of a sweep is common to it: sweep(cases, survey=...)"),
    "survey_frame": ("lab", "the survey of a sweep is common to it: sweep(cases, survey=...)"),
    "survey_bins": (None, _BINS_SOLO),
    "survey_period": (None, _BINS_SOLO),
    "survey_phase0": (None, _BINS_SOLO),
}


class _RecordedWakes:
    """hist[r, 0 | 1] of LUDVM._store_march_results for a member: the wake's x / z after the steps the device recorded."""

    def __init__(self):
        self.rows = {}

    def __getitem__(self, key):
        r, k = key
        rec = self.rows.get(int(r))
        return None if rec is None else rec[k]


def _check_case(idx, kw, first):
    """Everything that can be refused from the keywords alone (no device, no engine call)."""
    who = f"sweep: member {idx}: "
    for key in ("engine", "device", "snapshot_steps", "verbose", "probes", "probe_frame", "particles", "particle_release",
                "particle_frame", "particle_steps", "survey_phases", "survey_grad", "integrals", "energy_steps"):
        if key in kw:
            raise ValueError(who + f"`{key}` belongs to the sweep, not to a member")
    if "survey_precision" in kw:
        raise ValueError(who + f"survey_precision={kw['survey_precision']!r}: the survey of a sweep is evaluated in float64 (fp32 "
                         "survey sums: run the member on its own, LUDVM(..., survey=..., survey_precision='f32'))")
    if "tracer_precision" in kw:
        raise ValueError(who + f"tracer_precision={kw['tracer_precision']!r}: the tracers of a sweep are advected in float64 (fp32 "
                         "tracer sums: run the member on its own, LUDVM(..., tracers=..., tracer_precision='f32x2'))")
    if "tracer_gradient" in kw:
        raise ValueError(who + f"tracer_gradient={kw['tracer_gradient']!r}: the tracers of a sweep carry no deformation gradient (run "
                         "the member on its own, LUDVM(..., tracers=..., tracer_gradient=True))")
    if "survey_gradient" in kw:
        raise ValueError(who + f"survey_gradient={kw['survey_gradient']!r}: the survey of a sweep carries no gradient sums (run the "
                         "member on its own, LUDVM(..., survey=..., survey_gradient=True))")
    for key in ("wake_integrals", "wake_energy_steps"):
        if key in kw:
            raise ValueError(who + f"{key}={kw[key]!r}: {_INTEGRALS_SOLO}")
    for key, (fine, why) in _REFUSED.items():
        if key in kw and not (kw[key] is fine or (fine is not None and kw[key] == fine)):
            raise ValueError(who + f"{key}={kw[key]!r}: {why}")
    if kw.get("precision", "auto") not in ("auto", "f64"):
        raise ValueError(who + f"precision={kw['precision']!r}: the members of a sweep run in float64 ('auto' or 'f64')")
    if kw.get("history", "auto") == "full":
        raise ValueError(who + "history='full': a sweep keeps rows at snapshot_steps and the last step only")
    if kw.get("method", "Faure") not in ("Faure", "Ramesh"):
        raise ValueError(who + "method must be 'Faure' or 'Ramesh'")
    npoints, ncoef = int(kw.get("Npoints", 80)), int(kw.get("Ncoeffs", 30))
    if npoints < 3:
        raise ValueError(who + f"Npoints={npoints}: a section has at least 3 points (2 panels)")
    if not (npoints - 1 <= 256 and 4 <= ncoef <= 64):
        raise ValueError(who + f"Npoints={npoints}, Ncoeffs={ncoef}: a sweep takes 3 <= Npoints <= 257 and 4 <= Ncoeffs <= 64")
    if first is not None and (npoints, ncoef) != first:
        raise ValueError(who + f"Npoints / Ncoeffs = {npoints} / {ncoef} differ from member 0's {first[0]} / {first[1]}: "
                         "they are common to a sweep")
    t0, tf, dt = kw.get("t0", 0), kw.get("tf", 12), kw.get("dt", 1.5e-2)
    nt = len(np.arange(t0, tf + dt, dt))
    g = kw.get("circulation_freevort")
    nf = len(g) if (g is not None and kw.get("xy_freevort") is not None) else 1
    if nt < 2:
        raise ValueError(who + "no time step to run")
    if nt - 1 > _ffi.ENSEMBLE_MAX_STEPS or nf + 2 * (nt - 1) > _ffi.ENSEMBLE_MAX_WAKE:
        raise ValueError(who + f"{nt - 1} steps / a wake of up to {nf + 2 * (nt - 1)} vortices is over the limits of a sweep member "
                         f"({_ffi.ENSEMBLE_MAX_STEPS} steps, {_ffi.ENSEMBLE_MAX_WAKE} vortices); it can be run on its own: LUDVM(...)")
    return npoints, ncoef


def _check_sweep_probes(probes, probe_frame, merged):
    """The sweep's probe points [2, P] (None: no probes), refused from the keywords alone like a member's."""
    if probes is None:
        if probe_frame not in ("lab", "tunnel"):
            raise ValueError("probe_frame must be 'lab' or 'tunnel'")
        return None
    xz = LUDVM._check_probes(probes, probe_frame)
    if xz.shape[1] > _ffi.ENSEMBLE_MAX_PROBES:
        raise ValueError(f"sweep: probes: at most {_ffi.ENSEMBLE_MAX_PROBES} points in a sweep (got {xz.shape[1]}); a member can "
                         "be run on its own with up to 4096: LUDVM(..., probes=...)")
    rows = sum(len(np.arange(kw.get("t0", 0), kw.get("tf", 12) + kw.get("dt", 1.5e-2), kw.get("dt", 1.5e-2))) for kw in merged)
    size = 2 * 8 * rows * xz.shape[1]
    if size > _ffi.ENSEMBLE_PROBE_BYTES:
        raise ValueError(f"sweep: probes: {rows} time levels x {xz.shape[1]} points are {size} bytes ({size / 2**30:.2f} GiB) of "
                         f"probe rows, over the {_ffi.ENSEMBLE_PROBE_BYTES >> 30} GiB one launch returns: split the case list")
    return xz


def _time_levels(kw):
    return len(np.arange(kw.get("t0", 0), kw.get("tf", 12) + kw.get("dt", 1.5e-2), kw.get("dt", 1.5e-2)))


def _check_sweep_particles(particles, particle_release, particle_frame, particle_steps, snapshot_steps, merged):
    """The sweep's tracers -> (seeds [2, M], release steps [M], recorded steps >= 1 or None for the default), or None without
    `particles`; refused from the keywords alone like a member's."""
    if particles is None:
        if particle_frame not in ("lab", "tunnel"):
            raise ValueError("particle_frame must be 'lab' or 'tunnel'")
        if particle_release is not None or particle_steps is not None:
            raise ValueError("particle_release / particle_steps need `particles`")
        return None
    try:
        xz, rel, steps = LUDVM._check_tracers(particles, particle_release, particle_frame, particle_steps)
    except ValueError as e:
        raise ValueError("sweep: particles: " + str(e).replace("tracer_", "particle_").replace("tracers", "particles")) from e
    M = xz.shape[1]
    if M > _ffi.ENSEMBLE_MAX_TRACERS:
        raise ValueError(f"sweep: particles: at most {_ffi.ENSEMBLE_MAX_TRACERS} tracers in a sweep (got {M}); a member can be run on "
                         f"its own with up to {_ffi.MARCH_MAX_TRACERS}: LUDVM(..., tracers=...)")
    last = max(_time_levels(kw) for kw in merged) - 1
    if steps is None:
        rec = None
        nrec = len({int(s) for s in snapshot_steps if 1 <= int(s) <= last})
    else:
        if steps and (steps[0] < 1 or steps[-1] > last):
            raise ValueError(f"sweep: particle_steps must lie in [1, {last}] (the longest member's last step)")
        rec, nrec = steps, len(steps)
    size = len(merged) * (nrec + 1) * 2 * 8 * M
    if size > _ffi.ENSEMBLE_TRACER_BYTES:
        raise ValueError(f"sweep: particles: {len(merged)} members x {nrec + 1} records x {M} tracers are {size} bytes "
                         f"({size / 2**30:.2f} GiB) of tracer records, over the {_ffi.ENSEMBLE_TRACER_BYTES >> 30} GiB one launch "
                         "returns: split the case list or record fewer steps")
    return xz, rel, rec


def _check_sweep_survey(survey, survey_frame, survey_steps, merged):
    """The sweep's survey -> (points [2, K], the results' shape, (first, stop, every)), or None without `survey`; refused from
    the keywords alone like a member's."""
    if survey is None:
        if survey_frame not in ("lab", "tunnel"):
            raise ValueError("survey_frame must be 'lab' or 'tunnel'")
        if survey_steps is not None:
            raise ValueError("survey_steps needs `survey`")
        return None
    try:
        xz, shape, win = LUDVM._check_survey(survey, survey_frame, survey_steps)
    except ValueError as e:
        raise ValueError("sweep: " + str(e)) from e
    K = xz.shape[1]
    if K > _ffi.ENSEMBLE_MAX_SURVEY:
        raise ValueError(f"sweep: survey: at most {_ffi.ENSEMBLE_MAX_SURVEY} points in a sweep (got {K}); a member can be run on its "
                         f"own with up to {_ffi.MARCH_MAX_SURVEY}: LUDVM(..., survey=...)")
    size = len(merged) * 5 * 8 * K
    if size > _ffi.ENSEMBLE_SURVEY_BYTES:
        raise ValueError(f"sweep: survey: {len(merged)} members x {K} points are {size} bytes ({size / 2**30:.2f} GiB) of survey "
                         f"sums, over the {_ffi.ENSEMBLE_SURVEY_BYTES >> 30} GiB one launch returns: split the case list")
    for idx, kw in enumerate(merged):
        nt = _time_levels(kw)
        if min(win[1], nt) <= win[0]:
            raise ValueError(f"sweep: member {idx}: survey_steps: the window [{win[0]}, {min(win[1], nt)}) holds no time step of "
                             f"its {nt - 1}")
    return xz, shape, win


def _check_sweep_phases(survey_phases, surveyed, merged):
    """The sweep's bins -> (one table int64 [nt] per member: the bin of every sampled step, -1 elsewhere; B; the bin centres [B]
    or None for explicit tables), or None without `survey_phases`; refused from the keywords alone.  A member's table is the one
    a solo run builds (LUDVM._check_survey_bins) from its own time levels, t0 and frequency, its window clipped to its nt."""
    if survey_phases is None:
        return None
    most = _ffi.ENSEMBLE_MAX_SURVEY_BINS
    form = "survey_phases must be an int B or a sequence of one integer array [nt] per member"
    if surveyed is None:
        raise ValueError("sweep: survey_phases needs `survey`")
    if isinstance(survey_phases, (bool, np.bool_)):
        raise ValueError("sweep: " + form)
    K, win = surveyed[0].shape[1], surveyed[2]
    given = None
    if isinstance(survey_phases, (int, np.integer)):
        B = int(survey_phases)
        if not 1 <= B <= most:
            raise ValueError(f"sweep: survey_phases: 1 <= B <= {most} (got {B})")
    else:
        try:
            given = list(survey_phases)
        except TypeError as e:
            raise ValueError("sweep: " + form) from e
        if len(given) != len(merged):
            raise ValueError(f"sweep: survey_phases: one table per member ({len(given)} tables for {len(merged)} members)")
        tops = []
        for idx, (raw, kw) in enumerate(zip(given, merged)):
            nt = _time_levels(kw)
            try:
                raw = np.asarray(raw)
            except (TypeError, ValueError) as e:
                raise ValueError(f"sweep: member {idx}: " + form) from e
            if raw.dtype.kind not in "iu" or raw.shape != (nt,):
                raise ValueError(f"sweep: member {idx}: survey_phases: a table holds one integer per time step, [nt] with nt = {nt}")
            if raw.min() < -1:
                raise ValueError(f"sweep: member {idx}: survey_phases: a table's entries are -1 (no bin) or a bin 0 .. B-1")
            given[idx] = raw.astype(np.int64)
            tops.append(int(raw.max()))
        B = max(tops) + 1
        if B > most:
            raise ValueError(f"sweep: member {int(np.argmax(tops))}: survey_phases: at most {most} bins (the table's largest entry is "
                             f"{B - 1})")
    size = len(merged) * (B + 1) * 5 * 8 * K
    if size > _ffi.ENSEMBLE_SURVEY_BYTES:
        raise ValueError(f"sweep: survey_phases: {len(merged)} members x ({B} bins + 1) x {K} points are {size} bytes "
                         f"({size / 2**30:.2f} GiB) of survey sums, over the {_ffi.ENSEMBLE_SURVEY_BYTES >> 30} GiB one launch "
                         "returns: split the case list")
    tables, phase = [], None
    for idx, kw in enumerate(merged):
        t0, tf, dt = kw.get("t0", 0), kw.get("tf", 12), kw.get("dt", 1.5e-2)
        t = np.arange(t0, tf + dt, dt)
        f = kw.get("k", 0.2 * np.pi) * kw.get("Uinf", 1) / (2 * np.pi * kw.get("chord", 1))
        if given is None and not f > 0:
            raise ValueError(f"sweep: member {idx}: survey_phases={B}: the motion has no period (k = 0): give the sweep one table per "
                             "member, or run the member on its own with survey_period")
        try:
            table, _, phase = LUDVM._check_survey_bins(B if given is None else given[idx], None, None, K,
                                                       (win[0], min(win[1], len(t)), win[2]), t, t0, f)
        except ValueError as e:
            raise ValueError(f"sweep: member {idx}: " + str(e).replace("survey_bins", "survey_phases")) from e
        tables.append(table)
    return tables, B, phase


def _check_sweep_grad(survey_grad, surveyed, binned, merged):
    """The sweep's `survey_grad` -> bool; refused from the keywords alone."""
    if isinstance(survey_grad, str) and survey_grad == "f32x2":
        raise ValueError("sweep: survey_grad='f32x2': the gradient sums of a sweep are float64 -- survey_grad=True (hi+lo fp32 "
                         "gradient sums: run a member on its own, LUDVM(..., survey=..., survey_gradient='f32x2'))")
    if not isinstance(survey_grad, (bool, np.bool_)):
        raise ValueError(f"sweep: survey_grad={survey_grad!r}: survey_grad must be True or False")
    if not survey_grad:
        return False
    if surveyed is None:
        raise ValueError("sweep: survey_grad needs `survey`")
    K, B = surveyed[0].shape[1], 0 if binned is None else binned[1]
    size = len(merged) * (B + 1) * 10 * 8 * K
    if size > _ffi.ENSEMBLE_SURVEY_BYTES:
        raise ValueError(f"sweep: survey_grad: {len(merged)} members x ({B} bins + 1) x {K} points are {size} bytes "
                         f"({size / 2**30:.2f} GiB) of survey and gradient sums, over the {_ffi.ENSEMBLE_SURVEY_BYTES >> 30} GiB one "
                         "launch returns: split the case list")
    return True


def _check_sweep_integrals(integrals, energy_steps, merged):
    """The sweep's `integrals` / `energy_steps` -> None without integrals, else (the energy window (first, stop, every) as given, or
    None without samples,); refused from the keywords alone."""
    if not isinstance(integrals, (bool, np.bool_)):
        raise ValueError(f"sweep: integrals={integrals!r}: integrals must be True or False")
    try:
        win = LUDVM._check_wake_integrals(bool(integrals), energy_steps)
    except ValueError as e:
        raise ValueError("sweep: " + str(e).replace("wake_energy_steps", "energy_steps").replace("wake_integrals", "integrals")) from e
    if not integrals:
        return None
    for idx, kw in enumerate(merged):
        nt = _time_levels(kw)
        if win is not None and min(win[1], nt) <= win[0]:
            raise ValueError(f"sweep: member {idx}: energy_steps: the window [{win[0]}, {min(win[1], nt)}) holds no time step of "
                             f"its {nt - 1}")
    return (win,)


def sweep(cases, *, engine=None, device=0, snapshot_steps=(), probes=None, probe_frame="lab", particles=None, particle_release=None,
          particle_frame="lab", particle_steps=None, survey=None, survey_frame="lab", survey_steps=None, survey_phases=None, survey_grad=False,
          integrals=False, energy_steps=None, verbose=False, cls=LUDVM,
          **common):
    """Run `cases` -- a list of dicts of LUDVM constructor keywords, each merged over `common` -- as ONE device launch and
    return the list of LUDVM objects, in order.  Each carries what a solo
    `LUDVM(**kw, precision='f64', history='sparse', snapshot_steps=snapshot_steps)` run carries: Cl, Cd, Cm, Cn, Cs, Ct, Fn, Fs, L,
    D, T, M, LESP, LESP_prev, LEV_shed, itev, ilev, fourier, every circulation[...] entry, and path['TEV' | 'LEV' | 'FREE'] as
    SparseHistory with rows at snapshot_steps and the last step -- `flowfield` works on a member for any stored step.  A member
    differs from its solo run by summation order only; its bits do not depend on the other members or on its place in the list.

    probes: None, or points [2, P] (x row, z row; 1 <= P <= 1024) common to the sweep, like LUDVM(..., probes=...): every member
    also carries `probe_u`, `probe_w` float64 [nt, P] -- the field that convects its wake in each step, evaluated at the points
    inside the one launch (row 0: the field of its free vortices) -- with `probe_xz`, `probe_frame` and `probe_positions(step)`.
    probe_frame='tunnel' measures x from each member's own pivot (x + xpiv[step]: xpiv depends on the member's Uinf and dt).
    Everything else a member returns is bit-identical to the sweep without probes.

    particles: None, or seeds [2, M] (1 <= M <= 4096) of passive tracers common to the sweep, with particle_release (None: all 1,
    or one release step >= 1 per tracer), particle_frame ('lab' | 'tunnel') and particle_steps -- the meaning of LUDVM(...,
    tracers=, tracer_release=, tracer_frame=, tracer_steps=), under sweep-level names because `tracers` itself stays refused in a
    sweep.  Seeds, release steps and recorded steps are common; particle_frame='tunnel' adds each member's own xpiv[step] to the
    seeds.  Every member is advected inside the one launch and carries the attributes of a solo run with tracers:
    `tracer_path` (a SparseHistory step -> [2, M]; row 0, the seeds, always there), `tracer_last`, `tracer_xz`,
    `tracer_release`, `tracer_frame`, `tracer_released(step)`.  particle_steps=None records snapshot_steps and each member's
    last step; otherwise every entry lies in [1, the largest nt - 1 of the members], and a member shorter than a listed step
    has no row for it (`tracer_last` is its last step either way).  `probes` and `particles` compose in one launch; everything else a
    member returns, its probe rows included, is bit-identical to the sweep without particles.

    survey: None, or the points of a wake survey common to the sweep -- a [2, K] array or a dict(xmin, xmax, zmin, zmax, dr) mesh,
    1 <= K <= 4096 -- with survey_frame ('lab' | 'tunnel') and survey_steps (first, stop, every), the meaning of LUDVM(..., survey=,
    survey_frame=, survey_steps=).  Points and window are common; survey_frame='tunnel' adds each member's own xpiv[step] to the
    points, and a member samples first <= i < min(stop, its nt), (i - first) % every == 0.  The five raw sums are accumulated
    inside the one launch and every member carries the attributes of a solo run with a survey: `survey_x`, `survey_z`
    (mesh-shaped for a dict), `survey_count`, `survey_sums`, `survey_mean_u`, `survey_mean_w`, `survey_uu`, `survey_ww`,
    `survey_uw`, `survey_frame`, and `survey_steps` with stop clipped to the member's nt.  `survey` composes with `probes` and
    `particles` in one launch; everything else a member returns, probe rows and tracer paths included, is bit-identical to the
    sweep without a survey.

    survey_phases: None, or the bins of a phase-locked survey, the sweep-level form of LUDVM(..., survey_bins=) (which, with
    survey_period and survey_phase0, stays a solo keyword and is refused here).  An int B (1 .. 64) bins every member by its OWN
    motion -- period 1 / f of the member, phase 0 at its t0, the table a solo run of the member builds with survey_bins=B -- so
    members of different k, dt or tf get different tables under one B; a member without a period (k = 0) is refused by name.  Or
    a sequence with one integer array [nt] per member, entries -1 (no bin) .. B - 1 with the meaning of the solo table; B is 1 + the
    largest entry over all members, at most 64.  The bin sums are accumulated inside the one launch, by the lane that adds the
    plain sums, and every member carries the attributes of a solo run with survey_bins: `survey_nbins`, `survey_bin_of_step`,
    `survey_bin_count`, `survey_bin_sums` [B, 5, ...], `survey_bin_mean_u` / `_w`, `survey_bin_uu` / `_ww` / `_uw` (nan for an empty
    bin), `survey_phase` (None for tables), `survey_coherent_*`, `survey_random_*`, beside the plain survey attributes.  Composes
    with `probes` and `particles`; everything else a member returns, the plain survey sums included, is bit-identical to the sweep
    without survey_phases, and bin b's sums are bit for bit the plain sums of a sweep that samples exactly bin b's steps.

    survey_grad: False, or True for the gradient sums of the survey, the sweep-level form of LUDVM(..., survey_gradient=True)
    (which stays a solo keyword and is refused here; the name matches flowfield(grad=)).  In every sampled step of a member the
    closed-form gradient of the survey's field -- the same sources, its wake and bound vortices of that step -- at the survey's
    shifted points adds ux = -A / pi, e = B / (2 pi), om = -v_core^4 C / pi, om^2 and Q = om^2 / 4 - ux^2 - e^2 to five more raw
    float64 sums per point inside the one launch, and with survey_phases the same five terms to the step's bin block.  Every member
    carries the attributes of a solo run with survey_gradient=True, formed by the solo code: `survey_gradient` (True),
    `survey_grad_sums` [5, ...], `survey_mean_ux` / `_strain` / `_omega` / `_uz` / `_wx` / `_q`, `survey_omega2`, `survey_omega_var`,
    `survey_production`, and with bins `survey_bin_grad_sums` [B, 5, ...], `survey_bin_mean_ux` / `_strain` / `_omega` / `_q`,
    `survey_bin_omega2`, `survey_coherent_omega2`, `survey_random_omega2`.  Composes with `probes`, `particles`, `survey_frame`,
    `survey_steps` and `survey_phases`; everything else a member returns, the velocity sums and their bins included, is
    bit-identical to the sweep without survey_grad, and bin b's gradient block is bit for bit the gradient sums of a sweep that
    samples exactly bin b's steps.  A sweep without it makes the engine calls it made before.

    integrals: False, or True for the wake integrals of every member, the sweep-level form of LUDVM(..., wake_integrals=True,
    wake_energy_steps=) (which stay solo keywords and are refused here), with energy_steps = (first, stop, every) in survey_steps'
    form, None: no energy samples.  In every step of a member the six moments -- count, sum G, sum G x, sum G z, sum G (x^2 + z^2),
    sum G^2 -- of its vortex system (the sources its probes see: wake before the Euler update, the step's shed vortices, the bound
    vortices) by class ('FREE', 'TEV', 'LEV', 'BOUND') and sign are accumulated inside the member's workgroup, in float64, and at the
    sampled steps (first <= i < min(stop, its nt), (i - first) % every == 0) W = 1/2 sum G_a psi(x_a) over the same sources with the
    member's own v_core: an O((n + Npoints - 1)^2) float64 pair sum with a logarithm per pair inside ONE workgroup (a member at the
    8192-vortex limit: about 7e7 pairs per sample), so sample sparingly.  Every member carries the attributes of a solo run with
    wake_integrals=True, formed by the solo code: `wake_integrals` (True), `wake_energy_steps` (stop clipped to its nt),
    `integral_sums` [nt, 4, 2, 6] (row 0: its free vortices), `wake_energy` [nt] (NaN where not sampled), and `wake_circulation`,
    `wake_centroid`, `wake_impulse`, `wake_angular_impulse`, `impulse_force`, `impulse_Cl`, `impulse_Cd`, `wake_energy_interaction`.
    Composes with `probes`, `particles`, `survey`, `survey_phases` and `survey_grad` in one launch; everything else a member returns
    is bit-identical to the sweep without integrals, a member's rows do not depend on the batch, and a sampled step's W does not
    depend on the window.  A sweep without it makes the engine calls it made before.

    Npoints (3 .. 257) and Ncoeffs (4 .. 64) are common to a sweep; everything else may differ per member (dt, tf, method, LESPcrit, the section,
    kinematics, free vortices).  Refused with ValueError before any device work, naming the member: differing Npoints / Ncoeffs, or ones outside those ranges,
    a member over the limits (2048 steps, 8192 wake vortices: run it on its own), precision other than 'auto' / 'f64',
    history='full', checkpoint_*, distributed, devices, march=False, run=False, an engine without ensemble_run; `probes` or
    `probe_frame` inside a member's dict (they belong to the sweep), more than 1024 probes, points that are not finite, a
    probe_frame other than 'lab' / 'tunnel', an engine without ensemble_run_probed, and probe rows (16 bytes x all members' time
    levels x P) over 1 GiB: split the case list; `particles` / `particle_*` inside a member's dict, `tracers` / `tracer_*`
    anywhere (use `particles=`), more than 4096 particles, seeds that are not finite, release steps < 1 or not one integer per
    tracer, a particle_frame other than 'lab' / 'tunnel', particle_steps outside [1, the largest nt - 1], an engine without
    ensemble_run_traced, and tracer records (16 bytes x members x (recorded steps + 1) x M) over 1 GiB; `survey` / `survey_steps` /
    survey_frame='tunnel' inside a member's dict (they belong to the sweep), more than 4096 survey points, points that are not
    finite, a survey_frame other than 'lab' / 'tunnel', survey_steps that are not three integers with first >= 1 and every >= 1
    or that hold no step of some member (named), survey_steps without `survey`, `survey_precision`, `tracer_precision`, `tracer_gradient` or `survey_gradient` anywhere (the sweep's or a member's), an engine without
    ensemble_run_surveyed, and
    survey sums (40 bytes x members x K) over 1 GiB: split the case list; `survey_phases` inside a member's dict, without `survey`,
    a bool, B outside 1 .. 64, a sequence that does not hold one table per member, a table (member named) that is not an integer
    array [nt] or has entries below -1, a member none of whose sampled steps has a bin, `survey_bins` / `survey_period` /
    `survey_phase0` anywhere, an engine without ensemble_run_surveyed_binned, and plain and bin sums (40 bytes x members x (B + 1)
    x K) over 1 GiB: split the case list; `survey_grad` inside a member's dict, without `survey`, a value that is not a bool
    ('f32x2': a sweep's sums are float64), an engine without ensemble_run_surveyed_graded, and plain, bin and gradient sums (80
    bytes x members x (B + 1) x K) over 1 GiB: split the case list; `integrals` / `energy_steps` inside a member's dict,
    `wake_integrals` / `wake_energy_steps` anywhere (solo keywords: use `integrals=`), an `integrals` that is not a bool,
    energy_steps without integrals=True, not three integers with first >= 1 and every >= 1, or holding no step of some member
    (named), and an engine without ensemble_run_integrals.

    Out of scope: per-member probe, seed or survey point sets and windows, per-member energy windows, an fp32 or hi+lo fp32 wake energy, an energy walk that visits each pair once, wake integrals of a sweep on several GPUs, harmonic sums of a survey in a sweep, hi+lo fp32 gradient sums in a sweep, tracers or a survey of a sweep on several GPUs, fp32 tracer or survey sums in a sweep (a solo run has tracer_precision='f32x2' and survey_precision='f32'), fp32 members, dense history, checkpoint / resume of a sweep, sweeps over several GPUs (members are independent:
    split the list per device), members above the limits; a solo run executes exactly as before."""
    if "survey_precision" in common:
        raise ValueError(f"sweep: survey_precision={common['survey_precision']!r}: the survey of a sweep is evaluated in float64 "
                         "(fp32 survey sums: run a member on its own, LUDVM(..., survey=..., survey_precision='f32'))")
    if "tracer_precision" in common:
        raise ValueError(f"sweep: tracer_precision={common['tracer_precision']!r}: the tracers of a sweep are advected in float64 "
                         "(fp32 tracer sums: run a member on its own, LUDVM(..., tracers=..., tracer_precision='f32x2'))")
    if "tracer_gradient" in common:
        raise ValueError(f"sweep: tracer_gradient={common['tracer_gradient']!r}: the tracers of a sweep carry no deformation gradient "
                         "(run a member on its own, LUDVM(..., tracers=..., tracer_gradient=True))")
    if "survey_gradient" in common:
        raise ValueError(f"sweep: survey_gradient={common['survey_gradient']!r}: the survey of a sweep carries no gradient sums "
                         "(run a member on its own, LUDVM(..., survey=..., survey_gradient=True))")
    for key in ("survey_bins", "survey_period", "survey_phase0"):
        if common.get(key) is not None:
            raise ValueError(f"sweep: {key}={common[key]!r}: {_BINS_SOLO}")
    for key in ("wake_integrals", "wake_energy_steps"):
        if key in common:
            raise ValueError(f"sweep: {key}={common[key]!r}: {_INTEGRALS_SOLO}")
    cases = list(cases)
    if not cases:
        return []
    merged, first = [], None
    for idx, case in enumerate(cases):
        kw = dict(common)
        kw.update(case)
        dims = _check_case(idx, kw, first)
        first = first or dims
        merged.append(kw)
    probe_xz = _check_sweep_probes(probes, probe_frame, merged)
    traced = _check_sweep_particles(particles, particle_release, particle_frame, particle_steps, snapshot_steps, merged)
    surveyed = _check_sweep_survey(survey, survey_frame, survey_steps, merged)
    binned = _check_sweep_phases(survey_phases, surveyed, merged)
    graded = _check_sweep_grad(survey_grad, surveyed, binned, merged)
    integrated = _check_sweep_integrals(integrals, energy_steps, merged)
    if engine is None:
        from .engine import Engine
        engine = Engine(device)
    if not hasattr(engine, "ensemble_run"):
        raise ValueError("sweep: this engine has no ensemble_run")
    if probe_xz is not None and not hasattr(engine, "ensemble_run_probed"):
        raise ValueError("sweep: probes: this engine has no ensemble_run_probed")
    if traced is not None and not hasattr(engine, "ensemble_run_traced"):
        raise ValueError("sweep: particles: this engine has no ensemble_run_traced")
    if surveyed is not None and not hasattr(engine, "ensemble_run_surveyed"):
        raise ValueError("sweep: survey: this engine has no ensemble_run_surveyed")
    if binned is not None and not hasattr(engine, "ensemble_run_surveyed_binned"):
        raise ValueError("sweep: survey_phases: this engine has no ensemble_run_surveyed_binned")
    if graded and not hasattr(engine, "ensemble_run_surveyed_graded"):
        raise ValueError("sweep: survey_grad: this engine has no ensemble_run_surveyed_graded")
    if integrated is not None and not hasattr(engine, "ensemble_run_integrals"):
        raise ValueError("sweep: integrals: this engine has no ensemble_run_integrals")
    snaps = sorted({int(s) for s in snapshot_steps})
    dev_snaps = [s for s in snaps if s >= 1]
    if len(dev_snaps) > _ffi.ENSEMBLE_MAX_SNAPSHOTS:
        raise ValueError(f"sweep: at most {_ffi.ENSEMBLE_MAX_SNAPSHOTS} snapshot steps")

    # host: geometry, kinematics and tables of every member, packed
    sims, loops = [], []
    sc, tb, kn, ini, fr, shift = [], [], [], [], [], []
    desc = np.zeros([len(merged), _ffi.ENSEMBLE_DESC], dtype=np.int64)
    kin_off = free_off = row_off = wake_off = 0
    nrec = len(dev_snaps) + 1
    for idx, kw in enumerate(merged):
        kw = dict(kw, precision="f64", history="sparse")
        if integrated is not None:      # (the solo constructor and _loop_begin: the attributes, row 0, the window clipped to nt)
            kw.update(wake_integrals=True, wake_energy_steps=integrated[0])
        sim = cls(**kw, engine=engine, snapshot_steps=snaps, verbose=False, run=False)
        if sims and (sim.Npoints, sim.Ncoeffs) != (sims[0].Npoints, sims[0].Ncoeffs):       # (a .dat section sets its own)
            raise ValueError(f"sweep: member {idx}: Npoints / Ncoeffs differ from member 0's: they are common to a sweep")
        S = sim._loop_begin(resident=False)
        sim._free_slot = None
        S.fsl = slice(0, S.nf)
        S.sb, S.have_next = None, False
        scalars, tables, kin = sim._march_inputs(S)
        tev_xy, lev_xy = sim._next_placement(S, 1)
        free0 = np.array(sim.xy_freevort, dtype=float).reshape(2, S.nf)
        sc.append(np.asarray(scalars, dtype=float))
        tb.append(tables)
        kn.append(kin)
        ini.append(np.concatenate([[tev_xy[0], lev_xy[0], tev_xy[1], lev_xy[1], sim.LESPcrit, 0.0, 0.0, 0.0], sim.fourier[0, 0, :]]))
        fr.append(np.concatenate([free0[0], free0[1], np.asarray(sim.circulation_freevort, dtype=float).reshape(-1)]))
        if probe_xz is not None:
            sim.probe_xz, sim.probe_frame = probe_xz.copy(), probe_frame
        if traced is not None:
            sim.tracer_xz, sim.tracer_release, sim.tracer_frame = traced[0].copy(), traced[1].copy(), particle_frame
        if surveyed is not None:
            sim._survey_xz, sim._survey_shape = surveyed[0].copy(), surveyed[1]
            sim.survey_x, sim.survey_z = sim._survey_xz[0].reshape(surveyed[1]), sim._survey_xz[1].reshape(surveyed[1])
            sim.survey_frame, sim.survey_steps = survey_frame, (surveyed[2][0], min(surveyed[2][1], sim.nt), surveyed[2][2])
            if binned is not None:
                if len(binned[0][idx]) != sim.nt:       # (a .dat section or a subclass that sets its own time levels)
                    raise ValueError(f"sweep: member {idx}: survey_phases: the member has {sim.nt} time levels, its table {len(binned[0][idx])}")
                sim.survey_nbins, sim.survey_bin_of_step, sim.survey_phase = binned[1], binned[0][idx], binned[2]
        if probe_xz is not None or traced is not None or surveyed is not None:
            shift.append(np.asarray(sim.xpiv, dtype=float))
        nt, nf = sim.nt, S.nf
        desc[idx] = [nt, kin_off, nf, free_off, row_off, wake_off]
        kin_off, free_off, row_off = kin_off + nt, free_off + nf, row_off + nt - 1
        wake_off += nrec * 3 * (nf + 2 * (nt - 1))
        sims.append(sim)
        loops.append(S)
    npan, ncoef = sims[0].Npoints - 1, sims[0].Ncoeffs

    # device: one launch
    packed = (npan, ncoef, np.stack(sc), np.stack(tb), np.concatenate(kn), np.stack(ini), np.concatenate(fr), desc, dev_snaps)
    targs = {}
    if traced is not None:
        # recorded steps: the listed ones, or snapshot_steps (each member's last step is always the final record)
        trec = [s for s in (dev_snaps if traced[2] is None else traced[2]) if 1 <= s <= max(sim.nt for sim in sims) - 1]
        targs = dict(seed_x=traced[0][0], seed_z=traced[0][1], release=traced[1], record_steps=trec,
                     shift_x=np.concatenate(shift) if particle_frame == "tunnel" else None)
    if integrated is not None:
        # (every observer is optional in this call; the energy window as given: the device clips it to each member's nt)
        targs["energy_steps"] = integrated[0]
        if surveyed is not None:
            targs.update(survey_x=surveyed[0][0], survey_z=surveyed[0][1], survey_steps=surveyed[2],
                         survey_shift_x=np.concatenate(shift) if survey_frame == "tunnel" else None, grad=graded)
            if binned is not None:
                targs.update(bin_of_step=np.concatenate(binned[0]), nbins=binned[1])
        if probe_xz is not None:
            targs.update(probe_x=probe_xz[0], probe_z=probe_xz[1], probe_shift_x=np.concatenate(shift) if probe_frame == "tunnel" else None)
        *out, ssums, bsums, gsums, bgsums, isums, wsums = engine.ensemble_run_integrals(*packed, **targs)
        if probe_xz is not None:
            rows, wakes, wake_n, trows, pu, pw = out
        else:
            rows, wakes, wake_n, trows = out
    elif surveyed is not None:
        # (the window as given: the device clips it to each member's nt)
        targs.update(survey_x=surveyed[0][0], survey_z=surveyed[0][1], survey_steps=surveyed[2],
                     survey_shift_x=np.concatenate(shift) if survey_frame == "tunnel" else None)
        if probe_xz is not None:
            targs.update(probe_x=probe_xz[0], probe_z=probe_xz[1], probe_shift_x=np.concatenate(shift) if probe_frame == "tunnel" else None)
        gsums = bgsums = None
        if graded:
            if binned is not None:
                targs.update(bin_of_step=np.concatenate(binned[0]), nbins=binned[1])
            *out, ssums, bsums, gsums, bgsums = engine.ensemble_run_surveyed_graded(*packed, **targs)
        elif binned is not None:
            # (one entry per kinematics row, like the offsets: member m's step i at [kin_off + i])
            *out, ssums, bsums = engine.ensemble_run_surveyed_binned(*packed, **targs, bin_of_step=np.concatenate(binned[0]),
                                                                     nbins=binned[1])
        else:
            *out, ssums = engine.ensemble_run_surveyed(*packed, **targs)
        if probe_xz is not None:
            rows, wakes, wake_n, trows, pu, pw = out
        else:
            rows, wakes, wake_n, trows = out
    elif traced is not None:
        if probe_xz is not None:
            targs.update(probe_x=probe_xz[0], probe_z=probe_xz[1], probe_shift_x=np.concatenate(shift) if probe_frame == "tunnel" else None)
            rows, wakes, wake_n, trows, pu, pw = engine.ensemble_run_traced(*packed, **targs)
        else:
            rows, wakes, wake_n, trows = engine.ensemble_run_traced(*packed, **targs)
    elif probe_xz is None:
        rows, wakes, wake_n = engine.ensemble_run(*packed)
    else:
        rows, wakes, wake_n, pu, pw = engine.ensemble_run_probed(
            *packed, probe_x=probe_xz[0], probe_z=probe_xz[1], shift_x=np.concatenate(shift) if probe_frame == "tunnel" else None)

    # host: every member's rows into its result arrays, by the routine that stores a solo march
    for idx, (sim, S) in enumerate(zip(sims, loops)):
        nt, k0, nf, _, r0, w0 = (int(v) for v in desc[idx])
        if probe_xz is not None:
            sim.probe_u, sim.probe_w = pu[k0:k0 + nt].copy(), pw[k0:k0 + nt].copy()
        if traced is not None:
            sim.tracer_path = SparseHistory(nt)
            sim.tracer_path.store(0, sim._tracer_seeds(0))
            for r, step in enumerate(trec):
                if step <= nt - 1:
                    sim.tracer_path.store(step, trows[idx, r].copy())
            sim.tracer_last = trows[idx, len(trec)].copy()
            if traced[2] is None:               # (the solo rule of a sparse history: snapshot_steps and the last step)
                sim.tracer_path.store(nt - 1, sim.tracer_last.copy())
        if surveyed is not None:
            first, stop, every = sim.survey_steps
            sim._survey_results(ssums[idx], len(range(first, stop, every)))
            if binned is not None:              # (the samples of a bin: counted on the host from the member's table)
                table = sim.survey_bin_of_step
                sim._survey_bin_results(bsums[idx], np.bincount(table[table >= 0], minlength=sim.survey_nbins))
            if graded:
                sim.survey_gradient = True
                sim._survey_gradient_results(gsums[idx], None if binned is None else bgsums[idx])
        if integrated is not None:          # (row 0 and the NaN of the energy are _loop_begin's, as in a solo run)
            sim.integral_sums[1:] = isums[k0 + 1:k0 + nt]
            if wsums is not None:
                sim.wake_energy[1:] = wsums[k0 + 1:k0 + nt]
        cap = nf + 2 * (nt - 1)
        R = rows[r0:r0 + nt - 1]
        hist = _RecordedWakes()
        for r, step in enumerate(dev_snaps + [nt - 1]):
            n = int(wake_n[idx, r])
            if n < 0 or (r < len(dev_snaps) and step > nt - 1):
                continue
            rec = wakes[w0 + r * 3 * cap:w0 + (r + 1) * 3 * cap]
            hist.rows[step - 1] = (rec[:n], rec[cap:cap + n])
        n_shed = int((R[:, 2] != 0).sum())
        n_end = int(wake_n[idx, nrec - 1])
        last = wakes[w0 + (nrec - 1) * 3 * cap:w0 + nrec * 3 * cap]
        st = np.zeros(16 + ncoef)
        st[0], st[1], st[2] = n_end, nt - 1, n_shed
        shed_rows = R[R[:, 2] != 0]
        st[4] = sim.LESPcrit                      # ... with the sign of A0 at the last shedding (:802-805)
        if len(shed_rows):
            st[4] = -abs(sim.LESPcrit) if shed_rows[-1, 4] < 0 else abs(sim.LESPcrit)
        st[5], st[6] = R[:, 0].sum(), R[:, 1].sum()
        if n_end >= 2:
            st[12:16] = [last[n_end - 2], last[n_end - 1], last[cap + n_end - 2], last[cap + n_end - 1]]
        sim._store_march_results(S, 1, nt, st, R, hist)
        sim.compute_coefficients()
        if verbose:
            print(f"sweep: member {idx}: {nt - 1} steps, {sim.itev + 1} TEV, {S.ilev} LEV, mean Cl {sim.Cl.mean():.6f}")
    return sims
