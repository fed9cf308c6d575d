"""Shared by tests/test_survey_gradient_f32x2_host.py and tests/test_gpu_survey_gradient_f32x2.py: the derived tolerance of the
survey's gradient sums in hi+lo fp32 (march_f32x2_grad_survey_partial, LUDVM(..., survey=, survey_gradient='f32x2'); DESIGN.md
section 4.20), the references it is held against and the conditions a chosen point set has to meet.

The walk is tests/tracer_gradient_f32x2_common.py's (hilo_field_grad_f32): its per-pair products and two-level sums are those of
tests/gradient_f32x2_common.py, so per sampled step and point, against the np.longdouble closed forms,

    b    = gradient_f32x2_common.gradient_reference(...)[1]   bounds ux = -A / pi and e = B / (2 pi):
           (128 + 24) 2^-23 mag + (ns + 16) 2^-52 mag,  mag = sum |G| / (2 pi s)
    b_om = gradient_f32x2_common.omega_reference(...)[1]      bounds om (mag = sum |G| v_core^4 / (pi s^3))
    om^2 is within  b_om (2 |om| + b_om)                       (|a^2 - a'^2| = |a - a'| |a + a'|)
    Q    is within  b_om (2 |om| + b_om) / 4 + b (2 |ux| + b) + b (2 |e| + b)

The tolerance of a sum is the sum of its steps' terms plus the float64 allowance of tests/survey_gradient_common.py (the sums, the
splits and the finisher are float64 in another order): MEAN_BOUND n gmax for the sums of ux, e, om and SQUARE_BOUND n gmax^2 for
those of om^2 and Q, with gmax = max(|ux|, |uz|, |wx|) over the sampled steps and points.  Nothing here is taken from the code
under test.

Two conditions on a point set, both from the reference alone (caps, not measurements):
    * at every point the tolerance is below 1e-2 of n gmax (n gmax^2 for om^2 and Q)
    * the reference sums over the sources of step i - 1 instead of i (step 1 keeps its own: there is no roll-up before it) differ
      from the reference by more than ten tolerances at some point: a wake taken one step late cannot pass

The velocity sums of such a survey are the fused walk's: means within tracers_f32x2_common.VELOCITY_VS_F64 of max|u| of the field
(observer_sources_common.field) and raw second moments within three times that of max|u|^2 (survey_common's product rule)."""
import numpy as np

import gradient_f32x2_common as GF
import survey_common as SC
import survey_gradient_common as SG
from tracers_f32x2_common import VELOCITY_VS_F64

CAP = 1e-2                      # of n gmax (n gmax^2): the largest tolerance a point set may have
LATE = 10.0                     # tolerances by which the sums over a wake one step late must differ somewhere
MOMENT_VS_F64 = 3 * VELOCITY_VS_F64
LATE_POINTS = 64                # points at which the sums over a wake one step late are formed


def step_tolerance(sources, px, pz, v_core, terms):
    """-> [5, K]: the bounds above of one step's five terms at the points; `terms` [5, K]: the step's reference terms"""
    g, x, z = SG.all_sources(sources)
    b = GF.gradient_reference(g, x, z, px, pz, v_core)[1]
    b_om = GF.omega_reference(g, x, z, px, pz, v_core)[1]
    ux, e, om = np.abs(terms[0]), np.abs(terms[1]), np.abs(terms[2])
    sq = b_om * (2 * om + b_om)
    return np.stack([b, b, b_om, sq, sq / 4 + b * (2 * ux + b) + b * (2 * e + b)])


def reference(steps, points_of, sources_of, v_core, late=True):
    """-> dict(ref [5, K], gmax, per {i: [5, K]}, tol [5, K], late [5, K] or None): survey_gradient_common.reference_sums, the summed
    tolerance with its float64 allowance, and the sums over the sources of the step before"""
    ref, gmax, per = SG.reference_sums(steps, points_of, sources_of, v_core)
    n = len(steps)
    tol = np.zeros_like(ref)
    for i in steps:
        px, pz = points_of(i)
        tol += step_tolerance(sources_of(i), px, pz, v_core, per[i])
    tol[:3] += SG.MEAN_BOUND * n * gmax
    tol[3:] += SG.SQUARE_BOUND * n * gmax ** 2
    behind = None
    if late:
        # ("at some point": the first LATE_POINTS points serve, and keep the reference's cost down)
        first = lambda i: tuple(c[:LATE_POINTS] for c in points_of(i))       # noqa: E731
        behind = SG.reference_sums(steps, first, lambda i: sources_of(max(i - 1, 1)), v_core)[0]
    return dict(ref=ref, gmax=gmax, per=per, tol=tol, late=behind, n=n)


def scales(R):
    """[5, 1]: n gmax for the sums of ux, e, om and n gmax^2 for those of om^2 and Q"""
    return np.array([R["n"] * R["gmax"]] * 3 + [R["n"] * R["gmax"] ** 2] * 2)[:, None]


def check_conditions(R, what):
    """the two conditions of a point set, from the reference alone"""
    cap = float((R["tol"] / scales(R)).max())
    assert R["gmax"] > 0.0 and cap < CAP, (what, cap)
    if R["late"] is not None:
        m = R["late"].shape[1]
        off = float((np.abs(R["late"] - R["ref"][:, :m]) / R["tol"][:, :m]).max())
        assert off > LATE, (what, off)
        return cap, off
    return cap, None


def check_sums(gsums, R, what):
    """gsums [5, K] against the reference within the tolerance, printed first; -> (worst error / tolerance, worst error / scale)"""
    cap, off = check_conditions(R, what)
    d = np.abs(np.asarray(gsums).reshape(5, -1) - R["ref"])
    ratio, of_scale = float((d / R["tol"]).max()), float((d / scales(R)).max())
    print(f"{what}: {R['n']} steps, {d.shape[1]} points: worst error {ratio:.3f} of the tolerance, {of_scale:.2e} of max|grad u| "
          f"({R['gmax']:.3f}; squares: of its square); largest tolerance {cap:.2e} of that"
          + ("" if off is None else f"; a wake one step late is off by {off:.0f} tolerances"))
    assert ratio <= 1.0, (what, ratio, [float((d[k] / R["tol"][k]).max()) for k in range(5)])
    return ratio, of_scale


def check_velocity(sums, steps, points_of, sources_of, v_core, iv, field, what):
    """The five velocity sums [5, K] of the fused walk against the field of the step's sources (`field`:
    observer_sources_common.field over `iv`), added in step order"""
    K = np.asarray(sums).reshape(5, -1).shape[1]
    ref, umax = np.zeros([5, K]), 0.0
    for i in steps:
        px, pz = points_of(i)
        u, w = field(iv, sources_of(i), px, pz, v_core)
        for acc, term in zip(ref, (u, w, u * u, w * w, u * w)):
            acc += term
        umax = max(umax, float(np.abs(u).max()), float(np.abs(w).max()))
    e_mean, e_sq = SC.sums_errors(sums, ref, len(steps), umax)
    print(f"{what}: velocity sums: means {e_mean:.2e} of max|u| ({umax:.3f}), second moments {e_sq:.2e} of max|u|^2")
    assert umax > 0.0 and e_mean <= VELOCITY_VS_F64 and e_sq <= MOMENT_VS_F64, (what, e_mean, e_sq)
    return e_mean, e_sq
