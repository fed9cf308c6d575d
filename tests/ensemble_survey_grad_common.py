"""Shared by tests/test_ensemble_survey_grad_host.py and tests/test_gpu_ensemble_survey_grad.py: the sources of every step of a
run with a dense history (tests/tracers_common.py's run_sources, and the first step as tests/test_gpu_survey_gradient.py builds
it), and the long-double gradient sums of a survey over them, plain and per bin (tests/survey_gradient_common.py)."""
import numpy as np

import survey_gradient_common as SG
from survey_common import window
from tracers_common import run_sources

GRAD_ATTRS = ("survey_grad_sums", "survey_mean_ux", "survey_mean_strain", "survey_mean_omega", "survey_mean_uz", "survey_mean_wx",
              "survey_mean_q", "survey_omega2", "survey_omega_var", "survey_production")
BIN_GRAD_ATTRS = ("survey_bin_grad_sums", "survey_bin_mean_ux", "survey_bin_mean_strain", "survey_bin_mean_omega", "survey_bin_mean_q",
                  "survey_bin_omega2", "survey_coherent_omega2", "survey_random_omega2")


def first_step_sources(sim):
    """run_sources for step 1 (it starts at 2): the free vortices as row 0 holds them, the first TEV half a step behind the
    initial trailing edge (LUDVM.py:672-681), an LEV shed in step 1 at the leading edge, the bound vortices of step 1."""
    P, C, foil, gp = sim.path, sim.circulation, sim.path["airfoil"], sim.path["airfoil_gamma_points"]
    new = [foil[0, :, -1] + np.array([0.5 * sim.Uinf * sim.dt, 0.0])]
    g_new = [C["TEV"][0]]
    if sim.LEV_shed[1] != -1:
        new.append(foil[1, :, 0])
        g_new.append(C["LEV"][0])
    new = np.array(new).T
    g = np.concatenate([np.asarray(C["FREE"], float), g_new])
    return (g, np.concatenate([P["FREE"][0, 0], new[0]]), np.concatenate([P["FREE"][0, 1], new[1]]), C["airfoil"][0], gp[1, 0],
            gp[1, 1])


def sources_of(sim):
    return lambda i: first_step_sources(sim) if i == 1 else run_sources(sim, i)


def points_of(xz, frame, twin, pick=None):
    """step -> the survey's points of that step for a member whose pivot path is the twin's."""
    x, z = (np.asarray(xz)[0], np.asarray(xz)[1]) if pick is None else (np.asarray(xz)[0][pick], np.asarray(xz)[1][pick])
    return lambda i: ((x + twin.xpiv[int(i)] if frame == "tunnel" else x), z)


def reference_of(twin, xz, frame, steps, table=None, nbins=0, pick=None, lag=0):
    """-> (gsums [5, K], gmax, bin gsums [nbins, 5, K] or None): the long-double terms of every step of `steps` at the survey's
    points of that step over the twin's sources of step max(i - lag, 1), added in step order; a bin's block adds its steps'
    terms."""
    src = sources_of(twin)
    ref, gmax, per = SG.reference_sums(steps, points_of(xz, frame, twin, pick), lambda i: src(max(i - lag, 1)), twin.v_core)
    if not nbins:
        return ref, gmax, None
    bref = np.zeros((nbins,) + ref.shape)
    for i in steps:
        if table[i] >= 0:
            bref[table[i]] += per[i]
    return ref, gmax, bref


def member_window(steps, nt):
    first, stop, every = steps or (1, 10 ** 9, 1)
    return [int(i) for i in window(first, stop, every, nt)]
