"""Drop-in `LUDVM` class: the reference's constructor keywords, methods and result attributes
(jcatalang/LUDVM, LUDVM.py:132-1372), with the O(N^2) Vatistas-core Biot-Savart sums evaluated by
the gfx950 engine (libludvm_hip.so through ludvm_amd.engine.Engine).

What runs where
  * device: every induced-velocity evaluation -- wake -> chord points, unit new TEV/LEV -> chord
    points, wake+foil -> wake (fused with the explicit-Euler update), wake+foil -> flow-field grid,
    the vorticity stencil;  the wake stays resident on the device across time steps;
  * host (float64 NumPy, O(Npanels * Ncoeffs) per step): kinematics, vortex placement, the Gamma_TEV /
    Gamma_LEV solve, Fourier projection A0..A_N, bound-vorticity reconstruction, loads.  These are
    written as small matrix products (trapezoid weights, cos/sin tables) instead of the reference's
    interpreted loops (LUDVM.py:770-773, :994-1010).

There is no CPU implementation of the pair sum in this package: without the HIP library and an
MI355X the constructor raises.

Citations are file:line into the reference's LUDVM.py.
"""
import inspect
import timeit

import numpy as np

from . import _ffi
from .engine import Engine

__all__ = ["LUDVM", "SparseHistory"]

# The reference's dense trajectory arrays path['TEV'|'LEV'] are [nt, 2, nt-1] float64 (LUDVM.py:615-616): 32 nt^2 bytes.
# 'auto' keeps them -- and float64 pair sums, which cost nothing at those wake sizes -- while they fit this budget
# (nt <= 8191: every case the reference itself can run in a few minutes); beyond it rows are kept at
# snapshot_steps only and the wake-on-wake sums run in fp32 with local origins.
_DENSE_HISTORY_BUDGET_BYTES = 2 << 30


def _dense_history_fits(nt):
    return 32 * nt * nt <= _DENSE_HISTORY_BUDGET_BYTES


def naca4_mean_line(digits, x):
    """NACA 4-digit mean line (m = d0/100 at p = d1/10), x in chord fractions."""
    m, p = int(digits[0]) / 100.0, int(digits[1]) / 10.0
    x = np.asarray(x, dtype=float)
    if m == 0.0 or p == 0.0:
        return np.zeros_like(x)
    return np.where(x < p, m / p**2 * (2 * p * x - x**2), m / (1 - p) ** 2 * ((1 - 2 * p) + 2 * p * x - x**2))


class SparseHistory:
    """Trajectory rows kept only for selected time steps (the reference's dense [nt, 2, n] arrays are
    O(nt^2): 2 x 40 GB at dt = 1e-3, t in [0, 50]).  Indexing follows the dense arrays for the rows
    that exist: h[i] -> [2, n_i], h[i, 0, :k] -> view; other rows raise KeyError."""

    def __init__(self, nt):
        self.nt = nt
        self.rows = {}

    def store(self, i, row):
        self.rows[int(i)] = row

    def steps(self):
        return sorted(self.rows)

    def __contains__(self, i):
        return int(i) in self.rows

    def __getitem__(self, key):
        if isinstance(key, tuple):
            i, rest = key[0], key[1:]
        else:
            i, rest = key, ()
        i = int(i)
        if i < 0:
            i += self.nt
        if i not in self.rows:
            raise KeyError(f"time step {i} was not recorded (history='sparse'; recorded: {self.steps()[:8]}...)")
        row = self.rows[i]
        return row[rest] if rest else row


class LUDVM:
    """LESP-modulated unsteady discrete vortex method (see the reference's class docstring,
    LUDVM.py:133-229) on an MI355X.

    Same positional/keyword parameters as the reference constructor (LUDVM.py:231-236) and, like it,
    the whole simulation runs inside the constructor.  Keyword-only extras:
      engine     an existing ludvm_amd.engine.Engine to use (default: a new one on `device`)
      device     HIP device ordinal
      precision  arithmetic of the wake-on-wake pair sums: 'f32' (fp32 on local-origin positions: offsets from the
                 origin of each 256-vortex block of the wake), 'f32x2' (hi+lo fp32 positions), 'f64', or 'auto'
                 (default): 'f64' for runs short enough to keep the reference's dense history (nt <= 8191, wake
                 <= 16 000 vortices: fp64 costs little there and the reference's numbers are reproduced to ~1e-5
                 over the whole README run), 'f32' beyond.  The Npanels-target sums always run in fp64
      history    'full' (dense path arrays as in the reference), 'sparse' (rows only at
                 snapshot_steps + last step) or 'auto' (full while the arrays fit 2 GiB, nt <= 8191)
      snapshot_steps  iterable of time-step indices to record when history is sparse
      run        False builds geometry and kinematics only
      checkpoint_every, checkpoint_path   write an .npz checkpoint every so many steps (0 = never);
                 `LUDVM.resume(path)` continues such a run (the reference has no checkpointing)
      march      True (default): stretches of time steps whose history row is not recorded run as a
                 device-resident march (Gamma solve on the GPU, no host round trip per step);
                 False: one device round trip per step throughout
      probes     None (default), or points [2, P] (x row, z row; 1 <= P <= 4096) at which every time step also records the
                 velocity field that convects the wake in that step (LUDVM.py:1095-1106 with xp, zp = the points: wake before
                 the step's roll-up incl. the vortices shed in it, plus the step's bound vortices; Vatistas core, no freestream
                 term): `probe_u`, `probe_w` float64 [nt, P] (row 0: the field of the initial free vortices), `probe_xz` as
                 given, `probe_positions(step)` -> lab coordinates [2, P].  Evaluated inside the device-resident march (or from
                 two engine calls per step on the per-step path), always in float64: the signal the reference would compute
                 from its dense history, for runs that cannot keep one.  One GPU only.  Results are unchanged by it, bit for bit
      probe_frame  'lab' (default): the points are fixed in the lab frame; 'tunnel': x is measured from the pivot's
                 x-coordinate -- the lab position at step i is (x + xpiv[i], z) (the frame translates only)
      tracers    None (default), or seeds [2, M] (x row, z row; 1 <= M <= 262144) of passive tracers: particles advected by
                 the field that convects the wake, inside the device-resident march (or from two engine calls per step on
                 the per-step path), always in float64.  Tracer m is held at its seed until its release step r_m >= 1; in
                 step i >= r_m it moves from `start` -- the seed if i == r_m, else its position after step i - 1 -- to
                 start + dt (u, w)_i(start), (u, w)_i being exactly the field of `probes`.  Released at step 1 in the lab
                 frame this is, to rounding, the path['FREE'] trajectory of a zero-circulation free vortex at the same
                 seed -- but a tracer is no source of the roll-up, does not grow the wake, can be released during the run
                 and needs no dense history.  Results: `tracer_path`, a SparseHistory step -> [2, M] (row 0, the seeds,
                 always present), `tracer_last` [2, M] (positions after the final step), `tracer_xz`, `tracer_release`,
                 `tracer_frame` as given, `tracer_released(step)` -> bool [M].  Every other result is unchanged, bit for
                 bit.  A sweep takes them as sweep(..., particles=).  Out of scope: tracers on several GPUs, fp32 tracer
                 sums in a sweep, higher-order time integration (the reference's wake is forward Euler, and the tracers
                 follow it), tracers that interact with the foil
      tracer_release  None (all 1), or one integer release step >= 1 per tracer (a step >= nt: never released)
      tracer_frame  'lab' (default): seeds fixed in the lab frame; 'tunnel': a held tracer rides with the pivot -- its seed
                 at step i is (x + xpiv[i], z) -- and is released into the lab frame from there
      tracer_steps  time steps whose positions `tracer_path` keeps; None (default): every step when the run keeps a dense
                 history, snapshot_steps and the last step otherwise
      tracer_precision  'f64' (default): the tracers' pair sums in float64.  'f32x2': the pair arithmetic in fp32 on hi+lo
                 positions, inside the device-resident march only -- every float64 source and tracer position split into
                 (float)v and the float remainder, dx = (xh_p - xh_s) + (xl_p - xl_s), the sources in tiles of 256, a tile's
                 pairs summed in fp32, the tile sums, the source splits, the Euler update and the positions in float64.  No
                 origins and no fall-back: the error does not depend on where the wake is or how far it has rolled up.
                 Velocities within 2e-6 of max|u| of the 'f64' ones (DESIGN.md section 4.9 has the figures and the cost); every
                 other result keeps its bits, and the paths repeat bit for bit however the run is cut, checkpoints included
                 (they carry the value).  Refused: without `tracers`, with march=False, in a sweep; a run that cannot take the
                 march raises instead of falling back to float64.  The object carries `tracer_precision` as used
      tracer_gradient  False (default).  True: every tracer carries the deformation gradient of its own path with respect to
                 its seed, F = [[dx/dX, dx/dZ], [dz/dX, dz/dZ]].  The sources of a step do not depend on a tracer, so the exact
                 derivative of the discrete forward-Euler map is one 2 x 2 product per step, F <- (I + dt G_i(start)) F with G_i
                 the gradient of (u, w)_i in closed form (`velocity_gradient`) at the step's start position; F is the identity
                 while a tracer is held and at its release.  Evaluated inside the device-resident march by a gradient version of
                 the float64 tracer kernels under the same launch plan.  Results: `tracer_F_path`, a SparseHistory step ->
                 [4, M] in the order F11, F12, F21, F22 (row 0: the identity; the steps of `tracer_path`), `tracer_F_last`
                 [4, M], `tracer_ftle(step=None)` -> [M], the finite-time Lyapunov exponent ln sigma_max(F) / T with T = dt (step
                 - release + 1), NaN for a tracer not yet released (`ftle_from_F(F, T)` for any F).  The tracer positions and
                 every other result keep their bits; F repeats bit for bit however the run is cut, checkpoints included (they
                 carry it).  Refused: without `tracers`, with march=False, with tracer_precision='f32x2', in a sweep, with
                 `distributed` or more than one device; a run that cannot take the march raises.  Out of scope: backward-time
                 FTLE, the gradient on the per-step path.
                 'f32x2' (needs tracer_precision='f32x2'): the same F from ONE walk over the sources in packed fp32 on hi+lo
                 positions -- per pair the plain 'f32x2' tracers' operations for u and w, then the gradient's three raw sums
                 from the same differences and reciprocal square root; the tile sums, the Euler update and the product in
                 float64.  The positions are, bit for bit, the plain 'f32x2' tracers'; each component of G_i is within
                 (152 * 2^-23 + (ns + 16) * 2^-52) sum|G| / (2 pi v_core^2) of the exact sum wherever the wake is (DESIGN.md
                 section 4.18 has the cost).  Same results, same refusals, `tracer_gradient` holds 'f32x2'
      survey     None (default), or the points of a wake survey: a [2, K] array (x row, z row), or a dict(xmin, xmax, zmin, zmax,
                 dr) meaning the mesh arange(xmin, xmax, dr) x arange(zmin, zmax, dr), x-major as `flowfield` builds it
                 (1 <= K <= 1048576).  In every sampled step the field of `probes` is evaluated at the points and added to
                 five raw float64 sums per point (u, w, u^2, w^2, u w) -- inside the device-resident march, beside the resident
                 wake, with storage that does not depend on the number of steps (or from two engine calls per sampled step on
                 the per-step path).  Results, mesh-shaped [nx, nz] for a dict and [K] otherwise: `survey_x`, `survey_z`,
                 `survey_count` (sampled steps), `survey_sums` [5, ...], `survey_mean_u`, `survey_mean_w`, and the central
                 second moments `survey_uu`, `survey_ww`, `survey_uw` = sum(ab)/n - (sum(a)/n)(sum(b)/n) (the Reynolds
                 stresses of the time-averaged wake); `survey_frame`, `survey_steps` as used.  No freestream term.  Every
                 other result is unchanged, bit for bit; the sums repeat bit for bit however the run is cut (chunks,
                 snapshot_steps, history, checkpoint / resume).  A sweep takes it as sweep(..., survey=).  Out of scope: a survey on
                 several GPUs, fp32 sums in a sweep, field snapshots (`flowfield` on snapshot_steps), thrust integration
      survey_frame  'lab' (default): the points are fixed in the lab frame; 'tunnel': x is measured from the pivot's
                 x-coordinate -- in step i point k sits at (x[k] + xpiv[i], z[k])
      survey_steps  (first, stop, every): the sampled steps are first <= i < stop with (i - first) % every == 0; first >= 1,
                 every >= 1, stop is clipped to nt; default (1, nt, 1).  An empty window is refused
      survey_precision  'f64' (default): the survey's pair sums in float64.  'f32': the pair arithmetic in fp32 on local origins,
                 inside the device-resident march only -- the sources in tiles of 256, two origin classes of 128 per tile by index
                 parity, each referred to the float64 position of its middle member; a class's 128 pairs summed in fp32, the
                 class sums, the source splits and the five moments in float64; a class wider than 300 v_core is evaluated in
                 float64.  Means within 1e-5 of max|u| of the 'f64' survey, raw second moments within 3e-5 of max|u|^2, at a
                 quarter of the cost per sampled step where the classes are compact and 0.8 of it on a long run's rolled-up
                 wake; every other result keeps its bits, and the sums repeat bit for bit
                 however the run is cut, checkpoints included (they carry the value).  Refused: without `survey`, with
                 march=False, in a sweep; a run that cannot take the march raises instead of falling back to float64.  The
                 object carries `survey_precision` as used
      survey_bins  None (default), or the bins of a phase-locked (conditional) survey: an int B (1 .. 64) divides the motion's
                 period into B equal phase bins -- with t = self.t, tau = (t - survey_phase0) / survey_period, the bin of a step is
                 floor(B (tau - floor(tau)) + 1e-9) % B -- or an integer array [nt] with values -1 .. B-1 (B = max + 1) gives the
                 bin of every time step by any criterion (-1: none).  In a sampled step whose bin is b >= 0 the five terms the
                 step adds to the survey's sums are added to bin b's own five sums as well (inside the device-resident march: one
                 finisher kernel per sampled step, as without bins; or beside the plain sums on the per-step path); B x K <=
                 4194304.  Results, mesh-shaped as the survey's: `survey_nbins`, `survey_bin_of_step` (int64 [nt]: the table as
                 the run uses it, -1 where a step is not sampled or has no bin), `survey_bin_count` [B], `survey_bin_sums`
                 [B, 5, ...], `survey_bin_mean_u`, `survey_bin_mean_w`, the central moments within each bin `survey_bin_uu`,
                 `survey_bin_ww`, `survey_bin_uw` (nan for an empty bin), `survey_phase` [B] (bin centres (b + 0.5) / B; None for
                 a table), and the triple decomposition over the binned samples (N = sum n_b): `survey_coherent_uu`, `_ww`, `_uw`
                 = sum_b n_b (a_b - a)(b_b - b) / N of the bin means about the mean, `survey_random_uu`, `_ww`, `_uw` = sum_b
                 n_b survey_bin_ab[b] / N; coherent + random is the total central moment, `survey_uu` / `ww` / `uw` when every
                 sampled step has a bin.  A bin's sums are, bit for bit, the plain sums of a survey that samples that bin's steps;
                 the plain sums and every other result keep their bits; the bin sums repeat bit for bit however the run is cut,
                 checkpoints included.  Refused: without `survey`, B outside 1 .. 64, B x K over the
                 cap, a table that is not [nt] integers >= -1, a window in which no sampled step has a bin, in a sweep
      survey_period  the period, a time, of the int form of `survey_bins`; default 1 / self.f, the period of the motion (refused
                 when that is infinite, and when not finite and positive)
      survey_phase0  the time of phase 0 of the int form of `survey_bins`; default t0
      survey_gradient  False (default).  True: every sampled step also adds the closed-form gradient of the survey's field at the
                 survey points to five more raw float64 sums per point, ux = du/dx, e = (du/dz + dw/dx) / 2, omega = dw/dx - du/dz,
                 omega^2 and Q = omega^2 / 4 - ux^2 - e^2 (= -ux^2 - uz wx; Q > 0 marks a vortex core) -- inside the device-resident
                 march, under the plain survey's launch plan, so every velocity sum keeps its bits -- and, with `survey_bins`, to
                 the step's bin block.  Results, shaped like `survey_x`: `survey_grad_sums` [5, ...], `survey_mean_ux`,
                 `survey_mean_strain` (mean e), `survey_mean_omega`, `survey_mean_uz` = mean e - mean omega / 2, `survey_mean_wx`
                 = mean e + mean omega / 2, `survey_omega2` (sum omega^2 / n: twice the mean enstrophy), `survey_omega_var`,
                 `survey_mean_q`, and `survey_production` = -(uu ux + uw 2 e - ww ux), the production of fluctuation energy from
                 the survey's own Reynolds stresses and these means (dw/dz = -du/dx).  With bins: `survey_bin_grad_sums`
                 [B, 5, ...], `survey_bin_mean_ux`, `_strain`, `_omega`, `_q`, `survey_bin_omega2`, and `survey_coherent_omega2` /
                 `survey_random_omega2`, the variance of omega split as the velocity moments are.  The counts are the velocity
                 sums' own.  The sums are bit-identical however the run is cut, checkpoints included.  The
                 per-step path (march=False) adds the same terms from `Engine.gradient_field`.  Refused: not a bool or 'f32x2',
                 without `survey`, with survey_precision='f32', in a sweep, with `devices` > 1 or `distributed`.
                 'f32x2': the same ten sums and result attributes with the pair arithmetic in fp32 -- in every sampled step u, w
                 and the raw sums A, B, C at every survey point come from ONE walk over the step's sources, in packed fp32 on
                 hi+lo positions (the walk of tracer_gradient='f32x2'); tile sums, splits and all sums stay float64.  The fused
                 walk takes the place of the survey's pair walk, so the VELOCITY sums of such a survey are the fused walk's too:
                 hi+lo tier (means within 2e-6 of max|u| of the float64 survey's), not float64 bits.  The error does not depend
                 on where the wake is or how far it has rolled up; every other result of the run keeps its bits; the sums are
                 bit-identical however the run is cut, and a bin is still the plain sums of its steps.
                 Not a survey precision: refused with survey_precision other than 'f64' (it brings its own arithmetic), with
                 march=False, and with a run that cannot take the march (RuntimeError, no float64 in its place)
      wake_integrals  False (default).  True: every time step also records the classical integrals of its vortex SYSTEM -- what
                 the probes see: the wake before the step's Euler update, the vortices shed in the step at their placement, the
                 bound vortices of the step, in the lab frame -- inside the device-resident march, float64.  `integral_sums`
                 [nt, 4, 2, 6]: for every class of `integral_classes` = ('FREE', 'TEV', 'LEV', 'BOUND') and sign (slot 0: Gamma >= 0,
                 slot 1: Gamma < 0) the count, sum G, sum G x, sum G z, sum G (x^2 + z^2), sum G^2 (row 0: the initial free
                 vortices).  From them, on the host: `wake_circulation(cls, sign)`, `wake_centroid(cls, sign)`, `wake_impulse`
                 [nt, 2] = rho (-sum G z, sum G x), `wake_angular_impulse`, `impulse_force` = -dI/dt, `impulse_Cl`, `impulse_Cd` (a
                 check of `Cl`, `Cd` by another route through the physics).  The rows are bit-identical however the run is cut,
                 checkpoints included, and every other result of the run keeps its bits.  The per-step
                 path (march=False) forms the same rows on the host.  Refused: not a bool, in a sweep (a solo keyword), with
                 `devices` > 1 or `distributed`
      wake_energy_steps  None (default), or (first, stop, every) in `survey_steps`' form: at those steps the Hamiltonian of the
                 system, W = 1/2 sum_a sum_b G_a G_b / (4 pi) ln((r_ab^2 + s_ab) / 2) = 1/2 sum_a G_a psi(x_a) over all its vortices
                 (a = b included; the pair term of `stream_function`), goes to `wake_energy` [nt] (NaN where not sampled);
                 `wake_energy_interaction` is W minus the self part ln(v_core^2 / 2) / (8 pi) sum G^2.  Gamma is clockwise-positive
                 (its vorticity is -Gamma), so the kinetic energy per unit span is -rho W: W falls as the foil works on the
                 fluid.  An O(N^2) float64 pair sum per sample.  Needs wake_integrals=True
      devices    several GPUs of this node in ONE process, no launcher: an int G (devices 0 .. G-1) or a list of ordinals.  One host
                 thread, one engine and one replica per device, the library's own RCCL communicator over them (ncclCommInitAll);
                 the object returned is a front whose attributes are replica 0's and whose methods run on all replicas
                 (ludvm_amd/multi.py; `close()` ends the threads).  One device: an ordinary run on it
      distributed  None (default): one GPU.  'rccl': the simulation is shared by the processes of one launch (one per GPU;
                 rank and world from the launcher's environment), connected by the library's own RCCL communicator --
                 no torch.distributed (ludvm_amd/comm.py).  True or a torch.distributed process group: the same through
                 torch's collectives (ludvm_amd/distributed.py).  Either way every rank constructs the same object and
                 calls the same methods; flowfield shards the grid rows, induced_velocity the targets, time_loop the
                 roll-up's unordered pairs (one integer all-reduce per step over RCCL), and every rank ends up with the
                 reference's full result arrays
    """

    def __new__(cls, *args, devices=None, **kwargs):
        # devices=[...] with more than one GPU: ONE process, one host thread and one replica per device, the library's own
        # communicator over them (ludvm_amd/multi.py) -- the object returned is that front, not an instance of this class
        if devices is not None and cls is LUDVM:
            from .multi import MultiDeviceLUDVM, normalise_devices
            devs = normalise_devices(devices)
            if len(devs) > 1:
                if kwargs.get('probes') is not None:
                    cls._check_probes(kwargs['probes'], kwargs.get('probe_frame', 'lab'))
                    raise ValueError("probes run on one GPU: not with more than one device in `devices`")
                if kwargs.get('wake_integrals', False) is not False or kwargs.get('wake_energy_steps') is not None:
                    cls._check_wake_integrals(kwargs.get('wake_integrals', False), kwargs.get('wake_energy_steps'))
                    raise ValueError("wake_integrals runs on one GPU: not with more than one device in `devices`")
                if kwargs.get('tracer_gradient', False) is not False:
                    cls._check_tracer_gradient(kwargs['tracer_gradient'], kwargs.get('tracers') is not None,
                                               kwargs.get('march', True), kwargs.get('tracer_precision', 'f64'))
                    raise ValueError("tracer_gradient runs on one GPU: not with more than one device in `devices`")
                if kwargs.get('tracers') is not None:
                    cls._check_tracers(kwargs['tracers'], kwargs.get('tracer_release'), kwargs.get('tracer_frame', 'lab'))
                    raise ValueError("tracers run on one GPU: not with more than one device in `devices`")
                if kwargs.get('survey_gradient', False) is not False:
                    cls._check_survey_gradient(kwargs['survey_gradient'], kwargs.get('survey') is not None,
                                               kwargs.get('survey_precision', 'f64'), kwargs.get('march', True))
                    raise ValueError("survey_gradient runs on one GPU: not with more than one device in `devices`")
                if kwargs.get('survey') is not None:
                    cls._check_survey(kwargs['survey'], kwargs.get('survey_frame', 'lab'), kwargs.get('survey_steps'))
                    raise ValueError("a survey runs on one GPU: not with more than one device in `devices`")
                return MultiDeviceLUDVM(args, kwargs, devs)
        return super().__new__(cls)

    @staticmethod
    def _check_probes(probes, probe_frame):
        """-> float64 [2, P], or ValueError (nothing else has been created yet)."""
        if probe_frame not in ('lab', 'tunnel'):
            raise ValueError("probe_frame must be 'lab' or 'tunnel'")
        try:
            xz = np.array(probes, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("probes must be an array-like [2, P] of numbers") from e
        if xz.ndim != 2 or xz.shape[0] != 2 or xz.shape[1] < 1:
            raise ValueError(f"probes must be [2, P] with P >= 1 (x row, z row); got shape {xz.shape}")
        if xz.shape[1] > 4096:
            raise ValueError(f"probes: at most 4096 points (got {xz.shape[1]})")
        if not np.isfinite(xz).all():
            raise ValueError("probes must be finite")
        return np.ascontiguousarray(xz)

    @staticmethod
    def _check_survey(survey, survey_frame, survey_steps=None, nt=None):
        """-> (float64 [2, K], the results' shape (nx, nz) or (K,), (first, stop, every) with stop clipped to nt), or ValueError
        (nothing else has been created yet)."""
        if survey_frame not in ('lab', 'tunnel'):
            raise ValueError("survey_frame must be 'lab' or 'tunnel'")
        most = 1048576
        if isinstance(survey, dict):
            if set(survey) != {'xmin', 'xmax', 'zmin', 'zmax', 'dr'}:
                raise ValueError("survey: a dict has exactly the keys xmin, xmax, zmin, zmax, dr")
            try:
                xmin, xmax, zmin, zmax, dr = (float(survey[k]) for k in ('xmin', 'xmax', 'zmin', 'zmax', 'dr'))
            except (TypeError, ValueError) as e:
                raise ValueError("survey: xmin, xmax, zmin, zmax, dr must be numbers") from e
            if not np.isfinite([xmin, xmax, zmin, zmax, dr]).all():
                raise ValueError("survey must be finite")
            if not dr > 0.0:
                raise ValueError(f"survey: dr must be > 0 (got {dr})")
            if not (xmax > xmin and zmax > zmin):
                raise ValueError("survey: the mesh is empty (xmax > xmin and zmax > zmin)")
            if np.ceil((xmax - xmin) / dr) * np.ceil((zmax - zmin) / dr) > most:      # (before any mesh is built)
                raise ValueError(f"survey: at most {most} points")
            x1, z1 = np.arange(xmin, xmax, dr), np.arange(zmin, zmax, dr)
            x, z = np.meshgrid(x1, z1, indexing='ij')
            xz, shape = np.stack([x.ravel(), z.ravel()]), (len(x1), len(z1))
        else:
            try:
                xz = np.array(survey, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError("survey must be an array-like [2, K] of numbers, or a dict(xmin, xmax, zmin, zmax, dr)") from e
            if xz.ndim != 2 or xz.shape[0] != 2:
                raise ValueError(f"survey must be [2, K] (x row, z row); got shape {xz.shape}")
            shape = (xz.shape[1],)
        K = xz.shape[1]
        if K < 1:
            raise ValueError("survey: at least one point")
        if K > most:
            raise ValueError(f"survey: at most {most} points (got {K})")
        if not np.isfinite(xz).all():
            raise ValueError("survey must be finite")
        if survey_steps is None:
            survey_steps = (1, nt if nt is not None else 1 << 62, 1)
        try:
            raw = list(survey_steps)
            first, stop, every = (int(v) for v in raw)
        except (TypeError, ValueError) as e:
            raise ValueError("survey_steps must be three integers (first, stop, every)") from e
        if any(int(v) != v for v in raw):
            raise ValueError("survey_steps must be three integers (first, stop, every)")
        if first < 1 or every < 1:
            raise ValueError("survey_steps: first >= 1 and every >= 1")
        if nt is not None:
            stop = min(stop, nt)
        if stop <= first:
            raise ValueError(f"survey_steps: the window [{first}, {stop}) holds no time step")
        return np.ascontiguousarray(xz), shape, (first, stop, every)

    @staticmethod
    def _check_wake_integrals(wake_integrals, wake_energy_steps, nt=None):
        """-> the energy window (first, stop, every) with stop clipped to nt, or None; ValueError from the keywords alone (nothing
        else has been created yet)."""
        if not isinstance(wake_integrals, (bool, np.bool_)):
            raise ValueError(f"wake_integrals must be a bool (got {wake_integrals!r})")
        if wake_energy_steps is None:
            return None
        if not wake_integrals:
            raise ValueError("wake_energy_steps needs wake_integrals=True")
        # (survey_steps' form and validation: one point stands in for the survey)
        try:
            return LUDVM._check_survey(np.zeros([2, 1]), 'lab', wake_energy_steps, nt=nt)[2]
        except ValueError as e:
            raise ValueError(str(e).replace('survey_steps', 'wake_energy_steps')) from e

    @staticmethod
    def _check_survey_precision(survey_precision, surveyed, march=True):
        """ValueError from the keywords alone (nothing else has been created yet)."""
        if not isinstance(survey_precision, str) or survey_precision not in ('f64', 'f32'):
            raise ValueError(f"survey_precision must be 'f64' or 'f32' (got {survey_precision!r})")
        if survey_precision != 'f64' and not surveyed:
            raise ValueError("survey_precision needs `survey`")
        if survey_precision == 'f32' and not march:
            raise ValueError("survey_precision='f32' is evaluated inside the device-resident march: not with march=False")

    @staticmethod
    def _check_survey_bins(survey_bins, survey_period, survey_phase0, K, win, t, t0, f):
        """-> (survey_bin_of_step int64 [nt]: the bin of every sampled step, -1 elsewhere; B; the bin centres [B] or None for an
        explicit table), or ValueError (nothing else has been created yet).  K: survey points; win: the window as used; t: the
        time levels; f: the motion's frequency."""
        most, nt = _ffi.MARCH_MAX_SURVEY_BINS, len(t)
        if survey_bins is None:
            raise ValueError("survey_period / survey_phase0 need `survey_bins`")
        for name, v in (("survey_period", survey_period), ("survey_phase0", survey_phase0)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v)):
                raise ValueError(f"{name} must be a finite number (got {v!r})")
        if survey_period is not None and not survey_period > 0:
            raise ValueError(f"survey_period must be finite and > 0 (got {survey_period!r})")
        if isinstance(survey_bins, bool):
            raise ValueError("survey_bins must be an int B or an integer array [nt]")
        if isinstance(survey_bins, (int, np.integer)):
            B = int(survey_bins)
            if not 1 <= B <= most:
                raise ValueError(f"survey_bins: 1 <= B <= {most} (got {B})")
            if survey_period is None:
                if not f > 0:
                    raise ValueError("survey_bins: the motion has no period (k = 0): give survey_period")
                survey_period = 1.0 / f
            tau = (t - (t0 if survey_phase0 is None else survey_phase0)) / survey_period
            table = (np.floor(B * (tau - np.floor(tau)) + 1e-9).astype(np.int64)) % B
            phase = (np.arange(B) + 0.5) / B
        else:
            if survey_period is not None or survey_phase0 is not None:
                raise ValueError("survey_period / survey_phase0 go with survey_bins=B (an int), not with an explicit table")
            try:
                raw = np.asarray(survey_bins)
            except (TypeError, ValueError) as e:
                raise ValueError("survey_bins must be an int B or an integer array [nt]") from e
            if raw.dtype.kind not in 'iu' or raw.shape != (nt,):
                raise ValueError(f"survey_bins: a table holds one integer per time step, [nt] with nt = {nt}")
            table = raw.astype(np.int64)
            if table.min() < -1:
                raise ValueError("survey_bins: a table's entries are -1 (no bin) or a bin 0 .. B-1")
            B, phase = int(table.max()) + 1, None
            if B > most:
                raise ValueError(f"survey_bins: at most {most} bins (the table's largest entry is {B - 1})")
        if B * K > _ffi.MARCH_MAX_SURVEY_BIN_POINTS:
            raise ValueError(f"survey_bins: {B} bins x {K} points: at most {_ffi.MARCH_MAX_SURVEY_BIN_POINTS} bins x points "
                             "(40 bytes of sums each)")
        first, stop, every = win
        sampled = np.zeros(nt, dtype=bool)
        sampled[first:stop:every] = True
        table = np.where(sampled, table, -1)
        if B < 1 or not (table >= 0).any():
            raise ValueError("survey_bins: no sampled step of the window has a bin")
        return table, B, phase

    @staticmethod
    def _check_tracer_precision(tracer_precision, traced, march=True):
        """ValueError from the keywords alone (nothing else has been created yet)."""
        if not isinstance(tracer_precision, str) or tracer_precision not in ('f64', 'f32x2'):
            raise ValueError(f"tracer_precision must be 'f64' or 'f32x2' (got {tracer_precision!r})")
        if tracer_precision != 'f64' and not traced:
            raise ValueError("tracer_precision needs `tracers`")
        if tracer_precision == 'f32x2' and not march:
            raise ValueError("tracer_precision='f32x2' is evaluated inside the device-resident march: not with march=False")

    @staticmethod
    def _check_tracer_gradient(tracer_gradient, traced, march=True, tracer_precision='f64'):
        """ValueError from the keywords alone (nothing else has been created yet)."""
        f32x2 = isinstance(tracer_gradient, str) and tracer_gradient == 'f32x2'
        if not f32x2 and not isinstance(tracer_gradient, (bool, np.bool_)):
            raise ValueError(f"tracer_gradient must be True or False, or 'f32x2' (got {tracer_gradient!r})")
        if not tracer_gradient:
            return
        if not traced:
            raise ValueError("tracer_gradient needs `tracers`")
        if not march:
            raise ValueError("tracer_gradient is evaluated inside the device-resident march: not with march=False")
        if f32x2:
            if tracer_precision != 'f32x2':
                raise ValueError("tracer_gradient='f32x2' needs tracer_precision='f32x2' (its positions are the hi+lo fp32 tracers'): "
                                 f"not with tracer_precision={tracer_precision!r}")
        elif tracer_precision != 'f64':
            raise ValueError(f"tracer_gradient needs float64 tracers: not with tracer_precision={tracer_precision!r} "
                             "(tracer_gradient='f32x2' is the fp32 route)")

    @staticmethod
    def _check_survey_gradient(survey_gradient, surveyed, survey_precision='f64', march=True):
        """ValueError from the keywords alone (nothing else has been created yet)."""
        f32x2 = isinstance(survey_gradient, str) and survey_gradient == 'f32x2'
        if not f32x2 and not isinstance(survey_gradient, (bool, np.bool_)):
            raise ValueError(f"survey_gradient must be True or False, or 'f32x2' (got {survey_gradient!r})")
        if not survey_gradient:
            return
        if not surveyed:
            raise ValueError("survey_gradient needs `survey`")
        if f32x2:
            if survey_precision != 'f64':
                raise ValueError("survey_gradient='f32x2' brings its own arithmetic (one hi+lo fp32 walk for the velocity and the "
                                 f"gradient sums): not with survey_precision={survey_precision!r}")
            if not march:
                raise ValueError("survey_gradient='f32x2' is evaluated inside the device-resident march: not with march=False")
        elif survey_precision != 'f64':
            raise ValueError(f"survey_gradient needs a float64 survey: not with survey_precision={survey_precision!r}")

    @staticmethod
    def ftle_from_F(F, T):
        """Finite-time Lyapunov exponent ln sigma_max(F) / T of deformation gradients F [4, ...] (F11, F12, F21, F22) over the
        times T (a number or an array of the trailing shape): sigma_max^2 = (|F|^2 + sqrt(|F|^4 - 4 det^2)) / 2 with |F| the
        Frobenius norm -- the radicand formed as its factors ((F11 - F22)^2 + (F12 + F21)^2) ((F11 + F22)^2 + (F12 - F21)^2), which
        do not cancel where the two singular values are close (F near the identity or a rotation).  Plain numpy; NaN where
        T <= 0."""
        F = np.asarray(F, dtype=np.float64)
        if F.shape[0] != 4:
            raise ValueError(f"ftle_from_F: F must be [4, ...] (F11, F12, F21, F22); got shape {F.shape}")
        f11, f12, f21, f22 = F
        n2 = f11 * f11 + f12 * f12 + f21 * f21 + f22 * f22
        rad = ((f11 - f22)**2 + (f12 + f21)**2) * ((f11 + f22)**2 + (f12 - f21)**2)       # = |F|^4 - 4 det^2
        s2 = 0.5 * (n2 + np.sqrt(rad))
        T = np.broadcast_to(np.asarray(T, dtype=np.float64), s2.shape)
        out = np.full(s2.shape, np.nan)
        ok = T > 0
        with np.errstate(divide='ignore', invalid='ignore'):
            out[ok] = 0.5 * np.log(s2[ok]) / T[ok]
        return out

    @staticmethod
    def _check_tracers(tracers, tracer_release, tracer_frame, tracer_steps=None, nt=None):
        """-> (float64 [2, M], int64 [M], sorted steps or None), or ValueError (nothing else has been created yet)."""
        if tracer_frame not in ('lab', 'tunnel'):
            raise ValueError("tracer_frame must be 'lab' or 'tunnel'")
        try:
            xz = np.array(tracers, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("tracers must be an array-like [2, M] of numbers") from e
        if xz.ndim != 2 or xz.shape[0] != 2 or xz.shape[1] < 1:
            raise ValueError(f"tracers must be [2, M] with M >= 1 (x row, z row); got shape {xz.shape}")
        M = xz.shape[1]
        if M > 262144:
            raise ValueError(f"tracers: at most 262144 (got {M})")
        if not np.isfinite(xz).all():
            raise ValueError("tracers must be finite")
        if tracer_release is None:
            rel = np.ones(M, dtype=np.int64)
        else:
            try:
                rel = np.asarray(tracer_release)
            except (TypeError, ValueError) as e:
                raise ValueError("tracer_release must be integers [M]") from e
            if rel.dtype.kind not in 'iu' or rel.shape != (M,):
                raise ValueError(f"tracer_release must be integers [M] with M = {M} (one release step per tracer)")
            if rel.min() < 1:
                raise ValueError("tracer_release: release steps are >= 1")
            rel = rel.astype(np.int64)
        steps = None
        if tracer_steps is not None:
            try:
                raw = [s for s in tracer_steps]
                steps = sorted({int(s) for s in raw})
            except (TypeError, ValueError) as e:
                raise ValueError("tracer_steps must be an iterable of time steps") from e
            if any(int(s) != s for s in raw):
                raise ValueError("tracer_steps must be integers")
            if nt is not None and steps and (steps[0] < 0 or steps[-1] >= nt):
                raise ValueError(f"tracer_steps must lie in [0, {nt})")
        return np.ascontiguousarray(xz), rel, steps

    def __init__(self, t0=0, tf=12, dt=1.5e-2, chord=1, rho=1.225, Uinf=1,
                 Npoints=80, Ncoeffs=30, LESPcrit=0.2, Naca='0012',
                 foil_filename=None, G=1, T=2, alpha_m=0,
                 alpha_max=10, k=0.2 * np.pi, phi=90, h_max=1,
                 verbose=True, method='Faure',
                 circulation_freevort=None, xy_freevort=None, *,
                 engine=None, device=0, precision='auto', history='auto', snapshot_steps=(), run=True,
                 checkpoint_every=0, checkpoint_path=None, march=True, distributed=None, devices=None,
                 probes=None, probe_frame='lab', tracers=None, tracer_release=None, tracer_frame='lab', tracer_steps=None,
                 survey=None, survey_frame='lab', survey_steps=None, survey_precision='f64', tracer_precision='f64',
                 survey_bins=None, survey_period=None, survey_phase0=None, tracer_gradient=False, survey_gradient=False,
                 wake_integrals=False, wake_energy_steps=None):
        # refused before any engine, thread or communicator exists
        energy_win = self._check_wake_integrals(wake_integrals, wake_energy_steps, nt=len(np.arange(t0, tf + dt, dt)))
        if wake_integrals and distributed is not None and distributed is not False:
            raise ValueError("wake_integrals runs on one GPU: not with `distributed`")
        if probes is not None:
            # refused before any engine, thread or communicator exists
            probe_xz = self._check_probes(probes, probe_frame)
            if distributed is not None and distributed is not False:
                raise ValueError("probes run on one GPU: not with `distributed`")
        elif probe_frame not in ('lab', 'tunnel'):
            raise ValueError("probe_frame must be 'lab' or 'tunnel'")
        if tracers is not None:
            # refused before any engine, thread or communicator exists
            tracer_xz, tracer_rel, tracer_rec = self._check_tracers(tracers, tracer_release, tracer_frame, tracer_steps,
                                                                    nt=len(np.arange(t0, tf + dt, dt)))
            if distributed is not None and distributed is not False:
                raise ValueError("tracers run on one GPU: not with `distributed`")
        elif tracer_frame not in ('lab', 'tunnel'):
            raise ValueError("tracer_frame must be 'lab' or 'tunnel'")
        elif tracer_release is not None or tracer_steps is not None:
            raise ValueError("tracer_release / tracer_steps need `tracers`")
        self._check_tracer_precision(tracer_precision, tracers is not None, march)
        self._check_tracer_gradient(tracer_gradient, tracers is not None, march, tracer_precision)
        if tracer_gradient and distributed is not None and distributed is not False:
            raise ValueError("tracer_gradient runs on one GPU: not with `distributed`")
        if survey is not None:
            # refused before any engine, thread or communicator exists
            survey_xz, survey_shape, survey_win = self._check_survey(survey, survey_frame, survey_steps,
                                                                     nt=len(np.arange(t0, tf + dt, dt)))
            if distributed is not None and distributed is not False:
                raise ValueError("a survey runs on one GPU: not with `distributed`")
        elif survey_frame not in ('lab', 'tunnel'):
            raise ValueError("survey_frame must be 'lab' or 'tunnel'")
        elif survey_steps is not None:
            raise ValueError("survey_steps needs `survey`")
        self._check_survey_gradient(survey_gradient, survey is not None, survey_precision, march)
        if survey_gradient and distributed is not None and distributed is not False:
            raise ValueError("survey_gradient runs on one GPU: not with `distributed`")
        self._check_survey_precision(survey_precision, survey is not None, march)
        binned = survey_bins is not None or survey_period is not None or survey_phase0 is not None
        if binned:
            if survey is None:
                raise ValueError("survey_bins / survey_period / survey_phase0 need `survey`")
            bin_table, bin_count, bin_phase = self._check_survey_bins(
                survey_bins, survey_period, survey_phase0, survey_xz.shape[1], survey_win, np.arange(t0, tf + dt, dt), t0,
                k * Uinf / (2 * np.pi * chord))
        # the smallest section the method runs: two panels; the loads read A0 .. A3 (LUDVM.py:1035-1090)
        if Npoints < 3:
            raise ValueError(f"Npoints={Npoints}: a section has at least 3 points (2 panels)")
        if Ncoeffs < 4:
            raise ValueError(f"Ncoeffs={Ncoeffs}: at least 4 Fourier coefficients (the loads use A0 .. A3)")
        if devices is not None:             # (one device: an ordinary single-GPU run on it)
            from .multi import normalise_devices
            device = normalise_devices(devices)[0]
        self._ctor = dict(t0=t0, tf=tf, dt=dt, chord=chord, rho=rho, Uinf=Uinf, Npoints=Npoints, Ncoeffs=Ncoeffs,
                          LESPcrit=LESPcrit, Naca=Naca, foil_filename=foil_filename, G=G, T=T, alpha_m=alpha_m,
                          alpha_max=alpha_max, k=k, phi=phi, h_max=h_max, method=method, precision=precision,
                          history=history, snapshot_steps=sorted(int(s) for s in snapshot_steps))
        if probes is not None:              # (a run without probes keeps the attributes -- and the checkpoints -- it had)
            self._ctor.update(probes=probe_xz.tolist(), probe_frame=probe_frame)
            self.probe_xz, self.probe_frame = probe_xz, probe_frame
        if tracers is not None:             # (likewise)
            self._ctor.update(tracers=tracer_xz.tolist(), tracer_release=tracer_rel.tolist(), tracer_frame=tracer_frame,
                              tracer_steps=tracer_rec)
            self.tracer_xz, self.tracer_release, self.tracer_frame = tracer_xz, tracer_rel, tracer_frame
            self._tracer_steps = tracer_rec
            self.tracer_precision = tracer_precision
            if self.tracer_precision != 'f64':      # (float64 tracers keep the checkpoints they had)
                self._ctor.update(tracer_precision=self.tracer_precision)
            self.tracer_gradient = 'f32x2' if isinstance(tracer_gradient, str) else bool(tracer_gradient)
            if self.tracer_gradient:                # (tracers without it likewise)
                self._ctor.update(tracer_gradient=self.tracer_gradient)
        if survey is not None:              # (likewise; a mesh travels as its five numbers)
            self._ctor.update(survey={k: float(v) for k, v in survey.items()} if isinstance(survey, dict) else survey_xz.tolist(),
                              survey_frame=survey_frame, survey_steps=list(survey_win))
            self._survey_xz, self._survey_shape = survey_xz, survey_shape
            self.survey_x, self.survey_z = survey_xz[0].reshape(survey_shape), survey_xz[1].reshape(survey_shape)
            self.survey_frame, self.survey_steps = survey_frame, survey_win
            self.survey_precision = survey_precision
            if self.survey_precision != 'f64':      # (a float64 survey keeps the checkpoints it had)
                self._ctor.update(survey_precision=self.survey_precision)
            if binned:                              # (a survey without bins keeps the checkpoints it had)
                self._ctor.update(survey_bins=int(survey_bins) if np.ndim(survey_bins) == 0 else [int(v) for v in np.asarray(survey_bins).reshape(-1)],
                                  survey_period=None if survey_period is None else float(survey_period),
                                  survey_phase0=None if survey_phase0 is None else float(survey_phase0))
                self.survey_nbins, self.survey_bin_of_step, self.survey_phase = bin_count, bin_table, bin_phase
            self.survey_gradient = 'f32x2' if isinstance(survey_gradient, str) else bool(survey_gradient)
            if self.survey_gradient:                # (a survey without it likewise)
                self._ctor.update(survey_gradient=self.survey_gradient)
        self.wake_integrals = bool(wake_integrals)
        if self.wake_integrals:                     # (a run without them keeps the checkpoints it had)
            self._ctor.update(wake_integrals=True, wake_energy_steps=None if energy_win is None else list(energy_win))
            self.wake_energy_steps = energy_win
        # parameters (LUDVM.py:237-263)
        self.t0, self.tf, self.dt = t0, tf, dt
        self.chord, self.rho, self.Uinf = chord, rho, Uinf
        self.Npoints, self.Ncoeffs = Npoints, Ncoeffs
        self.piv = 0.25 * chord
        self.LESPcrit = LESPcrit
        self.maxerror, self.maxiter, self.epsilon = 1e-10, 50, 1e-4
        self.xgamma = 0.25
        self.method = method
        self.t = np.arange(t0, tf + dt, dt)
        self.nt = len(self.t)
        self.verbose = verbose
        self.dt_star = dt * Uinf / chord
        self.v_core = 1.3 * self.dt_star * chord
        self.ilev2 = 0
        self.alpha_m = alpha_m
        # free vortices (LUDVM.py:268-277): default is one zero-strength vortex at the origin
        if circulation_freevort is not None and xy_freevort is not None:
            self.n_freevort = len(circulation_freevort)
            self.circulation_freevort = circulation_freevort
            self.xy_freevort = xy_freevort
        else:
            self.n_freevort = 1
            self.circulation_freevort = np.array([0])
            self.xy_freevort = np.array([0, 0])[:, np.newaxis]

        if precision not in ('auto', 'f32', 'f32x2', 'f64'):
            raise ValueError("precision must be 'auto', 'f32', 'f32x2' or 'f64'")
        if history not in ('auto', 'full', 'sparse'):
            raise ValueError("history must be 'auto', 'full' or 'sparse'")
        fits = _dense_history_fits(self.nt)
        if (precision == 'auto' or history == 'auto') and not fits and verbose:
            import warnings
            warnings.warn(f"LUDVM: nt = {self.nt}: the reference's dense trajectory history would need "
                          f"{32 * self.nt * self.nt / 2**30:.1f} GiB; 'auto' keeps rows at snapshot_steps only "
                          "(history='sparse') and runs the wake-on-wake sums in fp32 with local origins "
                          "(precision='f32').  Pass history='full' / precision='f64' to override.", stacklevel=2)
        if precision == 'auto':
            # an fp32 rounding difference grows ~10x per 12 steps once the wake rolls up: in fp32
            # the README case ends 0.1 away from the reference on Cl, in fp64 4e-5 -- at the same speed for small wakes.
            # Long runs (config 2) are chaotic beyond ~1000 steps in any arithmetic: 'f32' (local origins) passes the
            # whole-horizon statistical test against float64 runs (tests/test_gpu_cfg2_stats.py)
            precision = 'f64' if fits else 'f32'
        self.precision = precision
        self.history = ('full' if fits else 'sparse') if history == 'auto' else history
        self.snapshot_steps = {int(s) for s in snapshot_steps}
        self.checkpoint_every, self.checkpoint_path = int(checkpoint_every), checkpoint_path
        self.march = bool(march)
        if self.checkpoint_every and not checkpoint_path:
            raise ValueError("checkpoint_every needs a checkpoint_path")
        self.engine = engine if engine is not None else Engine(device)  # raises without the HIP library / GPU
        self._shard = None
        if isinstance(distributed, str) and distributed == 'rccl':
            from .comm import LibraryGroup          # the library's own communicator: no torch.distributed
            self._shard = LibraryGroup(self.engine)
        elif distributed is not None and distributed is not False:
            if hasattr(distributed, 'gather_blocks'):          # a ShardGroup or LibraryGroup
                self._shard = distributed
            else:
                from .distributed import ShardGroup
                self._shard = ShardGroup(None if distributed is True else distributed)

        self.start_time = timeit.default_timer()
        if Naca is not None:
            self.airfoil_generation(Naca=Naca)
        else:
            self.airfoil_generation(Naca=None, filename=foil_filename)
        self.motion_sinusoidal(alpha_m=alpha_m, alpha_max=alpha_max, h_max=h_max, k=k, phi=phi, h0=0, x0=0,
                               motion='cos')
        if run:
            self.time_loop()
            self.compute_coefficients()
            if self.verbose:
                print('Elapsed time:', timeit.default_timer() - self.start_time)

    # ------------------------------------------------------------------------------------------
    # geometry and kinematics (host, run once)
    # ------------------------------------------------------------------------------------------
    def airfoil_generation(self, Naca='0012', filename=None, Npoints=None, uniform_spacing='theta'):
        """Mean line on theta-uniform nodes, panel quarter points and slopes (LUDVM.py:299-380).
        NACA 4-digit mean lines come from the published formula (the reference takes them from the
        PyPI package `airfoils`); Selig-format .dat files are averaged upper/lower as at :316-324."""
        if Npoints is None:
            Npoints = self.Npoints
        c = self.chord
        from_file = Naca is None and filename is not None
        if from_file or str(Naca)[:2] != '00':
            # (symmetric NACA 00xx sections -- every BASELINE config -- have a zero mean line whatever its source)
            import warnings
            warnings.warn("LUDVM: the mean line of a cambered NACA section / a .dat file is restated from the published "
                          "NACA 4-digit formula (or the averaged surfaces of the file); the reference takes it from the PyPI "
                          "package `airfoils` (LUDVM.py:301-335: mean of the interpolated surfaces), which is not available "
                          "to this build -- the mean line itself (that package's point distribution and formula) and .dat "
                          "sections are UNPINNED.  Everything downstream of a NACA 4-digit mean line -- interpolation, slopes, "
                          "the camber terms of downwash and solve, the bound-vortex positions, the loads, the flow field -- is "
                          "pinned to the reference on the published mean line (fixture group G10); symmetric 00xx sections "
                          "are pinned throughout.", RuntimeWarning, stacklevel=3)
        if from_file:
            xa, etaa = self._mean_line_from_dat(filename, Npoints)
        else:
            xs = np.linspace(0.0, 1.0, Npoints)
            xa, etaa = c * xs, c * naca4_mean_line(Naca, xs)
        if uniform_spacing == 'theta':
            theta = np.linspace(0, np.pi, self.Npoints)
            x = c / 2 * (1 - np.cos(theta))
            eta = np.interp(x, xa, etaa)
        else:
            x, eta = xa, etaa
            theta = np.arccos(1 - 2 * x / c)
        x_panel = x[:-1] + self.xgamma * (x[1:] - x[:-1])
        eta_panel = np.interp(x_panel, x, eta)
        theta_panel = np.arccos(1 - 2 * x_panel / c)

        def slope(f, s):  # one-sided at the ends; the reference's interior form divides by 2*(s[i+1]-s[i-1])
            d = np.empty(len(f))
            d[0] = (f[1] - f[0]) / (s[1] - s[0])
            d[-1] = (f[-1] - f[-2]) / (s[-1] - s[-2])
            d[1:-1] = (f[2:] - f[:-2]) / (2 * (s[2:] - s[:-2]))
            return d

        self.Npoints = len(eta)
        self.airfoil = {'x': x, 'theta': theta, 'eta': eta,
                        'detadx': slope(eta, x), 'detadtheta': slope(eta, theta),
                        'x_panel': x_panel, 'theta_panel': theta_panel, 'eta_panel': eta_panel,
                        'detadx_panel': slope(eta_panel, x_panel),
                        'detadtheta_panel': slope(eta_panel, theta_panel)}
        return None

    def _mean_line_from_dat(self, filename, Npoints):
        from scipy.interpolate import interp1d
        pts = []
        with open(filename) as fh:
            for line in fh:
                tok = line.split()
                if len(tok) == 2:
                    try:
                        pts.append((float(tok[0]), float(tok[1])))
                    except ValueError:
                        pass
        pts = np.array([p for p in pts if -0.01 <= p[0] <= 1.01])
        ile = int(np.argmin(pts[:, 0]))
        upper, lower = pts[: ile + 1][::-1], pts[ile:]
        n = int(np.floor(Npoints / 2))
        xs = np.linspace(0, 1, n)
        yu = interp1d(upper[:, 0], upper[:, 1], kind='cubic', bounds_error=False, fill_value='extrapolate')(xs)
        yl = interp1d(lower[:, 0], lower[:, 1], kind='cubic', bounds_error=False, fill_value='extrapolate')(xs)
        return self.chord * xs, self.chord * 0.5 * (yu + yl)

    def _rigid_body_path(self, xpiv, hpiv, alpha):
        """Node positions under pitch about the pivot (LUDVM.py:431-448)."""
        ca, sa = np.cos(-alpha)[:, None], np.sin(-alpha)[:, None]
        path = np.zeros([self.nt, 2, self.Npoints])
        path[:, 0, 0] = xpiv - self.piv * ca[:, 0]
        path[:, 1, 0] = hpiv + self.piv * sa[:, 0]
        xq, eq = self.airfoil['x'][1:], self.airfoil['eta'][1:]
        path[:, 0, 1:] = path[:, 0, :1] + ca * xq - sa * eq
        path[:, 1, 1:] = path[:, 1, :1] + sa * xq + ca * eq
        gpts = path[:, :, :-1] + self.xgamma * (path[:, :, 1:] - path[:, :, :-1])
        self.path = {'airfoil': path, 'airfoil_gamma_points': gpts}

    def motion_sinusoidal(self, alpha_m=0, alpha_max=10, h_max=1, k=0.2 * np.pi, phi=90, h0=0, x0=0.25,
                          motion='cos'):
        """h(t) = h0 + h_max cos(2 pi f t), alpha(t) = alpha_m + alpha_max cos(2 pi f t + phi),
        x(t) = x0 - Uinf t  (LUDVM.py:382-457); angles in degrees."""
        pi, U, t = np.pi, self.Uinf, self.t
        f = k * U / (2 * pi * self.chord)
        self.f = f
        alpha_m, alpha_max, phi = alpha_m * pi / 180, alpha_max * pi / 180, phi * pi / 180
        wt = 2 * pi * f * t
        if motion == 'cos':
            alpha, alpha_dot = alpha_m + alpha_max * np.cos(wt + phi), -alpha_max * 2 * pi * f * np.sin(wt + phi)
            h, h_dot = h0 + h_max * np.cos(wt), -h_max * 2 * pi * f * np.sin(wt)
        elif motion == 'sin':
            alpha, alpha_dot = alpha_m + alpha_max * np.sin(wt + phi), alpha_max * 2 * pi * f * np.cos(wt + phi)
            h, h_dot = h0 + h_max * np.sin(wt), -h_max * 2 * pi * f * np.cos(wt)
        else:
            raise ValueError("motion must be 'cos' or 'sin'")
        x = x0 - U * t
        self._rigid_body_path(x, h, alpha)
        self.phi, self.h_max = phi, h_max
        self.alpha, self.alpha_dot = alpha, alpha_dot
        self.alpha_e = alpha - np.arctan2(h_dot, U)
        self.hpiv, self.h_dot = h, h_dot
        self.xpiv, self.x_dot = x, -U * np.ones(self.nt)
        return None

    # ------------------------------------------------------------------------------------------
    # the hot path
    # ------------------------------------------------------------------------------------------
    def induced_velocity(self, circulation, xw, zw, xp, zp, viscous=True):
        """Velocity (u, w) induced at points (xp, zp) by vortices (circulation, xw, zw): Vatistas core
        v_core when `viscous == True`, point vortices otherwise (LUDVM.py:549-570).  Any array-likes
        in, two new float64 arrays out; evaluated on the GPU in `self.precision`."""
        v_core = self.v_core if viscous == True else 0  # noqa: E712  (the reference's comparison, :562)
        sh = self._shard
        if sh is not None and sh.world > 1 and len(xp) >= sh.min_targets and len(xp) * len(xw) >= getattr(sh, 'min_pairs', 0):
            # targets in contiguous blocks over the ranks (sources replicated), one all-gather of the (u, w) blocks -- for calls
            # large enough to repay it (many targets AND enough pairs: comm.py, MIN_TARGETS / MIN_PAIRS)
            xt, zt = np.asarray(xp, dtype=float).reshape(-1), np.asarray(zp, dtype=float).reshape(-1)
            lo, hi, _ = sh.block(len(xt))
            ul, wl = self.engine.induce(circulation, xw, zw, xt[lo:hi], zt[lo:hi], v_core, precision=self.precision)
            uw = sh.gather_blocks(np.stack([ul, wl], axis=1), len(xt))
            return np.ascontiguousarray(uw[:, 0]), np.ascontiguousarray(uw[:, 1])
        return self.engine.induce(circulation, xw, zw, xp, zp, v_core, precision=self.precision)

    def _scalar_field(self, kind, what, circulation, xw, zw, xp, zp, viscous):
        if self._shard is not None and self._shard.world > 1:
            raise ValueError(f"{what} runs on one GPU: not with `distributed` or more than one device in `devices`")
        if not hasattr(self.engine, 'scalar_field'):
            raise RuntimeError(f"{what}: this engine has no scalar_field")
        v_core = self.v_core if viscous == True else 0  # noqa: E712  (as induced_velocity)
        return self.engine.scalar_field(kind, circulation, xw, zw, xp, zp, v_core)

    def stream_function(self, circulation, xw, zw, xp, zp, viscous=True):
        """Stream function psi at points (xp, zp) of vortices (circulation, xw, zw), the arguments of `induced_velocity`:
        psi = sum G / (4 pi) ln((r^2 + s) / 2) with s = sqrt(r^4 + v_core^4), so that d psi / dz = u and -d psi / dx = w of
        `induced_velocity` exactly (LUDVM.py:565-568); with `viscous=False` the point vortex's G / (2 pi) ln r in the same
        gauge.  One new float64 array, evaluated on the GPU in float64 whatever the run's `precision`.  A point on top of a
        vortex is finite with a core (that term is ln(v_core^2 / 2)) and IEEE's -/+ inf or NaN without one."""
        return self._scalar_field('psi', 'the stream function', circulation, xw, zw, xp, zp, viscous)

    def vorticity(self, circulation, xw, zw, xp, zp, viscous=True):
        """Vorticity omega = dw/dx - du/dz at points (xp, zp) of the velocity field `induced_velocity` gives for vortices
        (circulation, xw, zw), in closed form: -sum G v_core^4 / (pi s^3), s = sqrt(r^4 + v_core^4) -- the sign convention of
        `ome_ff`, no grid and no differences.  One new float64 array, float64 on the GPU whatever the run's `precision`; 0
        with `viscous=False` (NaN at a point on top of a vortex).  (The hi+lo fp32 route of the sum:
        `engine.scalar_field('omega', ..., precision='f32x2')`, or `flowfield(omega=True, field_precision='f32x2')` on a mesh.)"""
        return self._scalar_field('omega', 'the analytic vorticity', circulation, xw, zw, xp, zp, viscous)

    def velocity_gradient(self, circulation, xw, zw, xp, zp, viscous=True):
        """Velocity gradient (ux, uz, wx) = (du/dx, du/dz, dw/dx) at points (xp, zp) of the velocity field `induced_velocity`
        gives for vortices (circulation, xw, zw), in closed form: no grid and no differences.  dw/dz = -ux (the field is
        divergence free), wx - uz is `vorticity`, and Q = -ux^2 - uz wx is positive in a vortex core and negative in a
        shear layer.  Three new float64 arrays, float64 on the GPU whatever the run's `precision`; with `viscous=False` the
        point vortex's gradient (NaN at a point on top of a vortex).  (The hi+lo fp32 route of the sums:
        `engine.gradient_field(..., precision='f32x2')`, or `flowfield(grad=True, field_precision='f32x2')` on a mesh.)"""
        if self._shard is not None and self._shard.world > 1:
            raise ValueError("the velocity gradient runs on one GPU: not with `distributed` or more than one device in `devices`")
        if not hasattr(self.engine, 'gradient_field'):
            raise RuntimeError("the velocity gradient: this engine has no gradient_field")
        v_core = self.v_core if viscous == True else 0  # noqa: E712  (as induced_velocity)
        return self.engine.gradient_field(circulation, xw, zw, xp, zp, v_core)

    def _chord_frame(self, u1, w1, i):
        a = self.alpha[i]
        return u1 * np.cos(a) - w1 * np.sin(a), u1 * np.sin(a) + w1 * np.cos(a)

    def _downwash_from(self, u1, w1, i):
        """W(x, t) from global-frame induced velocities at the bound-vortex points (LUDVM.py:586-593)."""
        a, ad, hd = self.alpha[i], self.alpha_dot[i], self.h_dot[i]
        u, w = self._chord_frame(u1, w1, i)
        af = self.airfoil
        return af['detadx_panel'] * (self.Uinf * np.cos(a) + hd * np.sin(a) + u - ad * af['eta_panel']) \
            - self.Uinf * np.sin(a) - ad * (af['x_panel'] - self.piv) + hd * np.cos(a) - w

    def airfoil_downwash(self, circulation, xw, zw, i):
        """Normal downwash W on the chord at time step i from the given vortices (LUDVM.py:572-595)."""
        g = self.path['airfoil_gamma_points']
        u1, w1 = self.induced_velocity(circulation, xw, zw, g[i, 0, :], g[i, 1, :])
        return self._downwash_from(u1, w1, i)

    # ------------------------------------------------------------------------------------------
    # time loop
    # ------------------------------------------------------------------------------------------
    def _setup_projection(self):
        """Trapezoid weights on theta_panel and the cos/sin tables: integral(y dtheta) = y @ wq,
        A_n = Cproj[n] @ (W/U), sum_n A_n sin(n theta_j) = A[1:] @ Ssin."""
        th = self.airfoil['theta_panel']
        d = np.diff(th)
        wq = np.zeros_like(th)
        wq[:-1] += d / 2
        wq[1:] += d / 2
        n = np.arange(self.Ncoeffs)[:, None]
        cproj = 2 / np.pi * np.cos(n * th[None, :]) * wq
        cproj[0] = -1 / np.pi * wq
        self._wq, self._cproj = wq, cproj
        self._cm1 = (np.cos(th) - 1) * wq
        self._ssin = np.sin(n[1:] * th[None, :])

    def _record_row(self, i):
        return self.history == 'full' or i in self.snapshot_steps or i == self.nt - 1

    def time_loop(self, print_dt=50, BCcheck=False, _resume=None):
        """Time marching (LUDVM.py:597-1171): per step place the new TEV, solve Gamma_TEV (and
        Gamma_LEV when |A0| reaches LESPcrit), rebuild the bound vorticity, integrate the loads and
        convect the wake.  `BCcheck` is accepted for signature compatibility; the reference's check
        (:1144-1161) raises a shape error and has no effect on the results.  `_resume` is the state a
        checkpoint holds (see `resume`).

        The loop itself: every step is MARCHED on the device where the engine offers it (`_march_call`: stretches of steps
        in one ludvm_march_run); the per-step path (`_host_step`: one device round trip, solve on the host) serves
        march=False and engines without the march."""
        S = self._loop_begin()
        if _resume is not None:
            self._loop_restore(S, _resume)
        self._free_slot = S.fslot
        S.fsl = slice(0, S.nf) if S.fslot is None else S.fslot
        self._loop_prepare_engine(S)
        eng, nt = self.engine, self.nt
        try:
            if self._shard is not None:
                # the roll-up's unordered pairs in tile blocks over the ranks, one integer all-reduce per step (attached
                # inside the try: whatever goes wrong from here on, the engine is left unsharded)
                self._shard.attach(eng, S.nf + 2 * (nt - 1) + self.Npoints - 1 + 2)
            i = S.first_step
            while i < nt:
                if S.can_march:
                    j, rec_i = self._march_extent(S, i)
                    if j > i:
                        self._march_call(S, i, j, rec_i, print_dt)
                        i = j
                        continue
                self._host_step(S, i, print_dt)
                i += 1
            if S.tracers is not None:
                self.tracer_last = eng.march_tracer_state() if S.can_march else S.tcur
                if self.tracer_gradient:
                    self.tracer_F_last = eng.march_tracer_gradient_state()
            if S.survey is not None:
                self._survey_results(*(eng.march_survey() if S.can_march else (S.ssums, S.scount)))
            if S.sbins is not None:
                self._survey_bin_results(*(eng.march_survey_bins() if S.can_march else (S.sbsums, S.sbcounts)))
            if S.sgsums is not None:        # (after the velocity results: the counts and the Reynolds stresses are theirs)
                self._survey_gradient_results(*(eng.march_survey_gradient() if S.can_march else (S.sgsums, S.sbgsums)))
        finally:
            if self._shard is not None:
                self._shard.detach(eng)
        return None

    # ---- the state a time loop carries, and its set-up --------------------------------------------------------------------
    class _Loop:
        """Scalars carried from step to step (counters, Kelvin sums, the newest shed vortices, the slot maps of the resident
        wake) and the constant tables of a run."""
        __slots__ = (
            # constants of the run
            'nf', 'x_gamma', 'detadx', 'gpts', 'foil', 'one_plus_cos_over_sin', 'half_c_sin_dth', 'wx', 'sum_free', 'first_step',
            'fslot', 'fsl', 'sb', 'prec_code', 'can_march', 'dense_march', 'march_chunk', 'probes', 'integrals',
            'tracers', 'trec', 'tcur', 'tF', 'survey', 'ssums', 'scount', 'sbins', 'sbsums', 'sbcounts', 'sgsums', 'sbgsums',
            # carried from step to step
            'itev', 'ilev', 'lesp_crit', 'sum_tev', 'sum_lev', 'last_tev', 'last_lev', 'LEV_shed', 'tev_slot', 'lev_slot', 'have_next')

    def _loop_begin(self, resident=True):
        """Result arrays (LUDVM.py:615-641), projection tables, the device wake with the free vortices in it
        (resident=False: the engine's resident wake is left alone -- a member of a sweep lives in a slab of its own)."""
        pi, U, c = np.pi, self.Uinf, self.chord
        eng = self.engine
        nt, nv, nf, npan = self.nt, self.nt - 1, self.n_freevort, self.Npoints - 1
        S = LUDVM._Loop()
        S.nf = nf
        th, thp = self.airfoil['theta'], self.airfoil['theta_panel']
        S.x_gamma = self.airfoil['x_panel']
        S.detadx = self.airfoil['detadx_panel']
        S.gpts = self.path['airfoil_gamma_points']
        S.foil = self.path['airfoil']
        self._setup_projection()
        dth = th[1:] - th[:-1]
        S.one_plus_cos_over_sin = (1 + np.cos(thp)) / np.sin(thp)
        S.half_c_sin_dth = c / 2 * np.sin(thp) * dth
        S.wx = np.zeros(npan)                       # trapezoid weights on x_gamma (loads, :1071, :1090)
        dxg = np.diff(S.x_gamma)
        S.wx[:-1] += dxg / 2
        S.wx[1:] += dxg / 2

        full = self.history == 'full'
        P = self.path
        if full:
            P['TEV'] = np.zeros([nt, 2, nv])
            P['LEV'] = np.zeros([nt, 2, nv])
            P['FREE'] = np.zeros([nt, 2, nf])
        else:
            P['TEV'], P['LEV'], P['FREE'] = SparseHistory(nt), SparseHistory(nt), SparseHistory(nt)
        free0 = np.array(self.xy_freevort, dtype=float).reshape(2, nf)
        if full:
            P['FREE'][0] = free0
        else:
            P['TEV'].store(0, np.zeros([2, 0]))
            P['LEV'].store(0, np.zeros([2, 0]))
            P['FREE'].store(0, free0.copy())
        C = self.circulation = {'TEV': np.zeros(nv), 'LEV': np.zeros(nv), 'FREE': self.circulation_freevort,
                                'bound': np.zeros(nv), 'airfoil': np.zeros([nv, npan]),
                                'gamma_airfoil': np.zeros([nv, npan]), 'Gamma_airfoil': np.zeros([nv, npan])}
        self.BC = np.zeros([nv, self.Npoints])
        self.dp = np.zeros([nt, npan])
        self.Fn, self.Fs, self.L, self.D, self.T, self.M = (np.zeros(nt) for _ in range(6))
        self.fourier = np.zeros([nt, 2, self.Ncoeffs])
        self.LESP, self.LESP_prev = np.zeros(nt), np.zeros(nt)
        A0, A1 = np.sin(self.alpha_m), 0
        self.fourier[0, 0, :2] = A0, A1
        g_free = np.asarray(self.circulation_freevort, dtype=float)
        S.sum_free = np.sum(C['FREE'])
        C['IC'] = S.sum_free + U * c * pi * (A0 + A1 / 2)

        # device wake, in shedding order: FREE first, then each step's TEV (and LEV when shed)
        if resident:
            eng.wake_clear()
            eng.wake_reserve(nf + 2 * nv + npan + 2)
        # A cloud of free vortices (generate_flowfield_turbulence, LUDVM.py:98-130) arrives in no spatial order; the fp32
        # roll-up keeps its accuracy tier on compact 256-vortex blocks (a shed wake's stored order).  The engine names the
        # order it wants (Morton; the identity for a compact or small set): the cloud is STORED in it, `fslot[j]` is the
        # wake slot of the caller's free vortex j, and every path['FREE'] row is returned in the caller's order.
        fslot = None
        if resident and self.precision == 'f32' and nf >= 2048 and hasattr(eng, 'spatial_order'):
            order, reordered, extent = eng.spatial_order(free0[0], free0[1], with_extent=True)
            if extent > (150.0 if reordered else 300.0) * self.v_core > 0.0:
                # too sparse for its core: no order makes 128-vortex classes compact enough for fp32 offsets to resolve
                # v_core (ludvm_hip.h, ludvm_spatial_order) -- the roll-up takes hi+lo positions instead
                import warnings
                warnings.warn(f"LUDVM: the free-vortex cloud is too sparse for v_core = {self.v_core:g} to keep 1e-5 of max|u| "
                              f"in fp32 on local origins (mean 128-vortex class extent {extent:.3g} > {150 if reordered else 300} v_core); "
                              "the wake-on-wake sums of this run use hi+lo positions (precision='f32x2')",
                              RuntimeWarning, stacklevel=4)
                self.precision, reordered = 'f32x2', False
            if reordered:
                fslot = np.empty(nf, dtype=np.int64)
                fslot[order] = np.arange(nf)
                eng.wake_append(free0[0][order], free0[1][order], g_free[order])
        if fslot is None and resident:
            eng.wake_append(free0[0], free0[1], g_free)
        S.fslot = fslot
        S.tev_slot = np.zeros(nv, dtype=np.int64)
        S.lev_slot = np.zeros(nv, dtype=np.int64)
        S.sum_tev = S.sum_lev = 0.0                 # running Kelvin sums (:758-760)
        S.last_tev = S.last_lev = None              # newest shed vortices after their convection
        S.itev = S.ilev = 0
        S.lesp_crit = self.LESPcrit
        S.LEV_shed = -1 * np.ones(nt)
        S.first_step = 1
        S.probes = getattr(self, 'probe_xz', None)
        if S.probes is not None:
            # row 0: the field of the initial free vortices (:1202-1206)
            self.probe_u, self.probe_w = np.zeros([nt, S.probes.shape[1]]), np.zeros([nt, S.probes.shape[1]])
            p0 = self.probe_positions(0)
            self.probe_u[0], self.probe_w[0] = eng.induce(g_free, free0[0], free0[1], p0[0], p0[1], self.v_core, precision='f64')
        S.integrals = self.wake_integrals
        if S.integrals:
            # row 0: the initial free vortices, as `probe_u` has it; the energy has no sample there (its window begins at 1)
            self.integral_sums = np.zeros([nt, 4, 2, 6])
            self.wake_energy = np.full(nt, np.nan)
            self.integral_sums[0] = self._integral_row(np.zeros(nf, dtype=np.int64), g_free, free0[0], free0[1])
        S.tracers = getattr(self, 'tracer_xz', None)
        S.trec = S.tcur = None
        if S.tracers is not None:
            # recorded steps >= 1 (row 0, the seeds, is always kept); the positions the loop carries
            rec = self._tracer_steps
            if rec is None:
                rec = range(1, nt) if full else sorted(self.snapshot_steps | {nt - 1})
            S.trec = np.array([q for q in rec if 1 <= q < nt], dtype=np.int64)
            self.tracer_path = SparseHistory(nt)
            S.tcur = self._tracer_seeds(0)
            self.tracer_path.store(0, S.tcur.copy())
            S.tF = None
            if self.tracer_gradient:
                # the deformation gradient the march carries: the identity at the seeds (row 0)
                self.tracer_F_path = SparseHistory(nt)
                self.tracer_F_path.store(0, self._identity_F())
        S.survey = getattr(self, '_survey_xz', None)
        S.ssums, S.scount = None, 0
        if S.survey is not None:
            # the five raw sums the per-step path accumulates (the march keeps its own on the device), or a checkpoint's
            S.ssums = np.zeros([5, S.survey.shape[1]])
        S.sbins = getattr(self, 'survey_bin_of_step', None)
        S.sbsums = S.sbcounts = None
        if S.sbins is not None:
            # likewise for the bins: [B][5][K] and the samples of every bin
            S.sbsums = np.zeros([self.survey_nbins, 5, S.survey.shape[1]])
            S.sbcounts = np.zeros(self.survey_nbins, dtype=np.int64)
        S.sgsums = S.sbgsums = None
        if S.survey is not None and self.survey_gradient:
            # likewise for the gradient sums [5][K] and their bin blocks [B][5][K] (the counts are the velocity sums' own)
            S.sgsums = np.zeros([5, S.survey.shape[1]])
            if S.sbins is not None:
                S.sbgsums = np.zeros([self.survey_nbins, 5, S.survey.shape[1]])
        return S

    def _survey_sampled(self, step):
        """Is time step `step` one of the survey's sampled steps?"""
        first, stop, every = self.survey_steps
        return first <= step < stop and (step - first) % every == 0

    def _survey_points(self, step):
        """Lab coordinates (x [K], z [K]) of the survey points at time step `step` ('tunnel' frame: x + xpiv[step])."""
        x, z = self._survey_xz
        return (x + self.xpiv[int(step)] if self.survey_frame == 'tunnel' else x), z

    def _survey_results(self, sums, n):
        """The survey's attributes from the raw sums [5, K] over n sampled steps."""
        shape = self._survey_shape
        self.survey_count = int(n)
        self.survey_sums = np.array(sums, dtype=np.float64).reshape((5,) + shape)
        su, sw, suu, sww, suw = self.survey_sums
        with np.errstate(divide='ignore', invalid='ignore'):       # (n = 0: a run that stopped before its window)
            mu, mw = su / n, sw / n
            self.survey_mean_u, self.survey_mean_w = mu, mw
            self.survey_uu, self.survey_ww, self.survey_uw = suu / n - mu * mu, sww / n - mw * mw, suw / n - mu * mw

    def _survey_bin_results(self, sums, counts):
        """The binned survey's attributes from the raw sums [B, 5, K] and the samples [B] of every bin: the phase averages, the
        central moments within each bin, and the triple decomposition of the binned samples' fluctuation into its coherent part
        (the bin means about the overall mean) and its random part (the scatter within the bins)."""
        shape, B = self._survey_shape, self.survey_nbins
        self.survey_bin_count = np.array(counts, dtype=np.int64)
        self.survey_bin_sums = np.array(sums, dtype=np.float64).reshape((B, 5) + shape)
        n = self.survey_bin_count.reshape((B,) + (1,) * len(shape)).astype(np.float64)
        su, sw, suu, sww, suw = (self.survey_bin_sums[:, c] for c in range(5))
        with np.errstate(divide='ignore', invalid='ignore'):       # (an empty bin: nan, as n = 0 gives for the plain moments)
            mu, mw = su / n, sw / n
            self.survey_bin_mean_u, self.survey_bin_mean_w = mu, mw
            self.survey_bin_uu, self.survey_bin_ww, self.survey_bin_uw = suu / n - mu * mu, sww / n - mw * mw, suw / n - mu * mw
        N = float(self.survey_bin_count.sum())
        full = self.survey_bin_count > 0
        nb = n[full]
        with np.errstate(divide='ignore', invalid='ignore'):       # (N = 0: a run that stopped before its first binned step)
            tu, tw = su[full].sum(axis=0) / N, sw[full].sum(axis=0) / N          # the mean of the binned samples
            du, dw = mu[full] - tu, mw[full] - tw
            self.survey_coherent_uu, self.survey_coherent_ww = (nb * du * du).sum(axis=0) / N, (nb * dw * dw).sum(axis=0) / N
            self.survey_coherent_uw = (nb * du * dw).sum(axis=0) / N
            self.survey_random_uu = (nb * self.survey_bin_uu[full]).sum(axis=0) / N
            self.survey_random_ww = (nb * self.survey_bin_ww[full]).sum(axis=0) / N
            self.survey_random_uw = (nb * self.survey_bin_uw[full]).sum(axis=0) / N

    def _survey_gradient_results(self, gsums, bin_gsums):
        """The gradient survey's attributes from the raw sums [5, K] and -- with bins -- [B, 5, K]; the counts, the Reynolds
        stresses and the bins' decomposition weights are the velocity survey's (`_survey_results`, `_survey_bin_results`)."""
        shape, n = self._survey_shape, self.survey_count
        self.survey_grad_sums = np.array(gsums, dtype=np.float64).reshape((5,) + shape)
        sux, se, som, som2, sq = self.survey_grad_sums
        with np.errstate(divide='ignore', invalid='ignore'):       # (n = 0: a run that stopped before its window)
            ux, e, om = sux / n, se / n, som / n
            self.survey_mean_ux, self.survey_mean_strain, self.survey_mean_omega = ux, e, om
            self.survey_mean_uz, self.survey_mean_wx = e - 0.5 * om, e + 0.5 * om
            self.survey_omega2, self.survey_mean_q = som2 / n, sq / n
            self.survey_omega_var = self.survey_omega2 - om * om
            # -<u_i' u_j'> dU_i/dx_j with dw/dz = -du/dx and du/dz + dw/dx = 2 e
            self.survey_production = -(self.survey_uu * ux + self.survey_uw * (2.0 * e) - self.survey_ww * ux)
        if bin_gsums is None:
            return
        B = self.survey_nbins
        self.survey_bin_grad_sums = np.array(bin_gsums, dtype=np.float64).reshape((B, 5) + shape)
        nb_all = self.survey_bin_count.reshape((B,) + (1,) * len(shape)).astype(np.float64)
        bux, be, bom, bom2, bq = (self.survey_bin_grad_sums[:, c] for c in range(5))
        with np.errstate(divide='ignore', invalid='ignore'):       # (an empty bin: nan)
            self.survey_bin_mean_ux, self.survey_bin_mean_strain = bux / nb_all, be / nb_all
            self.survey_bin_mean_omega, self.survey_bin_mean_q = bom / nb_all, bq / nb_all
            self.survey_bin_omega2 = bom2 / nb_all
        N = float(self.survey_bin_count.sum())
        full = self.survey_bin_count > 0
        nb = nb_all[full]
        with np.errstate(divide='ignore', invalid='ignore'):       # (N = 0: a run that stopped before its first binned step)
            to = bom[full].sum(axis=0) / N                         # the mean of the binned samples
            mo = self.survey_bin_mean_omega[full]
            self.survey_coherent_omega2 = (nb * (mo - to) * (mo - to)).sum(axis=0) / N
            self.survey_random_omega2 = (nb * (self.survey_bin_omega2[full] - mo * mo)).sum(axis=0) / N

    def _tracer_seeds(self, step):
        """Lab coordinates [2, M] of the seeds at time step `step` ('tunnel' frame: x + xpiv[step])."""
        xz = self.tracer_xz.copy()
        if self.tracer_frame == 'tunnel':
            xz[0] = xz[0] + self.xpiv[int(step)]
        return xz

    def tracer_released(self, step):
        """bool [M]: the tracers that move in time step `step` (released at or before it)."""
        return self.tracer_release <= int(step)

    def _identity_F(self):
        F = np.zeros([4, self.tracer_xz.shape[1]])
        F[0], F[3] = 1.0, 1.0
        return F

    def tracer_ftle(self, step=None):
        """float64 [M]: the finite-time Lyapunov exponent ln sigma_max(F) / T of every tracer after time step `step` (None: the
        last step), T = dt (step - release + 1) -- NaN for a tracer not yet released at that step.  Needs tracer_gradient=True
        and, for a step other than the last, a step `tracer_F_path` holds."""
        if not getattr(self, 'tracer_gradient', False):
            raise ValueError("tracer_ftle needs a run with tracer_gradient=True")
        if step is None:
            step, F = self.nt - 1, self.tracer_F_last
        else:
            step = int(step) + (self.nt if int(step) < 0 else 0)
            F = self.tracer_F_path[step]
        return self.ftle_from_F(F, self.dt * (step - self.tracer_release + 1.0))

    # ---- wake integrals (wake_integrals=True) ---------------------------------------------------------
    integral_classes = ('FREE', 'TEV', 'LEV', 'BOUND')

    @staticmethod
    def _integral_row(cls, g, x, z):
        """float64 [4, 2, 6]: the six sums -- count, G, G x, G z, G (x^2 + z^2), G^2 -- of every class (0 .. 3) and sign (slot 0:
        G >= 0, slot 1: G < 0) over the vortices (cls, g, x, z), as the per-step path forms them."""
        cls, g, x, z = np.asarray(cls), np.asarray(g, dtype=float), np.asarray(x, dtype=float), np.asarray(z, dtype=float)
        row = np.zeros([4, 2, 6])
        neg = g < 0.0
        for c in range(4):
            for s in range(2):
                m = (cls == c) & (neg == bool(s))
                gm, xm, zm = g[m], x[m], z[m]
                row[c, s] = [m.sum(), gm.sum(), (gm * xm).sum(), (gm * zm).sum(), (gm * (xm * xm + zm * zm)).sum(), (gm * gm).sum()]
        return row

    def _wake_tags(self, S):
        """uint8 [wake size]: the class (0 FREE, 1 TEV, 2 LEV) of every vortex of the resident wake in its stored order, from the
        free-vortex count and the slot maps of the vortices shed so far."""
        tags = np.zeros(S.nf + S.itev + S.ilev, dtype=np.uint8)
        tags[S.tev_slot[:S.itev]] = 1
        tags[S.lev_slot[:S.ilev]] = 2
        return tags

    def _energy_sampled(self, step):
        """Is time step `step` one of the energy's sampled steps?"""
        if self.wake_energy_steps is None:
            return False
        first, stop, every = self.wake_energy_steps
        return first <= step < stop and (step - first) % every == 0

    def _integrals(self):
        if not getattr(self, 'wake_integrals', False) or not hasattr(self, 'integral_sums'):
            raise ValueError("the wake integrals need a run with wake_integrals=True")
        return self.integral_sums

    def _class_index(self, cls):
        if isinstance(cls, str):
            if cls.upper() not in self.integral_classes:
                raise ValueError(f"class must be one of {self.integral_classes} (got {cls!r})")
            return self.integral_classes.index(cls.upper())
        if int(cls) != cls or not 0 <= int(cls) < 4:
            raise ValueError(f"class must be one of {self.integral_classes} or 0 .. 3 (got {cls!r})")
        return int(cls)

    @staticmethod
    def _sign_index(sign):
        if sign in ('+', 1, 'pos'):
            return 0
        if sign in ('-', -1, 'neg'):
            return 1
        raise ValueError(f"sign must be '+' (Gamma >= 0) or '-' (Gamma < 0) (got {sign!r})")

    def wake_circulation(self, cls=None, sign=None):
        """float64 [nt]: the circulation the system of every step carries -- of class `cls` ('FREE', 'TEV', 'LEV', 'BOUND' or
        0 .. 3; None: all) and sign ('+': the vortices with Gamma >= 0, '-': those with Gamma < 0; None: both)."""
        sums = self._integrals()[:, :, :, 1]
        if cls is not None:
            sums = sums[:, [self._class_index(cls)]]
        if sign is not None:
            sums = sums[:, :, [self._sign_index(sign)]]
        return sums.sum(axis=(1, 2))

    def wake_centroid(self, cls, sign):
        """float64 [nt, 2]: (sum G x / sum G, sum G z / sum G) of the vortices of class `cls` and sign `sign`; NaN where there is
        none."""
        row = self._integrals()[:, self._class_index(cls), self._sign_index(sign)]
        with np.errstate(divide='ignore', invalid='ignore'):
            out = np.stack([row[:, 2] / row[:, 1], row[:, 3] / row[:, 1]], axis=1)
        out[row[:, 0] == 0] = np.nan
        return out

    @property
    def wake_impulse(self):
        """float64 [nt, 2]: the linear impulse rho (-sum G z, +sum G x) of the whole system (Gamma is clockwise-positive:
        u = +G dz / (2 pi s))."""
        tot = self._integrals().sum(axis=(1, 2))
        return self.rho * np.stack([-tot[:, 3], tot[:, 2]], axis=1)

    @property
    def wake_angular_impulse(self):
        """float64 [nt]: the angular impulse about the lab origin, rho / 2 sum G (x^2 + z^2) (clockwise-positive Gamma)."""
        return 0.5 * self.rho * self._integrals().sum(axis=(1, 2))[:, 4]

    @property
    def impulse_force(self):
        """float64 [nt, 2]: the force on the foil the impulse implies, -(I_i - I_(i-1)) / dt; NaN in row 0 (free vortices only:
        no foil) and in row 1, the first row of a system with the foil in it."""
        I = self.wake_impulse
        F = np.full_like(I, np.nan)
        F[2:] = -(I[2:] - I[1:-1]) / self.dt
        return F

    @property
    def impulse_Cl(self):
        """float64 [nt]: impulse_force's lab z component over rho Uinf^2 chord / 2, the axes and normalisation of `Cl`."""
        return self.impulse_force[:, 1] / (0.5 * self.rho * self.Uinf**2 * self.chord)

    @property
    def impulse_Cd(self):
        """float64 [nt]: impulse_force's lab x component (the foil moves towards -x) over rho Uinf^2 chord / 2, as `Cd`."""
        return self.impulse_force[:, 0] / (0.5 * self.rho * self.Uinf**2 * self.chord)

    @property
    def wake_energy_interaction(self):
        """float64 [nt]: `wake_energy` minus its self part ln(v_core^2 / 2) / (8 pi) sum G^2 (the a = b terms)."""
        self._integrals()
        return self.wake_energy - np.log(0.5 * self.v_core**2) / (8.0 * np.pi) * self.integral_sums.sum(axis=(1, 2))[:, 5]

    def probe_positions(self, step):
        """Lab coordinates [2, P] of the probes at time step `step` ('tunnel' frame: x + xpiv[step])."""
        xz = self.probe_xz.copy()
        if self.probe_frame == 'tunnel':
            xz[0] = xz[0] + self.xpiv[int(step)]
        return xz

    def _loop_restore(self, S, R):
        """The loop's state as a checkpoint holds it (`_write_checkpoint_file`)."""
        C, P, eng, nf = self.circulation, self.path, self.engine, S.nf
        S.first_step, S.itev, S.ilev = int(R['next_step']), int(R['itev']), int(R['ilev'])
        S.lesp_crit, S.sum_tev, S.sum_lev = float(R['lesp_crit']), float(R['sum_tev']), float(R['sum_lev'])
        S.last_tev = None if np.isnan(R['last_tev']).any() else R['last_tev'].copy()
        S.last_lev = None if np.isnan(R['last_lev']).any() else R['last_lev'].copy()
        S.LEV_shed, S.tev_slot, S.lev_slot = R['LEV_shed'].copy(), R['tev_slot'].copy(), R['lev_slot'].copy()
        for key in ('TEV', 'LEV', 'bound', 'airfoil', 'gamma_airfoil', 'Gamma_airfoil'):
            C[key][...] = R['circ_' + key]
        for name in ('Fn', 'Fs', 'L', 'D', 'T', 'M', 'fourier', 'LESP', 'LESP_prev'):
            getattr(self, name)[...] = R[name]
        if S.probes is not None:
            self.probe_u[:S.first_step], self.probe_w[:S.first_step] = R['probe_u'], R['probe_w']
        if S.integrals:
            self.integral_sums[:S.first_step], self.wake_energy[:S.first_step] = R['integral_sums'], R['wake_energy']
        if S.tracers is not None:
            S.tcur = R['tracer_cur'].copy()
            for srow, row in zip(R['tracer_rows_steps'], R['tracer_rows']):
                self.tracer_path.store(int(srow), row.copy())
            if self.tracer_gradient:
                S.tF = R['tracer_F_cur'].copy()
                for srow, row in zip(R['tracer_rows_steps'], R['tracer_F_rows']):
                    self.tracer_F_path.store(int(srow), row.copy())
        if S.survey is not None:
            S.ssums, S.scount = R['survey_sums'].copy(), int(R['survey_samples'])
        if S.sbins is not None:
            S.sbsums, S.sbcounts = R['survey_bin_sums'].copy(), R['survey_bin_counts'].astype(np.int64)
        if S.sgsums is not None:
            S.sgsums = R['survey_grad_sums'].copy()
            if S.sbgsums is not None:
                S.sbgsums = R['survey_bin_grad_sums'].copy()
        for key in ('TEV', 'LEV', 'FREE'):
            if self.history == 'full':
                P[key][:S.first_step] = R['path_' + key]
            else:
                for srow in R['rows_steps']:
                    P[key].store(int(srow), R[f'row_{key}_{int(srow)}'])
        eng.wake_clear()
        eng.wake_append(R['wake_x'], R['wake_z'], R['wake_g'])        # (in the stored order, free vortices included)
        S.fslot = R['free_slot'].astype(np.int64) if ('free_slot' in R.files and R['free_slot'].size == nf) else None
        self.ilev, self.itev, self.LEV_shed = int(R['self_ilev']), int(R['self_itev']), S.LEV_shed

    def _loop_prepare_engine(self, S):
        """Host buffers of the per-step path; tables and kinematics of the device-resident march."""
        eng = self.engine
        npan = self.Npoints - 1
        if S.tracers is not None and self.march and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_tracers'):
            raise RuntimeError("tracers: this engine marches but has no march_set_tracers (pass march=False for the per-step path)")
        if S.survey is not None and self.march and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_survey'):
            raise RuntimeError("survey: this engine marches but has no march_set_survey (pass march=False for the per-step path)")
        if S.sbins is not None and self.march and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_survey_bins'):
            raise RuntimeError("survey_bins: this engine marches but has no march_set_survey_bins (pass march=False for the per-step "
                               "path)")
        if S.integrals and self.march and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_integrals'):
            raise RuntimeError("wake_integrals: this engine marches but has no march_set_integrals (pass march=False for the per-step "
                               "path)")
        grad_tracers = S.tracers is not None and self.tracer_gradient
        # (tracer_gradient='f32x2': u, w and the gradient's sums from one hi+lo fp32 walk, so ONE setter for precision and gradient)
        grad_f32_tracers = isinstance(grad_tracers, str) and grad_tracers == 'f32x2'
        if grad_f32_tracers and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_tracer_gradient_f32x2'):
            raise RuntimeError("tracer_gradient='f32x2': this engine marches but has no march_set_tracer_gradient_f32x2")
        f32_tracers = S.tracers is not None and self.tracer_precision == 'f32x2'
        if f32_tracers and not grad_f32_tracers and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_tracer_precision'):
            raise RuntimeError("tracer_precision='f32x2': this engine marches but has no march_set_tracer_precision")
        if grad_tracers and not grad_f32_tracers and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_tracer_gradient'):
            raise RuntimeError("tracer_gradient: this engine marches but has no march_set_tracer_gradient")
        f32_survey = S.survey is not None and self.survey_precision == 'f32'
        if f32_survey and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_survey_precision'):
            raise RuntimeError("survey_precision='f32': this engine marches but has no march_set_survey_precision")
        grad_survey = S.sgsums is not None
        # (survey_gradient='f32x2': u, w and the gradient's sums of a sampled step from one hi+lo fp32 walk, a setter of its own)
        grad_f32_survey = grad_survey and isinstance(self.survey_gradient, str) and self.survey_gradient == 'f32x2'
        if grad_f32_survey and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_survey_gradient_f32x2'):
            raise RuntimeError("survey_gradient='f32x2': this engine marches but has no march_set_survey_gradient_f32x2")
        if grad_survey and not grad_f32_survey and self.march and hasattr(eng, 'march_run') and not hasattr(eng, 'march_set_survey_gradient'):
            raise RuntimeError("survey_gradient: this engine marches but has no march_set_survey_gradient (pass march=False for the "
                               "per-step path)")
        # preallocated host buffers for the two device calls of a step (engines that offer them)
        S.sb = eng.step_buffers(npan) if hasattr(eng, 'step_buffers') else None
        S.prec_code = {'f32': 0, 'f32x2': 1, 'f64': 2}[self.precision]
        S.have_next = False     # sb already holds step i's placement and chord sums (from the previous wake_step)

        # Device-resident march (ludvm_march_setup / ludvm_march_run): stretches of steps run without a host round trip
        # per step; the per-step path serves march=False and engines without the march.
        S.can_march = (self.march and self.method in ('Faure', 'Ramesh') and hasattr(eng, 'march_run') and npan <= 256
                       and 4 <= self.Ncoeffs <= 64)
        if S.can_march:
            eng.march_setup(npan, self.Ncoeffs, *self._march_inputs(S))
            if S.probes is not None:
                eng.march_set_probes(S.probes[0], S.probes[1], shift_x=self.xpiv if self.probe_frame == 'tunnel' else None)
            if S.tracers is not None:
                eng.march_set_tracers(S.tracers[0], S.tracers[1], release=self.tracer_release,
                                      shift_x=self.xpiv if self.tracer_frame == 'tunnel' else None, cur=S.tcur, record_steps=S.trec)
                if grad_f32_tracers:
                    eng.march_set_tracer_gradient_f32x2(F=S.tF)
                elif f32_tracers:
                    eng.march_set_tracer_precision('f32x2')
                elif grad_tracers:
                    eng.march_set_tracer_gradient(True, F=S.tF)
            if S.survey is not None:
                eng.march_set_survey(S.survey[0], S.survey[1], shift_x=self.xpiv if self.survey_frame == 'tunnel' else None,
                                     steps=self.survey_steps, sums=S.ssums if S.scount else None, samples=S.scount)
                if f32_survey:
                    eng.march_set_survey_precision('f32')
                if S.sbins is not None:
                    carried = bool(S.sbcounts.any())
                    eng.march_set_survey_bins(S.sbins, self.survey_nbins, sums=S.sbsums if carried else None,
                                              counts=S.sbcounts if carried else None)
                if grad_survey:
                    # (after the survey and its bins, which forget it; sums that are carried go together with their counts)
                    carried = bool(S.scount) or (S.sbins is not None and bool(S.sbcounts.any()))
                    if grad_f32_survey:
                        eng.march_set_survey_gradient_f32x2(gsums=S.sgsums if carried else None,
                                                            bin_gsums=S.sbgsums if carried else None)
                    else:
                        eng.march_set_survey_gradient(True, gsums=S.sgsums if carried else None,
                                                      bin_gsums=S.sbgsums if carried else None)
            if S.integrals:
                eng.march_set_integrals(True, self._wake_tags(S), energy_steps=self.wake_energy_steps)
        if S.integrals and self.wake_energy_steps is not None and not S.can_march and not hasattr(eng, 'scalar_field'):
            raise RuntimeError("wake_energy_steps: the per-step path needs an engine with scalar_field")
        if grad_f32_survey and not S.can_march:
            # (neither float64 nor the per-step path in its place)
            raise RuntimeError("survey_gradient='f32x2' is evaluated inside the device-resident march, which this run cannot take "
                               "(an engine without march_run, method, Npoints or Ncoeffs outside its limits)")
        if grad_survey and not S.can_march and not hasattr(eng, 'gradient_field'):
            raise RuntimeError("survey_gradient: the per-step path needs an engine with gradient_field")
        if grad_f32_tracers and not S.can_march:
            # (neither float64 nor the per-step path in its place)
            raise RuntimeError("tracer_gradient='f32x2' is evaluated inside the device-resident march, which this run cannot take "
                               "(an engine without march_run, method, Npoints or Ncoeffs outside its limits)")
        if f32_tracers and not S.can_march:
            # (no float64 in its place: the per-step path has no fp32 tracer sums)
            raise RuntimeError("tracer_precision='f32x2' is evaluated inside the device-resident march, which this run cannot take "
                               "(an engine without march_run, method, Npoints or Ncoeffs outside its limits)")
        if grad_tracers and not S.can_march:
            # (the per-step path carries no deformation gradient)
            raise RuntimeError("tracer_gradient is evaluated inside the device-resident march, which this run cannot take "
                               "(an engine without march_run, method, Npoints or Ncoeffs outside its limits)")
        if f32_survey and not S.can_march:
            # (no float64 in its place: the per-step path has no fp32 survey sums)
            raise RuntimeError("survey_precision='f32' is evaluated inside the device-resident march, which this run cannot take "
                               "(an engine without march_run, method, Npoints or Ncoeffs outside its limits)")
        # with the dense history every step's row is recorded: the march then keeps a snapshot of the wake per step on
        # the device (shorter calls, the snapshots are [steps, 2, wake size])
        S.dense_march = S.can_march and self.history == 'full'
        S.march_chunk = int(getattr(self, '_march_chunk', 512 if S.dense_march else 32768))   # steps per ludvm_march_run call

    def _march_inputs(self, S):
        """-> (scalars[12], tables, kin[nt, 7 + 2 npan]) as ludvm_march_setup takes them (include/ludvm_hip.h); a sweep packs
        the same three per member (ludvm_amd/ensemble.py)."""
        C = self.circulation
        tables = np.concatenate([S.detadx, self.airfoil['eta_panel'], S.x_gamma, self._cm1, self._wq, S.one_plus_cos_over_sin,
                                 S.half_c_sin_dth, S.wx, self._cproj.ravel(), self._ssin.ravel()])
        kin = np.concatenate([self.alpha[:, None], self.alpha_dot[:, None], self.h_dot[:, None], S.foil[:, :, -1],
                              S.foil[:, :, 0], S.gpts[:, 0, :], S.gpts[:, 1, :]], axis=1)
        scalars = [self.Uinf, self.chord, self.rho, self.dt, self.piv, self.v_core, C['IC'], S.sum_free,
                   float(self.method == 'Ramesh'), self.maxerror, self.maxiter, self.epsilon]
        return scalars, tables, kin

    def _progress(self, q, print_dt):
        if (q == 1 or q == self.nt - 1 or q / print_dt == int(q / print_dt)) and self.verbose == True:  # noqa: E712
            print('Step {} out of {}. Elapsed time {}'.format(q, self.nt - 1, timeit.default_timer() - self.start_time))

    def _next_placement(self, S, i):
        """New TEV: the first one half a step behind the initial trailing edge, then 1/3 of the way from the trailing edge to
        the previous TEV (:672-681).  Candidate LEV: only geometry and the previous LEV enter (:788-800), so it is known
        before the solve."""
        foil = S.foil
        te, le = foil[i, :, -1], foil[i, :, 0]
        tev_xy = foil[0, :, -1] + np.array([0.5 * self.Uinf * self.dt, 0.0]) if S.itev == 0 else te + (S.last_tev - te) / 3
        lev_xy = le + (S.last_lev - le) / 3 if (S.ilev > 0 and S.LEV_shed[i - 1] != -1) else le.copy()
        return tev_xy, lev_xy

    # ---- marched stretches --------------------------------------------------------------------------------------------------
    def _march_extent(self, S, i):
        """-> (j, rec_i): the stretch [i, j) the next ludvm_march_run call covers.  Every step is marched, whatever the
        history mode: a step whose row is recorded (sparse history) is a call of its own that also returns the wake's
        positions after it -- so a run's bits do not depend on which rows it keeps (rounds 1-3 took recorded steps through
        the per-step path, whose launches are sized from the exact wake size instead of the march's anchor bound: fp32
        rounding differed from the first recorded step on)."""
        nt = self.nt
        rec_i = (not S.dense_march) and self._record_row(i)
        j = i
        if rec_i:
            # a run of consecutive recorded steps is one call (its snapshots are [steps, 2, wake size] doubles:
            # at most 256 MB of them)
            n_now = S.nf + S.itev + S.ilev
            most = max(1, min(512, int(256e6 / (16.0 * (n_now + 1024)))))
            while j < nt and self._record_row(j) and j - i < most:
                j += 1
                if self.checkpoint_every and (j - 1) % self.checkpoint_every == 0:
                    break
        while (not rec_i) and j < nt and (S.dense_march or not self._record_row(j)) and j - i < S.march_chunk:
            j += 1
            if self.checkpoint_every and (j - 1) % self.checkpoint_every == 0:
                break
        if S.probes is not None:
            # one call's probe rows ([steps, 2, P] doubles) stay at or under 256 MB, like the history rows
            j = min(j, i + max(1, int(getattr(self, '_probe_call_bytes', 256e6) // (16 * S.probes.shape[1]))))
        if S.tracers is not None:
            # one call's recorded tracer rows ([rows, 2, M] doubles; with the deformation gradient [rows, 4, M] more) stay at or
            # under 256 MB as well
            row_bytes = 48 if self.tracer_gradient else 16
            most = max(1, int(getattr(self, '_tracer_call_bytes', 256e6) // (row_bytes * S.tracers.shape[1])))
            lo = int(np.searchsorted(S.trec, i))
            if int(np.searchsorted(S.trec, j)) - lo > most:
                j = int(S.trec[lo + most])      # (the call ends before its `most + 1`-th recorded step)
        return j, rec_i

    def _march_call(self, S, i, j, rec_i, print_dt):
        sb = S.sb
        if S.have_next:
            place = [sb.unit[0, 0], sb.unit[0, 1], sb.unit[1, 0], sb.unit[1, 1]]
        else:
            tev_xy, lev_xy = self._next_placement(S, i)
            place = [tev_xy[0], lev_xy[0], tev_xy[1], lev_xy[1]]
        self._march_stretch(S, i, j, place, record=S.dense_march or rec_i)
        S.have_next = False
        if self.verbose == True:  # noqa: E712
            for q in range(i, j):
                self._progress(q, print_dt)
        if self.checkpoint_every and (j - 1) % self.checkpoint_every == 0 and j - 1 < self.nt - 1:
            self._write_checkpoint(S, j)

    def _march_stretch(self, S, i, j, place, record=False):
        """Time steps [i, j) as one device-resident march (Engine.march_run) and everything the per-step path
        would have stored for them (LUDVM.py:765-1090): circulations, Fourier rows, LESP, loads, slot maps -- and,
        with `record` (dense history), the path[...] rows of every step (:1108-1127).
        `place` = [tev_x, lev_x, tev_z, lev_z] of step i.  The loop state S and the result arrays are updated in place."""
        nc, cnt = self.Ncoeffs, j - i
        nf, itev, ilev, LEV_shed = S.nf, S.itev, S.ilev, S.LEV_shed
        n_wake = nf + itev + ilev
        st = np.zeros(16 + nc)
        st[:11] = [n_wake, itev, ilev, float(LEV_shed[i - 1] != -1), S.lesp_crit, S.sum_tev, S.sum_lev] + list(place)
        # wake sizes after the four anchor steps before this call (ludvm_march_run, `anchors`): the launch geometry of
        # every step then follows from the step number and the run itself, not from where the stretches begin
        shed_before = np.cumsum(LEV_shed[:i] != -1)            # LEVs shed in steps 0 .. q (step 0 sheds none)
        anchors = [nf + a + int(shed_before[a]) for a in self.engine.march_anchor_steps(i)]      # (all of them < i)
        st[16:] = self.fourier[i - 1, 0, :]
        hist = None
        if record:
            R, hist = self.engine.march_run(i, cnt, S.prec_code, st, hist_nmax=n_wake + 2 * cnt, anchors=anchors)
        else:
            R = self.engine.march_run(i, cnt, S.prec_code, st, anchors=anchors)
        if S.probes is not None:
            self.probe_u[i:j], self.probe_w[i:j] = self.engine.march_probes(cnt)
        if S.integrals:
            self.integral_sums[i:j], self.wake_energy[i:j] = self.engine.march_integrals(cnt)
        if S.tracers is not None:
            for srow, row in zip(*self.engine.march_tracers()):
                self.tracer_path.store(int(srow), row)
            if self.tracer_gradient:
                for srow, row in zip(*self.engine.march_tracer_gradient()):
                    self.tracer_F_path.store(int(srow), row)
        self._store_march_results(S, i, j, st, R, hist)

    def _store_march_results(self, S, i, j, st, R, hist=None):
        """What time steps [i, j) leave in the result arrays and in the loop state S, from their device rows R
        (ludvm_march_run's layout; ludvm_ensemble_run returns the same), the state `st` after them (st[0] wake size, st[1]
        TEVs shed, st[4..6] LESPcrit and the Kelvin sums, st[12..15] the two newest vortices) and -- hist given -- the wake's
        positions after each recorded step, hist[r, 0 | 1] in wake order."""
        C, nc, npan, cnt = self.circulation, self.Ncoeffs, self.Npoints - 1, j - i
        nf, itev, ilev, LEV_shed, tev_slot, lev_slot = S.nf, S.itev, S.ilev, S.LEV_shed, S.tev_slot, S.lev_slot
        H = self.engine.MARCH_ROW_HEAD
        n_wake = nf + itev + ilev
        record = hist is not None
        steps = np.arange(i, j)
        tix = itev + np.arange(cnt)
        shed_v = R[:, 2] != 0
        n_shed = int(shed_v.sum())
        slot = R[:, 9].astype(np.int64)
        if int(st[1]) != itev + cnt or int(st[0]) != n_wake + cnt + n_shed:
            raise RuntimeError("device march returned an inconsistent state")
        C['TEV'][tix] = R[:, 0]
        C['bound'][tix] = R[:, 3]
        self.LESP_prev[tix], self.LESP[tix] = R[:, 4], R[:, 5]
        self.Fn[steps], self.Fs[steps], self.M[steps] = R[:, 6], R[:, 7], R[:, 8]
        ca, sa = np.cos(self.alpha[steps]), np.sin(self.alpha[steps])
        self.L[steps] = self.Fn[steps] * ca + self.Fs[steps] * sa             # :1077-1081
        self.D[steps] = self.Fn[steps] * sa - self.Fs[steps] * ca
        self.T[steps] = -self.D[steps]
        tev_slot[tix] = slot
        levs_before = ilev + np.cumsum(shed_v) - shed_v          # LEVs shed before each step
        lix = levs_before[shed_v]
        C['LEV'][lix] = R[shed_v, 1]
        lev_slot[lix] = slot[shed_v] + 1
        LEV_shed[steps[shed_v]] = lix
        self.fourier[steps, 0, :] = R[:, H:H + nc]
        self.fourier[steps, 1, :] = R[:, H + nc:H + 2 * nc]
        C['gamma_airfoil'][tix] = R[:, H + 2 * nc:H + 2 * nc + npan]
        C['airfoil'][tix] = R[:, H + 2 * nc + npan:]
        C['Gamma_airfoil'][tix] = np.cumsum(C['airfoil'][tix], axis=1)
        if record:
            self._store_marched_rows(S, i, cnt, R, hist, shed_v, levs_before)
        last_shed = bool(shed_v[-1])
        # as the per-step path leaves them: the counters before the last step's increment
        self.itev, self.ilev, self.LEV_shed = itev + cnt - 1, ilev + n_shed - int(last_shed), LEV_shed
        if last_shed:       # newest TEV at size - 2, newest LEV at size - 1
            S.last_tev, S.last_lev = np.array([st[12], st[14]]), np.array([st[13], st[15]])
        else:
            S.last_tev = np.array([st[13], st[15]])
        S.itev, S.ilev = itev + cnt, ilev + n_shed
        S.lesp_crit, S.sum_tev, S.sum_lev = float(st[4]), float(st[5]), float(st[6])

    def _store_marched_rows(self, S, i, cnt, R, hist, shed_v, levs_before):
        """History rows from the march's per-step snapshots (wake order -> TEV / LEV / FREE slots); on a step without LEV
        shedding the reference's zero-strength LEV slot lands at dt * (velocity at the origin)."""
        P, tev_slot, lev_slot, fsl = self.path, S.tev_slot, S.lev_slot, S.fsl
        for r in range(cnt):
            q, it, il = i + r, S.itev + r, int(levs_before[r])
            xs, zs = hist[r, 0], hist[r, 1]
            ts = tev_slot[:it + 1]
            ls = lev_slot[:il + 1] if shed_v[r] else lev_slot[:il]
            if self.history == 'full':
                P['TEV'][q, 0, :it + 1], P['TEV'][q, 1, :it + 1] = xs[ts], zs[ts]
                P['LEV'][q, 0, :len(ls)], P['LEV'][q, 1, :len(ls)] = xs[ls], zs[ls]
                if not shed_v[r]:
                    P['LEV'][q, :, il] = self.dt * R[r, 10:12]
                P['FREE'][q, 0, :], P['FREE'][q, 1, :] = xs[fsl], zs[fsl]
            elif self._record_row(q):
                # sparse history: the rows the per-step path would have stored (LEV row with the zero-strength slot)
                row_l = np.stack([xs[ls], zs[ls]])
                if not shed_v[r]:
                    row_l = np.concatenate([row_l, (self.dt * R[r, 10:12])[:, None]], axis=1)
                P['TEV'].store(q, np.stack([xs[ts], zs[ts]]))
                P['LEV'].store(q, row_l)
                P['FREE'].store(q, np.stack([xs[fsl], zs[fsl]]))

    # ---- the per-step path: one device round trip, solve on the host --------------------------------------------------------
    def _host_step(self, S, i, print_dt):
        self._progress(i, print_dt)
        n_wake = S.nf + S.itev + S.ilev
        tev_xy, lev_xy, sums = self._chord_sums(S, i, n_wake)
        g_tev, g_lev, shed, A = self._solve_circulations(S, i, sums)
        dGamma = self._bound_vorticity_and_loads(S, i, sums, g_tev, g_lev, shed, A)
        self._roll_up(S, i, n_wake, tev_xy, lev_xy, g_tev, g_lev, shed, dGamma)
        S.sum_tev += g_tev
        self.ilev, self.itev, self.LEV_shed = S.ilev, S.itev, S.LEV_shed
        if shed:
            S.sum_lev += g_lev
            S.ilev += 1
        S.itev += 1
        if self.checkpoint_every and i % self.checkpoint_every == 0 and i < self.nt - 1:
            self._write_checkpoint(S, i + 1)

    def _chord_sums(self, S, i, n_wake):
        """Existing wake -> chord (T1), unit new TEV -> chord (T2), unit candidate LEV -> chord (T3): one round trip
        (:743-754, :924-934).  -> (tev_xy, lev_xy, (u1, w1, ut1, wt1, ul1, wl1)) in the global frame."""
        eng, sb = self.engine, S.sb
        xg, zg = S.gpts[i, 0, :], S.gpts[i, 1, :]
        if S.have_next:
            # placed on the device right after the previous roll-up, sums already here
            tev_xy = np.array([sb.unit[0, 0], sb.unit[1, 0]])
            lev_xy = np.array([sb.unit[0, 1], sb.unit[1, 1]])
            return tev_xy, lev_xy, (sb.u, sb.w, sb.uu[0], sb.wu[0], sb.uu[1], sb.wu[1])
        tev_xy, lev_xy = self._next_placement(S, i)
        if sb is not None:
            sb.unit[0, 0], sb.unit[0, 1], sb.unit[1, 0], sb.unit[1, 1] = tev_xy[0], lev_xy[0], tev_xy[1], lev_xy[1]
            eng.wake_chord_sums_into(sb, n_wake, xg, zg, float(self.v_core))
            return tev_xy, lev_xy, (sb.u, sb.w, sb.uu[0], sb.wu[0], sb.uu[1], sb.wu[1])
        u1, w1, uu, wu = eng.wake_chord_sums(0, n_wake, xg, zg, [tev_xy[0], lev_xy[0]], [tev_xy[1], lev_xy[1]], self.v_core)
        return tev_xy, lev_xy, (u1, w1, uu[0], wu[0], uu[1], wu[1])

    def _solve_circulations(self, S, i, sums):
        """Gamma_TEV from Kelvin's condition (:758-760, or Ramesh's Newton :683-739), the Fourier projection (:765-773), the
        LESP test (:781) and, when it trips, Gamma_TEV / Gamma_LEV together (:944-954, :807-914).
        -> (g_tev, g_lev, shed, A)."""
        pi, U, c, dt = np.pi, self.Uinf, self.chord, self.dt
        C, itev, ilev = self.circulation, S.itev, S.ilev
        wq, cproj, cm1, detadx = self._wq, self._cproj, self._cm1, S.detadx
        u1, w1, ut1, wt1, ul1, wl1 = sums
        T1 = self._downwash_from(u1, w1, i)
        ut, un = self._chord_frame(ut1, wt1, i)
        T2 = detadx * ut - un
        I1, I2 = T1 @ cm1, T2 @ cm1
        kelvin = S.sum_tev + S.sum_lev + S.sum_free - C['IC']
        if self.method == 'Ramesh':
            g_tev = self._newton_tev(T1, T2, kelvin)                         # :683-739
        elif self.method == 'Faure':
            g_tev = -(I1 + kelvin) / (1 + I2)                                # :758-760
        else:
            raise ValueError("method must be 'Faure' or 'Ramesh'")
        g_lev = 0.0
        W = T1 + g_tev * T2
        A = cproj @ (W / U)
        C['bound'][itev] = I1 + g_tev * I2 if self.method == 'Faure' else U * c * pi * (A[0] + A[1] / 2)
        self.fourier[i, 0, :] = A
        self.fourier[i, 1, :] = (A - self.fourier[i - 1, 0, :]) / dt          # :772-773
        self.LESP_prev[itev] = A[0]

        shed = abs(A[0]) >= abs(S.lesp_crit)                                  # :781
        if shed:
            S.LEV_shed[i] = ilev
            S.lesp_crit = -abs(S.lesp_crit) if A[0] < 0 else abs(S.lesp_crit)   # :802-805
            ult, uln = self._chord_frame(ul1, wl1, i)
            T3 = detadx * ult - uln
            I3 = T3 @ cm1
            J1, J2, J3 = (-1 / pi * (T @ wq) for T in (T1, T2, T3))
            if self.method == 'Ramesh':
                g_tev, g_lev = self._newton_tev_lev(T1, T2, T3, kelvin, S.lesp_crit, g_tev)   # :807-914
            else:
                g_tev, g_lev = np.linalg.solve(np.array([[1 + I2, 1 + I3], [J2, J3]]),
                                               np.array([-(I1 + kelvin), S.lesp_crit - J1]))  # :944-954
            W = T1 + g_tev * T2 + g_lev * T3
            A = cproj @ (W / U)
            if self.method == 'Faure':
                C['bound'][itev] = I1 + g_tev * I2 + g_lev * I3
                A[0] = J1 + g_tev * J2 + g_lev * J3                           # :959
            else:
                C['bound'][itev] = U * c * pi * (A[0] + A[1] / 2)
            self.fourier[i, 0, :] = A       # derivatives keep their pre-LEV values (:963-966)
            C['LEV'][ilev] = g_lev
        C['TEV'][itev] = g_tev
        self.LESP[itev] = A[0]
        return g_tev, g_lev, shed, A

    def _bound_vorticity_and_loads(self, S, i, sums, g_tev, g_lev, shed, A):
        """Bound vorticity per panel (:987-1010) and the loads (:1035-1090).  The tangential velocity on the chord from the
        full wake (incl. the new TEV/LEV with their solved circulations) follows by linearity from u1 and the unit
        influences already evaluated: no further pair sum.  -> dGamma, the panel circulations."""
        pi, U, c, rho = np.pi, self.Uinf, self.chord, self.rho
        C, itev = self.circulation, S.itev
        u1, w1, ut1, wt1, ul1, wl1 = sums
        A0, A1, A2 = A[0], A[1], A[2]
        A0d, A1d, A2d, A3d = self.fourier[i, 1, :4]
        gamma = 2 * U * (A0 * S.one_plus_cos_over_sin + A[1:] @ self._ssin)
        dGamma = gamma * S.half_c_sin_dth
        C['airfoil'][itev], C['gamma_airfoil'][itev] = dGamma, gamma
        C['Gamma_airfoil'][itev] = np.cumsum(dGamma)

        uc1, wc1 = u1 + g_tev * ut1, w1 + g_tev * wt1
        if shed:
            uc1, wc1 = uc1 + g_lev * ul1, wc1 + g_lev * wl1
        u, _ = self._chord_frame(uc1, wc1, i)
        a, hd = self.alpha[i], self.h_dot[i]
        Ueff = U * np.cos(a) + hd * np.sin(a)
        self.Fn[i] = rho * pi * c * U * (Ueff * (A0 + 0.5 * A1) + c * (3 / 4 * A0d + 1 / 4 * A1d + 1 / 8 * A2d)) \
            + rho * ((u * gamma) @ S.wx)
        self.Fs[i] = rho * pi * c * U**2 * A0**2
        self.L[i] = self.Fn[i] * np.cos(a) + self.Fs[i] * np.sin(a)
        self.D[i] = self.Fn[i] * np.sin(a) - self.Fs[i] * np.cos(a)
        self.T[i] = -self.D[i]
        self.M[i] = self.piv * self.Fn[i] - rho * pi * c**2 * U * (
            Ueff * (1 / 4 * A0 + 1 / 4 * A1 - 1 / 8 * A2)
            + c * (7 / 16 * A0d + 3 / 16 * A1d + 1 / 16 * A2d - 1 / 64 * A3d)) \
            - rho * ((u * gamma * S.x_gamma) @ S.wx)
        return dGamma

    def _roll_up(self, S, i, n_wake, tev_xy, lev_xy, g_tev, g_lev, shed, dGamma):
        """Wake roll-up (:1095-1127): shed vortices join the resident wake, then one fused launch (wake + bound vortices ->
        every wake vortex, explicit Euler update on the device); the history row of a recorded step."""
        eng, sb, P, nt = self.engine, S.sb, self.path, self.nt
        itev, ilev, tev_slot, lev_slot = S.itev, S.ilev, S.tev_slot, S.lev_slot
        dt, vc = self.dt, self.v_core
        xg, zg = S.gpts[i, 0, :], S.gpts[i, 1, :]
        record = self._record_row(i)
        new_x, new_z, new_g = [tev_xy[0]], [tev_xy[1]], [g_tev]
        tev_slot[itev] = n_wake
        if shed:
            lev_slot[ilev] = n_wake + 1
            new_x.append(lev_xy[0]); new_z.append(lev_xy[1]); new_g.append(g_lev)
        elif record:
            # the reference also convects LEV slot `ilev` (zero strength, at the origin) on a
            # non-shedding step and stores it in path['LEV'][i]; reproduce that row entry
            new_x.append(0.0); new_z.append(0.0); new_g.append(0.0)
        if S.probes is not None:
            # the field that convects the wake in this step, at the probes: the old wake (still all the device holds) plus
            # one float64 call for the shed vortices and the bound vortices
            px, pz = self.probe_positions(i)
            ns = 2 if shed else 1          # (not the phantom LEV slot of a recorded step)
            uo, wo = eng.wake_induce_on_points(0, n_wake, px, pz, vc)
            un, wn = eng.induce(np.concatenate([new_g[:ns], dGamma]), np.concatenate([new_x[:ns], xg]), np.concatenate([new_z[:ns], zg]),
                                px, pz, vc, precision='f64')
            self.probe_u[i], self.probe_w[i] = uo + un, wo + wn
        if S.tracers is not None:
            # the same field at the released tracers' start positions, and their Euler step (held ones ride with the seed)
            seeds = self._tracer_seeds(i)
            rel, nxt = self.tracer_release, seeds
            free = rel <= i
            if free.any():
                first = (rel == i)[free]
                px = np.where(first, seeds[0][free], S.tcur[0][free])
                pz = np.where(first, seeds[1][free], S.tcur[1][free])
                ns = 2 if shed else 1
                uo, wo = eng.wake_induce_on_points(0, n_wake, px, pz, vc)
                un, wn = eng.induce(np.concatenate([new_g[:ns], dGamma]), np.concatenate([new_x[:ns], xg]),
                                    np.concatenate([new_z[:ns], zg]), px, pz, vc, precision='f64')
                nxt[0][free], nxt[1][free] = px + dt * (uo + un), pz + dt * (wo + wn)
            S.tcur = nxt
            k = int(np.searchsorted(S.trec, i))
            if k < len(S.trec) and S.trec[k] == i:
                self.tracer_path.store(i, nxt.copy())
        if S.survey is not None and self._survey_sampled(i):
            # the same field at the survey points, added to the five raw sums in step order
            px, pz = self._survey_points(i)
            ns = 2 if shed else 1
            uo, wo = eng.wake_induce_on_points(0, n_wake, px, pz, vc)
            un, wn = eng.induce(np.concatenate([new_g[:ns], dGamma]), np.concatenate([new_x[:ns], xg]), np.concatenate([new_z[:ns], zg]),
                                px, pz, vc, precision='f64')
            u, w = uo + un, wo + wn
            for acc, term in zip(S.ssums, (u, w, u * u, w * w, u * w)):
                acc += term
            S.scount += 1
            if S.sbins is not None and S.sbins[i] >= 0:
                # ... and to the sums of the step's bin, the same terms in the same order
                for acc, term in zip(S.sbsums[S.sbins[i]], (u, w, u * u, w * w, u * w)):
                    acc += term
                S.sbcounts[S.sbins[i]] += 1
            if S.sgsums is not None:
                # the gradient of that field over the step's sources in their order -- old wake, shed vortices, bound vortices --
                # in one call, and the five terms ux, e, omega, omega^2, Q.  gradient_field returns the two shear terms, so omega
                # is their difference here: its absolute error is an ulp of |uz|, far inside what the sums are compared to
                wx_, wz_, wg_ = eng.wake_read(0, n_wake, gamma=True) if n_wake else (np.empty(0),) * 3
                ux, uz, wx = eng.gradient_field(np.concatenate([wg_, new_g[:ns], dGamma]), np.concatenate([wx_, new_x[:ns], xg]),
                                                np.concatenate([wz_, new_z[:ns], zg]), px, pz, vc)
                e, om = 0.5 * (uz + wx), wx - uz
                terms = (ux, e, om, om * om, 0.25 * (om * om) - ux * ux - e * e)
                for acc, term in zip(S.sgsums, terms):
                    acc += term
                if S.sbgsums is not None and S.sbins[i] >= 0:
                    for acc, term in zip(S.sbgsums[S.sbins[i]], terms):
                        acc += term
        if S.integrals:
            # the step's sources in the march's order -- old wake, shed vortices, bound vortices -- and their classes
            ns = 2 if shed else 1
            wx_, wz_, wg_ = eng.wake_read(0, n_wake, gamma=True) if n_wake else (np.empty(0),) * 3
            g_all = np.concatenate([wg_, new_g[:ns], dGamma])
            x_all, z_all = np.concatenate([wx_, new_x[:ns], xg]), np.concatenate([wz_, new_z[:ns], zg])
            cls_all = np.concatenate([self._wake_tags(S), [1, 2][:ns], np.full(len(xg), 3)])
            self.integral_sums[i] = self._integral_row(cls_all, g_all, x_all, z_all)
            if self._energy_sampled(i):
                psi = eng.scalar_field('psi', g_all, x_all, z_all, x_all, z_all, vc)
                self.wake_energy[i] = 0.5 * float(np.sum(g_all * psi))
        n_after = n_wake + len(new_x)
        one_trip = (not record) and sb is not None and i < nt - 1 and hasattr(eng, 'wake_step_into')
        if not one_trip:
            eng.wake_append(new_x, new_z, new_g)

        if record:
            S.have_next = False
            eng.wake_advect(dt, xg, zg, dGamma, vc, precision=self.precision)
            xs, zs = eng.wake_read(0, n_after)
            row_t = np.stack([xs[tev_slot[:itev + 1]], zs[tev_slot[:itev + 1]]])
            lslots = lev_slot[:ilev + 1] if shed else np.append(lev_slot[:ilev], n_after - 1)
            row_l = np.stack([xs[lslots], zs[lslots]])
            row_f = np.stack([xs[S.fsl], zs[S.fsl]])
            if self.history == 'full':
                P['TEV'][i, :, :itev + 1] = row_t
                P['LEV'][i, :, :ilev + 1] = row_l
                P['FREE'][i] = row_f
            else:
                P['TEV'].store(i, row_t)
                P['LEV'].store(i, row_l)
                P['FREE'].store(i, row_f)
            S.last_tev = row_t[:, -1].copy()
            if shed:
                S.last_lev = row_l[:, -1].copy()
            elif len(new_x) == 2:
                eng.wake_truncate(n_after - 1)   # drop the phantom LEV slot
            return
        # only the newest TEV / LEV come back: they place the next ones (:680-681, :797-798)
        k = 2 if shed else 1
        S.have_next = False
        dt_f, vc_f = float(dt), float(vc)
        if one_trip:
            # append of the shed vortices + roll-up of this step + placement and chord sums of the
            # next one: one packed upload, one download
            foil, gpts = S.foil, S.gpts
            eng.wake_step_into(sb, np.array(new_x), np.array(new_z), np.array(new_g, dtype=float), dt_f, xg, zg,
                               dGamma, vc_f, S.prec_code, np.ascontiguousarray(foil[i + 1, :, -1]),
                               np.ascontiguousarray(foil[i + 1, :, 0]), shed, k, gpts[i + 1, 0, :],
                               gpts[i + 1, 1, :])
            xs, zs = sb.tail[0], sb.tail[1]
            S.have_next = True
        elif sb is not None:
            eng.wake_advect_tail_into(sb, dt_f, xg, zg, dGamma, vc_f, k, S.prec_code)
            xs, zs = sb.tail[0], sb.tail[1]
        else:
            xs, zs = eng.wake_advect_tail(dt, xg, zg, dGamma, vc, k, precision=self.precision)
        S.last_tev = np.array([xs[0], zs[0]])
        if shed:
            S.last_lev = np.array([xs[1], zs[1]])

    # ------------------------------------------------------------------------------------------
    # checkpoint / resume (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _write_checkpoint(self, S, next_step):
        # one simulation shared by several ranks: every rank holds the same state, rank 0 alone writes it (they would race on
        # the temporary file), and nobody goes on before the file is in place
        sh = self._shard if (self._shard is not None and self._shard.world > 1) else None
        if sh is None:
            return self._write_checkpoint_file(S, next_step)
        # The ranks meet in all_ok() -- the barrier -- and learn there whether the file is in place: if rank 0 could not
        # write it (disk full, bad path) everybody raises, instead of rank 0 raising alone and the others waiting for it in
        # a collective that has no timeout
        err = None
        if sh.rank == 0:
            try:
                self._write_checkpoint_file(S, next_step)
            except Exception as e:          # noqa: BLE001  (re-raised below, on every rank)
                err = e
        if not sh.all_ok(err is None):
            if err is not None:
                raise err
            raise RuntimeError(f"rank 0 could not write the checkpoint {self.checkpoint_path}")

    def _write_checkpoint_file(self, S, next_step):
        import json
        import os
        C, P = self.circulation, self.path
        itev, ilev, lesp_crit, sum_tev, sum_lev = S.itev, S.ilev, S.lesp_crit, S.sum_tev, S.sum_lev
        last_tev, last_lev, LEV_shed, tev_slot, lev_slot = S.last_tev, S.last_lev, S.LEV_shed, S.tev_slot, S.lev_slot
        n = self.engine.wake_size()
        wx, wz, wg = self.engine.wake_read(0, n, gamma=True)
        nan2 = np.full(2, np.nan)
        d = dict(ctor=np.array(json.dumps(self._ctor)), next_step=next_step, itev=itev, ilev=ilev, lesp_crit=lesp_crit,
                 sum_tev=sum_tev, sum_lev=sum_lev, last_tev=nan2 if last_tev is None else last_tev,
                 last_lev=nan2 if last_lev is None else last_lev, LEV_shed=LEV_shed, tev_slot=tev_slot,
                 lev_slot=lev_slot, self_itev=self.itev, self_ilev=self.ilev, wake_x=wx, wake_z=wz, wake_g=wg,
                 circulation_freevort=np.asarray(self.circulation_freevort),
                 free_slot=np.zeros(0, np.int64) if self._free_slot is None else self._free_slot,
                 xy_freevort=np.asarray(self.xy_freevort, dtype=float))
        for key in ('TEV', 'LEV', 'bound', 'airfoil', 'gamma_airfoil', 'Gamma_airfoil'):
            d['circ_' + key] = C[key]
        for name in ('Fn', 'Fs', 'L', 'D', 'T', 'M', 'fourier', 'LESP', 'LESP_prev'):
            d[name] = getattr(self, name)
        if S.probes is not None:        # (the definition travels in `ctor`)
            d['probe_u'], d['probe_w'] = self.probe_u[:next_step], self.probe_w[:next_step]
        if S.integrals:                 # (likewise; the tags are re-derived from the slot maps)
            d['integral_sums'], d['wake_energy'] = self.integral_sums[:next_step], self.wake_energy[:next_step]
        if S.tracers is not None:       # (likewise; the current positions and the rows recorded so far)
            d['tracer_cur'] = self.engine.march_tracer_state() if S.can_march else S.tcur
            steps_t = self.tracer_path.steps()
            d['tracer_rows_steps'] = np.array(steps_t, dtype=np.int64)
            d['tracer_rows'] = np.stack([self.tracer_path[q] for q in steps_t])
            if self.tracer_gradient:    # (the current deformation gradient and its rows, the steps of tracer_rows)
                d['tracer_F_cur'] = self.engine.march_tracer_gradient_state()
                d['tracer_F_rows'] = np.stack([self.tracer_F_path[q] for q in steps_t])
        if S.survey is not None:        # (likewise; the sums and the count of sampled steps so far)
            d['survey_sums'], d['survey_samples'] = self.engine.march_survey() if S.can_march else (S.ssums, S.scount)
        if S.sbins is not None:         # (likewise; the sums and the samples of every bin so far)
            d['survey_bin_sums'], d['survey_bin_counts'] = self.engine.march_survey_bins() if S.can_march else (S.sbsums, S.sbcounts)
        if S.sgsums is not None:        # (likewise; the gradient sums, whose counts are the two above)
            g, bg = self.engine.march_survey_gradient() if S.can_march else (S.sgsums, S.sbgsums)
            d['survey_grad_sums'] = g
            if bg is not None:
                d['survey_bin_grad_sums'] = bg
        if self.history == 'full':
            for key in ('TEV', 'LEV', 'FREE'):
                d['path_' + key] = P[key][:next_step]
        else:
            steps = P['TEV'].steps()
            d['rows_steps'] = np.array(steps, dtype=np.int64)
            for key in ('TEV', 'LEV', 'FREE'):
                for srow in steps:
                    d[f'row_{key}_{srow}'] = P[key][srow]
        tmp = self.checkpoint_path + '.tmp.npz'
        np.savez(tmp, **d)
        os.replace(tmp, self.checkpoint_path)      # a reader never sees a half-written file

    @classmethod
    def resume(cls, path, engine=None, device=0, verbose=True, checkpoint_every=0, checkpoint_path=None, march=True,
               distributed=None, devices=None):
        """Continue a run from a checkpoint written with `checkpoint_every` / `checkpoint_path`: rebuilds
        geometry and kinematics from the stored constructor arguments, uploads the wake and marches
        from the stored step to the end.  `distributed` as in the constructor: every rank of the group resumes from the
        same file; `devices` as in the constructor: one process, a replica per device, each resumed from the file."""
        import json
        if devices is not None:
            from .multi import MultiDeviceLUDVM, normalise_devices
            devs = normalise_devices(devices)
            if len(devs) > 1:
                if engine is not None or distributed is not None:
                    raise ValueError("devices=[...] creates the engines and their communicator itself: do not pass engine= / distributed=")
                if json.loads(str(np.load(path, allow_pickle=False)['ctor'])).get('probes') is not None:
                    raise ValueError("probes run on one GPU: this checkpoint cannot be resumed on more than one device")
                if json.loads(str(np.load(path, allow_pickle=False)['ctor'])).get('tracers') is not None:
                    raise ValueError("tracers run on one GPU: this checkpoint cannot be resumed on more than one device")
                if json.loads(str(np.load(path, allow_pickle=False)['ctor'])).get('wake_integrals'):
                    raise ValueError("wake_integrals runs on one GPU: this checkpoint cannot be resumed on more than one device")
                if json.loads(str(np.load(path, allow_pickle=False)['ctor'])).get('survey') is not None:
                    raise ValueError("a survey runs on one GPU: this checkpoint cannot be resumed on more than one device")
                return MultiDeviceLUDVM((), {}, devs, builder=lambda r, eng, grp: cls.resume(
                    path, engine=eng, verbose=verbose and r == 0, checkpoint_every=checkpoint_every, checkpoint_path=checkpoint_path,
                    march=march, distributed=grp))
            device = devs[0]
        R = np.load(path, allow_pickle=False)
        kw = json.loads(str(R['ctor']))
        free = {}
        if R['circulation_freevort'].size != 1 or float(np.abs(R['circulation_freevort']).sum()) != 0.0 \
                or float(np.abs(R['xy_freevort']).sum()) != 0.0:
            free = dict(circulation_freevort=R['circulation_freevort'], xy_freevort=R['xy_freevort'])
        sim = cls(**kw, **free, verbose=verbose, engine=engine, device=device, run=False,
                  checkpoint_every=checkpoint_every, checkpoint_path=checkpoint_path, march=march, distributed=distributed)
        sim.time_loop(_resume=R)
        sim.compute_coefficients()
        return sim

    @classmethod
    def sweep(cls, cases, **kwargs):
        """Many small simulations in one device launch: `ludvm_amd.sweep(cases, **kwargs)` (ludvm_amd/ensemble.py) building
        members of this class."""
        from .ensemble import sweep
        return sweep(cases, cls=cls, **kwargs)

    # Newton variants of the reference's 'Ramesh' method.  The downwash is linear in the circulations
    # of the vortices being shed, W = T1 + G_tev T2 + G_lev T3, so the reference's repeated
    # airfoil_downwash evaluations (:692, :707, :820, :837, :852) need no further pair sums here.
    def _kelvin_residual(self, W, kelvin, g_new):
        A0 = self._cproj[0] @ (W / self.Uinf)
        A1 = self._cproj[1] @ (W / self.Uinf)
        return self.Uinf * self.chord * np.pi * (A0 + A1 / 2) + kelvin + g_new, A0

    def _newton_tev(self, T1, T2, kelvin):
        eps = self.epsilon
        f, niter, g = 1.0, 1, -1.0
        while abs(f) > self.maxerror and niter < self.maxiter:
            f, _ = self._kelvin_residual(T1 + g * T2, kelvin, g)
            fd, _ = self._kelvin_residual(T1 + (g + eps) * T2, kelvin, g + eps)
            g = g - f / ((fd - f) / eps)
            niter += 1
        if niter >= self.maxiter:
            print('The solution did not converge during the Newton-Raphson iteration')
        return g

    def _newton_tev_lev(self, T1, T2, T3, kelvin, lesp_crit, guess):
        eps = self.epsilon
        g_tev = g_lev = guess
        f1 = f2 = 0.1
        niter = 1

        def res(gt, gl):
            f, A0 = self._kelvin_residual(T1 + gt * T2 + gl * T3, kelvin, gt + gl)
            return f, lesp_crit - A0

        while (abs(f1) > self.maxerror or abs(f2) > self.maxerror) and niter < self.maxiter:
            f1, f2 = res(g_tev, g_lev)
            f1t, f2t = res(g_tev + eps, g_lev)
            f1l, f2l = res(g_tev, g_lev + eps)
            J = np.array([[(f1l - f1) / eps, (f1t - f1) / eps], [(f2l - f2) / eps, (f2t - f2) / eps]])
            g_lev, g_tev = np.array([g_lev, g_tev]) - np.linalg.solve(J, np.array([f1, f2]))
            niter += 1
        if niter >= self.maxiter:
            print('The solution did not converge when solving the LEV-TEV nonlinear system')
        return g_tev, g_lev

    def compute_coefficients(self):
        """Force and moment coefficients (LUDVM.py:1173-1184)."""
        q = 0.5 * self.rho * self.Uinf**2
        qc = q * self.chord
        self.Cp = self.dp / q
        self.Cn, self.Cs = self.Fn / qc, self.Fs / qc
        self.Cl, self.Cd, self.Ct = self.L / qc, self.D / qc, self.T / qc
        self.Cm = self.M / (qc * self.chord)
        return None

    # ------------------------------------------------------------------------------------------
    # flow field
    # ------------------------------------------------------------------------------------------
    def _flowfield_sources(self, s):
        """Sources the reference gathers for time step s (LUDVM.py:1202-1215), index quirks kept:
        TEV/LEV positions from row s-1 with slots [:s+1] / [:ilev+1] (not-yet-shed slots sit at the
        origin but carry their final circulation), FREE from row s, every LEV dropped when
        LEV_shed[s] == -1; bound vortices of step s-1."""
        C, P = self.circulation, self.path
        g_free = np.asarray(C['FREE'], dtype=float)
        if s == 0:
            f0 = P['FREE'][0]
            return g_free, f0[0], f0[1]
        ilev = int(self.LEV_shed[s])

        def padded(row, n):
            out = np.zeros([2, n])
            m = min(n, row.shape[1])
            out[:, :m] = row[:, :m]
            return out
        tev = padded(P['TEV'][s - 1], s + 1)
        lev = padded(P['LEV'][s - 1], ilev + 1)
        free = P['FREE'][s]
        gp = self.path['airfoil_gamma_points'][s - 1]
        g = np.concatenate([C['TEV'][:s + 1], C['LEV'][:ilev + 1], g_free, C['airfoil'][s - 1, :]])
        xw = np.concatenate([tev[0], lev[0], free[0], gp[0]])
        zw = np.concatenate([tev[1], lev[1], free[1], gp[1]])
        return g, xw, zw

    @staticmethod
    def flowfield_rows_needed(tsteps):
        """History rows `flowfield(tsteps=...)` reads: the reference takes TEV / LEV positions from row s - 1 and FREE
        positions from row s (LUDVM.py:1212-1213).  A run with history='sparse' must have recorded them:
        LUDVM(..., snapshot_steps=LUDVM.flowfield_rows_needed(tsteps))."""
        return sorted({r for s in tsteps for r in ((int(s) - 1, int(s)) if int(s) > 0 else (0,))})

    def flowfield(self, xmin=-10, xmax=0, zmin=-4, zmax=4, dr=0.02, tsteps=[0, 1, 2], psi=False, omega=False, grad=False,
                  field_precision='f64'):
        """Velocity and vorticity on the uniform mesh arange(xmin, xmax, dr) x arange(zmin, zmax, dr)
        at the requested time steps (LUDVM.py:1186-1298).  The mesh points are generated on the
        device (x-major, as meshgrid(indexing='ij') ravels, :1194-1195); wake and bound vortices go in
        one launch; the vorticity stencil (:1224-1292) runs on the device on the velocity fields where they
        are, and the three fields come back together.  A run in precision 'f64' (what 'auto' picks for every case whose
        dense history the reference itself could hold) evaluates the field in float64 throughout, as the reference does
        (:1206, :1216-1217): u_ff, w_ff and ome_ff then equal the reference's to rounding; 'f32' / 'f32x2' runs evaluate
        it in fp32 on local-origin sources (~1e-6 of max|u|; the stencil amplifies that by 1 / (2 dr) in ome_ff).
        `psi=True` / `omega=True` add `psi_ff` / `omega_ff` [nsteps, nx, nz] from the same sources on the same mesh: the stream
        function whose contours are the streamlines (of the induced velocity, the fluid far away at rest; `psi_ff + Uinf * z_ff`
        in the frame that translates with the foil, a wind tunnel's) and the core model's vorticity in closed form
        (`stream_function`, `vorticity`) -- float64 whatever the run's precision, and, unlike the stencil's ome_ff, resolved at
        any dr.  `grad=True` adds the velocity gradient in closed form from the same sources on the same mesh
        (`velocity_gradient`): `ux_ff`, `uz_ff`, `wx_ff` and `q_ff` = -ux^2 - uz wx (the Q / Okubo-Weiss criterion: positive in a
        vortex core, negative in a shear layer), [nsteps, nx, nz] each.  One GPU only; u_ff, w_ff and ome_ff (and psi_ff,
        omega_ff) are what they are without the flags.  field_precision='f32x2' evaluates `omega_ff` and the gradient fields (and
        with them `q_ff`) with the pairs in hi+lo fp32: float64 arrays as before, <= 2e-6 of the field's maximum wherever the
        wake lies.  `psi_ff` stays float64 (its logarithm has no fp32 route); u_ff, w_ff and ome_ff follow the run's `precision`
        as they always do."""
        if field_precision not in ('f64', 'f32x2'):
            raise ValueError(f"field_precision must be 'f64' or 'f32x2', not {field_precision!r}")
        if field_precision == 'f32x2' and self._shard is not None and self._shard.world > 1:
            raise ValueError("gradient fields run on one GPU: not with `distributed` or more than one device in `devices`")
        scalars = [kind for kind, on in (('psi', psi), ('omega', omega)) if on]
        if scalars:
            if self._shard is not None and self._shard.world > 1:
                raise ValueError("psi / omega fields run on one GPU: not with `distributed` or more than one device in `devices`")
            if not hasattr(self.engine, 'flowfield_scalar'):
                raise RuntimeError("flowfield(psi=..., omega=...): this engine has no flowfield_scalar")
        if grad:
            if self._shard is not None and self._shard.world > 1:
                raise ValueError("gradient fields run on one GPU: not with `distributed` or more than one device in `devices`")
            if not hasattr(self.engine, 'flowfield_gradient'):
                raise RuntimeError("flowfield(grad=True): this engine has no flowfield_gradient")
        # the default calls the engine as it always was called; 'f32x2' needs an engine whose methods know the keyword
        omega_kw = grad_kw = {}
        if field_precision == 'f32x2':
            def route(name):
                try:
                    known = 'precision' in inspect.signature(getattr(self.engine, name)).parameters
                except (TypeError, ValueError):
                    known = False
                if not known:
                    raise RuntimeError(f"flowfield(field_precision='f32x2'): this engine's {name} has no precision='f32x2'")
                return {'precision': 'f32x2'}
            omega_kw = route('flowfield_scalar') if omega else {}
            grad_kw = route('flowfield_gradient') if grad else {}
        x1, z1 = np.arange(xmin, xmax, dr), np.arange(zmin, zmax, dr)
        nx, nz = len(x1), len(z1)
        x, z = np.meshgrid(x1, z1, indexing='ij')
        nsteps = len(tsteps)
        u = np.zeros([nsteps, nx, nz])
        w = np.zeros([nsteps, nx, nz])
        ome = np.zeros([nsteps, nx, nz])
        extra = {kind: np.zeros([nsteps, nx, nz]) for kind in scalars}
        gradient = np.zeros([3, nsteps, nx, nz]) if grad else None
        fused = hasattr(self.engine, 'flowfield_vorticity')
        sh = self._shard if (self._shard is not None and self._shard.world > 1) else None
        ffp = 'f64' if self.precision == 'f64' else 'f32'
        for ii, s in enumerate(tsteps):
            if self.verbose:
                print('Flowfield tstep =', s)
            try:
                g, xw, zw = self._flowfield_sources(int(s))
            except KeyError as e:
                raise KeyError(f"flowfield(tsteps=[{int(s)}]) reads the history rows of steps {int(s) - 1} and {int(s)}, "
                               f"which this run (history='sparse') did not record: construct it with "
                               f"snapshot_steps=LUDVM.flowfield_rows_needed(tsteps) = "
                               f"{self.flowfield_rows_needed(tsteps)}") from e
            if sh is not None:
                # grid rows in contiguous blocks over the ranks, nothing exchanged until the finished rows are gathered
                r0, r1, _ = sh.block(nx)
                if hasattr(self.engine, 'flowfield_rows'):
                    ub, wb, ob = self.engine.flowfield_rows(xmin, zmin, dr, nx, nz, r0, r1 - r0, g, xw, zw, self.v_core,
                                                            precision=ffp)
                else:       # engines without the row entry: the block with one halo row per interior side
                    h0, h1 = max(0, r0 - 1), min(nx, r1 + 1)
                    uh, wh = self.engine.flowfield(x1[h0] if h1 > h0 else xmin, zmin, dr, h1 - h0, nz, g, xw, zw, self.v_core)
                    oh = self.engine.vorticity(uh, wh, dr) if h1 - h0 >= 2 else np.zeros_like(uh)
                    ub, wb, ob = uh[r0 - h0:r1 - h0], wh[r0 - h0:r1 - h0], oh[r0 - h0:r1 - h0]
                fields = sh.gather_blocks(np.stack([ub, wb, ob], axis=1), nx)     # [nx, 3, nz]
                u[ii], w[ii], ome[ii] = fields[:, 0], fields[:, 1], fields[:, 2]
            elif fused:
                u[ii], w[ii], ome[ii] = self.engine.flowfield_vorticity(xmin, zmin, dr, nx, nz, g, xw, zw, self.v_core,
                                                                        precision=ffp)
            else:
                uf, wf = self.engine.flowfield(xmin, zmin, dr, nx, nz, g, xw, zw, self.v_core)
                u[ii], w[ii] = uf, wf
                ome[ii] = self.engine.vorticity(uf, wf, dr)
            for kind in scalars:
                extra[kind][ii] = self.engine.flowfield_scalar(kind, xmin, zmin, dr, nx, nz, g, xw, zw, self.v_core,
                                                               **(omega_kw if kind == 'omega' else {}))
            if grad:
                gradient[0, ii], gradient[1, ii], gradient[2, ii] = self.engine.flowfield_gradient(xmin, zmin, dr, nx, nz, g, xw, zw,
                                                                                                    self.v_core, **grad_kw)
        self.x_ff, self.z_ff = x, z
        self.u_ff, self.w_ff = u, w
        self.ome_ff = ome
        if psi:
            self.psi_ff = extra['psi']
        if omega:
            self.omega_ff = extra['omega']
        if grad:
            self.ux_ff, self.uz_ff, self.wx_ff = gradient
            self.q_ff = -self.ux_ff * self.ux_ff - self.uz_ff * self.wx_ff
        return None
