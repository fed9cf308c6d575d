"""Thin Python handle on one libludvm_hip context (one GPU, one stream).

Normalises what Python callers pass (any array-like, any dtype, any stride -- the reference's
induced_velocity takes non-contiguous views and integer circulations, LUDVM.py:549-570, :751) into
the contiguous float64 / float32 buffers the C ABI takes, and turns status codes into exceptions.
"""
import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import numpy as np

from . import _ffi
from ._ffi import PREC_F32, PREC_F32X2, PREC_F64, LudvmHipError

PRECISIONS = {"f32": PREC_F32, "f32x2": PREC_F32X2, "f64": PREC_F64}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _pd(a):
    return a.ctypes.data_as(POINTER(c_double)) if a is not None else None


def _pf(a):
    return a.ctypes.data_as(POINTER(c_float)) if a is not None else None


def _prec(p):
    if isinstance(p, str):
        return PRECISIONS[p]
    return int(p)


class Engine:
    """One HIP context.  Not thread-safe (one host thread at a time), like the reference."""

    def __init__(self, device=0, lib_path=None):
        self._lib = _ffi.load(lib_path)
        self._ctx = c_void_p()
        rc = self._lib.ludvm_create(int(device), byref(self._ctx))
        if rc != _ffi.OK:
            self._ctx = c_void_p()
            raise LudvmHipError(rc, {_ffi.E_NODEVICE: "no usable gfx950 device (MI355X required)",
                                     _ffi.E_ARG: "bad device ordinal"}.get(rc, "ludvm_create failed"))
        self.device = int(device)

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _ffi.OK:
            msg = self._lib.ludvm_last_error(self._ctx)
            err = LudvmHipError(rc, msg.decode() if msg else "")
            cause = getattr(self, "_hook_error", None)      # an exception raised inside the all-reduce hook (set_shard)
            if cause is not None:
                self._hook_error = None
                raise err from cause
            raise err

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.ludvm_destroy(self._ctx)
            self._ctx = c_void_p()
            self._hook_c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_info(self):
        cu, khz, mem = c_int(), c_int(), c_longlong()
        name = ctypes.create_string_buffer(256)
        self._check(self._lib.ludvm_device_info(self._ctx, byref(cu), byref(khz), byref(mem), name, 256))
        return {"cu_count": cu.value, "clock_khz": khz.value, "hbm_bytes": mem.value, "name": name.value.decode()}

    def set_stream(self, hip_stream):
        """Adopt an external hipStream_t given as an int handle, e.g.
        torch.cuda.current_stream().cuda_stream -- 0 is the device's default stream (torch's default).
        None goes back to the context's own stream."""
        if hip_stream is None:
            self._check(self._lib.ludvm_set_stream(self._ctx, None, 0))
        else:
            self._check(self._lib.ludvm_set_stream(self._ctx, c_void_p(int(hip_stream)), 1))

    def synchronize(self):
        self._check(self._lib.ludvm_synchronize(self._ctx))

    def set_tuning(self, targets_per_lane=0, source_splits=0):
        self._check(self._lib.ludvm_set_tuning(self._ctx, int(targets_per_lane), int(source_splits)))

    def set_sym_tuning(self, vortices_per_lane=0, rotation_split=0):
        """Tuning of the symmetric kernel (0 = heuristics): tile = 64 * vortices_per_lane (4 or 8), wavefronts
        sharing one tile pair's rotation steps (1, 2, 4)."""
        self._check(self._lib.ludvm_set_sym_tuning(self._ctx, int(vortices_per_lane), int(rotation_split)))

    def set_symmetric(self, mode=1):
        """0: always the direct kernel; 1: self-interaction launches may use the symmetric kernel (each unordered
        pair once, 64-bit fixed-point accumulation: also bitwise reproducible); n >= 2: the same from n vortices."""
        self._check(self._lib.ludvm_set_symmetric(self._ctx, int(mode)))

    def set_self_order(self, mode=1):
        """Symmetric launches on device arrays (induce_dev on one array, advect_dev over the whole array) in Morton order:
        0 never; 1 from the size the library's rule states (kSelfOrderMin); 2 whenever the symmetric kernel runs.  Results
        come back at the caller's indices either way."""
        self._check(self._lib.ludvm_set_self_order(self._ctx, int(mode)))

    def set_shard(self, rank, world, allreduce=None, d_acc=0, acc_bytes=0, min_vortices=0):
        """Evaluate only tile block `rank` of `world` of every symmetric roll-up of at least `min_vortices` vortices;
        `allreduce(count, stream)` must enqueue, on the hipStream_t `stream` (an int handle; 0 = the default stream), an
        in-place sum all-reduce of the first `count` int64 of the accumulator buffer at device address `d_acc`
        (ludvm_set_shard).  world = 1 undoes it."""
        if world > 1:
            def hook(_user, _buf, count, stream):
                try:
                    allreduce(int(count), int(stream or 0))
                    return 0
                except Exception as e:       # never let an exception cross the C frame
                    self._hook_error = e
                    return 1
            self._hook_c = _ffi.ALLREDUCE_FN(hook)        # kept alive as long as the library may call it
            self._check(self._lib.ludvm_set_shard(self._ctx, int(rank), int(world), int(min_vortices),
                                                  ctypes.cast(self._hook_c, c_void_p), None, c_void_p(int(d_acc)),
                                                  int(acc_bytes)))
        else:
            self._check(self._lib.ludvm_set_shard(self._ctx, 0, 1, 0, None, None, None, 0))
            self._hook_c = None

    # -- the library's own RCCL communicator -------------------------------------------------------
    def comm_unique_id(self):
        """128 bytes that identify a new communicator (rank 0 creates them and hands them to the other processes)."""
        _ffi.prefer_matching_rccl()
        buf = ctypes.create_string_buffer(_ffi.COMM_ID_BYTES)
        rc = self._lib.ludvm_comm_unique_id(buf, _ffi.COMM_ID_BYTES)
        if rc != _ffi.OK:
            raise LudvmHipError(rc, "ludvm_comm_unique_id failed (is librccl loadable? LUDVM_RCCL_LIB names it)")
        return buf.raw

    def comm_init(self, rank, world, unique_id, min_vortices=0):
        """Join the communicator `unique_id` as rank `rank` of `world` (one process per GPU; returns when all have joined)
        and shard this engine's symmetric roll-ups over it: one in-library ncclAllReduce per time step."""
        _ffi.prefer_matching_rccl()
        uid = bytes(unique_id)
        if len(uid) != _ffi.COMM_ID_BYTES:
            raise ValueError("comm_init: the identifier is 128 bytes (Engine.comm_unique_id)")
        self._check(self._lib.ludvm_comm_init(self._ctx, int(rank), int(world), uid, len(uid), int(min_vortices)))

    @staticmethod
    def comm_init_all(engines, min_vortices=0):
        """ONE process, one engine per device: the engines join a new communicator in one call (ncclCommInitAll; engines[k]
        becomes rank k) and are sharded as by comm_init.  Each engine is then driven by a host thread of its own
        (ludvm_amd/multi.py)."""
        _ffi.prefer_matching_rccl()
        engines = list(engines)
        arr = (c_void_p * len(engines))(*[e._ctx for e in engines])
        engines[0]._check(engines[0]._lib.ludvm_comm_init_all(arr, len(engines), int(min_vortices)))

    def comm_destroy(self):
        self._check(self._lib.ludvm_comm_destroy(self._ctx))

    def comm_info(self):
        """(rank, world) of the engine's communicator; world = 0 when it has none."""
        r, w = c_int(), c_int()
        self._check(self._lib.ludvm_comm_info(self._ctx, byref(r), byref(w)))
        return r.value, w.value

    def comm_allreduce_i64_dev(self, d_buf, count):
        self._check(self._lib.ludvm_comm_allreduce_i64_dev(self._ctx, d_buf, int(count)))

    def comm_allgather_dev(self, d_send, d_recv, bytes_per_rank):
        self._check(self._lib.ludvm_comm_allgather_dev(self._ctx, d_send, d_recv, int(bytes_per_rank)))

    def comm_allgather(self, local):
        """All ranks' copies of the contiguous array `local` (same shape and dtype everywhere) stacked along a new first
        axis: [world, *local.shape] (host arrays; synchronous)."""
        local = np.ascontiguousarray(local)
        _, world = self.comm_info()
        out = np.empty((world,) + local.shape, local.dtype)
        self._check(self._lib.ludvm_comm_allgather_host(self._ctx, local.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p),
                                                        local.nbytes))
        return out

    # -- stateless pair sum ----------------------------------------------------------------------
    def induce(self, circulation, xw, zw, xp, zp, v_core, precision="f32"):
        """(u, w) float64 arrays; host arrays in, host arrays out (LUDVM.py:549-570)."""
        g, xs, zs = _f64(circulation), _f64(xw), _f64(zw)
        # the same objects as targets (self-interaction) stay the same buffers, which lets the library
        # pick the symmetric kernel
        xt = xs if xp is xw else _f64(xp)
        zt = zs if zp is zw else _f64(zp)
        if not (len(g) == len(xs) == len(zs)) or len(xt) != len(zt):
            raise ValueError("induce: source arrays (and target arrays) must have equal lengths")
        u, w = np.empty(len(xt)), np.empty(len(xt))
        self._check(self._lib.ludvm_induce_f64(self._ctx, _pd(xs), _pd(zs), _pd(g), len(xs), _pd(xt), _pd(zt), len(xt),
                                               float(v_core), _prec(precision), _pd(u), _pd(w)))
        return u, w

    def spatial_order(self, x, z, with_extent=False):
        """(order, reordered[, mean_class_extent]): the order the library evaluates unordered points in -- Morton order, or
        the identity when the given order is already compact or there are fewer than 2048 points (ludvm_spatial_order).
        Position k of an array stored in that order holds the caller's element order[k].  mean_class_extent: how compact
        the 128-point origin classes are in that order (0.0 below 2048 points); fp32 on local origins keeps its tier up
        to about 150 v_core for a reordered cloud, 300 v_core for a set that is compact as given."""
        xs, zs = _f64(x), _f64(z)
        if len(xs) != len(zs):
            raise ValueError("x and z must have the same length")
        order = np.empty(len(xs), np.uint32)
        flag, ext = c_int(0), c_double(0.0)
        self._check(self._lib.ludvm_spatial_order(self._ctx, _pd(xs), _pd(zs), len(xs),
                                                  order.ctypes.data_as(POINTER(ctypes.c_uint)), byref(flag), byref(ext)))
        return (order, bool(flag.value), float(ext.value)) if with_extent else (order, bool(flag.value))

    def induce_f32(self, circulation, xw, zw, xp, zp, v_core):
        g, xs, zs, xt, zt = _f32(circulation), _f32(xw), _f32(zw), _f32(xp), _f32(zp)
        u, w = np.empty(len(xt), np.float32), np.empty(len(xt), np.float32)
        self._check(self._lib.ludvm_induce_f32(self._ctx, _pf(xs), _pf(zs), _pf(g), len(xs), _pf(xt), _pf(zt), len(xt),
                                               float(v_core), _pf(u), _pf(w)))
        return u, w

    def induce_dev(self, d_xs, d_zs, d_gs, ns, d_xt, d_zt, nt, v_core, d_u, d_w):
        """Raw device pointers (ints), fp32 SoA; asynchronous on the context stream."""
        self._check(self._lib.ludvm_induce_dev_f32(self._ctx, d_xs, d_zs, d_gs, ns, d_xt, d_zt, nt, float(v_core),
                                                   d_u, d_w))

    def advect_dev(self, d_xs, d_zs, d_gs, ns, t_first, nt, v_core, dt, d_x_out, d_z_out):
        self._check(self._lib.ludvm_advect_dev_f32(self._ctx, d_xs, d_zs, d_gs, ns, t_first, nt, float(v_core),
                                                   float(dt), d_x_out, d_z_out))

    def sym_scale_dev(self, d_g, n, v_core, d_scale):
        """Fixed-point scale of the symmetric kernel's raw sums for circulations d_g[n] -> the 32-byte device record
        d_scale (the same bits on every GPU that holds the same circulations)."""
        self._check(self._lib.ludvm_sym_scale_dev_f32(self._ctx, d_g, n, float(v_core), d_scale))

    def sym_accumulate_dev(self, d_x, d_z, d_g, n, tile_first, tile_count, v_core, d_scale, d_acc_u, d_acc_w, d_bad):
        """This owner's share of the unordered pairs, ADDED as 64-bit fixed-point integers into d_acc_u / d_acc_w
        (int64[n], zeroed by the caller); d_bad (int64[1]) counts non-finite partial sums."""
        self._check(self._lib.ludvm_sym_accumulate_dev_f32(self._ctx, d_x, d_z, d_g, n, tile_first, tile_count,
                                                           float(v_core), d_scale, d_acc_u, d_acc_w, d_bad))

    def advect_from_sums_dev(self, d_sum_u, d_sum_w, d_scale, d_bad, d_x, d_z, t_first, nt, dt, d_x_out, d_z_out):
        self._check(self._lib.ludvm_advect_from_sums_dev_f32(self._ctx, d_sum_u, d_sum_w, d_scale, d_bad, d_x, d_z,
                                                             t_first, nt, float(dt), d_x_out, d_z_out))

    # -- resident wake ---------------------------------------------------------------------------
    def wake_reserve(self, capacity):
        self._check(self._lib.ludvm_wake_reserve(self._ctx, int(capacity)))

    def wake_clear(self):
        self._check(self._lib.ludvm_wake_clear(self._ctx))

    def wake_size(self):
        n = c_size_t()
        self._check(self._lib.ludvm_wake_size(self._ctx, byref(n)))
        return n.value

    def wake_truncate(self, n):
        self._check(self._lib.ludvm_wake_truncate(self._ctx, int(n)))

    def wake_append(self, x, z, gamma):
        x, z, g = _f64(x), _f64(z), _f64(gamma)
        if not (len(x) == len(z) == len(g)):
            raise ValueError("wake_append: x, z, gamma must have equal lengths")
        self._check(self._lib.ludvm_wake_append(self._ctx, _pd(x), _pd(z), _pd(g), len(x)))

    def wake_write(self, first, x=None, z=None, gamma=None):
        arrs = [None if a is None else _f64(a) for a in (x, z, gamma)]
        lens = {len(a) for a in arrs if a is not None}
        if len(lens) != 1:
            raise ValueError("wake_write: give at least one field; all given fields must have equal lengths")
        self._check(self._lib.ludvm_wake_write(self._ctx, int(first), lens.pop(), _pd(arrs[0]), _pd(arrs[1]),
                                               _pd(arrs[2])))

    def wake_read(self, first, count, gamma=False):
        x, z = np.empty(count), np.empty(count)
        g = np.empty(count) if gamma else None
        self._check(self._lib.ludvm_wake_read(self._ctx, int(first), int(count), _pd(x), _pd(z), _pd(g)))
        return (x, z, g) if gamma else (x, z)

    def wake_induce_on_points(self, src_first, src_count, xp, zp, v_core):
        xt, zt = _f64(xp), _f64(zp)
        u, w = np.empty(len(xt)), np.empty(len(xt))
        self._check(self._lib.ludvm_wake_induce_on_points(self._ctx, int(src_first), int(src_count), _pd(xt), _pd(zt),
                                                          len(xt), float(v_core), _pd(u), _pd(w)))
        return u, w

    def wake_chord_sums(self, src_first, src_count, xp, zp, unit_x, unit_z, v_core):
        """(u_wake, w_wake)[nt] from the resident wake and (u_unit, w_unit)[n_unit, nt] from unit
        vortices at (unit_x, unit_z), in one round trip (fp64)."""
        xt, zt, ux, uz = _f64(xp), _f64(zp), _f64(unit_x), _f64(unit_z)
        nt, nu = len(xt), len(ux)
        u, w = np.empty(nt), np.empty(nt)
        uu, wu = np.empty([nu, nt]), np.empty([nu, nt])
        self._check(self._lib.ludvm_wake_chord_sums(self._ctx, int(src_first), int(src_count), _pd(xt), _pd(zt), nt,
                                                    _pd(ux), _pd(uz), nu, float(v_core), _pd(u), _pd(w), _pd(uu), _pd(wu)))
        return u, w, uu, wu

    def step_buffers(self, npoints):
        """Preallocated host buffers (and their ctypes pointers) for the two per-step calls of a time
        loop with `npoints` chord points: removes the per-call array allocation and pointer casting."""
        b = type("StepBuffers", (), {})()
        b.n = npoints
        b.unit = np.zeros([2, 2])                       # [x|z][tev, lev]
        b.u, b.w = np.empty(npoints), np.empty(npoints)
        b.uu, b.wu = np.empty([2, npoints]), np.empty([2, npoints])
        b.tail = np.empty([2, 2])                       # [x|z][newest two]
        b.p_unit_x, b.p_unit_z = _pd(b.unit[0]), _pd(b.unit[1])
        b.p_u, b.p_w, b.p_uu, b.p_wu = _pd(b.u), _pd(b.w), _pd(b.uu), _pd(b.wu)
        b.p_tx, b.p_tz = _pd(b.tail[0]), _pd(b.tail[1])
        return b

    def wake_chord_sums_into(self, b, src_count, xp, zp, v_core):
        """wake_chord_sums over sources [0, src_count) with the unit vortices in b.unit, results in
        b.u, b.w, b.uu, b.wu.  xp, zp must be contiguous float64 arrays of length b.n."""
        self._check(self._lib.ludvm_wake_chord_sums(self._ctx, 0, src_count, _pd(xp), _pd(zp), b.n, b.p_unit_x, b.p_unit_z,
                                                    2, v_core, b.p_u, b.p_w, b.p_uu, b.p_wu))

    def wake_advect_tail_into(self, b, dt, foil_x, foil_z, foil_dgamma, v_core, tail_count, precision):
        """wake_advect_tail with contiguous float64 foil arrays; newest positions land in b.tail[:, :tail_count]."""
        self._check(self._lib.ludvm_wake_advect_tail(self._ctx, dt, _pd(foil_x), _pd(foil_z), _pd(foil_dgamma),
                                                     len(foil_x), v_core, precision, tail_count, b.p_tx, b.p_tz))

    def wake_step_into(self, b, new_x, new_z, new_gamma, dt, foil_x, foil_z, foil_dgamma, v_core, precision, te, le,
                       lev_from_prev, tail_count, xp_next, zp_next):
        """Append this step's shed vortices, roll the wake up, and return the placement and chord sums
        of the next step -- one packed upload and one download (ludvm_wake_step).  Results:
        b.tail[:, :tail_count], b.unit (placed TEV / LEV candidate), b.u, b.w, b.uu, b.wu for the next
        step.  All array arguments contiguous float64."""
        self._check(self._lib.ludvm_wake_step(self._ctx, _pd(new_x), _pd(new_z), _pd(new_gamma), len(new_x), dt,
                                              _pd(foil_x), _pd(foil_z), _pd(foil_dgamma), len(foil_x), v_core, precision,
                                              _pd(te), _pd(le), 1 if lev_from_prev else 0, tail_count, _pd(xp_next),
                                              _pd(zp_next), b.n, b.p_tx, b.p_tz, b.p_unit_x, b.p_unit_z, b.p_u, b.p_w,
                                              b.p_uu, b.p_wu))

    def wake_advect_tail(self, dt, foil_x, foil_z, foil_dgamma, v_core, tail_count, precision="f32"):
        """Roll-up step, then the updated (x, z) of the last `tail_count` wake vortices."""
        fx, fz, fg = _f64(foil_x), _f64(foil_z), _f64(foil_dgamma)
        tx, tz = np.empty(tail_count), np.empty(tail_count)
        self._check(self._lib.ludvm_wake_advect_tail(self._ctx, float(dt), _pd(fx), _pd(fz), _pd(fg), len(fx),
                                                     float(v_core), _prec(precision), int(tail_count), _pd(tx), _pd(tz)))
        return tx, tz

    def wake_advect(self, dt, foil_x, foil_z, foil_dgamma, v_core, precision="f32", return_velocity=False):
        fx, fz, fg = _f64(foil_x), _f64(foil_z), _f64(foil_dgamma)
        u = w = None
        if return_velocity:
            n = self.wake_size()
            u, w = np.empty(n), np.empty(n)
        self._check(self._lib.ludvm_wake_advect(self._ctx, float(dt), _pd(fx), _pd(fz), _pd(fg), len(fx),
                                                float(v_core), _prec(precision), _pd(u), _pd(w)))
        return (u, w) if return_velocity else None

    # -- device-resident time march ----------------------------------------------------------------
    MARCH_ROW_HEAD = 12
    MARCH_STATE_HEAD = 16

    def march_setup(self, npan, ncoef, scalars, tables, kin):
        """Upload what a run keeps constant (ludvm_march_setup): scalars [Uinf, chord, rho, dt, piv, v_core, IC,
        sum(Gamma_free), method (0 Faure / 1 Ramesh), maxerror, maxiter, epsilon], the packed chord tables and the
        per-step kinematics rows [nt, 7 + 2 npan]."""
        sc, tb = _f64(scalars), _f64(tables)
        kin = np.ascontiguousarray(kin, dtype=np.float64)
        if kin.ndim != 2 or kin.shape[1] != 7 + 2 * npan or len(sc) != 12:
            raise ValueError("march_setup: kin must be [nt, 7 + 2 npan] and scalars 12 long")
        if len(tb) != 8 * npan + ncoef * npan + (ncoef - 1) * npan:
            raise ValueError("march_setup: wrong table length")
        self._check(self._lib.ludvm_march_setup(self._ctx, int(npan), int(ncoef), _pd(sc), _pd(tb), _pd(kin), kin.shape[0]))
        self._march_dims = (int(npan), int(ncoef))
        self._march_nprobes = 0          # (ludvm_march_setup forgets any probes)
        self._march_ntracers = 0         # (... and any tracers)
        self._march_nsurvey = 0          # (... and any survey)
        self._march_nbins = 0            # (... and its bins)

    def march_run(self, first_step, count, precision, state, hist_nmax=0, anchors=None):
        """Advance the resident wake through time steps [first_step, first_step + count) without a host round
        trip per step (ludvm_march_run).  `state` (16 + ncoef float64) is updated in place; returns the
        per-step rows [count, 12 + 2 ncoef + 2 npan] -- and, with hist_nmax > 0, the positions of every wake
        vortex after each step, [count, 2, hist_nmax] (the reference's dense history).  `anchors`: the wake sizes after
        the four anchor steps `march_anchor_steps(first_step)` (-1 = not given; None = none), which make the launch
        geometry -- and with it the fp32 rounding -- independent of where the calls begin."""
        npan, ncoef = self._march_dims
        if state.dtype != np.float64 or not state.flags.c_contiguous or len(state) != self.MARCH_STATE_HEAD + ncoef:
            raise ValueError("march_run: state must be contiguous float64 of length 16 + ncoef")
        rows = np.empty([int(count), self.MARCH_ROW_HEAD + 2 * ncoef + 2 * npan])
        hist = np.empty([int(count), 2, int(hist_nmax)]) if hist_nmax else None
        anc = None
        if anchors is not None:
            anc = (ctypes.c_longlong * 4)(*[int(v) for v in anchors])
        self._march_last = (int(first_step), int(count))
        self._check(self._lib.ludvm_march_run(self._ctx, int(first_step), int(count), _prec(precision), _pd(state), _pd(rows),
                                              _pd(hist), int(hist_nmax), anc))
        return (rows, hist) if hist_nmax else rows

    def march_set_probes(self, x, z, shift_x=None):
        """Points at which every marched step also evaluates the field that convects the wake (ludvm_march_set_probes);
        valid after `march_setup`, which forgets them.  shift_x: None, or one x offset per kinematics row -- in step i probe
        k sits at (x[k] + shift_x[i], z[k]).  Empty x removes the probes."""
        xs, zs = _f64(x), _f64(z)
        if len(xs) != len(zs):
            raise ValueError("march_set_probes: x and z must have the same length")
        sh = None if shift_x is None else _f64(shift_x)
        self._check(self._lib.ludvm_march_set_probes(self._ctx, _pd(xs), _pd(zs), len(xs), _pd(sh), 0 if sh is None else len(sh)))
        self._march_nprobes = len(xs)

    def march_probes(self, count):
        """(u, w), float64 [count, P]: the probe rows of the last `march_run` call, which ran `count` steps
        (ludvm_march_read_probes)."""
        u, w = np.empty([int(count), self._march_nprobes]), np.empty([int(count), self._march_nprobes])
        self._check(self._lib.ludvm_march_read_probes(self._ctx, _pd(u), _pd(w), int(count)))
        return u, w

    INTEGRAL_SUMS = 48

    def march_set_integrals(self, on, tags=(), energy_steps=None):
        """Wake integrals of every marched step (ludvm_march_set_integrals); valid after `march_setup`, which forgets them.
        tags: the class -- 0 FREE, 1 TEV, 2 LEV -- of every vortex of the resident wake, in its stored order (the library tags
        what later steps shed).  energy_steps: None (no energy samples) or (first, stop, every).  on = False turns the
        observer off."""
        if not hasattr(self._lib, "ludvm_march_set_integrals"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_integrals")
        raw = np.asarray(tags).reshape(-1)
        if len(raw) and (not np.issubdtype(raw.dtype, np.integer) or raw.min() < 0 or raw.max() > 255):
            raise ValueError("march_set_integrals: tags must be integers 0 .. 2")
        t = np.ascontiguousarray(raw, dtype=np.uint8)
        first, stop, every = (0, 0, 0) if energy_steps is None else (int(v) for v in energy_steps)
        self._check(self._lib.ludvm_march_set_integrals(self._ctx, 1 if on else 0, t.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                                        len(t), first, stop, every))

    def march_integrals(self, count):
        """(sums float64 [count, 4, 2, 6], energy float64 [count], NaN outside the window): the integral rows of the last
        `march_run` call, which ran `count` steps (ludvm_march_read_integrals)."""
        sums, energy = np.empty([int(count), 4, 2, 6]), np.empty(int(count))
        self._check(self._lib.ludvm_march_read_integrals(self._ctx, _pd(sums), _pd(energy), int(count)))
        return sums, energy

    def march_set_tracers(self, seed_x, seed_z, release=None, shift_x=None, cur=None, record_steps=()):
        """Passive tracers advected by every marched step (ludvm_march_set_tracers); valid after `march_setup`, which forgets
        them.  release: None (all released at step 1), or one step >= 1 per tracer -- before it a tracer is held at its
        seed.  shift_x: None, or one x offset per kinematics row (the seed of step i is (x + shift_x[i], z)).  cur: None
        (start from the seeds), or the current positions [2, M] of a run that is continued.  record_steps: the time steps,
        ascending, whose positions `march_run` keeps for `march_tracers`.  Empty seeds remove the tracers."""
        if not hasattr(self._lib, "ludvm_march_set_tracers"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_tracers")
        xs, zs = _f64(seed_x), _f64(seed_z)
        if len(xs) != len(zs):
            raise ValueError("march_set_tracers: seed_x and seed_z must have the same length")
        rel = None if release is None else np.ascontiguousarray(release, dtype=np.int64).reshape(-1)
        if rel is not None and len(rel) != len(xs):
            raise ValueError("march_set_tracers: one release step per tracer")
        sh = None if shift_x is None else _f64(shift_x)
        cx = cz = None
        if cur is not None:
            cur = np.asarray(cur, dtype=np.float64)
            if cur.shape != (2, len(xs)):
                raise ValueError("march_set_tracers: cur must be [2, M]")
            cx, cz = _f64(cur[0]), _f64(cur[1])
        rec = np.ascontiguousarray(list(record_steps), dtype=np.int64).reshape(-1)
        pl = POINTER(c_longlong)
        self._check(self._lib.ludvm_march_set_tracers(
            self._ctx, _pd(xs), _pd(zs), None if rel is None else rel.ctypes.data_as(pl), len(xs), _pd(sh),
            0 if sh is None else len(sh), _pd(cx), _pd(cz), rec.ctypes.data_as(pl) if len(rec) else None, len(rec)))
        self._march_ntracers = len(xs)
        self._march_tracer_record = rec

    def march_tracers(self):
        """(steps int64 [R], xz float64 [R, 2, M]): the tracer rows the last `march_run` call recorded, with their time steps
        (ludvm_march_read_tracers)."""
        first, count = self._march_last
        rec = self._march_tracer_record
        M, cap = self._march_ntracers, int(np.count_nonzero((rec >= first) & (rec < first + count)))
        x, z = np.empty([cap, M]), np.empty([cap, M])
        steps, n = np.zeros(max(cap, 1), dtype=np.int64), c_size_t(0)
        self._check(self._lib.ludvm_march_read_tracers(self._ctx, _pd(x), _pd(z), cap, steps.ctypes.data_as(POINTER(c_longlong)),
                                                       byref(n)))
        r = int(n.value)
        return steps[:r].copy(), np.stack([x[:r], z[:r]], axis=1)

    def march_tracer_state(self):
        """float64 [2, M]: the tracers' current positions (ludvm_march_tracer_state)."""
        xz = np.empty([2, self._march_ntracers])
        self._check(self._lib.ludvm_march_tracer_state(self._ctx, _pd(xz[0]), _pd(xz[1])))
        return xz

    def march_set_survey(self, x, z, shift_x=None, steps=(1, None, 1), sums=None, samples=0):
        """Wake-survey statistics accumulated by the marched steps (ludvm_march_set_survey); valid after `march_setup`, which
        forgets them.  In every step i of the window steps = (first, stop, every) -- first <= i < stop, (i - first) % every
        == 0; stop None: to the end of the kinematics table -- the probes' field at the points (x + shift_x[i], z) is added to
        five raw float64 sums per point (u, w, u^2, w^2, u w) on the device.  sums [5, K] and samples continue a run (what
        `march_survey` returned).  Empty points remove the survey."""
        if not hasattr(self._lib, "ludvm_march_set_survey"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_survey")
        xs, zs = _f64(x), _f64(z)
        if len(xs) != len(zs):
            raise ValueError("march_set_survey: x and z must have the same length")
        sh = None if shift_x is None else _f64(shift_x)
        first, stop, every = steps
        stop = (1 << 62) if stop is None else int(stop)
        sm = None
        if sums is not None:
            sm = np.ascontiguousarray(sums, dtype=np.float64)
            if sm.shape != (5, len(xs)):
                raise ValueError("march_set_survey: sums must be [5, K]")
        self._check(self._lib.ludvm_march_set_survey(self._ctx, _pd(xs), _pd(zs), len(xs), _pd(sh), 0 if sh is None else len(sh),
                                                     int(first), stop, int(every), _pd(sm), int(samples)))
        self._march_nsurvey = len(xs)
        self._march_nbins = 0            # (ludvm_march_set_survey forgets any bins)

    def march_set_survey_bins(self, table, nbins, sums=None, counts=None):
        """Bins of the survey (ludvm_march_set_survey_bins); valid while a survey is set.  table: one bin per kinematics row,
        -1 .. nbins - 1 -- a sampled step i with table[i] = b >= 0 also adds its five terms to bin b's own sums and one to
        bin b's count.  sums [nbins, 5, K] and counts [nbins] continue a run (what `march_survey_bins` returned), both or
        neither.  nbins = 0 removes the bins."""
        if not hasattr(self._lib, "ludvm_march_set_survey_bins"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_survey_bins")
        tb = np.ascontiguousarray(table, dtype=np.intc).reshape(-1)
        nbins = int(nbins)
        sm = cn = None
        if sums is not None:
            sm = np.ascontiguousarray(sums, dtype=np.float64)
            if sm.shape != (nbins, 5, getattr(self, "_march_nsurvey", 0)):
                raise ValueError("march_set_survey_bins: sums must be [nbins, 5, K]")
        if counts is not None:
            cn = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
            if len(cn) != nbins:
                raise ValueError("march_set_survey_bins: counts must be [nbins]")
        self._check(self._lib.ludvm_march_set_survey_bins(
            self._ctx, tb.ctypes.data_as(POINTER(ctypes.c_int)) if len(tb) else None, len(tb), nbins, _pd(sm),
            None if cn is None else cn.ctypes.data_as(POINTER(c_longlong))))
        self._march_nbins = nbins

    def march_survey_bins(self):
        """(sums float64 [B, 5, K], counts int64 [B]): the raw sums of every bin of the survey and the sampled steps each holds
        (ludvm_march_read_survey_bins)."""
        if not hasattr(self._lib, "ludvm_march_read_survey_bins"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_read_survey_bins")
        B = getattr(self, "_march_nbins", 0)
        sums, counts = np.empty([B, 5, getattr(self, "_march_nsurvey", 0)]), np.zeros(max(B, 1), dtype=np.int64)
        self._check(self._lib.ludvm_march_read_survey_bins(self._ctx, _pd(sums), counts.ctypes.data_as(POINTER(c_longlong))))
        return sums, counts[:B].copy()

    def march_set_tracer_precision(self, precision):
        """How the marched steps evaluate the field at the released tracers (ludvm_march_set_tracer_precision): 'f64' (what
        `march_set_tracers` leaves) or 'f32x2' -- fp32 pair arithmetic on hi+lo positions, float64 tile sums, splits, Euler update
        and positions -- or the library's own code (0 / 2; anything else is the library's LUDVM_E_ARG).  Valid while tracers
        are set."""
        if not hasattr(self._lib, "ludvm_march_set_tracer_precision"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_tracer_precision")
        code = _ffi.TRACER_PRECISIONS.get(precision, precision) if isinstance(precision, str) else precision
        if isinstance(code, bool) or not isinstance(code, int):
            raise ValueError("march_set_tracer_precision: 'f64' or 'f32x2' (or the library's code)")
        self._check(self._lib.ludvm_march_set_tracer_precision(self._ctx, code))

    def march_set_tracer_gradient(self, on=True, F=None):
        """Carry the tracers' deformation gradient through the marched steps (ludvm_march_set_tracer_gradient): F <- (I + dt
        grad(u, w)) F per step of a released tracer, the identity while it is held and at its release.  F: None (the identity),
        or [4, M] (F11, F12, F21, F22) of a run that is continued.  Valid while float64 tracers are set."""
        if not hasattr(self._lib, "ludvm_march_set_tracer_gradient"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_tracer_gradient")
        code = int(on) if isinstance(on, (bool, int, np.integer)) else None
        if code is None:
            raise ValueError("march_set_tracer_gradient: on is a flag (or the library's code)")
        f = None
        if F is not None:
            f = np.ascontiguousarray(F, dtype=np.float64)
            if f.shape != (4, getattr(self, "_march_ntracers", 0)):
                raise ValueError("march_set_tracer_gradient: F must be [4, M]")
        self._check(self._lib.ludvm_march_set_tracer_gradient(self._ctx, code, _pd(f)))

    def march_set_tracer_gradient_f32x2(self, F=None):
        """The tracers' deformation gradient in hi+lo fp32 (ludvm_march_set_tracer_gradient_f32x2): sets the tracers' precision
        to 'f32x2' and switches the gradient on -- u, w and the gradient's sums from one fp32 walk over the sources, the Euler
        update and F <- (I + dt grad(u, w)) F in float64.  F as `march_set_tracer_gradient`'s.  Valid while tracers are set;
        `march_set_tracer_gradient(False)` leaves plain 'f32x2' tracers."""
        if not hasattr(self._lib, "ludvm_march_set_tracer_gradient_f32x2"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_tracer_gradient_f32x2")
        f = None
        if F is not None:
            f = np.ascontiguousarray(F, dtype=np.float64)
            if f.shape != (4, getattr(self, "_march_ntracers", 0)):
                raise ValueError("march_set_tracer_gradient_f32x2: F must be [4, M]")
        self._check(self._lib.ludvm_march_set_tracer_gradient_f32x2(self._ctx, _pd(f)))

    def march_tracer_gradient(self):
        """(steps int64 [R], F float64 [R, 4, M]): the deformation-gradient rows the last `march_run` call recorded, the steps of
        `march_tracers` (ludvm_march_read_tracer_gradient)."""
        first, count = self._march_last
        rec = self._march_tracer_record
        M, cap = self._march_ntracers, int(np.count_nonzero((rec >= first) & (rec < first + count)))
        F = np.empty([cap, 4, M])
        steps, n = np.zeros(max(cap, 1), dtype=np.int64), c_size_t(0)
        self._check(self._lib.ludvm_march_read_tracer_gradient(self._ctx, _pd(F), cap, steps.ctypes.data_as(POINTER(c_longlong)),
                                                               byref(n)))
        r = int(n.value)
        return steps[:r].copy(), F[:r].copy()

    def march_tracer_gradient_state(self):
        """float64 [4, M]: the tracers' current deformation gradient (ludvm_march_tracer_gradient_state)."""
        F = np.empty([4, self._march_ntracers])
        self._check(self._lib.ludvm_march_tracer_gradient_state(self._ctx, _pd(F)))
        return F

    def march_set_survey_precision(self, precision):
        """How the marched steps evaluate the survey's field (ludvm_march_set_survey_precision): 'f64' (what `march_set_survey`
        leaves) or 'f32' -- fp32 pair arithmetic on local origins, float64 class sums, splits and moments -- or the library's
        own code (0 / 1; anything else is the library's LUDVM_E_ARG).  Valid while a survey is set."""
        if not hasattr(self._lib, "ludvm_march_set_survey_precision"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_survey_precision")
        code = _ffi.SURVEY_PRECISIONS.get(precision, precision) if isinstance(precision, str) else precision
        if isinstance(code, bool) or not isinstance(code, int):
            raise ValueError("march_set_survey_precision: 'f64' or 'f32' (or the library's code)")
        self._check(self._lib.ludvm_march_set_survey_precision(self._ctx, code))

    def march_survey(self):
        """(sums float64 [5, K], samples): the survey's raw sums -- u, w, u^2, w^2, u w per point -- and the number of sampled
        steps they hold (ludvm_march_read_survey)."""
        if not hasattr(self._lib, "ludvm_march_read_survey"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_read_survey")
        sums, n = np.empty([5, getattr(self, "_march_nsurvey", 0)]), c_longlong(0)
        self._check(self._lib.ludvm_march_read_survey(self._ctx, _pd(sums), byref(n)))
        return sums, int(n.value)

    def march_set_survey_gradient(self, on=True, gsums=None, bin_gsums=None):
        """Gradient sums of the survey (ludvm_march_set_survey_gradient): every sampled step also adds ux, e = (uz + wx) / 2,
        omega, omega^2 and Q = omega^2 / 4 - ux^2 - e^2 of the closed-form gradient at the survey points to five more raw
        float64 sums per point -- and, with bins, to the step's bin block.  gsums [5, K] and bin_gsums [nbins, 5, K] continue a
        run (what `march_survey_gradient` returned); None starts from zero.  Valid while a float64 survey is set, after
        `march_set_survey` and `march_set_survey_bins`, which forget it."""
        if not hasattr(self._lib, "ludvm_march_set_survey_gradient"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_survey_gradient")
        code = int(on) if isinstance(on, (bool, int, np.integer)) else None
        if code is None:
            raise ValueError("march_set_survey_gradient: on is a flag (or the library's code)")
        K, B = getattr(self, "_march_nsurvey", 0), getattr(self, "_march_nbins", 0)
        g = bg = None
        if gsums is not None:
            g = np.ascontiguousarray(gsums, dtype=np.float64)
            if g.shape != (5, K):
                raise ValueError("march_set_survey_gradient: gsums must be [5, K]")
        if bin_gsums is not None:
            bg = np.ascontiguousarray(bin_gsums, dtype=np.float64)
            if bg.ndim != 3 or bg.shape[1:] != (5, K) or (B and bg.shape[0] != B):
                raise ValueError("march_set_survey_gradient: bin_gsums must be [nbins, 5, K]")
        self._check(self._lib.ludvm_march_set_survey_gradient(self._ctx, code, _pd(g), _pd(bg)))

    def march_set_survey_gradient_f32x2(self, gsums=None, bin_gsums=None):
        """Gradient sums of the survey in hi+lo fp32 (ludvm_march_set_survey_gradient_f32x2): the ten sums of
        `march_set_survey_gradient`, with u, w and the gradient's raw sums of every sampled step from ONE fp32 walk over the
        sources on hi+lo positions; the tile sums, the splits and all ten sums stay float64.  The velocity sums of such a
        survey are that walk's too (hi+lo tier, not the float64 survey's bits).  gsums and bin_gsums as
        `march_set_survey_gradient`'s; valid while a float64 survey is set, after `march_set_survey` and
        `march_set_survey_bins`, which forget it.  `march_set_survey_gradient(False)` removes the sums and the route."""
        if not hasattr(self._lib, "ludvm_march_set_survey_gradient_f32x2"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_set_survey_gradient_f32x2")
        K, B = getattr(self, "_march_nsurvey", 0), getattr(self, "_march_nbins", 0)
        g = bg = None
        if gsums is not None:
            g = np.ascontiguousarray(gsums, dtype=np.float64)
            if g.shape != (5, K):
                raise ValueError("march_set_survey_gradient_f32x2: gsums must be [5, K]")
        if bin_gsums is not None:
            bg = np.ascontiguousarray(bin_gsums, dtype=np.float64)
            if bg.ndim != 3 or bg.shape[1:] != (5, K) or (B and bg.shape[0] != B):
                raise ValueError("march_set_survey_gradient_f32x2: bin_gsums must be [nbins, 5, K]")
        self._check(self._lib.ludvm_march_set_survey_gradient_f32x2(self._ctx, _pd(g), _pd(bg)))

    def march_survey_gradient(self):
        """(gsums float64 [5, K], bin_gsums float64 [B, 5, K] or None without bins): the survey's gradient sums -- ux, e, omega,
        omega^2, Q per point -- as they stand (ludvm_march_read_survey_gradient); their counts are `march_survey`'s and
        `march_survey_bins`'s."""
        if not hasattr(self._lib, "ludvm_march_read_survey_gradient"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_march_read_survey_gradient")
        K, B = getattr(self, "_march_nsurvey", 0), getattr(self, "_march_nbins", 0)
        g = np.empty([5, K])
        bg = np.empty([B, 5, K]) if B else None
        self._check(self._lib.ludvm_march_read_survey_gradient(self._ctx, _pd(g), _pd(bg)))
        return g, bg

    @staticmethod
    def march_anchor_steps(first_step):
        """The four steps whose wake sizes ludvm_march_run wants in `anchors` for a call that begins at first_step."""
        return [max(64 * (int(first_step) // 64 - 3 + q) - 1, 0) for q in range(4)]

    # -- ensemble of small simulations ---------------------------------------------------------------
    def ensemble_limits(self):
        """(max steps, max wake capacity, max snapshot steps) of a member of `ensemble_run`."""
        lim = (c_longlong * 3)()
        self._check(self._lib.ludvm_ensemble_limits(self._ctx, lim))
        return int(lim[0]), int(lim[1]), int(lim[2])

    def ensemble_run(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=()):
        """Many whole time loops in ONE device launch, a workgroup per member (ludvm_ensemble_run; the packed layouts are
        documented in include/ludvm_hip.h).  scalars [members, 12]; tables [members, T]; kin [rows, 7 + 2 npan]; init
        [members, 8 + ncoef]; free_xzg: 3 * (free vortices of all members) doubles; desc [members, 6] int64 = nt, kin_off,
        nfree, free_off, row_off, wake_off; snap_steps: increasing steps >= 1.
        -> (rows [sum(nt - 1), 12 + 2 ncoef + 2 npan], wakes (float64, flat), wake_n [members, len(snap_steps) + 1])."""
        return self._ensemble(npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, None)

    def ensemble_run_probed(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, probe_x, probe_z,
                            shift_x=None):
        """`ensemble_run` with velocity probes evaluated inside the launch (ludvm_ensemble_run_probed): probe_x, probe_z [P]
        are common to the batch; shift_x: None, or one x offset per row of `kin` -- in step i of a member probe k sits at
        (probe_x[k] + shift_x[kin_off + i], probe_z[k]).
        -> (rows, wakes, wake_n, probe_u, probe_w) with probe_u / probe_w [rows of kin, P]: a member's time level i is row
        kin_off + i (row 0: the field of its free vortices)."""
        px, pz = _f64(probe_x), _f64(probe_z)
        if len(px) != len(pz):
            raise ValueError("ensemble_run_probed: probe_x and probe_z must have the same length")
        sh = None if shift_x is None else _f64(shift_x)
        return self._ensemble(npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, (px, pz, sh))

    def ensemble_run_traced(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, seed_x, seed_z,
                            release, shift_x=None, record_steps=(), probe_x=None, probe_z=None, probe_shift_x=None):
        """`ensemble_run` with passive tracers advected inside the launch (ludvm_ensemble_run_traced): seed_x, seed_z [M] and
        release [M] (steps >= 1) are common to the batch; shift_x: None, or one x offset per row of `kin` -- in step i of a
        member the seed of tracer k sits at (seed_x[k] + shift_x[kin_off + i], seed_z[k]); record_steps: strictly increasing
        steps >= 1 whose positions are kept.  probe_x, probe_z (and probe_shift_x): the probes of `ensemble_run_probed`, in the
        same launch.
        -> (rows, wakes, wake_n, tracer_rows), plus (probe_u, probe_w) when probes are given; tracer_rows
        [members, len(record_steps) + 1, 2, M]: the positions after each recorded step and, last, after the member's final
        step (a recorded step the member does not have: zeros)."""
        if not hasattr(self._lib, "ludvm_ensemble_run_traced"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_ensemble_run_traced")
        sx, sz = _f64(seed_x), _f64(seed_z)
        rel = np.ascontiguousarray(release, dtype=np.int64).reshape(-1)
        if len(sx) != len(sz) or len(rel) != len(sx):
            raise ValueError("ensemble_run_traced: seed_x, seed_z and release must have the same length")
        sh = None if shift_x is None else _f64(shift_x)
        rec = np.ascontiguousarray(list(record_steps), dtype=np.int64).reshape(-1)
        probes = None
        if probe_x is not None or probe_z is not None:
            px, pz = _f64(probe_x), _f64(probe_z)
            if len(px) != len(pz):
                raise ValueError("ensemble_run_traced: probe_x and probe_z must have the same length")
            probes = (px, pz, None if probe_shift_x is None else _f64(probe_shift_x))
        return self._ensemble(npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, probes, (sx, sz, rel, sh, rec))

    def ensemble_run_surveyed(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, survey_x, survey_z,
                              survey_steps, survey_shift_x=None, seed_x=(), seed_z=(), release=(), shift_x=None, record_steps=(),
                              probe_x=None, probe_z=None, probe_shift_x=None):
        """`ensemble_run_traced` (tracers and probes optional) with a wake survey accumulated inside the launch
        (ludvm_ensemble_run_surveyed): survey_x, survey_z [K] and survey_steps = (first, stop, every) are common to the batch;
        survey_shift_x: None, or one x offset per row of `kin` -- in a sampled step i of a member (first <= i < min(stop, nt),
        (i - first) % every == 0) point k sits at (survey_x[k] + survey_shift_x[kin_off + i], survey_z[k]).
        -> `ensemble_run_traced`'s tuple with survey_sums [members, 5, K] appended: sum u, sum w, sum u^2, sum w^2, sum u w of
        each member over its sampled steps (counting them is the caller's)."""
        return self._ensemble_surveyed("ensemble_run_surveyed", None, npan, ncoef, scalars, tables, kin, init, free_xzg, desc,
                                       snap_steps, survey_x, survey_z, survey_steps, survey_shift_x, seed_x, seed_z, release, shift_x,
                                       record_steps, probe_x, probe_z, probe_shift_x)

    def ensemble_run_surveyed_binned(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, survey_x,
                                     survey_z, survey_steps, bin_of_step, nbins, survey_shift_x=None, seed_x=(), seed_z=(),
                                     release=(), shift_x=None, record_steps=(), probe_x=None, probe_z=None, probe_shift_x=None):
        """`ensemble_run_surveyed` (tracers and probes optional) with the survey's bins accumulated inside the launch
        (ludvm_ensemble_run_surveyed_binned): bin_of_step holds one integer per row of `kin` -- the bin 0 .. nbins - 1 of step i
        of a member at [kin_off + i], -1 for none (entries of steps the window does not sample are not used); 1 <= nbins <= 64.
        -> `ensemble_run_surveyed`'s tuple with bin_sums [members, nbins, 5, K] appended: block b of a member holds its five raw
        sums over its sampled steps of bin b (counting them is the caller's)."""
        if int(nbins) < 1:
            raise ValueError("ensemble_run_surveyed_binned: nbins >= 1 (without bins: ensemble_run_surveyed)")
        table = np.ascontiguousarray(bin_of_step, dtype=np.intc).reshape(-1)
        return self._ensemble_surveyed("ensemble_run_surveyed_binned", (table, int(nbins)), npan, ncoef, scalars, tables, kin, init,
                                       free_xzg, desc, snap_steps, survey_x, survey_z, survey_steps, survey_shift_x, seed_x, seed_z,
                                       release, shift_x, record_steps, probe_x, probe_z, probe_shift_x)

    def ensemble_run_surveyed_graded(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, survey_x,
                                     survey_z, survey_steps, bin_of_step=None, nbins=0, survey_shift_x=None, seed_x=(), seed_z=(),
                                     release=(), shift_x=None, record_steps=(), probe_x=None, probe_z=None, probe_shift_x=None):
        """`ensemble_run_surveyed_binned` (bins, tracers and probes optional) with the survey's gradient sums accumulated inside
        the launch (ludvm_ensemble_run_surveyed_graded): in every sampled step the closed-form gradient of the survey's field at
        the survey's shifted points adds ux, e, om, om^2 and Q = om^2 / 4 - ux^2 - e^2 to five more raw float64 sums per point,
        and in a step with a bin to the bin's block.  nbins = 0 (bin_of_step is not looked at): no bins.
        -> `ensemble_run_surveyed_binned`'s tuple (bin_sums None without bins) with grad_sums [members, 5, K] and bin_grad_sums
        [members, nbins, 5, K] (None without bins) appended."""
        nbins = int(nbins)
        if nbins < 0:
            raise ValueError("ensemble_run_surveyed_graded: nbins >= 0")
        table = np.ascontiguousarray(bin_of_step, dtype=np.intc).reshape(-1) if nbins else np.empty(0, dtype=np.intc)
        return self._ensemble_surveyed("ensemble_run_surveyed_graded", (table, nbins), npan, ncoef, scalars, tables, kin, init,
                                       free_xzg, desc, snap_steps, survey_x, survey_z, survey_steps, survey_shift_x, seed_x, seed_z,
                                       release, shift_x, record_steps, probe_x, probe_z, probe_shift_x, grad=True)

    def ensemble_run_integrals(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps=(), *, energy_steps=None,
                               survey_x=(), survey_z=(), survey_steps=(1, 0, 1), bin_of_step=None, nbins=0, grad=False,
                               survey_shift_x=None, seed_x=(), seed_z=(), release=(), shift_x=None, record_steps=(), probe_x=None,
                               probe_z=None, probe_shift_x=None):
        """`ensemble_run_surveyed_graded` (survey, bins, gradient sums -- grad=True --, tracers and probes all optional) with the
        wake integrals of every member accumulated inside the launch (ludvm_ensemble_run_integrals): in every step of a member the
        count, sum G, sum G x, sum G z, sum G (x^2 + z^2), sum G^2 of its sources by class (FREE, TEV, LEV, BOUND) and sign, and --
        energy_steps = (first, stop, every), None: no samples -- at the sampled steps W = 1/2 sum G_a psi(x_a) over them.
        -> `ensemble_run_surveyed_graded`'s tuple (survey_sums None without a survey, grad_sums None without grad) with
        integral_sums [rows of kin, 4, 2, 6] and energy [rows of kin] (None without energy_steps; NaN where not sampled) appended: a
        member's time level i is row kin_off + i (row 0 is the caller's: zeros)."""
        nbins = int(nbins)
        if nbins < 0:
            raise ValueError("ensemble_run_integrals: nbins >= 0")
        table = np.ascontiguousarray(bin_of_step, dtype=np.intc).reshape(-1) if nbins else np.empty(0, dtype=np.intc)
        win = None if energy_steps is None else tuple(int(v) for v in energy_steps)
        if win is not None and len(win) != 3:
            raise ValueError("ensemble_run_integrals: energy_steps = (first, stop, every)")
        return self._ensemble_surveyed("ensemble_run_integrals", (table, nbins), npan, ncoef, scalars, tables, kin, init, free_xzg, desc,
                                       snap_steps, survey_x, survey_z, survey_steps, survey_shift_x, seed_x, seed_z, release, shift_x,
                                       record_steps, probe_x, probe_z, probe_shift_x, grad=bool(grad), integrals=(win,))

    def _ensemble_surveyed(self, who, bins, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, survey_x, survey_z,
                           survey_steps, survey_shift_x, seed_x, seed_z, release, shift_x, record_steps, probe_x, probe_z,
                           probe_shift_x, grad=False, integrals=None):
        if not hasattr(self._lib, "ludvm_" + who):
            raise LudvmHipError(_ffi.E_STATE, f"this build of the library has no ludvm_{who}")
        vx, vz = _f64(survey_x), _f64(survey_z)
        if len(vx) != len(vz):
            raise ValueError(f"{who}: survey_x and survey_z must have the same length")
        first, stop, every = (int(v) for v in survey_steps)
        vsh = None if survey_shift_x is None else _f64(survey_shift_x)
        sx, sz = _f64(seed_x), _f64(seed_z)
        rel = np.ascontiguousarray(release, dtype=np.int64).reshape(-1)
        if len(sx) != len(sz) or len(rel) != len(sx):
            raise ValueError(f"{who}: seed_x, seed_z and release must have the same length")
        sh = None if shift_x is None else _f64(shift_x)
        rec = np.ascontiguousarray(list(record_steps), dtype=np.int64).reshape(-1)
        probes = None
        if probe_x is not None or probe_z is not None:
            px, pz = _f64(probe_x), _f64(probe_z)
            if len(px) != len(pz):
                raise ValueError(f"{who}: probe_x and probe_z must have the same length")
            probes = (px, pz, None if probe_shift_x is None else _f64(probe_shift_x))
        return self._ensemble(npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, probes, (sx, sz, rel, sh, rec),
                              (vx, vz, vsh, first, stop, every), bins, grad, integrals)

    def _ensemble(self, npan, ncoef, scalars, tables, kin, init, free_xzg, desc, snap_steps, probes, tracers=None, survey=None,
                  bins=None, grad=False, integrals=None):
        npan, ncoef = int(npan), int(ncoef)
        desc = np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, _ffi.ENSEMBLE_DESC)
        members = desc.shape[0]
        sc, tb, ini, fr = _f64(scalars), _f64(tables), _f64(init), _f64(free_xzg)
        kin = np.ascontiguousarray(kin, dtype=np.float64).reshape(-1, 7 + 2 * npan)
        snaps = np.ascontiguousarray(list(snap_steps), dtype=np.int64).reshape(-1)
        if members and (len(tb) != members * (8 * npan + ncoef * npan + (ncoef - 1) * npan)
                        or len(ini) != members * (_ffi.ENSEMBLE_INIT_HEAD + ncoef) or len(fr) % 3):
            raise ValueError("ensemble_run: wrong table / init / free-vortex array length")
        nrec = len(snaps) + 1
        rows_count = int(max((desc[:, 4] + desc[:, 0] - 1).max(), 0)) if members else 0
        cap = desc[:, 2] + 2 * (desc[:, 0] - 1)
        wake_doubles = int(max((desc[:, 5] + nrec * 3 * cap).max(), 0)) if members else 0
        rows = np.empty([rows_count, self.MARCH_ROW_HEAD + 2 * ncoef + 2 * npan])
        wakes = np.empty(wake_doubles)
        wake_n = np.empty([members, nrec], dtype=np.int64)
        pll = POINTER(c_longlong)
        args = (self._ctx, members, npan, ncoef, _pd(sc), len(sc), _pd(tb), _pd(kin), kin.shape[0], _pd(ini), _pd(fr), len(fr) // 3,
                desc.ctypes.data_as(pll), snaps.ctypes.data_as(pll), len(snaps), _pd(rows), rows_count, _pd(wakes), wake_doubles,
                wake_n.ctypes.data_as(pll))
        if tracers is not None:
            sx, sz, rel, tsh, rec = tracers
            px, pz, sh = probes if probes is not None else (np.empty(0), np.empty(0), None)
            pu, pw = np.empty([kin.shape[0], len(px)]), np.empty([kin.shape[0], len(px)])
            trows = np.zeros([members, len(rec) + 1, 2, len(sx)])
            if survey is not None:
                vx, vz, vsh, first, stop, every = survey
                sums = np.zeros([members, 5, len(vx)])
                sargs = (*args, _pd(px), _pd(pz), len(px), _pd(sh), 0 if sh is None else len(sh), _pd(pu), _pd(pw), _pd(sx), _pd(sz),
                         rel.ctypes.data_as(pll), len(sx), _pd(tsh), 0 if tsh is None else len(tsh), rec.ctypes.data_as(pll), len(rec),
                         _pd(trows), trows.size, _pd(vx), _pd(vz), len(vx), _pd(vsh), 0 if vsh is None else len(vsh), first, stop,
                         every, _pd(sums), sums.size)
                if integrals is not None:
                    (win,), (table, nbins), K = integrals, bins, len(vx)
                    bsums = np.zeros([members, nbins, 5, K]) if nbins else None
                    gsums = np.zeros([members, 5, K]) if grad else None
                    bgsums = np.zeros([members, nbins, 5, K]) if grad and nbins else None
                    isums = np.zeros([kin.shape[0], 4, 2, 6])
                    energy = None if win is None else np.empty(kin.shape[0])
                    self._check(self._lib.ludvm_ensemble_run_integrals(
                        *sargs, table.ctypes.data_as(POINTER(c_int)) if nbins else None, len(table), nbins, _pd(bsums),
                        0 if bsums is None else bsums.size, _pd(gsums), 0 if gsums is None else gsums.size, _pd(bgsums),
                        0 if bgsums is None else bgsums.size, _pd(isums), isums.size, _pd(energy), 0 if energy is None else energy.size,
                        *(win or (0, 0, 0))))
                    out = (rows, wakes, wake_n, trows) if probes is None else (rows, wakes, wake_n, trows, pu, pw)
                    return out + (sums if K else None, bsums, gsums, bgsums, isums, energy)
                if grad:
                    table, nbins = bins
                    K = len(vx)
                    bsums = np.zeros([members, nbins, 5, K]) if nbins else None
                    gsums = np.zeros([members, 5, K])
                    bgsums = np.zeros([members, nbins, 5, K]) if nbins else None
                    self._check(self._lib.ludvm_ensemble_run_surveyed_graded(
                        *sargs, table.ctypes.data_as(POINTER(c_int)) if nbins else None, len(table), nbins, _pd(bsums),
                        0 if bsums is None else bsums.size, _pd(gsums), gsums.size, _pd(bgsums), 0 if bgsums is None else bgsums.size))
                    out = (rows, wakes, wake_n, trows) if probes is None else (rows, wakes, wake_n, trows, pu, pw)
                    return out + (sums, bsums, gsums, bgsums)
                if bins is not None:
                    table, nbins = bins
                    bsums = np.zeros([members, nbins, 5, len(vx)])
                    self._check(self._lib.ludvm_ensemble_run_surveyed_binned(
                        *sargs, table.ctypes.data_as(POINTER(c_int)), len(table), nbins, _pd(bsums), bsums.size))
                    out = (rows, wakes, wake_n, trows) if probes is None else (rows, wakes, wake_n, trows, pu, pw)
                    return out + (sums, bsums)
                self._check(self._lib.ludvm_ensemble_run_surveyed(*sargs))
                return (rows, wakes, wake_n, trows, sums) if probes is None else (rows, wakes, wake_n, trows, pu, pw, sums)
            self._check(self._lib.ludvm_ensemble_run_traced(
                *args, _pd(px), _pd(pz), len(px), _pd(sh), 0 if sh is None else len(sh), _pd(pu), _pd(pw), _pd(sx), _pd(sz),
                rel.ctypes.data_as(pll), len(sx), _pd(tsh), 0 if tsh is None else len(tsh), rec.ctypes.data_as(pll), len(rec),
                _pd(trows), trows.size))
            return (rows, wakes, wake_n, trows) if probes is None else (rows, wakes, wake_n, trows, pu, pw)
        if probes is None:
            self._check(self._lib.ludvm_ensemble_run(*args))
            return rows, wakes, wake_n
        px, pz, sh = probes
        if not hasattr(self._lib, "ludvm_ensemble_run_probed"):
            raise LudvmHipError(_ffi.E_STATE, "this build of the library has no ludvm_ensemble_run_probed")
        pu, pw = np.empty([kin.shape[0], len(px)]), np.empty([kin.shape[0], len(px)])
        self._check(self._lib.ludvm_ensemble_run_probed(*args, _pd(px), _pd(pz), len(px), _pd(sh), 0 if sh is None else len(sh),
                                                        _pd(pu), _pd(pw)))
        return rows, wakes, wake_n, pu, pw

    # -- flow field ------------------------------------------------------------------------------
    def flowfield(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core):
        """(u, w) float32 [nx, nz] on the grid (xmin + i*dr, zmin + j*dr) (LUDVM.py:1193-1195)."""
        g, xs, zs = _f64(circulation), _f64(xw), _f64(zw)
        u, w = np.empty(nx * nz, np.float32), np.empty(nx * nz, np.float32)
        self._check(self._lib.ludvm_flowfield_f32(self._ctx, float(xmin), float(zmin), float(dr), int(nx), int(nz),
                                                  _pd(xs), _pd(zs), _pd(g), len(xs), float(v_core), _pf(u), _pf(w)))
        return u.reshape(nx, nz), w.reshape(nx, nz)

    def flowfield_vorticity(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, precision="f32"):
        """(u, w, ome) [nx, nz]: velocity field and its vorticity (LUDVM.py:1224-1292) in one device round trip -- the
        stencil runs on the fields where they are.  float32 arrays from fp32 arithmetic on local-origin sources, or,
        with precision='f64', float64 arrays from float64 arithmetic throughout (the reference's)."""
        return self.flowfield_rows(xmin, zmin, dr, nx, nz, 0, nx, circulation, xw, zw, v_core, precision=precision)

    def flowfield_rows(self, xmin, zmin, dr, nx, nz, row_first, row_count, circulation, xw, zw, v_core, vorticity=True,
                       precision="f32"):
        """Rows [row_first, row_first + row_count) of the nx x nz grid: (u, w, ome) [row_count, nz], bit for bit what the
        whole-grid call returns for those rows -- the unit a multi-GPU flow field shards by.  precision 'f32' (float32
        arrays) or 'f64' (float64 arrays, float64 arithmetic throughout)."""
        g, xs, zs = _f64(circulation), _f64(xw), _f64(zw)
        f64 = _prec(precision) == PREC_F64
        dt, ptr = (np.float64, _pd) if f64 else (np.float32, _pf)
        fn = self._lib.ludvm_flowfield_rows_f64 if f64 else self._lib.ludvm_flowfield_rows_f32
        u, w = np.empty(row_count * nz, dt), np.empty(row_count * nz, dt)
        ome = np.empty(row_count * nz, dt) if vorticity else None
        self._check(fn(self._ctx, float(xmin), float(zmin), float(dr), int(nx), int(nz), int(row_first), int(row_count),
                       _pd(xs), _pd(zs), _pd(g), len(xs), float(v_core), ptr(u), ptr(w), ptr(ome)))
        sh = (row_count, nz)
        return u.reshape(sh), w.reshape(sh), (ome.reshape(sh) if vorticity else None)

    def flowfield_dev(self, xmin, zmin, dr, nx, nz, d_xs, d_zs, d_gs, ns, v_core, d_u, d_w):
        self._check(self._lib.ludvm_flowfield_dev_f32(self._ctx, float(xmin), float(zmin), float(dr), int(nx), int(nz),
                                                      d_xs, d_zs, d_gs, int(ns), float(v_core), d_u, d_w))

    def vorticity(self, u, w, dr):
        nx, nz = u.shape
        uu, ww = _f32(u), _f32(w)
        ome = np.empty(nx * nz, np.float32)
        self._check(self._lib.ludvm_vorticity_f32(self._ctx, _pf(uu), _pf(ww), nx, nz, float(dr), _pf(ome)))
        return ome.reshape(nx, nz)

    def vorticity_dev(self, d_u, d_w, nx, nz, dr, d_ome):
        self._check(self._lib.ludvm_vorticity_dev_f32(self._ctx, d_u, d_w, int(nx), int(nz), float(dr), d_ome))

    # -- stream function and analytic vorticity ---------------------------------------------------
    def _field_kind(self, kind, fn):
        if not hasattr(self._lib, fn):
            raise LudvmHipError(_ffi.E_STATE, f"this build of the library has no {fn}")
        code = _ffi.FIELD_KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(code, bool) or not isinstance(code, int):
            raise ValueError("kind: 'psi' or 'omega' (or the library's code)")
        return code

    def _field_entry(self, what, f64_name, precision, code=None):
        """the library function of a field sum in `precision`: 'f64', or 'f32x2' (hi+lo fp32 pairs: 'omega' and the gradient);
        code: the scalar sums' kind"""
        if precision == "f64":
            return getattr(self._lib, f64_name)
        if precision != "f32x2":
            raise ValueError(f"{what}: precision must be 'f64' or 'f32x2', not {precision!r}")
        if code == _ffi.FIELD_KINDS["psi"]:
            raise ValueError(f"{what}: the stream function has no fp32 route (precision='f32x2' serves 'omega')")
        name = f64_name[:-len("f64")] + "f32x2"
        self._need(name)
        return getattr(self._lib, name)

    def scalar_field(self, kind, circulation, xw, zw, xp, zp, v_core, precision="f64"):
        """float64 [Np]: the stream function (kind 'psi': sum G / (4 pi) ln((r^2 + s) / 2), s = sqrt(r^4 + v_core^4), whose z and
        -x derivatives are `induce`'s u and w) or the core model's vorticity (kind 'omega': dw/dx - du/dz of that
        velocity in closed form, -sum G v_core^4 / (pi s^3)) of the
        vortices at the points, in float64 throughout (ludvm_scalar_f64).  precision='f32x2': 'omega' with the pair arithmetic in
        hi+lo fp32 (ludvm_scalar_f32x2: float64 in and out, <= 2e-6 of max|omega|, v_core >= 1e-6); 'psi' has no such route."""
        code = self._field_kind(kind, "ludvm_scalar_f64")
        fn = self._field_entry("scalar_field", "ludvm_scalar_f64", precision, code)
        g, xs, zs, xt, zt = _f64(circulation), _f64(xw), _f64(zw), _f64(xp), _f64(zp)
        if not (len(g) == len(xs) == len(zs)) or len(xt) != len(zt):
            raise ValueError("scalar_field: source arrays (and target arrays) must have equal lengths")
        out = np.empty(len(xt))
        self._check(fn(self._ctx, code, _pd(xs), _pd(zs), _pd(g), len(xs), _pd(xt), _pd(zt), len(xt), float(v_core), _pd(out)))
        return out

    def flowfield_scalar(self, kind, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None,
                         precision="f64"):
        """float64 [row_count, nz]: `scalar_field` on rows [row_first, row_first + row_count) of the flow-field grid
        (xmin + i*dr, zmin + j*dr), generated on the device; every row by default.  A block of rows carries the whole-grid
        call's bits (ludvm_flowfield_scalar_rows_f64; precision='f32x2': ludvm_flowfield_scalar_rows_f32x2, as `scalar_field`)."""
        code = self._field_kind(kind, "ludvm_flowfield_scalar_rows_f64")
        fn = self._field_entry("flowfield_scalar", "ludvm_flowfield_scalar_rows_f64", precision, code)
        g, xs, zs = _f64(circulation), _f64(xw), _f64(zw)
        if not (len(g) == len(xs) == len(zs)):
            raise ValueError("flowfield_scalar: source arrays must have equal lengths")
        nx, nz, row_first = int(nx), int(nz), int(row_first)
        row_count = nx - row_first if row_count is None else int(row_count)
        if nx < 0 or nz < 0 or row_first < 0 or row_count < 0:
            raise ValueError("flowfield_scalar: nx, nz, row_first and row_count must not be negative")
        out = np.empty(max(row_count, 0) * nz)
        self._check(fn(self._ctx, code, float(xmin), float(zmin), float(dr), nx, nz, row_first, row_count, _pd(xs), _pd(zs), _pd(g),
                       len(xs), float(v_core), _pd(out)))
        return out.reshape(row_count, nz)

    # -- velocity gradient ------------------------------------------------------------------------
    def _need(self, fn):
        if not hasattr(self._lib, fn):
            raise LudvmHipError(_ffi.E_STATE, f"this build of the library has no {fn}")

    def gradient_field(self, circulation, xw, zw, xp, zp, v_core, precision="f64"):
        """(ux, uz, wx), float64 [Np] each: du/dx, du/dz and dw/dx of `induce`'s velocity at the points, in closed form and in
        float64 throughout (ludvm_gradient_f64); dw/dz = -ux, wx - uz is `scalar_field('omega', ...)`.  precision='f32x2': the
        pair arithmetic in hi+lo fp32 (ludvm_gradient_f32x2: float64 in and out, <= 2e-6 of max|grad u|, v_core >= 1e-6)."""
        self._need("ludvm_gradient_f64")
        fn = self._field_entry("gradient_field", "ludvm_gradient_f64", precision)
        g, xs, zs, xt, zt = _f64(circulation), _f64(xw), _f64(zw), _f64(xp), _f64(zp)
        if not (len(g) == len(xs) == len(zs)) or len(xt) != len(zt):
            raise ValueError("gradient_field: source arrays (and target arrays) must have equal lengths")
        ux, uz, wx = np.empty(len(xt)), np.empty(len(xt)), np.empty(len(xt))
        self._check(fn(self._ctx, _pd(xs), _pd(zs), _pd(g), len(xs), _pd(xt), _pd(zt), len(xt), float(v_core), _pd(ux), _pd(uz),
                       _pd(wx)))
        return ux, uz, wx

    def flowfield_gradient(self, xmin, zmin, dr, nx, nz, circulation, xw, zw, v_core, row_first=0, row_count=None,
                           precision="f64"):
        """(ux, uz, wx), float64 [row_count, nz] each: `gradient_field` on rows [row_first, row_first + row_count) of the
        flow-field grid (xmin + i*dr, zmin + j*dr), generated on the device; every row by default.  A block of rows carries
        the whole-grid call's bits (ludvm_flowfield_gradient_rows_f64; precision='f32x2': ludvm_flowfield_gradient_rows_f32x2, as
        `gradient_field`)."""
        self._need("ludvm_flowfield_gradient_rows_f64")
        fn = self._field_entry("flowfield_gradient", "ludvm_flowfield_gradient_rows_f64", precision)
        g, xs, zs = _f64(circulation), _f64(xw), _f64(zw)
        if not (len(g) == len(xs) == len(zs)):
            raise ValueError("flowfield_gradient: source arrays must have equal lengths")
        nx, nz, row_first = int(nx), int(nz), int(row_first)
        row_count = nx - row_first if row_count is None else int(row_count)
        if nx < 0 or nz < 0 or row_first < 0 or row_count < 0:
            raise ValueError("flowfield_gradient: nx, nz, row_first and row_count must not be negative")
        ux, uz, wx = (np.empty(max(row_count, 0) * nz) for _ in range(3))
        self._check(fn(self._ctx, float(xmin), float(zmin), float(dr), nx, nz, row_first, row_count, _pd(xs), _pd(zs), _pd(g),
                       len(xs), float(v_core), _pd(ux), _pd(uz), _pd(wx)))
        return ux.reshape(row_count, nz), uz.reshape(row_count, nz), wx.reshape(row_count, nz)

    def fixed_point_probe(self, values, scale_log2):
        """int64 units the symmetric kernel adds to an accumulator for fp32 partial sums `values` at scale
        2**scale_log2 (ludvm_fixed_point_probe): trunc(value * scale), exact below 2**63."""
        v = _f32(values)
        out = np.empty(len(v), np.int64)
        self._check(self._lib.ludvm_fixed_point_probe(self._ctx, _pf(v), len(v), int(scale_log2),
                                                      out.ctypes.data_as(POINTER(c_longlong))))
        return out

    # -- measurement -----------------------------------------------------------------------------
    def kernel_timing(self, enable=True):
        self._check(self._lib.ludvm_kernel_timing(self._ctx, 1 if enable else 0))

    def kernel_time_ms(self, reset=True):
        ms, n = c_double(), c_longlong()
        self._check(self._lib.ludvm_kernel_time_ms(self._ctx, 1 if reset else 0, byref(ms), byref(n)))
        return ms.value, n.value
