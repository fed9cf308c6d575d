/*
 * ludvm_hip.h -- C ABI of libludvm_hip.so, the MI355X (gfx950) all-pairs vortex-induction engine
 * that sits behind the LUDVM Python class.
 *
 * The reference (jcatalang/LUDVM) has no FFI: its "operator boundary" for this path is the Python
 * method surface of class LUDVM.  Each entry point below cites the reference code it replaces
 * (file:line into LUDVM.py).  The Python host (ludvm_amd/_ffi.py, ctypes) binds exactly these
 * symbols; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns an int status: 0 = LUDVM_OK, otherwise one of LUDVM_E_*; nothing
 *     throws across the ABI and nothing calls exit();
 *   - ludvm_last_error(ctx) returns a human-readable message for the last failure on that context
 *     (pointer owned by the context, valid until the next call on it);
 *   - plain pointers and sizes only; "host" pointers are ordinary process memory, "dev" pointers
 *     are HIP device memory on the context's device (e.g. a torch tensor's data_ptr());
 *   - host-pointer entry points are synchronous (results are in the output arrays on return);
 *     dev-pointer entry points are asynchronous on the context's stream (ludvm_set_stream /
 *     ludvm_synchronize);
 *   - a context is not thread-safe: one host thread at a time per context (the reference is
 *     single-threaded); distinct contexts are independent;
 *   - coordinates follow the reference: x (horizontal), z (vertical), circulation Gamma, and the
 *     Vatistas core radius v_core (= 1.3*dt*Uinf, LUDVM.py:259-260); v_core = 0 means point
 *     vortices (the reference's `viscous != True` branch, LUDVM.py:562-563), for which a
 *     coincident source/target pair yields NaN exactly as the reference's 0/0 does.
 */
#ifndef LUDVM_HIP_H
#define LUDVM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUDVM_ABI_VERSION 7

enum {
  LUDVM_OK = 0,
  LUDVM_E_ARG = 1,      /* bad argument (null pointer, range outside the wake, ...) */
  LUDVM_E_HIP = 2,      /* a HIP runtime call failed; message has the HIP error string */
  LUDVM_E_NOMEM = 3,    /* device or host allocation failed */
  LUDVM_E_NODEVICE = 4, /* no usable gfx950 device */
  LUDVM_E_STATE = 5,    /* call not valid in the current state (e.g. wake not reserved) */
  LUDVM_E_COMM = 6      /* RCCL could not be opened, or one of its calls failed; message has its error string */
};

/* Arithmetic the pair sum is evaluated in. */
enum {
  LUDVM_PREC_F32 = 0,   /* fp32 arithmetic (headline kernel).  Wherever the library lays the positions out itself (host
                           float64 inputs, the resident wake) they are stored as fp32 offsets from the origin of their
                           256-vortex block and the origin difference is added once per block pair ("local origins"):
                           same speed as plain fp32, and a wake at |x| ~ 50 with vortices 1e-3 apart keeps ~1e-5 of
                           max|u| instead of ~1e-3.  Device fp32 inputs are used as they are. */
  LUDVM_PREC_F32X2 = 1, /* positions as hi+lo fp32 pairs: dx = (xh_p - xh_w) + (xl_p - xl_w), rest fp32.
                           Removes the cancellation error of |x| ~ 50 vs spacing ~ 1e-3. */
  LUDVM_PREC_F64 = 2    /* fp64 throughout (parity / debug mode, and the small chord-target calls) */
};

typedef struct ludvm_ctx ludvm_ctx;

/* ---- lifecycle -------------------------------------------------------------------------- */

int ludvm_abi_version(void);
/* Create a context bound to HIP device `device_ordinal` (must be a gfx950 part).  Owns one stream and its workspaces.
 * The library's results never depend on the environment: a production build reads LUDVM_RCCL_LIB (which librccl to open)
 * and LUDVM_COMM_FORCE (tests) and nothing else; the A/B switches of the measurement build (libludvm_hip_exp.so,
 * -DLUDVM_EXPERIMENTS) are listed in INTEGRATION.md. */
int ludvm_create(int device_ordinal, ludvm_ctx** out);
int ludvm_destroy(ludvm_ctx* ctx);
const char* ludvm_last_error(const ludvm_ctx* ctx);
/* Device facts for the roofline: CU count, max shader clock (kHz), HBM bytes, name (NUL-terminated). */
int ludvm_device_info(ludvm_ctx* ctx, int* cu_count, int* clock_khz, long long* hbm_bytes, char* name,
                      int name_len);
/* external != 0: use the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) for all
 * subsequent launches -- a NULL handle then means the device's default (null) stream, which is what
 * torch's default stream is.  external == 0: go back to the context's own stream. */
int ludvm_set_stream(ludvm_ctx* ctx, void* hip_stream, int external);
int ludvm_synchronize(ludvm_ctx* ctx);
/* Launch shape knobs (0 keeps the built-in heuristic): targets per lane {1,2,4}, source splits.  For the symmetric
 * kernels the second number is the count of d-chunks (work items) per tile -- the rule gives at most 64 -- or, in the quad
 * variant, per quad of tiles, where k > 0 asks for k uniform chunks instead of the rule's tapered ones (long items
 * first, the last eighth of the ring offsets in short ones).  Results change only through the partition into fp32
 * partial sums. */
int ludvm_set_tuning(ludvm_ctx* ctx, int targets_per_lane, int source_splits);

/* Self-interaction launches (targets are exactly the sources: wake roll-up, all-pairs calls on one
 * array) may use the symmetric kernel, which evaluates each unordered pair once (K(i->j) = -K(j->i)): ~1.5x
 * faster.  It accumulates in 64-bit fixed point (integer atomics, scale from sum|Gamma| / v_core), so its results
 * do not depend on the order of the atomics: a launch repeats bit for bit, like the direct kernel and like the
 * reference.  Launches with v_core = 0 (no bound on the kernel) always take the direct kernel.
 * mode 0 = never (direct kernel), 1 = automatic (default; fp32, N >= 16384),
 * mode >= 2 = automatic with that value as the smallest N that takes the symmetric kernel. */
int ludvm_set_symmetric(ludvm_ctx* ctx, int mode);
/* Symmetric launches on plain fp32 DEVICE arrays (ludvm_induce_dev_f32 with the sources as targets, ludvm_advect_dev_f32
 * over the whole array; LUDVM.py:549-570 on one array) may be evaluated in Morton order: box, keys, stable sort and gather
 * on the context's stream, the pair kernel on the ordered copies, every result written at the caller's own index by the
 * finisher.  The sum does not care about the order; the kernel's operands become spatially coherent, which lets the chip
 * hold a higher clock under it.  Keys, sort and fixed-point sums depend on the input alone: a call repeats bit for bit.
 * mode 0 = never, 1 = from the size the library's rule states (default; csrc/sym_rule.hpp, kSelfOrderMin; smaller
 * launches are what they were, bit for bit), 2 = whenever the symmetric kernel runs (tests, A/B). */
int ludvm_set_self_order(ludvm_ctx* ctx, int mode);
/* Tuning of the symmetric kernel (tests; 0 = the library's rule by launch size): vortices per lane (4: 256-vortex tiles,
 * 8: 512-vortex tiles; plain fp32 positions only) and the number of wavefronts (1, 2, 4) that share the 64 rotation steps
 * of one tile pair.  Results change only through the partition into fp32 partial sums.  (The measurement build also takes
 * three negative codes that force a variant at every size; a production build answers them with LUDVM_E_ARG.) */
int ludvm_set_sym_tuning(ludvm_ctx* ctx, int vortices_per_lane, int rotation_split);

/* Sharding ONE simulation's roll-up over several GPUs (LUDVM.time_loop, LUDVM.py:1095-1127, with a wake too large
 * for one GPU to be quick about).  Every GPU holds the whole wake and runs the whole time loop -- chord sums, solve,
 * Euler step: everything that is O(N) or smaller -- but evaluates only tile block `rank` of `world` of the symmetric
 * kernel's unordered pairs, accumulating into d_acc (caller-owned device memory, e.g. a torch int64 tensor; at
 * least 16 (wake capacity + 64) + 16 bytes).  Before each Euler finisher the library calls
 *     allreduce(user, d_buf, count, hip_stream)
 * which must enqueue, on hip_stream, an in-place SUM all-reduce of the `count` 64-bit integers at d_buf (a prefix of
 * d_acc) over all owners, and return 0 (e.g. torch.distributed.all_reduce on RCCL).  Integer sums commute, so every
 * owner reads the same bits -- those one GPU owning all tiles would have produced -- and the replicated state cannot
 * drift apart.  Roll-ups of fewer than min_vortices vortices (a collective per step costs more than it saves there;
 * ~1e5 on xGMI) are done whole by every owner, without the hook.  world == 1 restores the unsharded behaviour.  On a
 * sharded context every symmetric launch of min_vortices or more is collective: all owners must issue the same calls
 * in the same order. */
typedef int (*ludvm_allreduce_fn)(void* user, void* d_buf, size_t count, void* hip_stream);
int ludvm_set_shard(ludvm_ctx* ctx, int rank, int world, size_t min_vortices, ludvm_allreduce_fn allreduce, void* user,
                    void* d_acc, size_t acc_bytes);

/* ---- the library's own communicator: one simulation, or one synthetic wake, on the GPUs of a node ----------------
 *
 * One process per GPU, each with its own context; the collectives run on RCCL over xGMI INSIDE the library, on the
 * context's stream -- a caller needs no communication library of its own, only a way to hand 128 bytes from rank 0 to
 * the other processes (a file, an environment variable, MPI, torch.distributed ...).  librccl.so is opened when the
 * first of these calls is made (environment LUDVM_RCCL_LIB names the file, default librccl.so.1); a process that never
 * calls them does not need RCCL.
 *
 *   ludvm_comm_unique_id   rank 0: the identifier of a new communicator (LUDVM_COMM_ID_BYTES bytes).
 *   ludvm_comm_init        every rank, with the same identifier: joins the communicator (returns when all `world` ranks
 *                          have) and shards the context's symmetric roll-ups over it exactly as ludvm_set_shard does
 *                          (LUDVM.time_loop's roll-up, LUDVM.py:1095-1127: every rank holds the whole wake and runs the
 *                          whole loop, but evaluates only tile block `rank` of `world` of the unordered pairs) -- with
 *                          the ONE collective per time step, an in-place ncclAllReduce (int64 sum) of the fixed-point
 *                          accumulators and their NaN counter, issued by the library between the symmetric kernel and the
 *                          Euler finisher.  Integer sums commute: every rank reads the bits one GPU would have produced.
 *                          Roll-ups of fewer than min_vortices vortices are done whole by every rank, without a collective.
 *   ludvm_comm_init_all    ONE PROCESS, several devices ("one RCCL communicator, single process, ncclCommInitAll"):
 *                          the n contexts -- one per device, ctxs[k] becomes rank k -- join a new communicator in one call
 *                          from one thread; no identifier, nothing to exchange.  Each context is sharded exactly as by
 *                          ludvm_comm_init.  From then on every context is driven by a HOST THREAD OF ITS OWN, which issues
 *                          the same calls in the same order as a process-per-GPU rank would (RCCL: one thread per device, or
 *                          grouped calls; the entry points that contain the collective -- ludvm_wake_advect*, ludvm_wake_step,
 *                          ludvm_march_run: LUDVM.time_loop's roll-up, LUDVM.py:1095-1127 -- enqueue it between their own
 *                          kernels, so grouping them from one thread would mean cutting each entry point in two).
 *                          ludvm_amd/multi.py is that driver: LUDVM(..., devices=[0, 1, ...]) with no launcher.  ABI 5.
 *   ludvm_comm_destroy     leaves the communicator (collective in RCCL's sense: every rank calls it) and unshards the context.
 *   ludvm_comm_info        rank and world of the context's communicator (world = 0: none).
 *   ludvm_comm_allreduce_i64_dev / ludvm_comm_allgather_dev
 *                          the two collectives of the synthetic-wake step (BASELINE config 4, ludvm_amd/sharded.py) on
 *                          caller-owned device buffers, asynchronous on the context's stream: in-place int64 sum (the
 *                          symmetric variant's accumulators) and an all-gather of bytes_per_rank bytes per rank into
 *                          d_recv[world * bytes_per_rank] (the direct variant's positions -- the north star's "single RCCL
 *                          all-gather of sources per step").
 *   ludvm_comm_allgather_host
 *                          the same all-gather for host buffers (synchronous): how the ranks of one simulation exchange
 *                          their blocks of a flow field (LUDVM.py:1186-1298) or of an induced_velocity call (:549-570).
 */
#define LUDVM_COMM_ID_BYTES 128
int ludvm_comm_unique_id(void* id_out, size_t id_bytes);
int ludvm_comm_init(ludvm_ctx* ctx, int rank, int world, const void* id, size_t id_bytes, size_t min_vortices);
int ludvm_comm_init_all(ludvm_ctx** ctxs, int n, size_t min_vortices);
int ludvm_comm_destroy(ludvm_ctx* ctx);
int ludvm_comm_info(ludvm_ctx* ctx, int* rank, int* world);
int ludvm_comm_allreduce_i64_dev(ludvm_ctx* ctx, long long* d_buf, size_t count);
int ludvm_comm_allgather_dev(ludvm_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank);
int ludvm_comm_allgather_host(ludvm_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank);

/* ---- stateless pair sum: backs LUDVM.induced_velocity (LUDVM.py:549-570) ------------------ */

/* u[p] =  sum_w g[w]*(zt[p]-zs[w]) / (2 pi sqrt(r^4 + vcore^4))
 * w[p] = -sum_w g[w]*(xt[p]-xs[w]) / (2 pi sqrt(r^4 + vcore^4)),  r^2 = dx^2+dz^2.
 * Host float64 in/out (what the reference passes and returns); `precision` selects the device
 * arithmetic.  ns == 0 or nt == 0 is valid (u, w zero-filled / untouched).
 * The reference's float64 sum (LUDVM.py:565-569) does not depend on the order of its arrays; LUDVM_PREC_F32 here keeps
 * 1e-5 of max|u| for ANY order: sources and targets that are not stored compactly (a user's array, a turbulence cloud of
 * :98-130 -- unlike a shed wake) are evaluated in Morton order on the device and the results returned in the caller's
 * order (the given order is kept, and with it every result bit, whenever it is already compact: within 3 x of an
 * area-filling arrangement, or of a line across its bounding box, or within 1.5 x of what Morton order achieves); a call
 * with fewer than 2048 sources or targets -- too few to make 128-point origin classes compact -- runs in float64 while
 * ns * nt <= 2^28 (~0.2 ms at most) and on hi+lo positions beyond (a few probe points in a wake of millions: 1.3 x the
 * fp32 time instead of the float64 rate on every pair); and a set too sparse for its core (mean class extent > 150 v_core
 * in Morton order, > 300 v_core for a set that is compact as given: fp32 offsets cannot resolve a core that small) takes
 * hi+lo positions as LUDVM_PREC_F32X2 does.  The arithmetic of a LUDVM_PREC_F32 call, and with it the last bits of its
 * result, therefore depends on the SIZES and the COMPACTNESS of what is passed (never on anything else: same arrays, same
 * bits); a set that evolves slowly across one of these thresholds changes route from one call to the next, within the
 * stated 1e-5 either way. */
int ludvm_induce_f64(ludvm_ctx* ctx, const double* xs, const double* zs, const double* gs, size_t ns,
                     const double* xt, const double* zt, size_t nt, double vcore, int precision,
                     double* u, double* w);
/* The order the library itself would evaluate the n points (x, z) in: order[k] = index of the point that takes position
 * k.  Morton order when the given order is not compact (see ludvm_induce_f64), else the identity (*reordered = 0; also
 * for n < 2048).  For callers of the RESIDENT wake, whose slots are the caller's indices: LUDVM uploads a cloud of free
 * vortices (LUDVM.py:98-130, :274-277) in this order and returns history rows in its own, so that fp32 roll-ups of an
 * unordered cloud keep the accuracy tier of a shed wake.  *mean_class_extent (may be NULL) = mean over the 128-point origin
 * classes, in that order, of (xmax - xmin) + (zmax - zmin); fp32 on local origins keeps 1e-5 of max|u| up to about
 * 150 v_core for a cloud that had to be reordered, 300 v_core for a set that is compact as given (beyond:
 * LUDVM_PREC_F32X2).  Deterministic. */
int ludvm_spatial_order(ludvm_ctx* ctx, const double* x, const double* z, size_t n, unsigned* order, int* reordered,
                        double* mean_class_extent);
/* Same with host float32 buffers (always LUDVM_PREC_F32 arithmetic). */
int ludvm_induce_f32(ludvm_ctx* ctx, const float* xs, const float* zs, const float* gs, size_t ns,
                     const float* xt, const float* zt, size_t nt, float vcore, float* u, float* w);
/* Device-resident fp32 SoA (torch tensors): asynchronous on the context stream.  Used by the
 * benchmark, the multi-GPU shard step and the flow-field path. */
int ludvm_induce_dev_f32(ludvm_ctx* ctx, const float* d_xs, const float* d_zs, const float* d_gs, size_t ns,
                         const float* d_xt, const float* d_zt, size_t nt, float vcore, float* d_u,
                         float* d_w);
/* One explicit-Euler advection step on device fp32 SoA (LUDVM.py:1105-1127 with the wake as both
 * source and target set): (u,w) induced by all ns sources on targets [t_first, t_first+nt) of the
 * same arrays, then x_out[i] = x[t_first+i] + dt*u[i], z_out likewise.  x_out/z_out must not alias
 * the source arrays (the multi-GPU step all-gathers them into the next source buffer). */
int ludvm_advect_dev_f32(ludvm_ctx* ctx, const float* d_xs, const float* d_zs, const float* d_gs, size_t ns,
                         size_t t_first, size_t nt, float vcore, float dt, float* d_x_out, float* d_z_out);

/* Multi-GPU building blocks of the symmetric roll-up (ludvm_amd/sharded.py: BASELINE config 4, bench.py's N > 1 line).
 * Reading the benchmark across GPU counts: bench.py's `value` at N = 1 is config 3 (N = 1e6, one ludvm_induce_dev_f32 call per
 * step); at N > 1 it is config 4 (N = 8e6, these entry points + one collective per step).  The same-work denominator of
 * "8 GPUs vs 1" is the N = 1 line's `config4_one_gpu.value` (config 4's step on one GPU), which every N > 1 line names in
 * `scaling_denominator` -- not the N = 1 line's `value`.
 * Vortices are cut into
 * tiles of LUDVM_SYM_TILE; the caller owns tiles [tile_first, tile_first + tile_count) of the
 * ceil(n / LUDVM_SYM_TILE) tiles.
 *   ludvm_sym_scale_dev_f32 derives the fixed-point scale of the raw sums from sum|Gamma| / v_core (summed in a
 *     fixed order: every GPU holding the same circulations gets the same record) into d_scale, a caller-owned
 *     device record of LUDVM_SYM_SCALE_BYTES; v_core must be > 0.
 *   ludvm_sym_accumulate_dev_f32 evaluates this owner's share of the unordered pairs (its tiles against the cyclic
 *     half of the tile ring) and ADDS the raw sums of both partners, as 64-bit fixed-point integers, into
 *     d_acc_u / d_acc_w (n each, zeroed by the caller); *d_bad (zeroed by the caller) is incremented when a partial
 *     sum was not finite.  Integer sums are order-independent: summed over all owners (a sum all-reduce of the
 *     three buffers) they are bit for bit what one GPU owning all tiles produces.
 *   ludvm_advect_from_sums_dev_f32 turns the summed values of targets [t_first, t_first + nt) (d_sum_*[i] belongs to
 *     target t_first + i) into the Euler step x_out[i] = x[t_first + i] + dt * u, z_out likewise
 *     (LUDVM.py:1108-1109); NaN when *d_bad != 0, as the reference's sum over a NaN source would be. */
#define LUDVM_SYM_TILE 512
#define LUDVM_SYM_OWNER_ALIGN 4   /* an owner's tile block starts and ends on multiples of this many tiles (or ends with the
                                     ring): large launches add the partial sums of four consecutive tiles' wavefronts in fp32
                                     before they are converted to fixed point, so such a quad must not be cut between owners */
#define LUDVM_SYM_SCALE_BYTES 32
int ludvm_sym_scale_dev_f32(ludvm_ctx* ctx, const float* d_g, size_t n, float vcore, void* d_scale);
int ludvm_sym_accumulate_dev_f32(ludvm_ctx* ctx, const float* d_x, const float* d_z, const float* d_g, size_t n,
                                 size_t tile_first, size_t tile_count, float vcore, const void* d_scale,
                                 long long* d_acc_u, long long* d_acc_w, long long* d_bad);
int ludvm_advect_from_sums_dev_f32(ludvm_ctx* ctx, const long long* d_sum_u, const long long* d_sum_w,
                                   const void* d_scale, const long long* d_bad, const float* d_x, const float* d_z,
                                   size_t t_first, size_t nt, float dt, float* d_x_out, float* d_z_out);

/* ---- resident wake: backs LUDVM.time_loop (LUDVM.py:597-1171) ----------------------------- */
/* The wake (TEV, LEV and FREE vortices, in an order the host chooses) lives on the device across
 * time steps as float64 master copies plus the fp32 (hi, lo) SoA the pair kernel reads. */

int ludvm_wake_reserve(ludvm_ctx* ctx, size_t capacity);      /* grow-only; keeps contents */
int ludvm_wake_clear(ludvm_ctx* ctx);                          /* size := 0 */
int ludvm_wake_size(ludvm_ctx* ctx, size_t* n);
/* Drop the vortices past the first n (n <= size).  The phantom LEV slot of a non-shedding step
 * (LUDVM.py:1112-1118 moves slot ilev although nothing was shed) is appended, advected, read back
 * and dropped this way. */
int ludvm_wake_truncate(ludvm_ctx* ctx, size_t n);
/* Append `count` vortices (new TEV / LEV placement, LUDVM.py:672-681, 788-800). */
int ludvm_wake_append(ludvm_ctx* ctx, const double* x, const double* z, const double* gamma, size_t count);
/* Overwrite positions and/or circulation of [first, first+count); NULL leaves that field as is.
 * The circulation of the newest TEV/LEV is solved after placement (LUDVM.py:758-760, 953-954). */
int ludvm_wake_write(ludvm_ctx* ctx, size_t first, size_t count, const double* x, const double* z,
                     const double* gamma);
/* Read back [first, first+count) (history rows of path['TEV'|'LEV'|'FREE'], LUDVM.py:615-618).
 * Any of x, z, gamma may be NULL. */
int ludvm_wake_read(ludvm_ctx* ctx, size_t first, size_t count, double* x, double* z, double* gamma);
/* Velocity induced by wake vortices [src_first, src_first+src_count) at nt host points (the
 * Npoints-1 bound-vortex points of the chord: LUDVM.py:582-584, 1049-1054).  fp64 arithmetic:
 * these O(Npanels x Nw) sums feed the Gamma solve and the loads and cost <1 % of a step. */
int ludvm_wake_induce_on_points(ludvm_ctx* ctx, size_t src_first, size_t src_count, const double* xt,
                                const double* zt, size_t nt, double vcore, double* u, double* w);
/* One call for everything a time step needs at the chord before the Gamma solve: the sum of
 * ludvm_wake_induce_on_points over wake vortices [src_first, src_first+src_count) -> (u_wake, w_wake)[nt],
 * plus the velocity induced there by n_unit (<= 4) unit-strength vortices at (unit_x, unit_z) -- the new
 * TEV and the candidate LEV (LUDVM.py:751, :926, :931) -> u_unit, w_unit as [n_unit][nt] rows.  fp64.
 * One host->device copy, one device->host copy, one synchronisation. */
int ludvm_wake_chord_sums(ludvm_ctx* ctx, size_t src_first, size_t src_count, const double* xt, const double* zt,
                          size_t nt, const double* unit_x, const double* unit_z, size_t n_unit, double vcore,
                          double* u_wake, double* w_wake, double* u_unit, double* w_unit);
/* Wake roll-up, fused (LUDVM.py:1095-1127): for every wake vortex i in [0, size):
 *   (u,w)_i = induced by all wake vortices  +  induced by the nfoil bound vortices (foil_x, foil_z,
 *   foil_dgamma: LUDVM.py:1096,1099-1100), both with the same core radius;
 *   x_i += dt*u_i ; z_i += dt*w_i   (explicit Euler, float64 update of the master copy).
 * `precision` selects the pair arithmetic.  If u_out/w_out are non-NULL the induced velocities
 * (before the update) are also returned (size doubles each). */
int ludvm_wake_advect(ludvm_ctx* ctx, double dt, const double* foil_x, const double* foil_z,
                      const double* foil_dgamma, size_t nfoil, double vcore, int precision, double* u_out,
                      double* w_out);
/* Same, and read back the updated positions of the last tail_count wake vortices (the newest TEV / LEV,
 * which place the next ones: LUDVM.py:680-681, 797-798) in the same call; synchronous when
 * tail_count > 0. */
int ludvm_wake_advect_tail(ludvm_ctx* ctx, double dt, const double* foil_x, const double* foil_z,
                           const double* foil_dgamma, size_t nfoil, double vcore, int precision, size_t tail_count,
                           double* tail_x, double* tail_z);

/* One round trip per time step -- one packed upload, one staging kernel, the pair kernels, one download:
 *   1. append the n_new vortices shed this step (new_x/z/gamma; LUDVM.py:672-681, 788-800, 953-954);
 *   2. the roll-up of step i exactly as ludvm_wake_advect (LUDVM.py:1095-1127);
 *   3. what step i+1 needs before its Gamma solve:
 *      - placement of the next TEV and of the candidate LEV from the advected positions: one third of the
 *        way from the trailing edge te[2] / leading edge le[2] (of step i+1) to the newest TEV (vortex
 *        size - tail_count) / newest LEV (vortex size - 1, used when lev_from_prev != 0 and tail_count == 2;
 *        otherwise the candidate sits on the leading edge)  (LUDVM.py:680-681, :788-800);
 *      - ludvm_wake_chord_sums over the whole advected wake at the nt points (xt, zt) of step i+1 with those
 *        two unit vortices.
 * Outputs: tail_x/z[tail_count] (updated newest vortices), unit_x/z[2] (the placed TEV, LEV candidate),
 * u_wake/w_wake[nt], u_unit/w_unit[2][nt].  tail_count is 1 or 2. */
int ludvm_wake_step(ludvm_ctx* ctx, const double* new_x, const double* new_z, const double* new_gamma, size_t n_new,
                    double dt, const double* foil_x, const double* foil_z, const double* foil_dgamma, size_t nfoil,
                    double vcore, int precision, const double* te, const double* le, int lev_from_prev,
                    size_t tail_count, const double* xt, const double* zt, size_t nt, double* tail_x, double* tail_z,
                    double* unit_x, double* unit_z, double* u_wake, double* w_wake, double* u_unit, double* w_unit);

/* ---- device-resident time march: many steps of LUDVM.time_loop per call (LUDVM.py:597-1171) --------
 *
 * ludvm_wake_step still costs one host round trip per time step, because the Gamma solve between two
 * roll-ups (LUDVM.py:743-1090) runs on the host.  These two calls move that solve to the device: 'Faure' method,
 * closed-form Gamma_TEV :758-760 and the 2x2 TEV/LEV system :944-954; 'Ramesh', the Newton iterations of :683-739
 * and :807-914 on the six projections of T1, T2, T3 (the downwash is linear in the circulations); for both, the
 * Fourier coefficients :765-773, LESP criterion :781-805, bound vorticity :987-1010 and loads :1035-1090.  So `count`
 * consecutive steps are enqueued back to back; whether a LEV is shed -- and hence the wake size -- is decided on the
 * device.
 *
 * ludvm_march_setup uploads what does not change during a run:
 *   scalars[12] = Uinf, chord, rho, dt, piv, v_core, IC (:647), sum(Gamma_free), method (0 'Faure', 1 'Ramesh'),
 *                 maxerror, maxiter, epsilon (the Newton controls of 'Ramesh', :253-255; ignored for 'Faure');
 *   tables     = detadx_panel[np] | eta_panel[np] | x_panel[np] | cm1[np] | wq[np] | opcs[np] | hcsd[np] | wx[np]
 *                | cproj[nc][np] | ssin[nc-1][np]
 *                with np = npan, nc = ncoef and, on theta_panel with trapezoid weights wq:
 *                cm1 = (cos(theta) - 1) wq, opcs = (1 + cos)/sin, hcsd = c/2 sin(theta) dtheta, wx = trapezoid
 *                weights on x_panel, cproj[0] = -wq/pi, cproj[n] = 2/pi cos(n theta) wq, ssin[n-1] = sin(n theta);
 *   kin        = one row per time step i, [alpha, alpha_dot, h_dot, te_x, te_z, le_x, le_z, xg[np], zg[np]]
 *                (airfoil_gamma_points and the edges of path['airfoil'] at step i).
 * 1 <= npan <= 256, 4 <= ncoef <= 64.
 *
 * ludvm_march_run advances the resident wake through time steps [first_step, first_step + count), all inside
 * the kinematics table.  state (16 + ncoef doubles, in and out):
 *   [0] wake size (in: must equal ludvm_wake_size)   [1] TEVs shed   [2] LEVs shed
 *   [3] a LEV was shed in the previous step          [4] LESPcrit with its current sign (:802-805)
 *   [5] sum Gamma_TEV   [6] sum Gamma_LEV            [7..10] tev_x, lev_x, tev_z, lev_z of the coming step
 *   [11] out: vortices shed by the last step (1 or 2)
 *   [12..15] out: x[size-2], x[size-1], z[size-2], z[size-1] after the last roll-up (ignored on input)
 *   [16..16+ncoef) Fourier coefficients of the previous step.
 * rows (out): count rows of 12 + 2 ncoef + 2 npan doubles:
 *   g_tev, g_lev, shed(0/1), bound, LESP_prev, LESP, Fn, Fs, M, wake slot of the new TEV,
 *   velocity (u, w) at the origin on a step that sheds no LEV (the reference convects a zero-strength LEV slot
 *   from there and stores where it lands, :1112-1118), A[ncoef], dA/dt[ncoef], gamma[npan], dGamma[npan].
 * hist (out, may be NULL): the reference's dense trajectory history (:1108-1127) -- after each step's roll-up the
 *   positions of all wake vortices, count rows of x[hist_nmax] | z[hist_nmax] in wake (shedding) order;
 *   hist_nmax >= wake size + 2 count.
 * anchors (in, may be NULL): the wake sizes after the four anchor steps max(64 (floor(first_step / 64) - 3 + q) - 1, 0),
 *   q = 0 .. 3 (the caller knows the wake size after every step it has run; step 0 = the initial wake); -1 = not given.
 *   Each step's launch geometry is derived from the wake size two 64-step periods back -- read from the device inside a
 *   call, given here across calls -- so a run's bits do not depend on where its calls begin.  Every given size is checked
 *   against state[0] (one or two vortices per step since the anchor), LUDVM_E_ARG otherwise.  NULL / all -1: the bounds
 *   restart at this call (results then depend on the chunking, to fp32 rounding, near the tile thresholds).
 * Synchronous: returns when the last step has finished.  `precision` selects the roll-up arithmetic as in
 * ludvm_wake_advect; the solve is float64.  From the symmetric-kernel threshold on, a step's chord sums and solve run on
 * a second stream beside the symmetric kernel.  The launch
 * geometry of every step is a function of the step number and of the simulation itself (never of host timing, nor -- with
 * `anchors` given -- of where the calls begin), and every sum is order-independent or done in a fixed order: two runs
 * return the same bits, however they are cut into calls. */
int ludvm_march_setup(ludvm_ctx* ctx, int npan, int ncoef, const double* scalars, const double* tables, const double* kin,
                      size_t kin_rows);
int ludvm_march_run(ludvm_ctx* ctx, long long first_step, long long count, int precision, double* state, double* rows,
                    double* hist, size_t hist_nmax, const long long* anchors);

/* ---- velocity probes: time series at fixed points, evaluated in the march (ABI 7) ----------------
 *
 * For time step i >= 1 and probe point p, (u, w)_i(p) is the field that convects the wake in step i, evaluated at p:
 * LUDVM.py:1095-1106 with xp, zp = p,
 *   induced_velocity(circulation_wake, xw, zw, p) + induced_velocity(circulation_foil, xa, za, p)
 * -- the sources are the wake BEFORE the Euler update of step i, including the vortices shed in step i at their placement,
 * and the bound vortices of step i at airfoil_gamma_points[i]; Vatistas core v_core (a probe that coincides with a vortex
 * gets 0 from it); no freestream term.  (The reference obtains such a signal by calling induced_velocity on the stored
 * history of every step, which a run too long for the dense history does not have.)  The sums are float64 whatever the
 * roll-up's precision, each formed in a fixed order that depends on the probe count and on the step's anchor-derived bound
 * of the wake size only: a run repeats bit for bit, however it is cut into calls.
 *
 * ludvm_march_set_probes: valid after ludvm_march_setup (LUDVM_E_STATE otherwise); count <= LUDVM_MARCH_MAX_PROBES points
 *   (x[k], z[k]); count = 0 removes the probes.  shift_x: NULL, or one x offset per kinematics row (shift_rows must equal
 *   ludvm_march_setup's kin_rows): in step i probe k sits at (x[k] + shift_x[i], z[k]) -- a frame that translates with the
 *   pivot.  Everything is validated (finite values included) before anything is changed: a call refused with LUDVM_E_ARG
 *   leaves the probes that were set -- and the rows of the last run -- as they were.  A call that passes validation and
 *   then fails in the runtime (LUDVM_E_HIP, LUDVM_E_NOMEM: the buffers are replaced) leaves the context WITHOUT probes.
 *   ludvm_march_setup forgets any probes.
 * ludvm_march_read_probes: copies the rows of the LAST ludvm_march_run call as u[rows][count], w[rows][count]; `rows` must
 *   equal that call's `count` (LUDVM_E_ARG otherwise); LUDVM_E_STATE when no probes are set, or when no ludvm_march_run call
 *   has succeeded since they were set.
 * Guarantee: with probes set, `rows`, `state`, `hist` and the resident wake of ludvm_march_run are bit-identical to a call
 *   without them (the probe kernels read the wake and write only buffers of their own). */
#define LUDVM_MARCH_MAX_PROBES 4096
int ludvm_march_set_probes(ludvm_ctx* ctx, const double* x, const double* z, size_t count, const double* shift_x,
                           size_t shift_rows);
int ludvm_march_read_probes(ludvm_ctx* ctx, double* u, double* w, size_t rows);

/* ---- wake integrals: class moments and kinetic energy of the vortex system (an addition to ABI 7: detect it by symbol) ----
 *
 * The SYSTEM of time step i >= 1 is what the probes see (above): the wake before the Euler update of step i, the vortices
 * shed in step i at their placement, the bound vortices of step i at airfoil_gamma_points[i], in the lab frame.  Float64.
 *
 * Moments: classes FREE (0), TEV (1), LEV (2), BOUND (3), signs slot 0: Gamma >= 0, slot 1: Gamma < 0; for every class and
 *   sign six sums over its vortices, in this order: the count (a double), sum G, sum G x, sum G z, sum G (x^2 + z^2),
 *   sum G^2 -- 48 doubles per step, sums[row][class][sign][moment].  Every workgroup owns a fixed chunk of source indices,
 *   combines its sums by a fixed tree, and the chunk partials are added in chunk order: a run repeats bit for bit however it
 *   is cut into calls.
 * Energy: W_i = 1/2 sum_a sum_b G_a G_b / (4 pi) ln((r_ab^2 + s_ab) / 2), s = sqrt(r^4 + v_core^4), over ALL sources of
 *   step i, the bound vortices and a = b included -- 1/2 sum_a G_a psi(x_a) with the stream function's pair term
 *   (ludvm_scalar_f64, LUDVM_FIELD_PSI).  The self part is ln(v_core^2 / 2) / (8 pi) times the row's sum of moment 6.
 *   Evaluated at the sampled steps first <= i < stop, (i - first) % every == 0, under a launch plan that is a function of
 *   the step's anchor-derived bound of the source count alone.
 *
 * ludvm_march_set_integrals: valid after ludvm_march_setup (LUDVM_E_STATE otherwise; LUDVM_E_STATE as well on a sharded or
 *   multi-device context).  on = 0 turns the observer off (nothing else is looked at).  tags[ntags]: the class, 0 .. 2, of
 *   every vortex of the resident wake in its stored order -- ntags must equal the wake the context holds (initial free
 *   vortices, or the wake of a run that is continued); the library tags the vortices every later step sheds and keeps the
 *   tags across the calls of one run.  energy_every = 0: no energy samples; otherwise energy_first >= 1,
 *   energy_stop > energy_first, energy_every >= 1.  LUDVM_E_ARG for a tag outside 0 .. 2, a wrong ntags or a malformed window;
 *   everything is validated before anything is changed: a refused call leaves the previous state -- and the rows of the
 *   last run -- as they were.  A call that passes validation and then fails in the runtime leaves the observer off.
 *   ludvm_march_setup forgets the observer; changing the resident wake other than through ludvm_march_run makes the next
 *   ludvm_march_run fail with LUDVM_E_STATE until the observer is set again.
 * ludvm_march_read_integrals: the rows of the LAST ludvm_march_run call, sums[rows][48] and energy[rows] (NaN for a step
 *   outside the window); `rows` must equal that call's `count` (LUDVM_E_ARG otherwise); LUDVM_E_STATE when the observer is
 *   off, or when no ludvm_march_run call has succeeded since it was set.
 * Guarantee: with the observer on, every other result of ludvm_march_run -- `rows`, `state`, `hist`, the resident wake, the
 *   probe rows, the tracer paths, the survey sums -- is bit-identical to a call without it (its kernels read the wake and
 *   write only buffers of their own). */
#define LUDVM_INTEGRAL_SUMS 48
int ludvm_march_set_integrals(ludvm_ctx* ctx, int on, const unsigned char* tags, size_t ntags, long long energy_first,
                              long long energy_stop, long long energy_every);
int ludvm_march_read_integrals(ludvm_ctx* ctx, double* sums, double* energy, size_t rows);

/* ---- passive tracers: particles advected inside the march (an addition to ABI 7: detect it by symbol) ----------
 *
 * A tracer is a probe that moves with what it measures.  Tracer m has a seed (xs, zs) and a release step r_m >= 1; with
 * shift[i] the frame offset of step i (0 without shift_x):
 *   step i <  r_m: held -- its position of step i is (xs + shift[i], zs), and it takes part in no pair sum;
 *   step i >= r_m: start = (xs + shift[i], zs) if i == r_m, otherwise its position after step i - 1;
 *                  its position after step i is  start + dt * (u, w)_i(start),
 * (u, w)_i being EXACTLY the probes' field above: the wake before the Euler update of step i with the vortices shed in step
 * i at their placement, plus the bound vortices of step i; Vatistas core, no freestream term, float64 whatever the roll-up's
 * precision.  With r_m = 1 and no shift this is, to rounding, the trajectory the reference gives a free vortex of zero
 * circulation seeded at the same point (path['FREE'], convected by LUDVM.py:1120-1127) -- without making the particle a
 * source of the roll-up, without growing the wake, and with release during the run.  Forward Euler, like the reference's
 * wake.  Every sum is formed in a fixed order that depends on the tracer count and on the step's anchor-derived bound of the
 * wake size only: a trajectory repeats bit for bit, however a run is cut into calls.
 *
 * ludvm_march_set_tracers: valid after ludvm_march_setup (LUDVM_E_STATE otherwise); count <= LUDVM_MARCH_MAX_TRACERS;
 *   count = 0 removes the tracers.  release: NULL (all 1), or one step >= 1 per tracer.  shift_x: NULL, or one x offset per
 *   kinematics row (shift_rows must equal ludvm_march_setup's kin_rows).  cur_x, cur_z: NULL (start from the seeds:
 *   (xs + shift_x[0], zs)), or the current positions -- what ludvm_march_tracer_state returned when a run is continued.
 *   record_steps[nrecord]: the time steps whose positions ludvm_march_run keeps for ludvm_march_read_tracers, strictly
 *   ascending, 1 <= step < kin_rows (nrecord = 0: none).  Everything is validated (finite values, release >= 1 included)
 *   before anything is changed: a call refused with LUDVM_E_ARG leaves the tracers that were set -- their positions and the
 *   rows of the last run -- as they were.  A call that passes validation and then fails in the runtime (LUDVM_E_HIP,
 *   LUDVM_E_NOMEM: the buffers are replaced) leaves the context WITHOUT tracers.  ludvm_march_setup forgets any tracers.
 *   A ludvm_march_run call that fails leaves the tracers' positions undefined: set them again.
 * ludvm_march_read_tracers: the recorded rows of the LAST ludvm_march_run call -- those of record_steps inside
 *   [first_step, first_step + count) -- as x[rows][count], z[rows][count] with their step numbers in steps_out[rows];
 *   *nrows_out = rows (also when rows_cap < rows, which is LUDVM_E_ARG and copies nothing; rows = 0 copies nothing and is
 *   LUDVM_OK).  LUDVM_E_STATE when no tracers are set, or when no ludvm_march_run call has succeeded since they were set.
 * ludvm_march_tracer_state: the current positions x[count], z[count] (after the last step run; held tracers at their seed
 *   with the last step's offset) -- for checkpoints and the final state.  LUDVM_E_STATE when no tracers are set.
 * Guarantee: with tracers set, `rows`, `state`, `hist`, the resident wake and any probe rows of ludvm_march_run are
 *   bit-identical to a call without them (the tracer kernels read the wake and write only buffers of their own).
 * Limits: one device (not sharded; a sweep has ludvm_ensemble_run_traced); float64 pair sums unless ludvm_march_set_tracer_precision
 *   says otherwise; tracers do not interact with the foil. */
#define LUDVM_MARCH_MAX_TRACERS 262144
int ludvm_march_set_tracers(ludvm_ctx* ctx, const double* seed_x, const double* seed_z, const long long* release, size_t count,
                            const double* shift_x, size_t shift_rows, const double* cur_x, const double* cur_z,
                            const long long* record_steps, size_t nrecord);
int ludvm_march_read_tracers(ludvm_ctx* ctx, double* x, double* z, size_t rows_cap, long long* steps_out, size_t* nrows_out);
int ludvm_march_tracer_state(ludvm_ctx* ctx, double* x, double* z);

/* ---- the tracers' pair sums in hi+lo fp32 (an addition to ABI 7: detect it by symbol) ---------------------------
 *
 * ludvm_march_set_tracer_precision: how the marched steps evaluate (u, w)_i at the released tracers.  0 (the default, and what
 *   ludvm_march_set_tracers and ludvm_march_setup reset it to): float64 pairs, everything above.  2: the pair arithmetic in
 *   fp32 on hi+lo positions -- every float64 source and tracer position v is split into hi = (float)v, lo = (float)(v - hi);
 *   dx = (xh_p - xh_s) + (xl_p - xl_s), dz likewise, and the pair in fp32 from there; the sources in tiles of 256 from each
 *   split's first one, a tile's pairs summed in fp32 (even and odd sources apart), the tile sums, the source splits, the
 *   Euler update and the positions in float64.  No origins, no classes, no fall-back: the error does not depend on where the
 *   wake is or on how far it has rolled up.  Within 2e-6 of max|u| of the float64 field (DESIGN.md section 4.9 has the
 *   figures).  A trajectory repeats bit for bit however a run is cut into calls, as the float64 ones do, but is not the
 *   float64 trajectory.  1 is left free (the survey's numbering: fp32 on local origins, which the tracers do not have).
 *   Valid only while tracers are set (LUDVM_E_STATE otherwise); a value other than 0 and 2 is LUDVM_E_ARG and changes nothing.
 *   It may be called between ludvm_march_run calls: the steps that follow use it.
 * Guarantee: as ludvm_march_set_tracers's -- every other result of ludvm_march_run keeps its bits -- and a context whose
 *   precision is 0 enqueues exactly what it enqueued before this entry existed. */
int ludvm_march_set_tracer_precision(ludvm_ctx* ctx, int precision);

/* ---- the tracers' deformation gradient (an addition to ABI 7: detect it by symbol) -------------------------------
 *
 * The sources of a step do not depend on a tracer, so the exact derivative of a released tracer's discrete map
 * start -> start + dt (u, w)_i(start) (LUDVM.py:1120-1127's forward-Euler step) with respect to its seed (X, Z) is one 2 x 2
 * product per step,  F <- (I + dt G_i(start)) F,  G_i = grad (u, w)_i in the closed form of ludvm_gradient_f64 (below) over the
 * step's sources.  F = [[dx/dX, dx/dZ], [dz/dX, dz/dZ]] is carried as four arrays F11 | F12 | F21 | F22; it is the identity while
 * a tracer is held and is reset to the identity at its release step.  The finite-time Lyapunov exponent of the flow map is
 * ln sigma_max(F) / T with T = dt (step - release + 1).
 *
 * ludvm_march_set_tracer_gradient: on = 1 makes the marched steps carry F (float64 tracers only: LUDVM_E_STATE while the
 *   tracer precision is 2, and ludvm_march_set_tracer_precision then refuses 2; ludvm_march_set_tracer_gradient_f32x2, below,
 *   is the hi+lo fp32 route); F is [4][count], or NULL for the identity (a run
 *   that is continued gives what ludvm_march_tracer_gradient_state returned).  on = 0 stops it.  Valid only while tracers are set
 *   (LUDVM_E_STATE otherwise); a flag other than 0 and 1 or an F that is not finite is LUDVM_E_ARG and changes nothing.
 *   ludvm_march_set_tracers and ludvm_march_setup reset it to off.
 * ludvm_march_read_tracer_gradient: the F rows of the steps ludvm_march_read_tracers returns for the last ludvm_march_run call,
 *   F [rows][4][count]; rows_cap, steps_out, nrows_out and the error codes as there (LUDVM_E_STATE also when the gradient is
 *   off or was switched on after that call).
 * ludvm_march_tracer_gradient_state: the current F [4][count].
 * Guarantee: the tracer positions and every other result of ludvm_march_run keep their bits (the gradient kernels run under the
 *   plain float64 tracers' launch plan and do their arithmetic for u and w operation for operation); F repeats bit for bit
 *   however a run is cut into calls; a context without the flag enqueues exactly what it enqueued before this entry existed. */
int ludvm_march_set_tracer_gradient(ludvm_ctx* ctx, int on, const double* F);
int ludvm_march_read_tracer_gradient(ludvm_ctx* ctx, double* F, size_t rows_cap, long long* steps_out, size_t* nrows_out);
int ludvm_march_tracer_gradient_state(ludvm_ctx* ctx, double* F);

/* ---- the tracers' deformation gradient in hi+lo fp32 (an addition to ABI 7: detect it by symbol) ------------------
 *
 * The two setters above each refuse while the other is on; this entry sets both.  Every marched step then evaluates (u, w)_i
 * AND the raw sums A, B, C of G_i at each released tracer in ONE walk over the step's sources (LUDVM.py:1095-1106's sources, as
 * for the probes), in packed fp32 on hi+lo positions: per pair the operations of precision 2 above for u and w, operation for
 * operation under the same launch plan, then the products of ludvm_gradient_f32x2 (below) from the same dx, dz, r2 and
 * reciprocal square root; a tile's 256 pairs summed in fp32 (even and odd sources apart), the tile sums, the source splits,
 * the Euler update, G_i and F <- (I + dt G_i) F in float64 as above (LUDVM.py:1120-1127's step and its exact derivative).
 *
 * ludvm_march_set_tracer_gradient_f32x2: sets the tracer precision to 2 and switches the deformation gradient on.  F has
 *   ludvm_march_set_tracer_gradient's contract: NULL is the identity, otherwise [4][count] finite values (LUDVM_E_ARG, and
 *   nothing changes, otherwise).  Valid only while tracers are set (LUDVM_E_STATE otherwise).  While it is on,
 *   ludvm_march_set_tracer_gradient(ctx, 0, NULL) switches the gradient off and leaves plain precision-2 tracers,
 *   ludvm_march_set_tracer_precision is LUDVM_E_STATE for either value, ludvm_march_read_tracer_gradient and
 *   ludvm_march_tracer_gradient_state answer as they do for the float64 gradient; ludvm_march_set_tracers and ludvm_march_setup
 *   reset everything.
 * Guarantee: the tracer positions are, bit for bit, those of plain precision-2 tracers, and every other result of
 *   ludvm_march_run keeps its bits; F repeats bit for bit however a run is cut into calls, but is not the float64 route's F: each
 *   component of G_i is within ludvm_gradient_f32x2's bound of the exact sum, wherever the wake is. */
int ludvm_march_set_tracer_gradient_f32x2(ludvm_ctx* ctx, const double* F);

/* ---- wake survey: running field moments inside the march (an addition to ABI 7: detect it by symbol) -----------
 *
 * The time-averaged wake on a survey grid without a time series: for survey point p, (u, w)_i(p) is EXACTLY the probes'
 * field above -- the reference's  induced_velocity(circulation_wake, xw, zw, p) + induced_velocity(circulation_foil, xa,
 * za, p)  of LUDVM.py:1095-1106 with xp, zp = p: the wake before the Euler update of step i with the vortices shed in step i
 * at their placement, plus the bound vortices of step i at airfoil_gamma_points[i]; Vatistas core, no freestream term,
 * float64 whatever the roll-up's precision.  The sampled steps are W = { i : first <= i < stop, (i - first) % every == 0 }
 * (stop is clipped to kin_rows).  In step i of W point k sits at (x[k] + shift_x[i], z[k]) (shift 0 without shift_x), and the
 * device adds to five raw float64 sums per point, sums[0..4][k] = sum u, sum w, sum u^2, sum w^2, sum u w; `samples` counts
 * the steps of W run so far.  Each point's sums are formed in step order by one lane, the source splits of a step are combined
 * in split order, no atomics; the splits depend on the point count and on the step's anchor-derived bound of the wake size
 * only: the sums repeat bit for bit, however a run is cut into ludvm_march_run calls.  Storage does not depend on the number
 * of steps; a step outside W launches nothing.
 *
 * ludvm_march_set_survey: valid after ludvm_march_setup (LUDVM_E_STATE otherwise, and on a sharded context);
 *   count <= LUDVM_MARCH_MAX_SURVEY; count = 0 removes the survey.  shift_x: NULL, or one x offset per kinematics row
 *   (shift_rows must equal ludvm_march_setup's kin_rows).  first >= 1, every >= 1.  sums: NULL (start from zero, samples is
 *   ignored), or [5][count] with samples >= 0 -- what ludvm_march_read_survey returned when a run is continued.  Everything is
 *   validated (finite values included) before anything is changed: a call refused with LUDVM_E_ARG leaves the survey that was
 *   set, and its sums, as they were.  A call that passes validation and then fails in the runtime (LUDVM_E_HIP,
 *   LUDVM_E_NOMEM: the buffers are replaced) leaves the context WITHOUT a survey.  ludvm_march_setup forgets any survey.  A
 *   ludvm_march_run call that fails leaves the sums undefined: set them again.
 * ludvm_march_read_survey: sums[5][count] and *samples as they stand, at any time after ludvm_march_set_survey (samples may be
 *   0).  LUDVM_E_STATE when no survey is set.
 * Guarantee: with a survey set, `rows`, `state`, `hist`, the resident wake, any probe rows and any tracer positions of
 *   ludvm_march_run are bit-identical to a call without it (the survey kernels read the wake and write only buffers of their
 *   own); a call without a survey enqueues exactly what it enqueued before.
 * Limits: one device (not sharded; a sweep has ludvm_ensemble_run_surveyed); float64 pair sums unless ludvm_march_set_survey_precision
 *   says otherwise; no freestream term. */
#define LUDVM_MARCH_MAX_SURVEY 1048576
int ludvm_march_set_survey(ludvm_ctx* ctx, const double* x, const double* z, size_t count, const double* shift_x,
                           size_t shift_rows, long long first, long long stop, long long every, const double* sums,
                           long long samples);
int ludvm_march_read_survey(ludvm_ctx* ctx, double* sums, long long* samples);

/* ---- the survey's pair sums in fp32 (an addition to ABI 7: detect it by symbol) --------------------------------
 *
 * ludvm_march_set_survey_precision: how the sampled steps evaluate (u, w)_i at the survey points.  0 (the default, and what
 *   ludvm_march_set_survey and ludvm_march_setup reset it to): float64 pairs, everything above.  1: the pair arithmetic in fp32
 *   on local origins -- the sources in tiles of 256 slots counted from slot 0, two origin classes of 128 per tile by index
 *   parity, each referred to the float64 position of its middle member; offsets, point differences (formed in float64, then
 *   rounded) and a class's 128 pairs in fp32; the class sums, the source splits, the five sums and everything else in
 *   float64.  A class whose extent (largest |offset| of a member) exceeds 300 v_core is evaluated in float64 instead.  Within
 *   1e-5 of max|u| of the float64 field for a wake of the march; a quarter of the cost where the classes are compact (a
 *   long run's rolled-up wake mostly is not: DESIGN.md section 4.11 has the figures).  The sums repeat bit for bit
 *   however a run is cut into calls, as the float64 ones do, but are not the float64 bits.
 *   Valid only while a survey is set (LUDVM_E_STATE otherwise); a value other than 0 and 1 is LUDVM_E_ARG and changes nothing.
 *   It may be called between ludvm_march_run calls: the steps that follow use it.
 * Guarantee: as ludvm_march_set_survey's -- every other result of ludvm_march_run keeps its bits -- and a context whose
 *   precision is 0 enqueues exactly what it enqueued before this entry existed. */
int ludvm_march_set_survey_precision(ludvm_ctx* ctx, int precision);

/* ---- bins of the survey: phase-locked (conditional) averages inside the march (an addition to ABI 7: detect it by symbol) ----
 *
 * A survey can carry nbins bins and a table with one bin per kinematics row.  In a sampled step i whose bin is b =
 * bin_of_row[i] >= 0, the five terms (u, w, u^2, w^2, u w) that the step adds to the plain sums -- the same (u, w)_i, formed
 * exactly as above -- are added to bin b's own five sums [5][count] as well, and bin b's count grows by one.  A sampled step
 * with bin -1 feeds the plain sums only; a step that is not sampled feeds nothing, whatever its entry.  With a table that
 * follows the phase of a periodic motion, bin b's sums give the phase-averaged field at that phase.
 * A binned step runs ONE finisher, as an unbinned one does (march_binned_survey_finish in place of march_survey_finish): the
 * partial slab is read once, the plain sums are updated with the same expressions in the same order, then the bin's block.
 * The host knows the bin of every step: no table goes to the device.  The bins' counts live on the host.
 *
 * ludvm_march_set_survey_bins: valid while a survey is set (LUDVM_E_STATE otherwise).  nbins = 0 removes the bins (the other
 *   arguments are not looked at).  Otherwise 1 <= nbins <= LUDVM_MARCH_MAX_SURVEY_BINS; nbins * count <=
 *   LUDVM_MARCH_MAX_SURVEY_BIN_POINTS (160 MiB of sums: a storage condition, not a measurement); rows must equal
 *   ludvm_march_setup's kin_rows; every entry of bin_of_row lies in [-1, nbins); sums ([nbins][5][count], finite) and counts
 *   ([nbins], >= 0) are both NULL (start from zero) or both given -- what ludvm_march_read_survey_bins returned when a run
 *   is continued.  Everything is validated before anything is changed: a call refused with LUDVM_E_ARG leaves the bins that
 *   were set, their sums and counts as they were.  A call that passes validation and then fails in the runtime leaves the
 *   context WITHOUT bins.  ludvm_march_set_survey and ludvm_march_setup forget the bins; ludvm_march_set_survey_precision
 *   does not.
 * ludvm_march_read_survey_bins: sums[nbins][5][count] and counts[nbins] as they stand, at any time after the set call.
 *   LUDVM_E_STATE when no bins are set.
 * Guarantees: with bins set, everything ludvm_march_run produced before keeps its bits, the plain survey sums and the sample
 *   count included; a context without bins enqueues exactly what it enqueued before.  Bin b's block equals, bit for bit, the
 *   plain sums of a survey that samples exactly bin b's steps: the same slab, the same plan for a given step, the same
 *   order.  The bin sums repeat bit for bit however a run is cut into ludvm_march_run calls (with sums and counts carried
 *   over where the context is set up again).  Both survey precisions are served: they differ in the partial kernel only. */
#define LUDVM_MARCH_MAX_SURVEY_BINS 64
#define LUDVM_MARCH_MAX_SURVEY_BIN_POINTS 4194304
int ludvm_march_set_survey_bins(ludvm_ctx* ctx, const int* bin_of_row, size_t rows, int nbins, const double* sums,
                                const long long* counts);
int ludvm_march_read_survey_bins(ludvm_ctx* ctx, double* sums, long long* counts);

/* ---- gradient sums of the survey: mean vorticity, strain and Q inside the march (an addition to ABI 7: detect it by symbol) ----
 *
 * In a sampled step i the closed-form gradient of the same field (u, w)_i at the same survey points -- the raw sums A, B, C of
 * ludvm_gradient_f64 (below) over the step's own sources [0, n + nfoil), added over the source splits in split order -- gives
 *   ux = -A / pi,  e = B / (2 pi) (= (du/dz + dw/dx) / 2),  om = -v_core^4 C / pi (= dw/dx - du/dz),
 *   Q = om^2 / 4 - ux^2 - e^2 (= -ux^2 - du/dz dw/dx)
 * and five more raw float64 sums per point grow in step order: gsums[0..4][k] = sum ux, sum e, sum om, sum om^2, sum Q.  om is
 * never formed as a difference of the two shear terms.  With bins, the sampled step's bin block bin_gsums[b][5][count] grows by
 * the same five terms formed the same way.  The sample count and the bin counts are the velocity sums' own: no second counter.
 * The gradient pair of kernels takes the place of the plain float64 pair under the same launch plan and does its arithmetic for
 * u and w operation for operation; a sampled step still runs one partial kernel and ONE finisher.
 *
 * ludvm_march_set_survey_gradient: on = 1 makes the sampled steps carry the gradient sums.  Valid while a survey is set in
 *   float64 precision: LUDVM_E_STATE when there is no survey, when the survey precision is 1, or when gsums is NULL although
 *   the survey or one of its bins already has samples (one count has to serve both).  gsums is [5][count], or NULL (start from
 *   zero); bin_gsums is [nbins][5][count], or NULL (start from zero) -- it is LUDVM_E_ARG when given without bins or without
 *   gsums.  A flag other than 0 and 1 is LUDVM_E_ARG.  Every value is checked finite (LUDVM_E_ARG) before anything changes: a
 *   refused call leaves the context as it was.  on = 0 removes the gradient sums (the other arguments are not looked at).
 *   ludvm_march_set_survey, ludvm_march_set_survey_bins and ludvm_march_setup reset it to off: the call order is survey, bins,
 *   gradient.  While it is on, ludvm_march_set_survey_precision(ctx, 1) is LUDVM_E_STATE and changes nothing.
 * ludvm_march_read_survey_gradient: gsums[5][count] and -- bin_gsums not NULL -- bin_gsums[nbins][5][count] as they stand, at any
 *   time after the set call.  LUDVM_E_STATE when the gradient sums are off; bin_gsums without bins is LUDVM_E_ARG.
 * Guarantees: with the gradient sums on, everything ludvm_march_run produced before keeps its bits, the plain and the binned
 *   velocity sums and their counts included; a context without the flag enqueues exactly what it enqueued before this entry
 *   existed.  Bin b's gradient block equals, bit for bit, the plain gradient sums of a survey that samples exactly bin b's steps.
 *   All sums repeat bit for bit however a run is cut into ludvm_march_run calls (carried over where the context is set up
 *   again). */
int ludvm_march_set_survey_gradient(ludvm_ctx* ctx, int on, const double* gsums, const double* bin_gsums);
int ludvm_march_read_survey_gradient(ludvm_ctx* ctx, double* gsums, double* bin_gsums);

/* ---- gradient sums of the survey in hi+lo fp32 (an addition to ABI 7: detect it by symbol) -----------------------
 *
 * The same ten sums with the pair arithmetic in fp32: every sampled step evaluates (u, w)_i AND the raw sums A, B, C at each
 * survey point in ONE walk over the step's sources, in packed fp32 on hi+lo positions -- the walk of
 * ludvm_march_set_tracer_gradient_f32x2 (above), per pair the operations of tracer precision 2 for u and w, then the products of
 * ludvm_gradient_f32x2 (below) from the same dx, dz, r2 and reciprocal square root; a tile's 256 pairs summed in fp32 (even and
 * odd sources apart), the tile sums, the source splits, ux, e, om, Q and all ten sums in float64 by the finishers of
 * ludvm_march_set_survey_gradient.  The walk takes the place of the survey's pair walk, so the VELOCITY sums of such a survey
 * are the fused walk's as well: hi+lo tier (within 2e-6 of max|u| of the float64 field), not the float64 survey's bits.  It is
 * not a survey precision: ludvm_march_set_survey_precision stays at 0, and no origins, classes or guard are involved -- the
 * error does not depend on where the wake is or on how far it has rolled up.
 *
 * ludvm_march_set_survey_gradient_f32x2: ludvm_march_set_survey_gradient's arguments without `on`, with its validation and its
 *   codes: LUDVM_E_STATE when there is no survey, when the survey precision is 1, or when gsums is NULL although the survey or
 *   one of its bins already has samples; LUDVM_E_ARG for bin_gsums without bins or without gsums and for a value that is not
 *   finite.  A refused call leaves the context as it was.  While the route is on, ludvm_march_set_survey_precision(ctx, 1) is
 *   LUDVM_E_STATE, ludvm_march_set_survey_gradient(ctx, 0, ..) removes the sums and the route,
 *   ludvm_march_set_survey_gradient(ctx, 1, ..) switches to the float64 pair, ludvm_march_read_survey_gradient answers as before;
 *   ludvm_march_set_survey, ludvm_march_set_survey_bins and ludvm_march_setup reset it: the call order stays survey, bins, gradient.
 * Guarantees: everything else ludvm_march_run produces keeps its bits (the survey reads the wake and writes buffers of its own);
 *   bin b's two blocks equal, bit for bit, the plain sums of such a survey that samples exactly bin b's steps; all sums repeat bit
 *   for bit however a run is cut into calls; each gradient term is within ludvm_gradient_f32x2's bound of the exact sum (DESIGN.md
 *   section 4.20).  A context without the route enqueues exactly what it enqueued before this entry existed. */
int ludvm_march_set_survey_gradient_f32x2(ludvm_ctx* ctx, const double* gsums, const double* bin_gsums);

/* ---- ensemble of small simulations: many whole runs of LUDVM.time_loop in one launch (LUDVM.py:597-1171) --------
 *
 * A parameter sweep (LESPcrit, k, alpha_max, dt, a gust vortex, 'Faure' / 'Ramesh') is `members` independent simulations,
 * each far too small to fill the device.  ludvm_ensemble_run runs them all in ONE kernel launch: one workgroup per member,
 * the whole time loop of LUDVM.py:659-1171 inside the kernel -- chord sums :746-751 / :921-931, Gamma_TEV :758-760 or Newton
 * :683-739, LESP test :781, the 2x2 system :944-954 or Newton :807-914, Fourier coefficients :765-773, bound vorticity
 * :987-1010, loads :1035-1090, roll-up :1095-1127, placement :672-681 / :788-800 -- all float64, with the pair arithmetic
 * of LUDVM_PREC_F64, so a member differs from a run of its own through ludvm_march_run(LUDVM_PREC_F64) by summation
 * order only.  Every sum is formed in an order that depends on the member's own data: a member's result bits do not
 * depend on `members`, on its index, on the other members or on where it ran, and a call repeats bit for bit.
 *
 * npan and ncoef are common to the batch; everything else is per member m (packed host arrays):
 *   scalars [members][12]     as ludvm_march_setup's; scalar_count = the number of doubles given, must be 12 members
 *   tables  [members][T]      as ludvm_march_setup's, T = 8 npan + ncoef npan + (ncoef - 1) npan
 *   kin     kin_rows rows     of 7 + 2 npan doubles as ludvm_march_setup's; member m owns rows [kin_off, kin_off + nt)
 *   init    [members][LUDVM_ENSEMBLE_INIT_HEAD + ncoef]
 *                             tev_x, lev_x, tev_z, lev_z of step 1 (:672-681, :788-800), LESPcrit, three reserved (0),
 *                             then the Fourier coefficients of step 0 (:645-646)
 *   free    3 free_count      the free vortices (:268-277): member m owns x[nfree] | z[nfree] | g[nfree] at double
 *                             3 free_off
 *   desc    [members][LUDVM_ENSEMBLE_DESC] integers
 *                             nt (time levels: steps 1 .. nt - 1 are run), kin_off (rows), nfree, free_off (vortices),
 *                             row_off (rows of `rows`), wake_off (doubles of `wakes`)
 *   snap_steps[nsnap]         strictly increasing steps >= 1, common to the batch, after which the wake is recorded;
 *                             steps beyond a member's nt - 1 are skipped for it
 * Outputs (host):
 *   rows    rows_count rows   of 12 + 2 ncoef + 2 npan doubles, exactly ludvm_march_run's row layout; member m's step s is
 *                             row row_off + s - 1
 *   wakes   wake_doubles      member m owns nsnap + 1 records of x[cap] | z[cap] | g[cap] from wake_off on, cap =
 *                             nfree + 2 (nt - 1): the wake in shedding order (free vortices first) after each snapshot step
 *                             and, last, after step nt - 1
 *   wake_n  [members][nsnap + 1]  the number of vortices in each record, -1 for a skipped snapshot.
 * Limits (ludvm_ensemble_limits returns them as max_steps, max_wake, max_snapshots): 1 <= npan <= 256, 4 <= ncoef <= 64,
 * nt - 1 <= LUDVM_ENSEMBLE_MAX_STEPS, cap <= LUDVM_ENSEMBLE_MAX_WAKE, nsnap <= LUDVM_ENSEMBLE_MAX_SNAPSHOTS: a member's
 * workgroup then stays around a second.  Everything -- the limits, every member's ranges inside the arrays given, the Newton
 * controls of a 'Ramesh' member -- is checked before anything is launched: LUDVM_E_ARG, the message names the member.
 * members = 0 is valid and does nothing.  Synchronous.  The call uses device buffers of its own: the resident wake, the
 * state of ludvm_march_setup, tuning, stream, shard and communicator of the context are as before it.  A sharded context
 * (ludvm_set_shard / ludvm_comm_init with world > 1) answers LUDVM_E_STATE: members are independent, a caller with several
 * devices splits the list. */
#define LUDVM_ENSEMBLE_MAX_STEPS 2048
#define LUDVM_ENSEMBLE_MAX_WAKE 8192
#define LUDVM_ENSEMBLE_MAX_SNAPSHOTS 1024
#define LUDVM_ENSEMBLE_INIT_HEAD 8
#define LUDVM_ENSEMBLE_DESC 6
int ludvm_ensemble_limits(ludvm_ctx* ctx, long long* limits3);
int ludvm_ensemble_run(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                       const double* tables, const double* kin, size_t kin_rows, const double* init, const double* free_xzg,
                       size_t free_count, const long long* desc, const long long* snap_steps, size_t nsnap, double* rows,
                       size_t rows_count, double* wakes, size_t wake_doubles, long long* wake_n);

/* ---- velocity probes in an ensemble: one set of points, a time series per member ----------------------------------
 *
 * ludvm_ensemble_run_probed is ludvm_ensemble_run with the probes of ludvm_march_set_probes evaluated inside the one launch.
 * The definition is the same (LUDVM.py:1095-1106 with xp, zp = the probe): for member m, step i >= 1 and probe p, the field
 * of the member's wake before the Euler update of step i -- the vortices shed in step i at their placement included -- plus
 * the bound vortices of step i; Vatistas core, no freestream term, float64.  Row 0 is the field of the member's free vortices.
 *   probe_x, probe_z [nprobe]   the points, common to the batch; nprobe <= LUDVM_ENSEMBLE_MAX_PROBES (a quarter of the solo
 *                               limit: a member's workgroup is meant to stay around a second)
 *   shift_x                     NULL, or one x offset per kinematics row (shift_rows must equal kin_rows): in step i of member
 *                               m probe k sits at (probe_x[k] + shift_x[kin_off + i], probe_z[k])
 *   probe_u, probe_w (host)     [kin_rows][nprobe]: member m's time level i is row kin_off + i, row 0 included; rows of `kin`
 *                               that no member owns are 0
 * Every other argument, output, limit and guarantee is ludvm_ensemble_run's, and those outputs are bit-identical to a call
 * without probes: the probe phase reads the member's wake and writes only the probe rows.  Each probe sum is formed in an
 * order that depends on nprobe and on the member's own wake size only, so a member's probe bits do not depend on the batch
 * either; a member differs from ludvm_march_run(LUDVM_PREC_F64) with the same probes by summation order only.  nprobe = 0 is
 * ludvm_ensemble_run itself (the probe arguments are not looked at).  Nothing is kept on the context: there is no state to
 * set, read back or forget.  Checked on the host before anything touches the device (LUDVM_E_ARG): nprobe over the limit,
 * null arrays, shift_rows != kin_rows, a point or offset that is not finite, and 2 * 8 * kin_rows * nprobe bytes of probe
 * rows over 1 GiB (the message gives the size: split the batch).  A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7 -- no existing signature or layout changes, LUDVM_ABI_VERSION and
 * LUDVM_ENSEMBLE_DESC stay as they are: a caller that may meet an older library of ABI 7 detects it by its symbol. */
#define LUDVM_ENSEMBLE_MAX_PROBES 1024
int ludvm_ensemble_run_probed(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                              const double* tables, const double* kin, size_t kin_rows, const double* init,
                              const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                              size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                              long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                              const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w);

/* ---- passive tracers in an ensemble: one set of seeds, paths for every member ---------------------------------------
 *
 * ludvm_ensemble_run_traced is ludvm_ensemble_run_probed (nprobe may be 0) with the tracers of ludvm_march_set_tracers
 * advected inside the one launch.  The definition is the same: tracer k of member m is held at (seed_x[k] + shift[i],
 * seed_z[k]) while i < release[k]; in step i >= release[k] it goes from `start` -- that seed if i == release[k], otherwise its
 * position after step i - 1 -- to start + dt (u, w)_i(start), (u, w)_i being the probes' field of step i of member m; Vatistas
 * core, no freestream term, float64, forward Euler.
 *   seed_x, seed_z, release [ntracer]  common to the batch; ntracer <= LUDVM_ENSEMBLE_MAX_TRACERS (a member's workgroup is
 *                               meant to stay around a second; a solo march takes LUDVM_MARCH_MAX_TRACERS); release >= 1 (a
 *                               step a member does not have: never released in it)
 *   tshift_x                    NULL, or one x offset per kinematics row (tshift_rows must equal kin_rows): shift[i] of member
 *                               m is tshift_x[kin_off + i]
 *   trec_steps [ntrec]          strictly increasing steps >= 1, common to the batch, whose positions are kept
 *   tracer_rows (host)          [members][ntrec + 1][2][ntracer] doubles (tracer_doubles = the number given): x row and z row
 *                               of all tracers after each recorded step (held ones at the seed of that step) and, record
 *                               ntrec, after the member's last step.  A record the member has no step for stays 0.
 * Every other argument, output, limit and guarantee is ludvm_ensemble_run_probed's, and those outputs -- the probe rows
 * included -- are bit-identical to a call without tracers: the tracer phase reads the member's wake and writes only the
 * member's tracer buffers.  Each tracer sum is formed in an order that depends on ntracer and on the member's own wake size
 * only, so a member's paths do not depend on the batch; a member differs from ludvm_march_run(LUDVM_PREC_F64) with the same
 * tracers by summation order only.  ntracer = 0 is ludvm_ensemble_run_probed itself (the tracer arguments are not looked
 * at).  Nothing is kept on the context.  Checked on the host before anything touches the device (LUDVM_E_ARG): ntracer over
 * the limit, null arrays, tshift_rows != kin_rows, a seed or offset that is not finite, release < 1, trec_steps not strictly
 * increasing or < 1, tracer_doubles too small, and members * (ntrec + 1) * 16 * ntracer bytes of records over 1 GiB (the
 * message gives the size: split the batch).  A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7: detect it by its symbol. */
#define LUDVM_ENSEMBLE_MAX_TRACERS 4096
int ludvm_ensemble_run_traced(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                              const double* tables, const double* kin, size_t kin_rows, const double* init,
                              const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                              size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                              long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                              const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w, const double* seed_x,
                              const double* seed_z, const long long* release, size_t ntracer, const double* tshift_x,
                              size_t tshift_rows, const long long* trec_steps, size_t ntrec, double* tracer_rows,
                              size_t tracer_doubles);

/* ---- wake survey in an ensemble: one set of points, time-averaged field for every member ---------------------------
 *
 * ludvm_ensemble_run_surveyed is ludvm_ensemble_run_traced (nprobe and ntracer may be 0) with the survey of
 * ludvm_march_set_survey accumulated inside the one launch.  The definition is the same: in a sampled step i of member m --
 * first <= i < min(stop, nt of m), (i - first) % every == 0 -- (u, w) is the probes' field of step i of member m at
 * (survey_x[k] + shift[i], survey_z[k]), and the member's five raw sums at point k grow by u, w, u^2, w^2, u w, in step
 * order; Vatistas core, no freestream term, float64.
 *   survey_x, survey_z [nsurvey]  common to the batch; nsurvey <= LUDVM_ENSEMBLE_MAX_SURVEY (a sampled step costs what a
 *                               tracer step of as many tracers costs; a solo march takes LUDVM_MARCH_MAX_SURVEY)
 *   sshift_x                    one x offset per kinematics row (sshift_rows = kin_rows): shift[i] of member m is
 *                               sshift_x[kin_off + i]; sshift_rows = 0: no offsets (sshift_x is not looked at)
 *   first, stop, every          the window, common to the batch; first >= 1, every >= 1 (a member the window misses keeps
 *                               sums of 0: the number of sampled steps is the caller's to count)
 *   survey_sums (host)          [members][5][nsurvey] doubles (survey_doubles = exactly that number): sum u, sum w, sum u^2,
 *                               sum w^2, sum u w of each member
 * Every other argument, output, limit and guarantee is ludvm_ensemble_run_traced's, and those outputs -- probe rows and tracer
 * records included -- are bit-identical to a call without a survey: the survey phase reads the member's wake and writes only
 * the member's sums.  (u, w) of a point are formed in the order a probe row of the same points is, which depends on nsurvey
 * and on the member's own wake size only, and each point's sums are added by one lane in step order: a member's sums do not
 * depend on the batch and repeat bit for bit; a member differs from ludvm_march_run(LUDVM_PREC_F64) with the same survey by
 * summation order only.  nsurvey = 0 is ludvm_ensemble_run_traced itself (the survey arguments are not looked at).  Nothing is
 * kept on the context.  Checked on the host before anything touches the device (LUDVM_E_ARG): nsurvey over the limit, null
 * arrays, sshift_rows neither 0 nor kin_rows, a point or offset that is not finite, first < 1, every < 1, survey_doubles !=
 * members * 5 * nsurvey, and members * 40 * nsurvey bytes of sums over 1 GiB (the message gives the size: split the batch).
 * A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7: detect it by its symbol. */
#define LUDVM_ENSEMBLE_MAX_SURVEY 4096
int ludvm_ensemble_run_surveyed(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars, size_t scalar_count,
                                const double* tables, const double* kin, size_t kin_rows, const double* init,
                                const double* free_xzg, size_t free_count, const long long* desc, const long long* snap_steps,
                                size_t nsnap, double* rows, size_t rows_count, double* wakes, size_t wake_doubles,
                                long long* wake_n, const double* probe_x, const double* probe_z, size_t nprobe,
                                const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w, const double* seed_x,
                                const double* seed_z, const long long* release, size_t ntracer, const double* tshift_x,
                                size_t tshift_rows, const long long* trec_steps, size_t ntrec, double* tracer_rows,
                                size_t tracer_doubles, const double* survey_x, const double* survey_z, size_t nsurvey,
                                const double* sshift_x, size_t sshift_rows, long long first, long long stop, long long every,
                                double* survey_sums, size_t survey_doubles);

/* ---- bins of the survey in an ensemble: phase-locked (conditional) averages for every member -------------------------
 *
 * ludvm_ensemble_run_surveyed_binned is ludvm_ensemble_run_surveyed with the bins of ludvm_march_set_survey_bins accumulated
 * inside the one launch.  In a sampled step i of member m whose entry b = bin_of_step[kin_off + i] is >= 0 the five terms u, w,
 * u^2, w^2, u w that have just been added to the member's plain sums at point k are added, by the same lane, with the same
 * expressions in the same order, to block b of the member's bin sums.
 *   bin_of_step [bin_rows]      one entry per kinematics row (bin_rows = kin_rows): the bin of step i of member m is
 *                               bin_of_step[kin_off + i], -1 for none; every entry lies in -1 .. nbins - 1.  Entries of steps
 *                               the window does not sample (row 0 included) are checked but not used; every member has a
 *                               table of its own, so one nbins serves members of different periods, dt and length
 *   nbins                       0 .. LUDVM_ENSEMBLE_MAX_SURVEY_BINS; 0 is ludvm_ensemble_run_surveyed itself (the bin arguments
 *                               are not looked at)
 *   bin_sums (host)             [members][nbins][5][nsurvey] doubles (bin_doubles = exactly that number).  The samples of a
 *                               bin are the caller's to count, from the table and the window
 * Every other argument, output, limit and guarantee is ludvm_ensemble_run_surveyed's, and those outputs -- rows, wake records,
 * wake_n, probe rows, tracer records and the plain survey sums -- keep the bits of the same call without bins: the bins add
 * five read-modify-writes per point to memory nothing else reads.  Block b of a member equals, bit for bit, the plain sums
 * the member gets from ludvm_ensemble_run_surveyed when the sampled steps are exactly bin b's steps ((u, w) of a step do
 * not depend on which other steps are sampled, and a block sees its steps in step order).  A member's bin sums do not depend
 * on the batch and repeat bit for bit; a member differs from ludvm_march_run(LUDVM_PREC_F64) with ludvm_march_set_survey_bins
 * by summation order only.  The library zero-fills both sum buffers on the call's stream and allocates everything before it
 * launches anything; nothing is kept on the context.  Checked on the host before anything touches the device (LUDVM_E_ARG):
 * nbins outside 0 .. 64, nbins > 0 with nsurvey = 0, null arrays, bin_rows != kin_rows, an entry outside -1 .. nbins - 1,
 * bin_doubles != members * nbins * 5 * nsurvey, and members * (nbins + 1) * 40 * nsurvey bytes of plain and bin sums over
 * 1 GiB (the message gives the size: split the batch).  A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7: detect it by its symbol. */
#define LUDVM_ENSEMBLE_MAX_SURVEY_BINS 64
int ludvm_ensemble_run_surveyed_binned(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars,
                                       size_t scalar_count, const double* tables, const double* kin, size_t kin_rows,
                                       const double* init, const double* free_xzg, size_t free_count, const long long* desc,
                                       const long long* snap_steps, size_t nsnap, double* rows, size_t rows_count, double* wakes,
                                       size_t wake_doubles, long long* wake_n, const double* probe_x, const double* probe_z,
                                       size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w,
                                       const double* seed_x, const double* seed_z, const long long* release, size_t ntracer,
                                       const double* tshift_x, size_t tshift_rows, const long long* trec_steps, size_t ntrec,
                                       double* tracer_rows, size_t tracer_doubles, const double* survey_x, const double* survey_z,
                                       size_t nsurvey, const double* sshift_x, size_t sshift_rows, long long first, long long stop,
                                       long long every, double* survey_sums, size_t survey_doubles, const int* bin_of_step,
                                       size_t bin_rows, int nbins, double* bin_sums, size_t bin_doubles);

/* ---- gradient sums of the survey in an ensemble: mean vorticity, strain and Q for every member -----------------------
 *
 * ludvm_ensemble_run_surveyed_graded is ludvm_ensemble_run_surveyed_binned (nbins = 0 allowed: no bins) with the gradient sums
 * of ludvm_march_set_survey_gradient accumulated inside the one launch.  The definition is the same: in a sampled step i of
 * member m the closed-form gradient of the survey's field -- the same sources, wake and bound vortices of step i -- at
 * (survey_x[k] + shift[i], survey_z[k]) gives, from the raw pair sums A, B, C of ludvm_gradient_f64,
 *   ux = -A / pi    e = B / (2 pi)    om = -vcore^4 C / pi    Q = om^2 / 4 - ux^2 - e^2
 * and the member's five gradient sums at point k grow by ux, e, om, om^2, Q, in step order, added by the lane that adds the
 * velocity terms.  In a step with a bin b the same five terms are added to block b of the member's bin gradient sums.
 *   grad_sums (host)            [members][5][nsurvey] doubles (grad_doubles = exactly that number): sum ux, sum e, sum om,
 *                               sum om^2, sum Q of each member
 *   bin_grad_sums (host)        [members][nbins][5][nsurvey] doubles (bin_grad_doubles = exactly that number); required exactly
 *                               when nbins > 0 (nbins = 0: NULL and 0)
 * grad_doubles = 0 with both arrays NULL is ludvm_ensemble_run_surveyed_binned itself.  Every other argument, output, limit and
 * guarantee is ludvm_ensemble_run_surveyed_binned's, and those outputs -- rows, wake records, wake_n, probe rows, tracer
 * records, the plain survey sums and the bin sums -- keep the bits of the same call without gradient sums: the pair walk forms
 * (u, w) with the same operations in the same order and carries three more accumulators.  Block b of a member's bin gradient
 * sums equals, bit for bit, the gradient sums the member gets when the sampled steps are exactly bin b's steps.  A member's
 * gradient sums do not depend on the batch and repeat bit for bit; a member differs from ludvm_march_run(LUDVM_PREC_F64) with
 * ludvm_march_set_survey_gradient by summation order only.  The library zero-fills all sum buffers on the call's stream and
 * allocates everything before it launches anything; nothing is kept on the context.  Checked on the host before anything
 * touches the device (LUDVM_E_ARG): grad_doubles > 0 with nsurvey = 0, grad_sums NULL, bin_grad_sums NULL with nbins > 0 or
 * given with nbins = 0, grad_doubles != members * 5 * nsurvey, bin_grad_doubles != members * nbins * 5 * nsurvey, and
 * members * (nbins + 1) * 80 * nsurvey bytes of plain, bin and gradient sums over 1 GiB (the message gives the size: split the
 * batch).  A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7: detect it by its symbol. */
int ludvm_ensemble_run_surveyed_graded(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars,
                                       size_t scalar_count, const double* tables, const double* kin, size_t kin_rows,
                                       const double* init, const double* free_xzg, size_t free_count, const long long* desc,
                                       const long long* snap_steps, size_t nsnap, double* rows, size_t rows_count, double* wakes,
                                       size_t wake_doubles, long long* wake_n, const double* probe_x, const double* probe_z,
                                       size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w,
                                       const double* seed_x, const double* seed_z, const long long* release, size_t ntracer,
                                       const double* tshift_x, size_t tshift_rows, const long long* trec_steps, size_t ntrec,
                                       double* tracer_rows, size_t tracer_doubles, const double* survey_x, const double* survey_z,
                                       size_t nsurvey, const double* sshift_x, size_t sshift_rows, long long first, long long stop,
                                       long long every, double* survey_sums, size_t survey_doubles, const int* bin_of_step,
                                       size_t bin_rows, int nbins, double* bin_sums, size_t bin_doubles, double* grad_sums,
                                       size_t grad_doubles, double* bin_grad_sums, size_t bin_grad_doubles);

/* ---- wake integrals in an ensemble: class moments and energy of every member's vortex system ---------------------------
 *
 * ludvm_ensemble_run_integrals is ludvm_ensemble_run_surveyed_graded (every observer optional: nprobe, ntracer, nsurvey, nbins
 * = 0 and the gradient arrays NULL are allowed) with the wake integrals of ludvm_march_set_integrals accumulated inside the one
 * launch.  The definition is the same, per member and in float64: the system of step i >= 1 of a member is the sources its
 * probes see -- its wake before the Euler update of step i, the vortices shed in step i at their placement, the npan bound
 * vortices of step i -- and for every class (0 FREE, 1 TEV, 2 LEV, 3 BOUND) and sign (slot 0: G >= 0, slot 1: G < 0) six sums
 * are formed: the count (as a double), sum G, sum G x, sum G z, sum G (x^2 + z^2), sum G^2.  At the sampled steps of the energy
 * (energy_first <= i < min(energy_stop, nt), (i - energy_first) % energy_every == 0) W = 1/2 sum_a G_a psi(x_a) over all those
 * sources, a = b included, psi being ludvm_scalar_f64's LUDVM_FIELD_PSI pair term with the member's own vcore: an
 * O((n + npan)^2) float64 pair sum with a logarithm per pair inside the member's workgroup (a member at the 8192-vortex limit:
 * about 7e7 pairs per sample).
 *   integral_sums (host)        [kin_rows][4][2][6] doubles (integral_doubles = exactly kin_rows * 48): a member's time level i
 *                               is row kin_off + i, like its probe rows; the launch writes rows 1 .. nt - 1, row 0 of a member
 *                               and rows no member owns are 0
 *   energy (host)               [kin_rows] doubles (energy_doubles = exactly kin_rows): W at the sampled steps, NaN elsewhere
 *                               (the entry fills the array with NaN before the launch)
 * integral_doubles = 0 with both arrays NULL (and energy_every = 0) is ludvm_ensemble_run_surveyed_graded itself: the same launch
 * and the same bits.  energy_every = 0 with energy NULL and energy_doubles = 0: no samples (energy_first / energy_stop are not
 * looked at).  Every other argument, output, limit and guarantee is ludvm_ensemble_run_surveyed_graded's, and those outputs keep
 * the bits of the same call without integrals: the two phases read the member's slab and write nothing but the two arrays.  The
 * order of every add depends on the member's own wake size and npan only (lane j adds the indices j, j + 256, ... in that
 * order, then a fixed tree; the energy walks the sources in index order and adds a lane's points in tile order): a member's rows
 * do not depend on the batch and repeat bit for bit, and a sampled step's W does not depend on the window.  A member differs
 * from ludvm_march_run(LUDVM_PREC_F64) with ludvm_march_set_integrals by summation order only.  Nothing is kept on the context.
 * Checked on the host before anything touches the device (LUDVM_E_ARG): an array NULL with its count non-zero (or given with a
 * count of 0), integral_doubles != kin_rows * 48, energy_doubles != kin_rows, energy (array, count or energy_every != 0) without
 * the integral sums, energy_first < 1, energy_every < 1 with an energy array (energy_every < 0 always), energy_stop <=
 * energy_first, and kin_rows * 49 * 8 bytes of rows over 1 GiB (split the batch).  A sharded context answers LUDVM_E_STATE.
 * The entry point is an addition to ABI 7: detect it by its symbol. */
int ludvm_ensemble_run_integrals(ludvm_ctx* ctx, size_t members, int npan, int ncoef, const double* scalars,
                                 size_t scalar_count, const double* tables, const double* kin, size_t kin_rows,
                                 const double* init, const double* free_xzg, size_t free_count, const long long* desc,
                                 const long long* snap_steps, size_t nsnap, double* rows, size_t rows_count, double* wakes,
                                 size_t wake_doubles, long long* wake_n, const double* probe_x, const double* probe_z,
                                 size_t nprobe, const double* shift_x, size_t shift_rows, double* probe_u, double* probe_w,
                                 const double* seed_x, const double* seed_z, const long long* release, size_t ntracer,
                                 const double* tshift_x, size_t tshift_rows, const long long* trec_steps, size_t ntrec,
                                 double* tracer_rows, size_t tracer_doubles, const double* survey_x, const double* survey_z,
                                 size_t nsurvey, const double* sshift_x, size_t sshift_rows, long long first, long long stop,
                                 long long every, double* survey_sums, size_t survey_doubles, const int* bin_of_step,
                                 size_t bin_rows, int nbins, double* bin_sums, size_t bin_doubles, double* grad_sums,
                                 size_t grad_doubles, double* bin_grad_sums, size_t bin_grad_doubles, double* integral_sums,
                                 size_t integral_doubles, double* energy, size_t energy_doubles, long long energy_first,
                                 long long energy_stop, long long energy_every);

/* ---- flow field: backs LUDVM.flowfield (LUDVM.py:1186-1298) -------------------------------- */

/* Grid targets generated on the device, x-major ravel like np.meshgrid(indexing='ij')
 * (LUDVM.py:1193-1195): point (i,j) = (xmin + i*dr, zmin + j*dr), i < nx, j < nz, index i*nz + j.
 * Sources are host float64 arrays (wake ++ foil as the caller gathered them, LUDVM.py:1202-1217).
 * Outputs u, w are host float32 arrays of nx*nz (fp32 arithmetic on local-origin positions: the sources as offsets
 * from the origin of their 256-source blocks, the grid points generated in float64 and referred to those origins).
 * d_u/d_w variants keep the result on the device for the vorticity stencil. */
int ludvm_flowfield_f32(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz,
                        const double* xs, const double* zs, const double* gs, size_t ns, double vcore,
                        float* u, float* w);
/* Velocity field and its vorticity (LUDVM.py:1224-1292) in one call: the stencil runs on the device on the
 * fields where they are, and u, w, ome (host float32, nx*nz each; ome may be NULL) come back together. */
int ludvm_flowfield_vorticity_f32(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz,
                                  const double* xs, const double* zs, const double* gs, size_t ns, double vcore,
                                  float* u, float* w, float* ome);
/* Rows [row_first, row_first + row_count) of that nx x nz grid only -- the same numbers, bit for bit, that the
 * whole-grid call returns for them (the grid coordinates are generated from the global row index and the split of the
 * sources into partial sums is planned from the whole grid, not from the block; with ome wanted, one halo row per
 * interior side is evaluated internally).  Outputs are row_count * nz each.  This is the unit a
 * multi-GPU flow field shards by: each GPU evaluates a block of rows, nothing is exchanged. */
int ludvm_flowfield_rows_f32(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz, size_t row_first,
                             size_t row_count, const double* xs, const double* zs, const double* gs, size_t ns,
                             double vcore, float* u, float* w, float* ome);
/* The same rows in float64 throughout -- pair sums, grid coordinates and the vorticity stencil with the mesh differences
 * taken from the mesh values, as the reference evaluates flowfield (LUDVM.py:1206, :1216-1217, :1224-1292): u, w and ome
 * then equal the reference's to rounding (~1e-13 of their maxima).  Outputs are host float64 arrays of row_count * nz;
 * the whole grid is row_first = 0, row_count = nx.  LUDVM.flowfield uses it when the run's precision is 'f64'. */
int ludvm_flowfield_rows_f64(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz, size_t row_first,
                             size_t row_count, const double* xs, const double* zs, const double* gs, size_t ns,
                             double vcore, double* u, double* w, double* ome);
/* Same as ludvm_flowfield_f32, device-resident fp32 sources and outputs (asynchronous). */
int ludvm_flowfield_dev_f32(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz,
                            const float* d_xs, const float* d_zs, const float* d_gs, size_t ns, float vcore,
                            float* d_u, float* d_w);
/* Vorticity dw/dx - du/dz on the uniform grid: centred differences inside, one-sided on edges and
 * corners (LUDVM.py:1224-1292).  Host float32 in/out, nx*nz each. */
int ludvm_vorticity_f32(ludvm_ctx* ctx, const float* u, const float* w, size_t nx, size_t nz, double dr,
                        float* ome);
int ludvm_vorticity_dev_f32(ludvm_ctx* ctx, const float* d_u, const float* d_w, size_t nx, size_t nz, float dr,
                            float* d_ome);

/* ---- stream function and analytic vorticity (an addition to ABI 7: detect it by symbol) --------------------------
 * Two scalar pair sums over the sources of the velocity sum (LUDVM.py:565-566), in float64 throughout.  For a target p and a
 * source j of circulation G_j: dx = xp - xj, dz = zp - zj, r2 = dx^2 + dz^2, s = sqrt(r2^2 + vcore^4) (the velocity sum's
 * denominator), a = (r2 + s) / 2, and
 *     LUDVM_FIELD_PSI:    psi(p)   = sum_j G_j / (4 pi) * ln(a_pj)
 *     LUDVM_FIELD_OMEGA:  omega(p) = -sum_j G_j * vcore^4 / (pi * s_pj^3)
 * d psi / dz = u and -d psi / dx = w of LUDVM.py:565-568 exactly; omega = dw/dx - du/dz of that field in closed form, with the
 * sign of the finite-difference ome_ff (LUDVM.py:1224-1292: a positive circulation turns clockwise, hence the minus), but
 * needing no grid.  vcore = 0 (inviscid): psi is the point
 * vortex's G / (2 pi) ln r in the same gauge and omega is 0.  A target on top of a source is finite when vcore > 0 (the term
 * is ln(vcore^2 / 2)); with vcore = 0 that pair gives what IEEE arithmetic gives (psi: -/+ inf or NaN, omega: NaN).
 * The sources are walked in the given order, in splits planned like the float64 velocity sum's and added in split order: the
 * results do not depend on how many workgroups ran.  Host arrays in and out; out has nt values.  nt = 0 is a no-op, ns = 0
 * writes zeros; an unknown kind or a null array with a non-zero count is LUDVM_E_ARG. */
enum { LUDVM_FIELD_PSI = 0, LUDVM_FIELD_OMEGA = 1 };
int ludvm_scalar_f64(ludvm_ctx* ctx, int kind, const double* xs, const double* zs, const double* gs, size_t ns,
                     const double* xt, const double* zt, size_t nt, double vcore, double* out);
/* The same sum on rows [row_first, row_first + row_count) of the grid of LUDVM.flowfield (LUDVM.py:1186-1298; the mesh of
 * ludvm_flowfield_rows_f64: point (i, j) = (xmin + i dr, zmin + j dr), index i nz + j), generated on the device, each coordinate by one fused multiply-add (one rounding).  out is a
 * host array of row_count * nz.  A block of rows is planned from the whole grid and carries the whole-grid call's bits.
 * row_count = 0 or nz = 0 is a no-op; rows outside the grid are LUDVM_E_ARG. */
int ludvm_flowfield_scalar_rows_f64(ludvm_ctx* ctx, int kind, double xmin, double zmin, double dr, size_t nx, size_t nz,
                                    size_t row_first, size_t row_count, const double* xs, const double* zs,
                                    const double* gs, size_t ns, double vcore, double* out);

/* ---- velocity gradient (an addition to ABI 7: detect it by symbol) -------------------------------------------------
 * The gradient of the velocity sum (LUDVM.py:565-568) in closed form, in float64 throughout.  With dx, dz, r2 and s as above and
 * y = 1 / s, three raw sums per target
 *     A = sum_j G_j r2 dx dz y^3,    B = sum_j G_j r2 (dx^2 - dz^2) y^3,    C = sum_j G_j y^3
 * give
 *     ux = du/dx = -A / pi                  (dw/dz = -ux: the field is divergence free)
 *     uz = du/dz = (B + vcore^4 C) / (2 pi)
 *     wx = dw/dx = (B - vcore^4 C) / (2 pi)
 * so that wx - uz is LUDVM_FIELD_OMEGA exactly, and Q = det grad u = -ux^2 - uz wx = omega^2 / 4 - (strain rate)^2 is positive in
 * a vortex core and negative in a shear layer.  One walk over the sources serves the three sums.  A target on top of a source
 * gives ux = 0, uz = -wx = G / (2 pi vcore^2) from that pair when vcore > 0, and IEEE's NaN when vcore = 0.  Splits, order and
 * reproducibility as ludvm_scalar_f64; host arrays in and out, ux, uz, wx of nt values each.  nt = 0 is a no-op, ns = 0 writes
 * zeros; a null array with a non-zero count is LUDVM_E_ARG. */
int ludvm_gradient_f64(ludvm_ctx* ctx, const double* xs, const double* zs, const double* gs, size_t ns, const double* xt,
                       const double* zt, size_t nt, double vcore, double* ux, double* uz, double* wx);
/* The same sums on rows [row_first, row_first + row_count) of the grid of LUDVM.flowfield (LUDVM.py:1186-1298), the mesh and
 * the rules of ludvm_flowfield_scalar_rows_f64: ux, uz, wx are host arrays of row_count * nz; a block of rows is planned from the
 * whole grid and carries the whole-grid call's bits. */
int ludvm_flowfield_gradient_rows_f64(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz,
                                      size_t row_first, size_t row_count, const double* xs, const double* zs,
                                      const double* gs, size_t ns, double vcore, double* ux, double* uz, double* wx);

/* ---- analytic vorticity and velocity gradient in hi+lo fp32 (an addition to ABI 7: detect it by symbol) ------------
 * LUDVM_FIELD_OMEGA of ludvm_scalar_f64 with the pair arithmetic in fp32: float64 arrays in and out, the same arguments.  Every
 * float64 coordinate is split into hi = (float)v and lo = (float)(v - hi); a difference is (hi_p - hi_s) + (lo_p - lo_s) and the
 * pair is fp32 from there (one unrefined reciprocal square root, G and vcore^4 rounded to float).  The sources go in tiles of 256
 * from the split's first one; within a tile the even sources are added in one fp32 accumulator and the odd ones in another, and
 * at the tile's end the even sum, then the odd sum, joins the target's float64 total.  No origins and no fall-back: the error is
 * about 1e-7 of the field's maximum (<= 2e-6, the hi+lo tier) wherever the sources lie.  The splits are a function of the target
 * and source counts alone and are added in split order: results repeat bit for bit.  nt = 0 is a no-op, ns = 0 writes zeros.
 * LUDVM_E_ARG: kind = LUDVM_FIELD_PSI ("the stream function has no fp32 route") or unknown, vcore not finite or below 1e-6 (this
 * is the viscous core's route: with a smaller core 1 / s^3 leaves fp32), a null array with a non-zero count. */
int ludvm_scalar_f32x2(ludvm_ctx* ctx, int kind, const double* xs, const double* zs, const double* gs, size_t ns,
                       const double* xt, const double* zt, size_t nt, double vcore, double* out);
/* The same sum on rows [row_first, row_first + row_count) of the grid, the mesh and the rules of ludvm_flowfield_scalar_rows_f64
 * (grid points generated in float64, then split): a block of rows is planned from the whole grid and carries the whole-grid
 * call's bits, and a grid point gets the bits ludvm_scalar_f32x2 gives the same point in an array of as many targets.
 * LUDVM_E_ARG as above, and for rows outside the grid. */
int ludvm_flowfield_scalar_rows_f32x2(ludvm_ctx* ctx, int kind, double xmin, double zmin, double dr, size_t nx, size_t nz,
                                      size_t row_first, size_t row_count, const double* xs, const double* zs,
                                      const double* gs, size_t ns, double vcore, double* out);
/* ludvm_gradient_f64 by the same scheme: the raw sums A, B, C in hi+lo fp32 pairs, ordered (G y) (y r2) (y dx dz) so that no
 * factor leaves fp32's range over |coordinates| <= 1e4 with vcore >= 1e-4; tiles, accumulators, splits and reproducibility as
 * ludvm_scalar_f32x2, and ux, uz, wx formed from the float64 totals as ludvm_gradient_f64 forms them.
 * LUDVM_E_ARG: vcore not finite or below 1e-6, a null array with a non-zero count. */
int ludvm_gradient_f32x2(ludvm_ctx* ctx, const double* xs, const double* zs, const double* gs, size_t ns, const double* xt,
                         const double* zt, size_t nt, double vcore, double* ux, double* uz, double* wx);
/* The same sums on rows of the grid, the rules of ludvm_flowfield_gradient_rows_f64 and the scheme of ludvm_gradient_f32x2: a
 * block of rows carries the whole-grid call's bits.  LUDVM_E_ARG as ludvm_gradient_f32x2, and for rows outside the grid. */
int ludvm_flowfield_gradient_rows_f32x2(ludvm_ctx* ctx, double xmin, double zmin, double dr, size_t nx, size_t nz,
                                        size_t row_first, size_t row_count, const double* xs, const double* zs,
                                        const double* gs, size_t ns, double vcore, double* ux, double* uz, double* wx);

/* ---- measurement ---------------------------------------------------------------------------- */

/* Probe of the symmetric kernel's fixed-point accumulation (the order-independent sums behind the roll-up of
 * LUDVM.py:1095-1127): units[i] = the 64-bit integer the kernel adds to an accumulator for the fp32 partial sum
 * values[i] at scale 2^scale_log2, i.e. trunc(values[i] * 2^scale_log2) -- exact for every |values[i] * 2^scale_log2|
 * < 2^63.  Host arrays; the conversion runs on the device with the kernel's own code. */
int ludvm_fixed_point_probe(ludvm_ctx* ctx, const float* values, size_t n, int scale_log2, long long* units);

/* Average device time (ms) of the pair kernel launches (main kernel only -- direct or symmetric --
 * not the split reduction / finisher) issued since the last call with reset != 0, measured with HIP events on the stream the
 * kernel is launched on; *launches = number of launches averaged.  Timing is off until
 * ludvm_kernel_timing(ctx, 1). */
int ludvm_kernel_timing(ludvm_ctx* ctx, int enable);
int ludvm_kernel_time_ms(ludvm_ctx* ctx, int reset, double* avg_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* LUDVM_HIP_H */
