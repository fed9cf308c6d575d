// Shared by the translation units of libludvm_hip.so: the context, error plumbing, the staging arena, and the internal
// host functions one unit offers the others.  Kernels are NOT here: templates and device helpers live in pair_kernels.hpp /
// pair_sym_kernels.hpp (includable anywhere; the symmetric launch rule, host and device, in sym_rule.hpp, the direct launch plan in plan_rule.hpp); every non-template kernel lives in a header that exactly one unit includes
// (sym_prepare_kernels.hpp -> launch.hip, induce_kernels.hpp -> induce.hip, wake_kernels.hpp -> wake.hip, march_kernels.hpp and
// ensemble_kernels.hpp -> march.hip, field_kernels.hpp -> flowfield.hip, order_kernels.hpp -> order.hip).
//
//   context.hip    lifecycle, streams, tuning, the error string, staging copies            (ludvm_create ... ludvm_set_self_order)
//   launch.hip     plans and launches of the pair kernels, direct and symmetric; timing    (internal; ludvm_kernel_time_ms)
//   comm.hip       the library's own RCCL communicator                                     (ludvm_comm_*)
//   order.hip      spatial order of unordered inputs                                       (ludvm_spatial_order)
//   induce.hip     stateless pair sums, the multi-GPU shard step's entry points            (ludvm_induce_*, ludvm_advect_dev_f32, ludvm_sym_*)
//   wake.hip       the resident wake and its roll-up                                       (ludvm_wake_*)
//   march.hip      the device-resident time march; the ensemble of small simulations       (ludvm_march_*, ludvm_ensemble_*)
//   flowfield.hip  flow-field grids, the vorticity stencil, stream function / vorticity    (ludvm_flowfield_*, ludvm_vorticity_*, ludvm_scalar_*, ludvm_gradient_*)
#pragma once
#pragma GCC visibility push(default)          // the C ABI is what the library exports; everything else is hidden (-fvisibility=hidden)
#include "../../include/ludvm_hip.h"
#pragma GCC visibility pop
#include "pair_kernels.hpp"
#include "pair_sym_kernels.hpp"
#include "march_types.hpp"
#include "spatial_order.hpp"

#include <hip/hip_ext.h>
#include <rccl/rccl.h>      // types and prototypes only: librccl is opened at run time by ludvm_comm_init (no link dependency)
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace ludvm;

// Measurement switches.  A PRODUCTION build reads two environment variables, neither of which can change a result bit:
// LUDVM_RCCL_LIB (which librccl to open) and LUDVM_COMM_FORCE (a one-rank communicator issues its collectives: tests).
// Everything else -- the A/B switches of rounds 1-3 (kernel variants, thresholds, chunking; six of them change the
// partition into fp32 partial sums and hence result bits) and the negative codes of ludvm_set_sym_tuning -- exists only in
// the measurement build, `make libludvm_hip_exp.so` (-DLUDVM_EXPERIMENTS), which tools/ and the tests of forced variants
// load.  In a production build the names below do not even reach the object file (tests/test_cabi.py checks).
#ifdef LUDVM_EXPERIMENTS
#define LUDVM_EXP_ENV(name) std::getenv(name)
#else
#define LUDVM_EXP_ENV(name) static_cast<const char*>(nullptr)
#endif

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
};

struct TimedLaunch {
  hipEvent_t e0, e1;
};

struct ludvm_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop;
  std::string err;

  int tune_tpl = 0;
  int tune_split = 0;
  int sym_mode = 1;
  int self_order = 1;                        // ludvm_set_self_order: 0 never, 1 by the rule (kSelfOrderMin), 2 always
  int tune_sym_t = 0, tune_sym_rsplit = 0;   // ludvm_set_sym_tuning (0 = heuristics)
  int xcd_run = 0;                           // chunks per run of the XCD placement (LUDVM_XCD_RUN; 0 = a launch's chunks / 8)
  long long sym_tail_items = kSymTailItems;  // mixed granularity: work kept for the fine-grained end (LUDVM_SYM_TAIL_ITEMS)
  int grid_kernel = 2;                       // flow-field grids (LUDVM_GRID_KERNEL): 1 = 4 points of a row per lane; 2 = patch,
                                             // 4 x 4 from 2^20 grid points and 2 x 4 below; 3 / 4 = always the 2 x 4 / 4 x 4 patch
  long long small_tile_max = kSmallTileMaxDefault;         // direct fp32 launches with at most this many sources use 256-source tiles
  bool sym_quad = true;                      // large symmetric launches: four I tiles per workgroup share each partner tile (LUDVM_SYM_QUAD=0: off)
  long long sym_quad_min_tiles = kSymQuadMinTiles;   //   ... from this many 512-vortex tiles on (LUDVM_SYM_QUAD_MIN_TILES)
  bool few_packed = true;                    // fp64 launches with <= 128 targets: several source splits per workgroup (LUDVM_FEW_PACKED=0: off)
  long long small_tile_max_f64 = kSmallTileMaxF64Default;     // fp64 launches with at most this many sources use 128-source tiles
                                             // (roll-up step 52 -> 26 us at 2400 vortices, 87 -> 72 at 8192 [MI355X])

  Buf part;   // partial slabs of the split reduction
  Buf acc;    // raw (u, w) sums of the symmetric kernel: [2][nt_pad] 64-bit fixed-point integers
  Buf symsc;  // SymScale of the current symmetric launch, followed by its NaN counter (long long)
  Buf arena;  // staging for the host-pointer entry points
  Buf orderws;  // spatial order of unordered inputs: two permutations, class extents, the sort's temporaries; or (self_order_f32)
                // one permutation, the three gathered fp32 arrays, the box and the sort's temporaries
  char* pin = nullptr;  // pinned host ring for small uploads from entry points that do not synchronize
  size_t pin_off = 0;
  char* pin_out = nullptr;  // pinned host buffer for small synchronous read-backs
  std::vector<double> pack;  // host staging of a time step's packed upload

  // resident wake (float64 master + fp32 mirrors)
  size_t wake_cap = 0, wake_n = 0;
  double *x64 = nullptr, *z64 = nullptr, *g64 = nullptr;
  float *xh = nullptr, *xl = nullptr, *zh = nullptr, *zl = nullptr, *g32 = nullptr;
  float *xr = nullptr, *zr = nullptr, *cx = nullptr, *cz = nullptr;   // local-origin offsets and block origins
  Mirrors mir() const { return Mirrors{xh, xl, zh, zl, xr, zr, cx, cz}; }

  // device-resident march (ludvm_march_setup / ludvm_march_run)
  Buf march_tab, march_kin, march_rows, march_state, march_hist;
  MarchSetup msetup{};
  size_t march_kin_rows = 0;
  double march_vcore = 0.0;
  bool march_ready = false;
  unsigned long long* progress = nullptr;      // host-mapped ring: slot s % kProgressRing = (s << 32 | wake size after step s)
  unsigned long long* progress_dev = nullptr;
  hipEvent_t march_ev[2] = {nullptr, nullptr};
  hipStream_t stream_b = nullptr;              // the solve chain beside the roll-up (overlapped march steps)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // velocity probes of the march (ludvm_march_set_probes): positions x[P] | z[P], the per-step x offsets, the partial slabs
  // of one step (a buffer of their own: the probe kernels never touch `part`), the rows of the last ludvm_march_run call
  Buf probe_xz, probe_shift, probe_part, probe_out;
  size_t probe_count = 0;                      // P (0: no probes)
  size_t probe_rows = 0;                       // steps of the last ludvm_march_run call that left rows (0: none to read)
  bool probe_shifted = false;
  // passive tracers of the march (ludvm_march_set_tracers): seeds x[M] | z[M], release steps [M] and the earliest release
  // of every tile, the per-step x offsets, the resident positions x[M] | z[M], the partial slabs of one step, the recorded
  // rows of the last ludvm_march_run call x[rows][M] | z[rows][M] -- buffers of the tracers' own, like the probes'
  Buf tracer_seed, tracer_release, tracer_shift, tracer_cur, tracer_part, tracer_out;
  size_t tracer_count = 0;                     // M (0: no tracers)
  bool tracer_shifted = false;
  bool tracer_ran = false;                     // a ludvm_march_run call has succeeded since the tracers were set
  std::vector<long long> tracer_record;        // steps whose rows are recorded, ascending
  std::vector<long long> tracer_rows;          // the recorded steps of the last ludvm_march_run call
  int tracer_precision = 0;                    // 0: float64 pair sums; 2: hi+lo fp32 (ludvm_march_set_tracer_precision)
  // the tracers' deformation gradient (ludvm_march_set_tracer_gradient): resident F11 | F12 | F21 | F22 [M], the five-column
  // slab of the gradient kernels, and the F rows of the last ludvm_march_run call [rows][4][M]
  Buf tracer_F, tracer_grad_part, tracer_F_out;
  bool tracer_gradient = false;
  bool tracer_grad_ran = false;                // the last ludvm_march_run call succeeded with the gradient on
  // wake survey of the march (ludvm_march_set_survey): points x[K] | z[K], the per-step x offsets, the five raw sums
  // [5][K], the partial slabs of one sampled step -- buffers of the survey's own, like the probes' and the tracers'
  Buf survey_xz, survey_shift, survey_sums, survey_part;
  size_t survey_count = 0;                     // K (0: no survey)
  bool survey_shifted = false;
  long long survey_first = 1, survey_stop = 0, survey_every = 1;   // sampled steps: first <= i < stop, (i - first) % every == 0
  long long survey_samples = 0;                // sampled steps the sums hold
  int survey_precision = 0;                    // 0: float64 pair sums; 1: fp32 on local origins (ludvm_march_set_survey_precision)
  // bins of the survey (ludvm_march_set_survey_bins): the bin of every time step on the host (-1: none), one block of five
  // sums per bin on the device [nbins][5][K], the samples of every bin on the host
  Buf survey_bin_sums;
  int survey_nbins = 0;                        // B (0: no bins)
  std::vector<int> survey_bin_of_row;          // [kinematics rows]
  std::vector<long long> survey_bin_samples;   // [B]
  // gradient sums of the survey (ludvm_march_set_survey_gradient): five more raw sums per point [5][K], the bins' blocks
  // [nbins][5][K] and the five-column partial slab of one sampled step; the sample counts are the velocity sums' own
  Buf survey_gsums, survey_bin_gsums, survey_grad_part;
  bool survey_gradient = false;
  // with survey_gradient: the five columns come from one walk in hi+lo fp32 under kObsSurveyF32's plan
  // (ludvm_march_set_survey_gradient_f32x2); survey_precision stays 0
  bool survey_gradient_f32x2 = false;
  // wake integrals of the march (ludvm_march_set_integrals): one class byte per wake vortex (sized for the run's cap when
  // the observer is set; the kernels add the tags of the vortices a step sheds), the chunk partials of one step
  // [chunks][48], the rows of the last ludvm_march_run call [rows][48]; the energy's slab [split][pad], its tile sums and
  // the call's samples [rows] -- buffers of the observer's own, like the probes'
  Buf integral_tags, integral_part, integral_out, energy_part, energy_tiles, energy_out;
  bool integrals_on = false;
  size_t integral_tagged = 0;                  // wake vortices that have a tag (= wake_n between the calls of a run)
  size_t integral_cap = 0;                     // wake vortices the tags and the energy's slab are sized for
  size_t integral_rows = 0;                    // steps of the last ludvm_march_run call that left rows (0: none to read)
  long long integral_first_step = 0;           // ... and its first step
  long long energy_first = 1, energy_stop = 0, energy_every = 0;   // sampled steps (every = 0: none)

  // ensemble of small simulations (ludvm_ensemble_run): inputs, the members' wake slabs, outputs -- buffers of its own, so
  // that a sweep leaves the resident wake and the march's state alone
  Buf ens_in, ens_work, ens_out;

  // sharded roll-up (ludvm_set_shard): this context evaluates tile block `shard_rank` of `shard_world`; the hook sums
  // the fixed-point accumulators over the contexts / processes before every Euler finisher
  int shard_rank = 0, shard_world = 1;
  long long shard_min_n = 0;    // wakes smaller than this are not worth a collective per step: every owner does them whole
  ludvm_allreduce_fn reduce_hook = nullptr;
  void* reduce_user = nullptr;
  void* ext_acc = nullptr;      // caller-owned accumulator memory (e.g. a torch tensor the hook all-reduces)
  size_t ext_acc_bytes = 0;
  // the library's own RCCL communicator (ludvm_comm_init): the all-reduce is then issued here, on the context's stream
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  bool comm_force = false;      // LUDVM_COMM_FORCE=1: issue the collectives even in a one-rank communicator (tests)

  // kernel timing
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<TimedLaunch> pool;
  double total_ms = 0.0;
  long long launches = 0;
};

namespace ludvm_host {

int fail(ludvm_ctx* c, int code, const std::string& msg);
int fail_hip(ludvm_ctx* c, const char* what, hipError_t e);

#define HIPCHK(c, call)                                     \
  do {                                                      \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return fail_hip((c), #call, e__); \
  } while (0)

#define CHK(call)                     \
  do {                                \
    int rc__ = (call);                \
    if (rc__ != LUDVM_OK) return rc__; \
  } while (0)

// ---- context.hip: device buffers and staging copies ---------------------------------------------------------------------
int ensure(ludvm_ctx* c, Buf& b, size_t bytes);
constexpr size_t kPinBytes = (size_t)1 << 20;
int h2d(ludvm_ctx* c, void* dst, const void* src, size_t bytes);
constexpr size_t kPinOutBytes = (size_t)1 << 16;
int d2h_small_sync(ludvm_ctx* c, const void* dsrc, size_t bytes, void** host_view);

// bump allocator over the staging arena
struct Arena {
  char* base;
  size_t off = 0;
  explicit Arena(void* p) : base(static_cast<char*>(p)) {}
  template <typename T>
  T* take(size_t n) {
    T* r = reinterpret_cast<T*>(base + off);
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
  static size_t need(size_t n, size_t elt) { return (n * elt + 255) & ~(size_t)255; }
};

inline unsigned blocks_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

inline bool valid_precision(int p) { return p == LUDVM_PREC_F32 || p == LUDVM_PREC_F32X2 || p == LUDVM_PREC_F64; }

// ---- launch.hip: plans and launches of the pair kernels -------------------------------------------------------------------
struct Plan {
  int tpl;
  int tile;
  int nsplit;
  long long chunk;
  long long nt_pad;
  dim3 grid;
};

// (the plan itself -- constants, arithmetic, which instantiation -- is plan_rule.hpp; make_plan hands it the context's settings)
Plan make_plan(const ludvm_ctx* c, long long nt_launch, long long ns, int precision, bool small_ok = true, long long plan_nt = 0,
               bool grid_patch = false);
int timed_begin(ludvm_ctx* c, TimedLaunch& t, bool& active);
int timed_end(ludvm_ctx* c, TimedLaunch& t, bool active);
int drain_timing(ludvm_ctx* c);
int launch_pair(ludvm_ctx* c, PairArgs a, const Plan& p, int precision, void* u, void* w);
int induce_device(ludvm_ctx* c, const PairArgs& a, long long nt, long long ns, int precision, void* u, void* w,
                  long long plan_nt = 0);
long long sym_threshold(const ludvm_ctx* c, bool march = false);
bool use_symmetric(const ludvm_ctx* c, long long n, double vc4, bool march = false);
bool use_self_order(const ludvm_ctx* c, long long n);
int sym_tile_t(const ludvm_ctx* c, long long n, bool hilo);

struct SymOperands {
  const float* x; const float* z; const float* g;
  const float* xl = nullptr; const float* zl = nullptr;     // hi+lo positions (T = 4)
  const float* cx = nullptr; const float* cz = nullptr;     // local origins: x, z are offsets from them
  long long* acc_u; long long* acc_w;
  const SymScale* scale; long long* bad;
};

int launch_sym_tiles(ludvm_ctx* c, int T, const SymOperands& o, long long n, long long i_first, long long i_count, double vc4,
                     const long long* n_dev = nullptr, long long n_lo = 0, bool sharded = false);
int acc_buffer(ludvm_ctx* c, long long nt_pad, long long** acc);
bool sharded_at(const ludvm_ctx* c, long long n);
void shard_tiles(const ludvm_ctx* c, long long ntiles, long long* first, long long* count);
inline SymScale* ctx_scale(ludvm_ctx* c) { return static_cast<SymScale*>(c->symsc.p); }
inline long long* ctx_bad(ludvm_ctx* c) { return reinterpret_cast<long long*>(static_cast<char*>(c->symsc.p) + 64); }
int launch_sym_prepare(ludvm_ctx* c, const float* g, long long n, double vc4, SymScale* scale, long long* bad);
int launch_sym(ludvm_ctx* c, SymOperands o, long long n, double vc4, long long* nt_pad_out, const long long** acc_out,
               const long long** bad_out, const long long* n_dev = nullptr, long long n_lo = 0);

// ---- comm.hip -----------------------------------------------------------------------------------------------------------
// Sum the accumulators (and their NaN counters) over all owners, in place and stream-ordered, before they are read.
int reduce_accumulators(ludvm_ctx* c, long long* acc, long long nt_pad);
// ludvm_destroy: the communicator goes before its stream and buffers do (no error to report to anyone)
void comm_release(ludvm_ctx* c);

// ---- order.hip ----------------------------------------------------------------------------------------------------------
constexpr size_t kOrderMin = 2048;     // below this many points on a side a stateless fp32 call does not run on local origins (see ludvm_induce_f64)
constexpr double kSmallSidePairsF64 = 268435456.0;   // 2^28 pairs: what float64 evaluates in ~0.2 ms [MI355X: 1.2-1.5e12 pairs/s]

struct OrderWs {
  unsigned* order[2];
  double* ext;
  double* sum;
  void* tmp;
  size_t tmp_bytes;
};

int order_workspace(ludvm_ctx* c, size_t nmax, OrderWs* w);
int class_extent_sum(ludvm_ctx* c, const OrderWs& w, const double* dx, const double* dz, const unsigned* order, size_t n, double* out,
                     double* box = nullptr);
int spatial_order_if_needed(ludvm_ctx* c, const OrderWs& w, int slot, const double* dx, const double* dz, size_t n,
                            const unsigned** order_out, double* mean_extent);
// d_k[i] = s_k[order[i]] for up to three float64 arrays (s2 / d2 may be NULL), and the way back for two: d_k[order[i]] = s_k[i]
int order_gather(ludvm_ctx* c, const double* s0, const double* s1, const double* s2, const unsigned* order, long long n, double* d0,
                 double* d1, double* d2);
int order_scatter(ludvm_ctx* c, const double* s0, const double* s1, const unsigned* order, long long n, double* d0, double* d1);
// Morton order of n plain fp32 device positions and the arrays gathered into it: x[k] = d_x[order[k]] ...  Everything is
// issued on the context's stream and lives in c->orderws until the next call that orders: no host synchronisation (once
// the workspace has its size), no host-side decision, nothing kept from call to call.
struct SelfOrdered {
  const unsigned* order;
  const float *x, *z, *g;
};
int self_order_f32(ludvm_ctx* c, const float* d_x, const float* d_z, const float* d_g, size_t n, SelfOrdered* out);
// fp32 on local origins resolves a pair difference to ~6e-8 of its class's extent; next to a core of radius v_core that is
// up to ~5e-8 extent / v_core of max|u| for an area-filling cloud [MI355X, profiles/r04_extent_rule_calibration.txt: 2e5 ... 2e6
// vortices in a 10 x 4 box, v_core 6.5e-4 ... 6.5e-2, Morton order: errors 0.5 ... 5e-8 per unit of extent / v_core, a tail
// statistic of the rare pairs closer than v_core that straddle two classes; 9e-6 at a ratio of 189, 1.2e-5 at 376] and ~1.5e-8
// for a shed wake, whose close pairs follow each other in the stored order (3.5e-6 at config 2's 230).  Beyond these ratios
// -- a set too SPARSE for its core, which no order can mend: a class is 128 points wherever they lie -- a stateless fp32
// call takes hi+lo positions (exact differences, +30 % time) and a flow field float64, so LUDVM_PREC_F32 keeps 1e-5 of
// max|u| for any input.
constexpr double kMaxExtentOverCore = 300.0;          // the given order was kept (compact as stored: sheet-like)
constexpr double kMaxExtentOverCoreCloud = 150.0;     // the set had to be put in Morton order (area-filling)
inline bool too_sparse(double mean_extent, bool reordered, double vcore) {
  return vcore > 0.0 && mean_extent > (reordered ? kMaxExtentOverCoreCloud : kMaxExtentOverCore) * vcore;
}

// ---- wake.hip -----------------------------------------------------------------------------------------------------------
int wake_grow(ludvm_ctx* c, size_t capacity);
int wake_refresh(ludvm_ctx* c, size_t first, size_t count, bool staged = false);
inline unsigned fin_blocks(long long n) { return (unsigned)((n + kFinBlock - 1) / kFinBlock); }
// (march) where a symmetric launch sized from an upper bound finds its scale and how small the wake may be
struct MarchSym { const SymScale* scale = nullptr; long long* bad = nullptr; long long n_lo = 0; bool march = false; };
// Roll-up launch on the resident wake (n vortices) with `nfoil` bound vortices already staged behind it
// at [n, n + nfoil) (masters and mirrors): pair kernel(s) + Euler finisher.  du/dw: optional device
// arrays receiving the induced velocities.  n_dev (march): the wake size is read on the device and `n` is
// only an upper bound that sizes the launch.
int advect_launch(ludvm_ctx* c, size_t n, const long long* n_dev, double dt, size_t nfoil, double vcore,
                  int precision, double* du, double* dw, TailDuty td = TailDuty{}, MarchSym ms = MarchSym{});

}  // namespace ludvm_host

using namespace ludvm_host;
