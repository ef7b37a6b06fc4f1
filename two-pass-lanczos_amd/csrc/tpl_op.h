// tpl_op.h — the handles behind the C ABI (include/tpl.h) and the helpers the host units
// share. Internal: tpl_operator.cpp (lifetime, buffers, schedule), tpl_dist.cpp (the
// rank-to-rank transport), tpl_passes.cpp (launch sequences, graph cache), the solver entry
// points — tpl_solvers.cpp (one column), tpl_solvers_multi.cpp (m functions of one b),
// tpl_solvers_batch.cpp (s right-hand sides), tpl_ftk_device.cpp (device f(T_k) probes), through
// tpl_solve.h (the steps they share) — and tpl_profile.cpp (timing, profiling, tuning) include it.
//
// Ownership: each handle's destructor releases what the handle owns, and nothing else
// does — tpl_*_destroy set the device, synchronise and delete, and a create that throws
// partway releases through the same destructor.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "tpl_batch.h"
#include "tpl_device.h"
#include "tpl_internal.h"
#include "tpl_launch.h"
#include "tpl_layout.h"
#include "tpl_partition.h"

typedef struct ncclComm* ncclComm_t;  // rccl/rccl.h's own typedef: only tpl_dist.cpp includes it

namespace tpl {

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      ::tpl::fail(e_ == hipErrorOutOfMemory ? TPL_ERR_OUT_OF_MEMORY : TPL_ERR_DEVICE,       \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                       \
  } while (0)

// keep_error: success leaves the thread's recorded error as it is (the destroy entry
// points: a binding's finalizer may run between a failed call and the caller's
// tpl_last_error_detail, and must not wipe what that call recorded).
template <class F>
tpl_status guarded(F&& f, bool keep_error = false) {
  try {
    f();
    if (!keep_error) set_last_error("");
    return TPL_OK;
  } catch (const Error& e) {
    // a failed HIP call leaves its status as the runtime's "last error", which the next
    // launch's hipGetLastError() check would report as its own: clear it here
    if (e.code == TPL_ERR_DEVICE || e.code == TPL_ERR_OUT_OF_MEMORY) (void)hipGetLastError();
    set_last_error(e.code, e.msg, e.det);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_last_error(TPL_ERR_OUT_OF_MEMORY, "host allocation failed", {});
    return TPL_ERR_OUT_OF_MEMORY;
  } catch (const std::exception& e) {
    set_last_error(TPL_ERR_INVALID_ARGUMENT, e.what(), {});
    return TPL_ERR_INVALID_ARGUMENT;
  }
}

// The device buffers of a Layout (and of its row order): rebuild_schedule replaces the set.
struct LayoutBufs {
  void *d_scol = nullptr, *d_sval = nullptr, *d_bcol = nullptr, *d_bval = nullptr;
  int32_t *d_srows = nullptr, *d_scbase = nullptr, *d_cbase = nullptr, *d_cwidth = nullptr;
  int32_t *d_bcbase = nullptr, *d_bhdr = nullptr;
  BinSeg* d_bseg = nullptr;
  double* d_P = nullptr;
  unsigned int* d_Pcnt = nullptr;
  int32_t *d_perm = nullptr, *d_iperm = nullptr;  // locality order (empty perm: nullptr)
  double* d_stage = nullptr;        // one host-order vector (host uploads / downloads)
  // the fused pass two's hub tables (Layout::fp2; nullptr: not eligible, or no open row)
  int32_t *d_hrow = nullptr, *d_hent = nullptr;
  double* d_hval = nullptr;
};

// The solver state of an operator, sized for kcap steps: ensure_state replaces the set.
struct SolverState {
  size_t kcap = 0;
  void* d_state = nullptr;  // flags | norms | alphas | betas | y | Pa | Pb | p2c | lu
  void* h_state = nullptr;  // pinned mirror of flags | norms | alphas | betas
  DevState S{};
  double* d_Pr = nullptr;   // reorthogonalisation partials (G * kcap)
  // Long-row cache (tpl_op_set_long_cache): yrows x n_long doubles, zeroed; row j - 1 holds
  // the long rows' sums (A v_j)_r of pass-one step j of the last tpl_lanczos_two_pass.
  // nullptr: yrows == 0
  double* d_ycache = nullptr;
  size_t yrows = 0;
  // the long rows' row indices, behind the sums in d_ycache's allocation; nullptr: the long
  // rows are the last rows (Layout::s_identity)
  int32_t* d_ylrow = nullptr;
};

// The buffers of a lock-step batch group (ensure_batch), for groups of nb columns and
// kcap steps under the current layout; nb == 0: none. Interleaved work vectors (ld x nb
// each): b, the ring R0..R2 (pass one's r, then pass two's v), W, x.
struct BatchBufs {
  int nb = 0;
  size_t kcap = 0;
  double* d_vecs = nullptr;
  double *b = nullptr, *R[3] = {nullptr, nullptr, nullptr}, *W = nullptr, *x = nullptr;
  void* d_state = nullptr;          // flags | norms | alphas | betas | y | p2c | Pa | Pb
  double* d_P = nullptr;            // the long rows' hand-off slots, nb per slice
  unsigned int* d_Pcnt = nullptr;   // and arrival counters of the batch's own
  double* d_stage = nullptr;        // n x nb, column-major: host B in, host X out
  // m functions per column (ensure_batch_multi), for this nb and kcap: mcols interleaved
  // result vectors (ld x nb each, one per function) and the coefficient table (function f,
  // column c at d_my + (f nb' + c) kcap for a group of nb' columns); nullptr: mcols == 0
  double *d_mx = nullptr, *d_my = nullptr;
  size_t mcols = 0;
  double* d_mstage = nullptr;       // n x (nb mstage_cols), column-major: host X out
  size_t mstage_cols = 0;
  // The group's long-row cache (tpl_op_set_long_cache_solvers bits 4 and 8): yrows x n_long
  // x nb doubles, zeroed; a group of nb' columns keeps the sums of its pass-one step j at
  // d_ycache + (j - 1) n_long nb', long row l's nb' sums adjacent. One allocation serves
  // every group of a call: each group's pass one rewrites the rows before its pass two reads
  // them. d_ylrow: the long rows' row indices behind the sums, or nullptr when they are the
  // last rows (as SolverState's). nullptr: yrows == 0
  double* d_ycache = nullptr;
  size_t yrows = 0;
  int32_t* d_ylrow = nullptr;
  // The per-(column, shift) state of tpl_lanczos_two_pass_batch_shifted_inv_tol's device path
  // (ensure_batch_stol), for kBatchNbMax columns, stol_m shifts and this kcap: one allocation
  // {tol, sig[m]} | per column {st[3 m], lu[4 kcap m], res[kcap m]} doubles | per column
  // {hits[m], nres[m]} int32, and the pinned mirror of flags | hits, nres | res of every
  // column; nullptr until the first call that takes that path. They come and go with the
  // batch buffers (free_batch)
  double* d_stol = nullptr;
  void* h_stol = nullptr;
  size_t stol_m = 0;
  BatchDev S{};
};

struct GraphExecDelete {
  void operator()(hipGraphExec_t g) const { hipGraphExecDestroy(g); }
};
using GraphExec = std::unique_ptr<hipGraphExec, GraphExecDelete>;

} // namespace tpl

// ---------------------------------------------------------------- objects
struct tpl_ctx_s {
  int device = 0;
  hipStream_t stream = nullptr;
  tpl_ctx_s() = default;
  tpl_ctx_s(const tpl_ctx_s&) = delete;
  ~tpl_ctx_s() {
    if (stream) hipStreamDestroy(stream);
  }
};

// A rank of a row-partitioned operator (tpl_dist_create*): its GPU and stream, and the
// transport of the per-step exchanges — RCCL over xGMI, or (tests) a host callback.
struct tpl_dist_s {
  tpl_ctx_s ctx;
  int rank = 0, nranks = 1;
  ncclComm_t comm = nullptr;
  tpl_allgather_fn host_fn = nullptr;
  void* host_user = nullptr;
  ~tpl_dist_s();  // the communicator, then (ctx) the stream; a plan's has neither
};

struct tpl_op_s {
  int device = 0;
  hipStream_t stream = nullptr;     // the ctx's or the dist's: not owned
  // this operator's rows, their CSR (h_rowptr / h_col / h_val keep the caller's order)
  // and its place in the partition; single GPU: dist == nullptr, n_glob == n
  tpl::RankPlan part;
  tpl_dist_s* dist = nullptr;
  bool eager = false;               // launch without graphs (host transport / no capture)
  double* d_yall = nullptr;         // nranks x y_ld1 (pass one: long-row partials + the
                                    // rank's short-chunk alpha partials, all-gathered
                                    // together); pass two: nranks x (n_long + 1)
  int32_t y_ld1 = 0;                // n_long + the most chunks of any rank
  int32_t pb_ld = 0;                // > 0: every rank's norm partials all-gathered (CsrDev::pb_ld)
  double* d_pball = nullptr;        // [nranks x pb_ld] gathered norm partials (pb_ld > 0)
  int32_t* d_nch = nullptr;
  int32_t* d_halo_send = nullptr;
  // dense operator (tpl_op_create_dense): the matrix whole on the device, row-major with the
  // padded leading dimension dense_ld (tpl_device.h DenseDev); every row is a long row of the
  // schedule, the layout holds no entries and bufs stays empty. false: a CSR operator
  bool dense = false;
  double* d_dense = nullptr;
  int64_t dense_ld = 0;
  tpl::SchedParams sp;
  tpl::Layout lay;
  tpl::LayoutBufs bufs;
  // vectors: b, R0..R2, W, x, V2_0..V2_2, tmp (n each, padded)
  double* d_vecs = nullptr;
  int64_t ld = 0;
  double *b = nullptr, *R[3] = {nullptr, nullptr, nullptr}, *W = nullptr, *x = nullptr,
         *V2[3] = {nullptr, nullptr, nullptr}, *tmp = nullptr;
  // gather sources of the SpMV: the same buffers on one GPU; with a partition, the
  // all-gathered vectors (nranks x ld) whose rank-th slice the local pointers view
  double *bG = nullptr, *RG[3] = {nullptr, nullptr, nullptr}, *V2G[3] = {nullptr, nullptr, nullptr},
         *tmpG = nullptr;
  double* d_rsum = nullptr;         // [nranks alpha totals][nranks norm totals] (partition)
  tpl::SolverState st;
  double* d_V = nullptr;    // standard-variant basis (n x vcols, ld = n); nullptr: vcols == 0
  size_t vcols = 0;
  // multi-function solves (ensure_multi): the result vectors X (xcols columns, ldx = ld
  // apart) and the coefficient table Y (xcols columns, ycap apart); nullptr: xcols == 0
  double *d_X = nullptr, *d_Y = nullptr;
  size_t xcols = 0, ycap = 0;
  // exp(t_i A) b at m times (ensure_exp_times): the times (TPL_MULTI_MAX doubles), the
  // kernel's hand-back entries (TPL_MULTI_MAX int32) and their pinned host mirror; nullptr
  // until the first tpl_lanczos_two_pass_exp_times / tpl_op_ftk_exp_times_device call
  double* d_exp_ts = nullptr;
  int32_t *d_exp_back = nullptr, *h_exp_back = nullptr;
  // the same for a batch group (ensure_exp_times_batch): the hand-back table of
  // k_ftk_exp_times_batch, kBatchNbMax * TPL_MULTI_MAX int32 (entry c m + i), and its pinned
  // host mirror; nullptr until the first tpl_lanczos_two_pass_batch_exp_times /
  // tpl_op_ftk_exp_times_batch_device call. The times are d_exp_ts
  int32_t *d_expb_back = nullptr, *h_expb_back = nullptr;
  // the inverse solve that stops at a residual tolerance (ensure_tol): {tol, res[tol_cap]}
  // on the device and the pinned mirror of flags | res; nullptr until the first
  // tpl_lanczos_two_pass_inv_tol call that takes the device path. tol_cap follows st.kcap
  double* d_tol = nullptr;
  void* h_tol = nullptr;
  size_t tol_cap = 0;
  // the step counts of a pass two with a per-column cut (ensure_col_steps: TPL_MULTI_MAX
  // int32, uploaded by the host-composed paths, written by k_ftk_inv_shifts on the device
  // path); nullptr until the first such call. No graph outlives it
  int32_t* d_col_steps = nullptr;
  // the shifted inverse solve that stops each shift at a tolerance (ensure_stol): one
  // allocation {tol, sig[m], st[3 m], lu[4 kcap m], res[kcap m]} doubles, then {hits[m],
  // nres[m]} int32, for stol_m shifts and stol_cap steps, and the pinned mirror of
  // flags | hits | nres | res; nullptr until the first call that needs them
  double* d_stol = nullptr;
  void* h_stol = nullptr;
  size_t stol_m = 0, stol_cap = 0;
  // the cut table of a batch-multi pass two with a cut per (column, function)
  // (ensure_batch_cut: kBatchNbMax * TPL_MULTI_MAX int32, entry c TPL_MULTI_MAX + f; uploaded
  // by the host-composed paths, written by k_ftk_inv_shifts on the device path); nullptr until
  // the first such call, never replaced
  int32_t* d_bcut = nullptr;
  tpl::BatchBufs bat;             // lock-step batch solves (ensure_batch)
  std::map<std::pair<int, size_t>, tpl::GraphExec> graphs;
  // device allocations of this operator (pointer -> bytes): tpl_op_device_bytes
  std::map<const void*, size_t> allocs;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // live timing (tpl_op_enable_timing): events recorded inside the captured passes
  bool timing = false;
  int device_ftk = 2;               // built-in inv on the device (one graph): 0 off, 1 on, 2 auto
  bool last_one_graph = false;      // the last tpl_lanczos_two_pass ran as one device graph
  // long-row cache: 0 off, 1 on within long_cache_budget bytes, 2 auto (the default budget)
  int long_cache = 2;
  uint64_t long_cache_budget = 0;
  // the solvers that use it when it is on (tpl_op_set_long_cache_solvers: TPL_LONG_CACHE_*)
  unsigned long_cache_solvers = TPL_LONG_CACHE_TWO_PASS;
  // set by a two-pass solver whose bit is in long_cache_solvers for the length of the call
  // (LongCacheScope): its passes one store the cache rows and its passes two read them — a
  // single column's in st, a batch group's in bat. Every other entry point leaves it false
  // and runs the full kernels
  bool use_long_cache = false;
  bool last_long_cache = false;     // the last pass two the operator ran read the cache
  // fused pass two (tpl_op_set_fused_pass_two): 0 off, 2 auto — whenever fused_p2 (below) holds
  int fused_p2 = 2;
  // the running call is tpl_lanczos_two_pass and asked for this many steps (LongCacheScope;
  // 0: any other entry point)
  size_t fused_call_k = 0;
  bool last_fused_p2 = false;       // the last pass two the operator ran was the fused one
  int64_t reorth_second = 0;        // second Gram-Schmidt passes of the last reorth solve
  // locality order (single GPU, tpl_op_set_reorder): the device works on P A P^T; vectors
  // cross the boundary through a gather (internal i <- caller's perm[i], back via iperm).
  int reorder = 2;                  // 0 off, 1 on, 2 auto (n <= kReorderAutoMaxRows)
  std::vector<int32_t> perm, iperm;
  double* d_Vext = nullptr;         // the callback's V_k view in the caller's order
  size_t vext_cols = 0;             // (nullptr: vext_cols == 0)
  hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t p2_launches = 0;
  // live timing of pass one's kernels: start stamps of the last timed solve's sampled
  // launches (2 kStampSteps + 1), tpl_op_step_samples
  unsigned long long* d_stamps = nullptr;
  int32_t p1_samples = 0;
  // tpl_plan_create: the host half of an operator only (rows, order, layout), for the
  // oracle's reduction order without a GPU; every device entry point refuses it
  bool plan_only = false;
  std::unique_ptr<tpl_dist_s> plan_dist;  // a plan's rank and rank count (no transport)
  // Graphs, every entry of allocs, the pinned mirror, the events. A host-only plan holds
  // none of them and its destructor makes no HIP call.
  ~tpl_op_s();
};

namespace tpl {

// ---- operator (tpl_operator.cpp) ---------------------------------------------------
int long_epi_blocks(const tpl_op_s* op);
CsrDev csr_dev(const tpl_op_s* op, bool pass1 = false);
inline void drop_graphs(tpl_op_s* op) { op->graphs.clear(); }
// The kernels' view of a dense operator's storage under its current slice count.
inline DenseDev dense_dev(const tpl_op_s* op) {
  return DenseDev{op->d_dense, op->dense_ld, (int32_t)op->part.n, op->lay.nslices};
}
// What a dense operator does not run: refused before any device work.
inline void refuse_dense(const tpl_op_s* op, const char* what) {
  if (op->dense) fail(TPL_ERR_UNSUPPORTED, std::string(what) + " of a dense operator");
}
// Leading dimension of the dense storage: whole 128-B lines per row, an odd number of them
// (rows a power of two apart would start on the same memory channel).
inline int64_t dense_stride(int64_t n) { return 16 * (((n + 15) / 16) | 1); }

// Device memory of an operator, accounted per allocation (tpl_op_device_bytes): the one
// allocation path. Test hook: with TPL_TEST_ALLOC_CAP=<bytes> set (read on every call), a
// request that would take the accounted bytes above the cap is refused on the host as
// hipErrorOutOfMemory is reported, and never reaches the runtime.
void dev_alloc_bytes(tpl_op_s* op, void** p, size_t bytes);
template <class T>
void dev_alloc(tpl_op_s* op, T** p, size_t bytes) {
  dev_alloc_bytes(op, reinterpret_cast<void**>(p), bytes);
}
template <class T>
void dev_free(tpl_op_s* op, T*& p) {
  if (!p) return;
  op->allocs.erase(p);
  hipFree(p);
  p = nullptr;
}
// Zeroes of a new allocation, in the order of the operator's stream. That stream is
// non-blocking: a hipMemset on the null stream is ordered neither with it nor, for device
// memory, with the host, so it can land after the first upload the call enqueues into the
// same buffer (seen: the cuts of a first tpl_lanczos_pass_two_multi_cut read back as zeros).
inline void dev_zero(tpl_op_s* op, void* p, size_t bytes) {
  if (bytes) HIPCHK(hipMemsetAsync(p, 0, bytes, op->stream));
}
uint64_t device_bytes(const tpl_op_s* op);

void rebuild_schedule(tpl_op_s* op, const SchedParams& cand, int reorder);
void ensure_state(tpl_op_s* op, size_t k, bool reorth = false);
// The long-row cache's budget rule (tpl_op_set_long_cache): steps cached for an operator of
// n rows, n_long of them long, whose state holds kcap steps.
uint64_t long_cache_default_budget(int64_t n);
uint64_t long_cache_rows(int mode, uint64_t budget_bytes, int64_t n, int64_t n_long, uint64_t kcap);
// Steps the operator's cache holds for the running two-pass solve (0: not in use): of a
// single column, and of a batch group.
inline size_t long_cache_steps(const tpl_op_s* op) {
  return op->use_long_cache ? op->st.yrows : 0;
}
// Pass two of the running call runs fused (k_p2_hub + k_p2_rows, tpl_k_p2_fused.hip) instead
// of its step launches: the mode is on, the layout's rows decouple (Layout::fp2) with the long
// rows last, the call is a single-GPU tpl_lanczos_two_pass, and the long-row cache holds every
// step the call asked for.
inline bool fused_p2(const tpl_op_s* op) {
  return op->fused_p2 != 0 && op->lay.fp2.eligible && op->lay.s_identity && !op->dist &&
         op->fused_call_k > 0 && long_cache_steps(op) >= op->fused_call_k;
}
inline size_t batch_cache_steps(const tpl_op_s* op) {
  return op->use_long_cache ? op->bat.yrows : 0;
}
void ensure_basis(tpl_op_s* op, size_t cols);
// The m result vectors and the m x kcap coefficient table of a multi-function solve, for
// the state's current kcap (ensure_state first). They grow with m and kcap; growing drops
// the cached graphs.
void ensure_multi(tpl_op_s* op, size_t m);
// The two small buffers of the exp-times calls (op->d_exp_ts, op->d_exp_back) and the pinned
// mirror of the second: allocated on the first such call, counted in device_bytes, freed
// with the operator. No graph holds them.
void ensure_exp_times(tpl_op_s* op);
// The batch sibling's buffers: the times (op->d_exp_ts, shared with ensure_exp_times:
// TPL_MULTI_MAX doubles, allocated by whichever comes first) and the hand-back table
// (op->d_expb_back, kBatchNbMax * TPL_MULTI_MAX int32 = 1,024 bytes) with its pinned mirror.
// Allocated on the first batch exp-times call, counted in device_bytes, freed with the
// operator. No graph holds them.
void ensure_exp_times_batch(tpl_op_s* op);
// The tolerance and residual history of tpl_lanczos_two_pass_inv_tol's device path
// (op->d_tol: 1 + kcap doubles) and the pinned mirror of flags | res, for the state's current
// kcap (ensure_state first). Counted in device_bytes, freed with the operator; replacing them
// drops the cached graphs, which hold the pointer (the first allocation drops nothing).
void ensure_tol(tpl_op_s* op);
// The device table of column step counts (op->d_col_steps: TPL_MULTI_MAX int32, 256 bytes),
// allocated on the first call that cuts pass two per column, counted in device_bytes, freed
// with the operator.
void ensure_col_steps(tpl_op_s* op);
// The per-shift state of tpl_lanczos_two_pass_shifted_inv_tol's device path and of
// tpl_op_ftk_inv_shifts_device (op->d_stol, op->h_stol) for m shifts and the state's current
// kcap (ensure_state first): 8 (1 + m (4 + 5 kcap)) + 8 m bytes, counted in device_bytes.
// They grow with m and follow kcap; replacing them drops the cached graphs, which hold the
// pointers (the first allocation drops nothing). -> the kernels' view for this call's m.
launch::ShiftTol ensure_stol(tpl_op_s* op, size_t m);
// The interleaved work vectors, per-column state and hand-off buffers of a batch group of
// nb (2 or 4) columns and k steps, allocated on demand and counted in device_bytes. They
// grow with nb and k; growing drops the cached graphs. A layout rebuild frees them
// (free_batch): the next batch call allocates for the new layout. The group's long-row
// cache comes and goes with them, and is resized alone (built aside; the graphs dropped)
// when only the cache's mode, budget or solver mask changed.
void ensure_batch(tpl_op_s* op, int nb, size_t k);
void free_batch(tpl_op_s* op);
// The m result vectors and the coefficient table of a batch-multi group, for the batch
// buffers' current nb and kcap (ensure_batch first), allocated on first use and counted
// in device_bytes. They grow with m (growing drops the cached graphs); whatever frees or
// regrows the batch buffers frees them (free_batch). stage: also the host-side staging
// block of the n x (nb m) result.
void ensure_batch_multi(tpl_op_s* op, size_t m, bool stage);
// The cut table of a batch-multi pass two (op->d_bcut: kBatchNbMax * TPL_MULTI_MAX int32,
// 1,024 bytes), allocated on the first call that cuts a group's pass two per (column,
// function), counted in device_bytes, freed with the operator.
void ensure_batch_cut(tpl_op_s* op);
// The per-(column, shift) state of tpl_lanczos_two_pass_batch_shifted_inv_tol's device path
// (op->bat.d_stol, op->bat.h_stol) for m shifts and the batch buffers' current kcap
// (ensure_batch first): 8 (1 + m) + kBatchNbMax (8 m (3 + 5 kcap) + 8 m) bytes, counted in
// device_bytes. They grow with m; replacing them drops the cached graphs, which hold the
// pointers (the first allocation drops nothing). -> the kernels' view for this call's m.
launch::BatchShiftTol ensure_batch_stol(tpl_op_s* op, size_t m);
double* ensure_view(tpl_op_s* op, size_t cols);
// Per-step second-pass records of the selective re-orthogonalisation (slot j - 1: step j).
int* reorth_records(const tpl_op_s* op);
void set_device(const tpl_op_s* op);
inline void sync_checked(tpl_op_s* op) { HIPCHK(hipStreamSynchronize(op->stream)); }
void check_b(const tpl_op_s* op, const double* b, int64_t b_len);
void upload_vec(tpl_op_s* op, double* dst, const double* src, int mem);
void download_vec(tpl_op_s* op, double* dst, const double* src, int64_t cols, int mem);
// `cols` device vectors `lds` apart (internal order) out to the caller's n x cols matrix
// (ld = n, the caller's order), a column at a time.
void download_cols(tpl_op_s* op, double* dst, const double* src, int64_t lds, int64_t cols,
                   int mem);
void set_stride(tpl_op_s* op);
std::unique_ptr<tpl_op_s> make_op(tpl_ctx_s* ctx, tpl_dist_s* dist, RankPlan&& part);
void init_op(tpl_op_s* op);

// ---- dist (tpl_dist.cpp): the exchanges of a row-partitioned operator ---------------
void dist_allgather(tpl_op_s* op, double* base, size_t count);
void halo_pack(tpl_op_s* op, double* G);
void gather_vec(tpl_op_s* op, double* G);
void enqueue_p1_exchange_a(tpl_op_s* op, const CsrDev& A);
void enqueue_p1_exchange_norm(tpl_op_s* op, const CsrDev& A, double* G);
void enqueue_p2_exchange(tpl_op_s* op, int j);

// ---- passes (tpl_passes.cpp) -------------------------------------------------------
// Live timing of pass one's kernels (tpl_op_step_samples): in a timed solve, workgroup 0
// of the k_p1_spmv and k_p1_axpy launches of kStampSteps consecutive middle steps (and of
// the next step's k_p1_spmv) records its start on the 100 MHz real-time clock; a kernel's
// launch time is the start-to-start interval, boundary included (as pass two's figure).
constexpr int kStampSteps = 8;
// Which built-in f(T_k) a solve evaluates on the device (kDevHost: none, f runs on the host).
enum DevF { kDevHost = -1, kDevInv = 0, kDevExp = 1 };

struct HostDecomp {
  int32_t flags[kFlagBytes / 4];
  double b_norm;
  const double* alphas;
  const double* betas;
  size_t steps;
};

bool use_graphs();
// `enqueue` captured on the operator's stream into an executable graph. nullptr: a
// partitioned operator's transport refused capture (or the graph could not be
// instantiated) and the operator launches eagerly from now on (op->eager); any other
// failure throws. No graph object outlives a failure.
GraphExec capture_graph(tpl_op_s* op, const std::function<void()>& enqueue);
void enqueue_reorth(tpl_op_s* op, int j, int mode);
void enqueue_p1_prologue(tpl_op_s* op);
void enqueue_p1_step(tpl_op_s* op, int j, int k, double* Vcol, bool elim = false,
                     unsigned long long* st1 = nullptr, unsigned long long* st2 = nullptr,
                     double* ycrow = nullptr);
void launch_p2_step(tpl_op_s* op, const CsrDev& A, int j, int t, int nflush, double* Vcol);
void launch_bp2_step(tpl_op_s* op, const CsrDev& A, int nb, int j);
void enqueue_pass2(tpl_op_s* op, size_t steps, double* Vout);
void enqueue_ftk_only(tpl_op_s* op, size_t k, int f, int scale);
void run_pass_one(tpl_op_s* op, const double* b, size_t k, int mem, bool storeV, int reorth,
                  bool elim = false);
void run_pass2(tpl_op_s* op, size_t steps);
// Pass two for the m coefficient columns of op->d_Y into op->d_X (ensure_multi): one graph
// per (steps, m).
void run_pass2_multi(tpl_op_s* op, size_t steps, size_t m);
// The same with a per-column cut: column i takes the terms below op->d_col_steps[i] only
// (k_p2_xacc_cut; 1 <= that count <= steps), so it holds the bits of the single pass two at
// that many steps. One graph per (steps, m): the counts are device data.
void run_pass2_multi_cut(tpl_op_s* op, size_t steps, size_t m);
// One group of a batch solve (ensure_batch first; the group's b interleaved in op->bat.b):
// pass one for the nb columns in lock-step, one graph per (k, nb); pass
// two up to the group's largest steps_taken, one graph per (kmax, nb).
void run_pass1_batch(tpl_op_s* op, size_t k, int nb);
void run_pass2_batch(tpl_op_s* op, size_t kmax, int nb);
// Pass two of a group for the m coefficient columns per right-hand side in op->bat.d_my
// into op->bat.d_mx (ensure_batch_multi first). steps: the nb columns' steps_taken, as the
// device state holds them. All equal (the normal case): one graph per (kmax, nb, m);
// otherwise the launch list depends on every steps_c and runs uncaptured.
void run_pass2_batch_multi(tpl_op_s* op, const size_t* steps, int nb, size_t m);
// The same with a cut per (column, function): result (f, c) takes the terms below
// op->d_bcut[c TPL_MULTI_MAX + f] only (k_bp2_xacc_cut; 1 <= that count <= steps_c, the
// device-held step count of column c), so it holds the bits of the single pass two at that
// many steps. steps: the group's largest steps_c. One graph per (steps, nb, m): the counts
// are device data.
void run_pass2_batch_multi_cut(tpl_op_s* op, size_t steps, int nb, size_t m);
// One group of the batch shifted inverse solve as one graph (ensure_batch, ensure_batch_multi,
// ensure_batch_cut first; the group's b interleaved in op->bat.b; tolerance, shifts and
// zeroed hit tables uploaded): pass one with k_bp1_axpy_stol, k_bp1_stol_fin,
// k_ftk_inv_shifts per column into op->bat.d_my and op->d_bcut, the batch-multi pass two
// with the cut. One graph per (kmax, nb, m).
void run_two_pass_batch_shifted_inv_tol(tpl_op_s* op, size_t kmax, int nb,
                                        const launch::BatchShiftTol& t);
void run_two_pass_dev(tpl_op_s* op, size_t k, int f);
// The one-graph inverse solve that stops at the tolerance in op->d_tol[0] (ensure_tol and
// the upload of the tolerance and of the zeroed hit words first): one graph per kmax.
void run_two_pass_inv_tol(tpl_op_s* op, size_t kmax);
// The one-graph shifted inverse solve (tolerance, shifts and zeroed hit tables uploaded
// first): pass one with k_p1_axpy_stol, k_p1_stol_fin, k_ftk_inv_shifts into op->d_Y and
// op->d_col_steps, the multi-function pass two with the cut. One graph per (kmax, m).
void run_two_pass_shifted_inv_tol(tpl_op_s* op, size_t kmax, const launch::ShiftTol& t);
HostDecomp fetch_decomp(tpl_op_s* op);

} // namespace tpl
