/*
 * tpl.h — C ABI of the MI355X two-pass Lanczos engine (libtpl_amd.so).
 *
 * This is the drop-in boundary for the hot path of lukefleed/two-pass-lanczos:
 * the Lanczos recurrence behind `solvers::lanczos` / `solvers::lanczos_two_pass`
 * and the low-level `algorithms::*` entry points. Every entry point below names
 * the reference item it replaces (file:line under the reference checkout).
 * The signatures are plain C (pointers + sizes, no torch / HIP types), so a
 * Rust `extern "C"` block, ctypes, or a C++ caller can bind them directly
 * (bindings: INTEGRATION.md).
 *
 * Conventions
 *   - All arithmetic is IEEE fp64 (every reference call site is f64).
 *   - Vectors `b`, `x_out`, `v_out` are host pointers when `mem == TPL_MEM_HOST`
 *     and device pointers on the operator's GPU when `mem == TPL_MEM_DEVICE`.
 *     Scalar arrays (alphas, betas, y) are always host pointers.
 *   - `v_out` matrices are column-major n x steps (leading dimension n), the
 *     layout of the reference's `Mat<f64>` V_k.
 *   - Every function returns a tpl_status; on failure tpl_last_error() returns
 *     the message, formatted exactly like the reference's `Display` strings
 *     (src/error.rs:20-58) for the Lanczos error kinds.
 *   - An operator owns one HIP stream and its device workspace; calls on one
 *     operator are not re-entrant (the reference is single-threaded, Par::Seq).
 */
#ifndef TPL_H_
#define TPL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: mirror LanczosErrorKind (src/error.rs:20-58) ---------- */
typedef enum tpl_status {
  TPL_OK = 0,
  TPL_ERR_BREAKDOWN = 1,           /* LanczosErrorKind::Breakdown (declared, never constructed by the reference) */
  TPL_ERR_DIMENSION_MISMATCH = 2,  /* LanczosErrorKind::DimensionMismatch (reference panics instead; we report) */
  TPL_ERR_INPUT = 3,               /* LanczosErrorKind::InputError  (src/algorithms/mod.rs:268-272, lanczos_two_pass.rs:229-235) */
  TPL_ERR_PARAMETER_MISMATCH = 4,  /* LanczosErrorKind::ParameterMismatch (src/solvers.rs:78-85,158-165; lanczos_two_pass.rs:220-227) */
  TPL_ERR_EVD = 5,                 /* LanczosErrorKind::EvdError (built-in exp solver only) */
  TPL_ERR_SOLVER = 6,              /* LanczosErrorKind::SolverError (src/solvers.rs:75,156) */
  /* engine / loader errors (no reference counterpart in LanczosErrorKind) */
  TPL_ERR_INVALID_ARGUMENT = 100,
  TPL_ERR_DEVICE = 101,            /* HIP runtime failure; message carries hipGetErrorString */
  TPL_ERR_OUT_OF_MEMORY = 102,
  TPL_ERR_DATA_LOADER = 103,       /* DataLoaderError (src/utils/data_loader.rs:16-43) */
  TPL_ERR_UNSUPPORTED = 104
} tpl_status;

enum { TPL_MEM_HOST = 0, TPL_MEM_DEVICE = 1 };

typedef struct tpl_ctx_s* tpl_ctx_t; /* one GPU + one HIP stream          */
typedef struct tpl_op_s* tpl_op_t;   /* device-resident CSR operator A    */

/* Thread-local message of the last failing call ("" after success). A successful
 * tpl_op_destroy / tpl_ctx_destroy / tpl_dist_destroy leaves it, and tpl_last_error_detail's
 * record, as they were: a binding's finalizer may run between a failed call and the
 * caller's read of its error.                                                          */
const char* tpl_last_error(void);
/* The fields of the last failing call's LanczosErrorKind (src/error.rs:20-58), so a
 * binding rebuilds the variant itself instead of parsing the message:
 *   TPL_ERR_INPUT              InputError(inner)
 *   TPL_ERR_PARAMETER_MISMATCH ParameterMismatch { param_name, expected, actual }
 *                              (src/solvers.rs:78-85,158-165; lanczos_two_pass.rs:220-227)
 *   TPL_ERR_DIMENSION_MISMATCH DimensionMismatch { operator_cols, vector_rows }
 *   TPL_ERR_SOLVER             SolverError(inner) (src/solvers.rs:75,156)
 *   TPL_ERR_EVD                EvdError(inner)
 *   TPL_ERR_BREAKDOWN          Breakdown { k = breakdown_step } (never raised: a
 *                              breakdown truncates steps_taken, as in the reference)
 * status is TPL_OK after a successful call. The strings stay valid until the next
 * tpl_* call on this thread. Returns TPL_ERR_INVALID_ARGUMENT only for out == NULL.  */
typedef struct tpl_error_detail {
  int32_t status;             /* tpl_status of the last call on this thread            */
  const char* message;        /* == tpl_last_error(): the variant's Display text        */
  const char* inner;          /* InputError / SolverError / EvdError payload, else ""  */
  const char* param_name;     /* ParameterMismatch::param_name, else ""                */
  uint64_t expected, actual;  /* ParameterMismatch                                      */
  uint64_t operator_cols, vector_rows; /* DimensionMismatch                             */
  uint64_t breakdown_step;    /* Breakdown::k                                           */
} tpl_error_detail;
tpl_status tpl_last_error_detail(tpl_error_detail* out);
/* Library version string, e.g. "tpl_amd 0.1.0 gfx950". */
const char* tpl_version(void);

/* ---- context ------------------------------------------------------------- */
tpl_status tpl_ctx_create(int device, tpl_ctx_t* out);
tpl_status tpl_ctx_destroy(tpl_ctx_t ctx);
/* Synchronise the context stream (all operators created on it share it). */
tpl_status tpl_ctx_synchronize(tpl_ctx_t ctx);
/* Number of visible GPUs (0 on a host without one; never fails). */
int tpl_device_count(void);

/* ---- operator: replaces faer `LinOp<f64>` for `SparseColMatRef<usize,f64>`
 *      (used at src/algorithms/mod.rs:177, src/algorithms/lanczos_two_pass.rs:186).
 *  A must be square n x n and SYMMETRIC (the Lanczos contract; A = [[D,E^T],[E,0]]
 *  for the KKT inputs), so its CSR arrays equal the reference's CSC arrays.
 *  Host arrays are borrowed for the call only; the operator copies them to HBM.
 *  Column indices must be sorted ascending within each row, 0 <= col < n.
 *  Limits: nnz < 2^31 (int32 offsets on device).                               */
tpl_status tpl_op_create_csr(tpl_ctx_t ctx, int64_t n, int64_t nnz,
                             const int64_t* row_ptr, const int32_t* col_idx,
                             const double* vals, tpl_op_t* out);
/* ---- dense operator: replaces faer `LinOp<f64>` for a dense `Mat<f64>` (the reference's
 *      tests/correctness.rs and src/bin/dense_tradeoff.rs). Element (i, j) is a[i*lda + j];
 *  A must be SYMMETRIC (not checked, as for CSR), which makes row- and column-major the same
 *  thing: faer's column-major Mat passes straight through with lda = its column stride.
 *  mem: TPL_MEM_HOST or TPL_MEM_DEVICE; `a` is borrowed for the call only. The device keeps
 *  the matrix whole (8 bytes per entry, rows a padded leading dimension apart; counted in
 *  tpl_op_device_bytes) and streams it once per step: no indices, no gathers.
 *  Reduction order: every row is a long row of the canonical order (tpl_op_schedule:
 *  n_short = 0, long_rows = 0 .. n-1, tpl_op_permutation the identity) over all n columns,
 *  explicit zeros included, in S = tpl_op_slices column slices (tpl_dense_schedule's rule;
 *  tpl_op_set_slices works). tpl_op_nnz is n * n; tpl_op_flags bit 10 is set.
 *  Runs tpl_op_apply and every single-right-hand-side solver. Refused with
 *  TPL_ERR_UNSUPPORTED before any device work: every *_batch* entry point,
 *  tpl_op_set_schedule, tpl_op_set_reorder(1), tpl_op_tune_order, tpl_op_set_order_groups,
 *  tpl_op_set_value_format, tpl_op_set_long_cache(1) and tpl_profile_kernel; the auto modes
 *  of the locality order, the long-row cache and the fused pass two resolve to off.
 *  Errors: NULL argument, n <= 0, lda < n: TPL_ERR_INVALID_ARGUMENT; n >= 2^31:
 *  TPL_ERR_UNSUPPORTED; TPL_ERR_OUT_OF_MEMORY leaves nothing behind.                    */
tpl_status tpl_op_create_dense(tpl_ctx_t ctx, int64_t n, const double* a, int64_t lda, int mem,
                               tpl_op_t* out);
/* The schedule rule of a dense operator of n rows (host only): *slices = slices_req (1, 2,
 * 4, 8), or for 0 the CSR auto rule (1 up to 65 536 columns); (*G2, *E) the element-wise
 * geometry of n rows under the default schedule parameters. Outputs may be NULL.          */
tpl_status tpl_dense_schedule(int64_t n, int32_t slices_req, int32_t* slices, int32_t* G2,
                              int64_t* E);
tpl_status tpl_op_destroy(tpl_op_t op);
int64_t tpl_op_nrows(tpl_op_t op); /* LinOp::nrows / ncols */
int64_t tpl_op_nnz(tpl_op_t op);
/* Bit 0: row-partitioned operator; bit 1: passes launched eagerly (no hipGraph —
 * a host transport, or a transport that refused stream capture); bit 2: values kept
 * as int8, bit 3 / bit 4: short-row / long-row column indices kept as uint16 offsets
 * (see tpl_op_set_value_format), bit 5: the last tpl_lanczos_two_pass / tpl_lanczos
 * evaluated f(T_k) on the device (one graph, no host round trip), bit 6: rows held in the locality order
 * (tpl_op_set_reorder, tpl_op_permutation; on a replicated-long-row partition the
 * rank's own short rows are in that order and tpl_op_local_rows, not
 * tpl_op_permutation, reports it), bit 7: a replicated-long-row partition whose ranks
 * all-gather their norm partials and reduce them inside pass one's SpMV (no rank-total
 * launch), bit 8: the last pass two the operator ran read long rows' sums
 * from the long-row cache (tpl_op_set_long_cache: a two-pass solve whose bit is in
 * tpl_op_set_long_cache_solvers' mask — by default tpl_lanczos_two_pass alone — with the
 * cache on; any other entry point's pass two reads 0), bit 9: that pass two ran fused — two
 * launches for all its steps (tpl_op_set_fused_pass_two; bit 8 is set as well), bit 10: a
 * dense operator (tpl_op_create_dense; bits 6, 8 and 9 read 0 on it).
 * -1 if op is NULL.                                                                    */
int tpl_op_flags(tpl_op_t op);
/* Locality order (single-GPU operators; rebuilds the layout). mode 1: the device
 * holds P A P^T, the short rows sorted by the long rows (hub columns) they reference
 * and the long rows last, so the hub rows' gathers touch compact runs; mode 0: the
 * caller's order; mode 2 (default, auto): on up to 2^20 rows (measured gain at the
 * 500k-arc KKT, none from 1M arcs, a loss at 5M arcs: DESIGN.md §3);
 * every vector crossing the boundary (b, x, apply's x / y, V_k, the callback's view)
 * is permuted on the device, so the caller sees its own row order throughout. The
 * permutation changes the device's reduction order (summation order within rows and of
 * the partials): results are bitwise those of the oracle run on P A P^T with the same
 * schedule, and agree with the unpermuted operator to rounding. No effect when the
 * matrix has no long rows, and none on row-partitioned operators.                   */
tpl_status tpl_op_set_reorder(tpl_op_t op, int mode);
/* perm[i] = the caller's row held at internal position i (n entries; the identity
 * when the operator is not reordered). tpl_op_schedule's row lists are internal.    */
tpl_status tpl_op_permutation(tpl_op_t op, int32_t* perm);
/* Tune the locality order's group count on this device (single GPU; switches the
 * order on): rebuilds the layout for each of the `count` group counts in `groups`
 * (count 0: 12..20, 22, 24), times `iters` launches each of the pass-one and pass-two
 * SpMV kernels, keeps the fastest and reports it in *chosen (*best_us: the sum of the
 * two kernels' average launch times). The choice depends on measured times, so two
 * tuned operators of one matrix may hold different orders (each bitwise against the
 * oracle given its own permutation); untuned operators are deterministic.          */
tpl_status tpl_op_tune_order(tpl_op_t op, const int32_t* groups, int32_t count, int32_t iters,
                             int32_t* chosen, double* best_us);
/* Pin the locality order's group count (single GPU; rebuilds the layout; 0 = the
 * default 16). Deterministic: operators of one matrix with one group count hold the
 * same order on every device and process, so their results are bit-identical. The
 * bench pins the count per instance (bench.py PINNED_ORDER_GROUPS, chosen offline from
 * profiles/r02_group_sweep.txt) instead of tuning on the box.                       */
tpl_status tpl_op_set_order_groups(tpl_op_t op, int32_t groups);
/* The group count of the order the device holds (0: caller's order; -1: NULL op). */
int32_t tpl_op_order_groups(tpl_op_t op);
/* The locality order's rule alone (host only, no device): perm (n entries) as
 * tpl_op_permutation would report it for this CSR (columns ascending per row),
 * short-row threshold (<= 0: auto) and group count (<= 0: 16); *applied = 0 when the
 * order is the identity.                                                           */
tpl_status tpl_locality_order(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                              int32_t short_row_max, int32_t groups, int32_t* perm,
                              int32_t* applied);
/* Storage format (rebuilds the layout): compress != 0 (default) keeps the values as
 * int8 when every one is an integer in [-128, 127] (not -0.0), and the column
 * indices as uint16 offsets from a per-chunk / per-bin base when the spans allow —
 * lossless, results are bit-identical; 0 keeps fp64 values and int32 columns.       */
tpl_status tpl_op_set_value_format(tpl_op_t op, int compress);

/* y = A x  — LinOp::apply (compatibility path; the solvers below keep the whole
 * recurrence on the device and never call this per step).                     */
tpl_status tpl_op_apply(tpl_op_t op, const double* x, double* y, int mem);

/* ---- f(T_k) solver callback: replaces the `f_tk_solver` closure
 *      `FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>` (src/solvers.rs:57,144).
 *  Called exactly once per solve, after pass one, with n_alphas = steps and
 *  n_betas = steps - 1. Write y' = f(T_k) e_1 into y_out (capacity y_cap = steps)
 *  and its length into *y_len. Return 0 on success; non-zero means Err(e): put
 *  e's text (NUL-terminated) into err_msg (capacity err_cap).                   */
typedef int (*tpl_ftk_fn)(const double* alphas, size_t n_alphas, const double* betas,
                          size_t n_betas, double* y_out, size_t y_cap, size_t* y_len,
                          char* err_msg, size_t err_cap, void* user);

/* Built-in f(T_k) solvers with the tpl_ftk_fn signature (user ignored):
 *  inv : y' = T_k^{-1} e_1, tridiagonal LU with partial pivoting
 *        (the harness's sp_lu / partial_piv_lu, src/bin/tradeoff.rs:245-258,
 *        tests/correctness.rs:171-179). A singular T_k yields non-finite y'
 *        exactly like an LU solve does (no error), matching the reference.
 *  exp : y' = Q exp(Lambda) Q^T e_1 via symmetric tridiagonal QL eigensolver
 *        (src/bin/stability.rs:175-193). Non-convergence -> non-zero return.
 *  sq  : y' = T_k^2 e_1 (tests/correctness.rs:287-299).                        */
int tpl_ftk_inv(const double* alphas, size_t n_alphas, const double* betas, size_t n_betas,
                double* y_out, size_t y_cap, size_t* y_len, char* err_msg, size_t err_cap,
                void* user);
int tpl_ftk_exp(const double* alphas, size_t n_alphas, const double* betas, size_t n_betas,
                double* y_out, size_t y_cap, size_t* y_len, char* err_msg, size_t err_cap,
                void* user);
int tpl_ftk_sq(const double* alphas, size_t n_alphas, const double* betas, size_t n_betas,
               double* y_out, size_t y_cap, size_t* y_len, char* err_msg, size_t err_cap,
               void* user);
/* The residual history of the inverse solve: res_out[m - 1], m = 1 .. L = min(n_alphas,
 * n_betas), is the relative Lanczos residual ||b - A x_m|| / ||b|| = beta_m |e_m^T T_m^{-1}
 * e_1| of the m-step iterate x_m = ||b|| V_m T_m^{-1} e_1, from tpl_ftk_inv's own
 * elimination: with the running row {d, b} after rows 0 .. m - 2 are eliminated,
 * res[m - 1] = fabs(betas[m - 1] * (b / d)) — an IEEE divide, a multiply, fabs, no
 * contraction. A zero pivot gives inf or NaN (neither is ever <= a finite tolerance). The
 * estimate follows the true residual down to about 1e-14 relative and keeps falling where
 * the true one stalls at rounding level; on a singular matrix it does not fall at all.
 * *res_len (may be NULL) receives L; non-zero return: res_cap < L or a NULL array with
 * L > 0. A k-step pass one has k - 1 betas, so its history has k - 1 entries.         */
int tpl_ftk_inv_residuals(const double* alphas, size_t n_alphas, const double* betas,
                          size_t n_betas, double* res_out, size_t res_cap, size_t* res_len);
/* exp_t: y' = exp(t T_k) e_1 — exp(tA) b at time t. `user` points to one double, t; NULL:
 * non-zero return with a message. tpl_ftk_exp on the arrays t * alphas, t * betas (every
 * entry times t, rounded once), so bitwise what a caller gets who scales T_k and calls
 * tpl_ftk_exp.                                                                  */
int tpl_ftk_exp_t(const double* alphas, size_t n_alphas, const double* betas, size_t n_betas,
                  double* y_out, size_t y_cap, size_t* y_len, char* err_msg, size_t err_cap,
                  void* user);

/* ---- high-level API: src/solvers.rs ------------------------------------- */
/* solvers::lanczos (src/solvers.rs:46-107): standard pass (V_k kept in HBM),
 * f(T_k), x = ||b|| V_k y' (device GEMV). x_out has n entries. With a built-in f on a
 * single-GPU operator f(T_k) runs on the device by the rules of tpl_op_set_device_ftk
 * (no host round trip); any other f is called on the host.                       */
tpl_status tpl_lanczos(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                       tpl_ftk_fn f, void* f_user, double* x_out, int mem);
/* solvers::lanczos_two_pass (src/solvers.rs:133-175): pass one (scalars only),
 * f(T_k), y = y' ||b||, pass two regenerates V_k on the fly. With f == tpl_ftk_inv (or
 * tpl_ftk_exp) on a single-GPU operator the solve runs as ONE device graph: f(T_k) on the
 * GPU (inv: the host solver's exact operations, bitwise the same y), no host round trip
 * between the passes (tpl_op_set_device_ftk). Any other f is called on the host between
 * the passes.
 * On an error x_out is unspecified.                                               */
tpl_status tpl_lanczos_two_pass(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                tpl_ftk_fn f, void* f_user, double* x_out, int mem);
/* x = A^{-1} b by the two-pass solve with the built-in inv, stopped at a residual tolerance
 * (an extension: the reference's solvers take a fixed k). With `steps_taken` steps of a
 * kmax-step pass one (fewer than kmax after a breakdown) and res = tpl_ftk_inv_residuals of
 * its decomposition: m* = the smallest m in 1 .. steps_taken - 1 with res[m - 1] <= tol and
 * *converged = 1, or m* = steps_taken and *converged = 0 if there is none. x_out is bitwise
 * tpl_lanczos_two_pass(op, b, m*, tpl_ftk_inv); *steps = m*. res_out (capacity kmax, or
 * NULL) receives the history up to the last entry that was formed, *res_len entries: the
 * first min(m*, steps_taken - 1) are always there and bitwise tpl_ftk_inv_residuals';
 * how many follow them is unspecified (*res_len is 0 when res_out is NULL). steps,
 * converged and res_len may be NULL.
 * Where tpl_lanczos_two_pass would run inv on the device for k = kmax
 * (tpl_op_set_device_ftk: a single GPU, mode 2 up to kmax = 500, mode 1 up to 1365) the
 * call is ONE graph, cached per kmax and replayed for any tol: pass one's elimination
 * workgroup forms each residual as its row is done and raises the stop on the device, about
 * two steps run past m*, every later launch of pass one returns at once, and pass two takes
 * m* from the device. tpl_op_flags bit 5 reads 1 afterwards, bits 8 and 9 as after
 * tpl_lanczos_two_pass with k = kmax; the long-row cache follows TPL_LONG_CACHE_TWO_PASS.
 * Everywhere else (mode 0, a larger kmax, a partitioned operator) the call is composed on
 * the host — tpl_lanczos_pass_one to kmax, the history and the rule, tpl_ftk_inv on the
 * first m* rows, tpl_lanczos_pass_two — with the same results, bit for bit.
 * Errors: NULL op or x_out, then tol NaN or negative: TPL_ERR_INVALID_ARGUMENT before any
 * device work (tol = +inf is valid: m* = 1 when kmax >= 2); every other error is
 * tpl_lanczos_two_pass's (a host-only plan, b's length, kmax = 0, a zero b). No live timing:
 * tpl_op_pass_timing keeps its values.                                                  */
tpl_status tpl_lanczos_two_pass_inv_tol(tpl_op_t op, const double* b, int64_t b_len, size_t kmax,
                                        double tol, double* x_out, int mem, size_t* steps,
                                        int32_t* converged, double* res_out, size_t* res_len);
/* ---- f_1(A) b ... f_m(A) b over one Krylov space (an extension: the reference's
 *      f_tk_solver returns a Mat and rejects ncols != 1, src/solvers.rs:78,158) ------
 * Pass one and the basis pass two regenerates depend on (A, b, k) only; the functions
 * differ in y = ||b|| f(T_k) e_1 alone. One call runs pass one once, calls fs[0..m) in
 * index order on the host (each once, with f_users[i] as its `user`; f_users may be NULL),
 * and runs ONE pass two that regenerates the basis once and accumulates all m results.
 * x_out is column-major n x m with leading dimension n; column i is bitwise what
 * tpl_lanczos_two_pass gives for fs[i] with f(T_k) on the host (tpl_op_set_device_ftk 0).
 * f is always evaluated on the host (tpl_op_flags bit 5 reads 0 afterwards). Errors are
 * those of the single solve, checked per column, the first failing index reported;
 * m == 0, m > TPL_MULTI_MAX, NULL fs or x_out: TPL_ERR_INVALID_ARGUMENT; a partitioned
 * operator: TPL_ERR_UNSUPPORTED. Not supported: v_out, re-orthogonalisation, live timing
 * (tpl_op_pass_timing keeps the last single solve's values).                          */
enum { TPL_MULTI_MAX = 64 };
tpl_status tpl_lanczos_two_pass_multi(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                      const tpl_ftk_fn* fs, void** f_users, size_t m,
                                      double* x_out, int mem);
/* The one-pass sibling: one standard pass (V_k in HBM), then x_i = ||b|| V_k y'_i per
 * function; column i is bitwise tpl_lanczos's host-f result for fs[i].                */
tpl_status tpl_lanczos_multi(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                             const tpl_ftk_fn* fs, void** f_users, size_t m,
                             double* x_out, int mem);
/* exp(t_i A) b for the m times ts[0..m) — the action of the matrix exponential at a list of
 * times — over one Krylov space: column i of x_out (column-major n x m, leading dimension
 * n) is ||b|| V_k exp(t_i T_k) e_1. One pass one; then, unless the operator's device-f mode
 * is 0 (tpl_op_set_device_ftk) or k > 1800, every exp(t_i T_k) e_1 at once on the device,
 * one workgroup per time (k_ftk_exp_times: tpl_lanczos_two_pass's device exp on the
 * tridiagonal t_i * alphas, t_i * betas, with its accuracy and its hand-back rules), with no
 * host work between the passes but one synchronisation; a time the device hands back, and
 * in mode 0 or past k = 1800 every time, is evaluated on the host by tpl_ftk_exp_t, in
 * index order; then ONE pass two for all m results. on_device (m entries, or NULL):
 * 1 where the device's y was used. Column i is bitwise tpl_lanczos_pass_two on pass one's
 * decomposition with the y that was used; in mode 0 the whole result is bitwise
 * tpl_lanczos_two_pass_multi's with fs[i] = tpl_ftk_exp_t, f_users[i] = &ts[i]. Errors: those
 * of tpl_lanczos_two_pass_multi (a host failure is reported for its index); m == 0,
 * m > TPL_MULTI_MAX, NULL ts or x_out, a non-finite t_i: TPL_ERR_INVALID_ARGUMENT, before any
 * device work; a partitioned operator: TPL_ERR_UNSUPPORTED. tpl_op_flags bit 5 reads 0
 * afterwards (the call is not one graph); the long-row cache follows the
 * TPL_LONG_CACHE_TWO_PASS_MULTI bit; no live timing.                                  */
tpl_status tpl_lanczos_two_pass_exp_times(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                          const double* ts, size_t m, double* x_out, int mem,
                                          int32_t* on_device);
/* (A + sigma_i I)^{-1} b for the m shifts sigmas[0..m) over one Krylov space, each stopped
 * at the residual tolerance of tpl_lanczos_two_pass_inv_tol (an extension). The Krylov space
 * of A + sigma I is A's and its tridiagonal is T_k + sigma I. The definition: ONE pass one of
 * kmax steps on A (alphas, betas, steps_taken, ||b||); for shift i, a_i[j] = alphas[j] +
 * sigmas[i] — one IEEE addition per entry, and no other expression forms a shifted entry,
 * on the host or on the device — then res_i = tpl_ftk_inv_residuals(a_i, betas); m*_i = the
 * smallest m in 1 .. steps_taken - 1 with res_i[m - 1] <= tol and converged[i] = 1, or
 * m*_i = steps_taken and converged[i] = 0 if there is none; y_i = ||b|| tpl_ftk_inv on
 * a_i[0..m*_i), betas[0..m*_i - 1); and column i of x_out (column-major n x m, leading
 * dimension n) is bitwise tpl_lanczos_pass_two on A's decomposition cut to m*_i steps, with
 * y_i. steps[i] = m*_i. res_out (column-major kmax x m, or NULL): the first
 * min(m*_i, steps_taken - 1) entries of column i are bitwise the history res_i, what follows
 * them is unspecified, res_len[i] entries were formed (0 when res_out is NULL). steps,
 * converged, res_out and res_len may each be NULL.
 * So: column i depends neither on m, nor on its position, nor on the other shifts; equal
 * shifts give equal columns; with m = 1 and sigma = 0 the call returns
 * tpl_lanczos_two_pass_inv_tol's x, steps and converged unless some alpha_j is -0 (since
 * -0 + 0 = +0); against an operator built explicitly as A + sigma I the result agrees to
 * rounding only, because Lanczos on A + sigma I rounds alpha differently.
 * On a single GPU with graphs in use, in mode 1 of tpl_op_set_device_ftk up to kmax = 1365
 * (the device inv's bound) and in mode 2 (auto) up to kmax = 64 — past that the graph's
 * launches after the stop were measured to cost more than the host-composed path's full pass
 * one — the call is ONE graph, cached per (kmax, m) and replayed for any
 * tolerance and any shift values: pass one's elimination workgroup runs one lane per shift, each keeping its
 * own history and stop, and raises the stop when every shift has met the tolerance (about
 * two steps run past M = max m*_i; a shift that never meets it keeps the pass running to
 * kmax); one workgroup per shift then solves on its own m*_i rows; the multi-function pass
 * two applies term t to column i only where t < m*_i. tpl_op_flags bit 5 reads 1 afterwards,
 * bit 8 as after tpl_lanczos_two_pass_multi (the long-row cache follows the
 * TPL_LONG_CACHE_TWO_PASS_MULTI bit), bit 9 reads 0. The first such call adds
 * 8 (1 + m (4 + 5 kcap)) + 8 m bytes (kcap: the state's step capacity) and a 256-byte table
 * of column step counts to tpl_op_device_bytes. Everywhere else (mode 0, a larger kmax,
 * TPL_NO_GRAPH=1) the call is composed on the host as defined above, with one pass two of M
 * steps; both paths give the same bits.
 * Errors, in this order and before any device work: NULL op, sigmas or x_out; m == 0 or
 * m > TPL_MULTI_MAX; tol NaN or negative; a non-finite sigma_i — each
 * TPL_ERR_INVALID_ARGUMENT. Then tpl_lanczos_two_pass_multi's: a host-only plan is refused
 * as by every solver, a partitioned operator is TPL_ERR_UNSUPPORTED, a zero b is the single
 * solve's input error. No live timing.
 * Measured on one MI355X (500k block with D, kmax = 500, shifts between 1 and
 * 100): m = 8 at tol 1e-4 takes 10.5 ms composed on the host and 10.8 ms as one graph,
 * against 44.0 ms for eight tpl_lanczos_two_pass_inv_tol calls on explicitly shifted
 * operators; m = 1 (m* = 116) 6.15 and 7.17 ms against 4.19 for the single solve, which has
 * the fused pass two. At kmax = 64 the graph is 0.98-1.01 of the host-composed path.     */
tpl_status tpl_lanczos_two_pass_shifted_inv_tol(tpl_op_t op, const double* b, int64_t b_len,
                                                size_t kmax, const double* sigmas, size_t m,
                                                double tol, double* x_out, int mem,
                                                size_t* steps, int32_t* converged,
                                                double* res_out, size_t* res_len);
/* ---- f(A) b_1 ... f(A) b_s in one lock-step run (an extension: the reference's
 *      solvers::lanczos_two_pass takes one b) -----------------------------------------
 * The other axis: one f, s right-hand sides. Every b_c has its own Krylov space, its own
 * alpha, beta, y and breakdown step; the s recurrences share the matrix bytes, every
 * launch and the address arithmetic of every gather. b_len is n, as elsewhere; B and x_out
 * are column-major n x s with leading dimension n (host or device, by `mem`).
 * tpl_lanczos_two_pass_batch runs pass one for all columns in lock-step, then calls f on
 * the host once per column, in column order, with that column's steps_c alphas and
 * steps_c - 1 betas, scales by ||b_c|| and runs ONE pass two for all columns. Column c of
 * x_out is bitwise what tpl_lanczos_two_pass(op, b_c, k, f) returns with f(T_k) on the host
 * (tpl_op_set_device_ftk(op, 0)); the pass_one_batch outputs of column c are bitwise
 * tpl_lanczos_pass_one's, pass_two_batch's x of column c is bitwise tpl_lanczos_pass_two's.
 * Columns are independent: column c's bits do not depend on s, on its position, or on what
 * the other columns hold, non-finite values included. A column that breaks down at step
 * j_c keeps steps_c = j_c and its truncated result, as in the single solve; the others run
 * on to their own end.
 * Grouping: the columns are taken in order, four per group while four remain, then two
 * per group; a last single column runs the single host-f solve (so a remainder of three is
 * a group of two and a single solve: no group is padded). The groups run one after the
 * other.
 * f is always evaluated on the host (tpl_op_flags bit 5 reads 0 afterwards). Errors are
 * those of the single solve, checked per column in ascending order: the first failing
 * column's error is reported, with the same message text (a zero column: the single
 * solve's zero-vector InputError). On an error x_out is unspecified. s == 0,
 * s > TPL_BATCH_MAX, NULL B / x_out / f: TPL_ERR_INVALID_ARGUMENT; a partitioned operator:
 * TPL_ERR_UNSUPPORTED. Not supported: v_out, re-orthogonalisation, live timing, device
 * f(T_k) (tpl_op_pass_timing keeps the last single solve's values).                    */
enum { TPL_BATCH_MAX = 64 };
/* B, x_out: column-major n x s, leading dimension n (host or device, by `mem`). */
tpl_status tpl_lanczos_two_pass_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      size_t k, tpl_ftk_fn f, void* f_user,
                                      double* x_out, int mem);
/* alphas, betas: column-major k x s (ld = k; betas uses k-1 per column);
 * steps, b_norms: s entries */
tpl_status tpl_lanczos_pass_one_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      size_t k, double* alphas, double* betas,
                                      size_t* steps, double* b_norms, int mem);
/* the decompositions as pass_one_batch wrote them (ld = the k they were made with);
 * y: ld x s, column c holding steps[c] entries (already scaled by ||b_c||) */
tpl_status tpl_lanczos_pass_two_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      const double* alphas, const double* betas, size_t ld,
                                      const size_t* steps, const double* b_norms,
                                      const double* y, double* x_out, int mem);
/* ---- f_i(A) b_c: m functions of s right-hand sides in one run (both axes at once) ------
 * X(c, i) = f_i(A) b_c, e.g. (A + sigma_i I)^-1 B for the poles of a rational approximation,
 * or exp(t_i A) b_c for several states and times. Per group of columns, pass one runs in
 * lock-step (as the batch solve's), every f_i runs on the host on every column's T_k, and
 * ONE pass two regenerates the group's bases once and accumulates all results of the group.
 * x_out is column-major n x (s m) with leading dimension n, the m results of b_c adjacent:
 * column (c m + i).
 * Parity: column (c, i) is bitwise tpl_lanczos_two_pass(op, b_c, k, fs[i]) with f(T_k) on
 * the host (tpl_op_set_device_ftk(op, 0)); hence also column i of tpl_lanczos_two_pass_multi
 * on b_c and column c of tpl_lanczos_two_pass_batch under fs[i]. It does not depend on s, on
 * m, on its position, or on what the other columns hold, non-finite values included. A
 * column that breaks down at step j_c keeps steps_c = j_c for all its m results; the others
 * run on to their own end.
 * Grouping: the batch solve's rule, unchanged: four columns per group while four remain,
 * then two, no group padded; a last single column runs the multi-function solve of that
 * b. m == 1 is the batch solve, s == 1 the multi-function solve.
 * Call order of f: per group, pass one first; then for each column c ascending the batch
 * solve's zero-vector check of that column, then fs[0..m) in index order on that column's
 * T_k, each exactly once, with f_users[i] (f_users may be NULL). The first failure ends the
 * call with the single solve's error text and detail. On an error x_out is unspecified.
 * f is always evaluated on the host (tpl_op_flags bit 5 reads 0 afterwards); live timing is
 * untouched (tpl_op_pass_timing keeps the last single solve's values).
 * s == 0, s > TPL_BATCH_MAX, m == 0, m > TPL_MULTI_MAX, NULL B / fs / x_out (pass_two: NULL
 * B / x_out / steps / b_norms, or arrays shorter than a column's steps):
 * TPL_ERR_INVALID_ARGUMENT; a partitioned operator: TPL_ERR_UNSUPPORTED; a host-only plan is
 * refused as by every solver. Not supported: v_out, re-orthogonalisation, device f(T_k). */
tpl_status tpl_lanczos_two_pass_batch_multi(tpl_op_t op, const double* B, int64_t b_len,
                                            size_t s, size_t k, const tpl_ftk_fn* fs,
                                            void** f_users, size_t m, double* x_out, int mem);
/* the decompositions as tpl_lanczos_pass_one_batch wrote them; y: column (c m + i) at
 * y + (c m + i) ld, holding steps[c] entries already scaled by ||b_c||. Result (c, i) is
 * bitwise tpl_lanczos_pass_two's for b_c and that y column. Every group of four or two
 * columns runs the fused pass two, whatever m. */
tpl_status tpl_lanczos_pass_two_batch_multi(tpl_op_t op, const double* B, int64_t b_len,
                                            size_t s, const double* alphas, const double* betas,
                                            size_t ld, const size_t* steps, const double* b_norms,
                                            const double* y, size_t m, double* x_out, int mem);
/* exp(t_i A) b_c for the m times ts[0..m) and the s columns of B in one run: the batch-multi
 * solve with every exp(t_i T_k) e_1 on the device. x_out is column-major n x (s m), result
 * (c, i) at column (c m + i), as tpl_lanczos_two_pass_batch_multi's; on_device (s m entries
 * at c m + i, or NULL): 1 where the device's y was used. Per group of four or two columns
 * (the batch solve's grouping rule, no group padded): the lock-step pass one; then, unless
 * the operator's device-f mode is 0 (tpl_op_set_device_ftk) or k > 1800, straight behind it
 * on the stream ONE launch of k_ftk_exp_times_batch, one workgroup per (time, column), each
 * column on its own device-held steps_c (tpl_lanczos_two_pass_exp_times's evaluation on the
 * tridiagonal t_i * alphas_c, t_i * betas_c, with its accuracy and its hand-back rules); one
 * synchronisation; then for each column c ascending the batch solve's zero-vector check and,
 * for i ascending, tpl_ftk_exp_t on the host for every (c, i) the device handed back (in mode
 * 0 or past k = 1800: for every (c, i)), only those columns being uploaded; then ONE pass two
 * for the group's nb m results. A last single column runs tpl_lanczos_two_pass_exp_times's
 * body on that b. m == 1 takes the same path.
 * Parity, in bits: result (c, .) and on_device[c m + .] are what
 * tpl_lanczos_two_pass_exp_times(op, b_c, k, ts, m) returns — result (c, i) is
 * tpl_lanczos_pass_two on column c's decomposition with the y that was used; in mode 0 the
 * whole result is tpl_lanczos_two_pass_batch_multi's with fs[i] = tpl_ftk_exp_t,
 * f_users[i] = &ts[i]. Nothing depends on s, on m, on a column's position, on the other
 * columns' contents (non-finite values included) or on the long-row cache mask; a column
 * that breaks down at step j_c keeps steps_c = j_c for all its m results.
 * Errors: those of tpl_lanczos_two_pass_batch_multi (the first failure ends the call with the
 * single solve's error text and detail); NULL ts or a non-finite t_i:
 * TPL_ERR_INVALID_ARGUMENT, before any device work; a partitioned operator:
 * TPL_ERR_UNSUPPORTED; a host-only plan is refused as by every solver. tpl_op_flags bit 5
 * reads 0 afterwards; the long-row cache follows the TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI bit,
 * the remainder column included; no live timing.
 * Device memory: the operator's first call of this entry point or of
 * tpl_op_ftk_exp_times_batch_device adds, beyond the batch-multi solve's buffers, exactly
 * 1,024 bytes (the hand-back table: 4 x TPL_MULTI_MAX int32) and, where no exp-times call
 * allocated them before, the 512 bytes of the times (TPL_MULTI_MAX doubles); a remainder
 * column adds what tpl_lanczos_two_pass_exp_times adds. As many bytes of pinned host memory
 * mirror the table.
 * Measured, 500k headline, k = 500: s = 4, m = 4 takes 32.3 ms against 91.2 ms
 * for tpl_lanczos_two_pass_batch_multi with exp_t closures (0.35), s = 2, m = 1 16.0 against
 * 23.3 ms (0.69); no measured shape (s, m in (2,1) (2,4) (4,1) (4,4) (4,8), also at 50k arcs
 * with k = 200) is slower than that baseline.                                         */
tpl_status tpl_lanczos_two_pass_batch_exp_times(tpl_op_t op, const double* B, int64_t b_len,
                                                size_t s, size_t k, const double* ts, size_t m,
                                                double* x_out, int mem, int32_t* on_device);
/* (A + sigma_i I)^{-1} b_c for the s columns of B and the m shifts sigmas[0..m) in one run,
 * every (column, shift) stopped at the residual tolerance: the batch sibling of
 * tpl_lanczos_two_pass_shifted_inv_tol. B is column-major n x s; x_out is column-major
 * n x (s m), result (c, i) at column (c m + i), as tpl_lanczos_two_pass_batch_multi's; steps,
 * converged and res_len hold s m entries at c m + i; res_out is column-major kmax x (s m).
 * steps, converged, res_out and res_len may each be NULL.
 * Definition, in bits: the outputs for (c, .) are what
 * tpl_lanczos_two_pass_shifted_inv_tol(op, b_c, kmax, sigmas, m, tol) returns — x, steps,
 * converged, the guaranteed prefix of each history (the first min(m*_{c,i}, steps_c - 1)
 * entries) and the res_len rules. So result (c, i) is also the fixed-k single solve at
 * k = m*_{c,i} with the shifted-inv closure, and depends neither on s, nor on m, nor on its
 * position, nor on what the other columns hold (non-finite values included), nor on the
 * long-row cache mask, nor on which path ran. A column that breaks down at step j_c keeps
 * steps_c = j_c for all its shifts; the others run on to their own end.
 * Grouping: the batch solve's rule, unchanged: four columns per group while four remain,
 * then two, no group padded; a last single column runs tpl_lanczos_two_pass_shifted_inv_tol's
 * body on that b, with that entry point's own routing.
 * Host-composed path (mode 0 of tpl_op_set_device_ftk, TPL_NO_GRAPH=1, an eager operator,
 * kmax past the line below; the oracle of the device path), per group: the lock-step pass one
 * to kmax; per column ascending the zero-vector check, then per shift the history, the stop
 * rule and y on the first m*_{c,i} rows, as the single call's host path; M_c = max_i m*_{c,i}
 * becomes column c's device-held step count; ONE pass two of max_c M_c steps whose flush
 * (k_bp2_xacc_cut) gives result (c, i) term t only where t < m*_{c,i}.
 * Device path, on a single GPU with graphs in use — in mode 1 up to kmax = 1365 (the device
 * inv's bound), in mode 2 (auto) up to kmax = 250, the largest measured kmax at which
 * the graph was no slower than the host-composed path at every measured (s, m) (below) —
 * one graph per group, cached per
 * (kmax, group width, m) and replayed for any tolerance, shifts and B: the elimination
 * workgroup of the batch pass one (k_bp1_axpy_stol) runs wave c for column c and lane i of it
 * for shift i; when every lane of wave c has stopped, column c stops (it stores nothing from
 * about two steps past M_c on) while the other columns run on, and once every column has
 * stopped the remaining launches return at once; k_ftk_inv_shifts then solves every (c, i) on
 * its own m*_{c,i} rows, one launch per column; the batch-multi pass two runs with the cut.
 * tpl_op_flags bit 5 reads 1 afterwards if and only if every group of four or two ran as one
 * graph (a call with s = 1 reports what the single-b call reports); bit 8 follows the
 * TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI bit, the remainder column included; bit 9 reads 0.
 * Device memory: beyond the batch-multi solve's buffers the operator's first call adds a
 * 1,024-byte table of cuts (4 x TPL_MULTI_MAX int32; tpl_lanczos_pass_two_batch_multi_cut adds
 * the same) and, on the device path, exactly 8 (1 + m) + 4 (8 m (3 + 5 kcap) + 8 m) bytes
 * (kcap: the batch buffers' step capacity, max(kmax, 16) on a first call); a remainder column
 * adds what tpl_lanczos_two_pass_shifted_inv_tol adds.
 * Errors, in this order and before any device work, each TPL_ERR_INVALID_ARGUMENT: NULL op, B,
 * sigmas or x_out; s == 0 or s > TPL_BATCH_MAX; m == 0 or m > TPL_MULTI_MAX; tol NaN or
 * negative (+inf is valid); a non-finite sigma_i. Then tpl_lanczos_two_pass_batch_multi's: a
 * host-only plan is refused as by every solver, a partitioned operator is
 * TPL_ERR_UNSUPPORTED, then b_len and kmax = 0; a zero column is the single solve's
 * zero-vector InputError, for the first such column in ascending order. On an error x_out is
 * unspecified. No live timing (tpl_op_pass_timing keeps its values).
 * Measured on one MI355X (profiles/batch_shifted_inv_tol_timing.txt; 500k block
 * with D, shifts between 1 and 100, medians): s = 4, m = 1, kmax = 500 at tol 1e-4 (the columns
 * stop at 110 - 128) takes 20.3 ms as one graph and 21.7 ms composed on the host, against
 * 24.8 ms for four tpl_lanczos_two_pass_shifted_inv_tol calls and 28.6 ms for
 * tpl_lanczos_two_pass_batch_multi with inv_shift closures at k = 500; s = 4, m = 8 (one shift
 * never stops: every pass runs to 500) 33.8, 33.5, 42.2 and 38.6 ms. The graph over the host
 * path: 0.96 - 1.01 at kmax = 250, every difference within the repetitions' noise; at 500, 0.93
 * - 0.95 where the four columns stop but 1.01 (+0.24 to +0.37 ms) where a shift never does; at
 * 125 and 64, where nothing stops, 0.99 - 1.02 (+0.10 ms at most) — so auto mode's graph is up
 * to 2 % slower than the host-composed path there, and mode 0 avoids that. At every measured
 * shape either path is 0.78 - 0.95 of the s single-b calls. Where no column stops and m = 1
 * (kmax = 64 and 125) the call is 5 - 11 % slower than tpl_lanczos_two_pass_batch_multi at the
 * fixed k, which then runs the batch solve's pass two without flush launches; with m >= 4 or
 * a stop it is 0.71 - 1.00 of it. */
tpl_status tpl_lanczos_two_pass_batch_shifted_inv_tol(
    tpl_op_t op, const double* B, int64_t b_len, size_t s, size_t kmax, const double* sigmas,
    size_t m, double tol, double* x_out, int mem, size_t* steps, int32_t* converged,
    double* res_out, size_t* res_len);
/* The kmax up to which auto mode (tpl_op_set_device_ftk mode 2) runs a group of the call
 * above as one graph. */
size_t tpl_batch_shifted_inv_tol_auto_k(void);
/* tpl_lanczos_pass_two_batch_multi with a cut per (column, function): col_steps holds s m
 * entries, 1 <= col_steps[c m + i] <= steps[c] (steps[c] >= 1), and result (c, i) is bitwise
 * tpl_lanczos_pass_two for b_c on column c's decomposition cut to col_steps[c m + i] steps with
 * the first that many entries of y's column (c m + i); the entries past the cut are never
 * used. The sibling of tpl_lanczos_pass_two_multi_cut, which a last single column runs.
 * Checked before any device work, each TPL_ERR_INVALID_ARGUMENT: a NULL argument, s, m, then
 * per column ascending steps[c] (>= 1, <= ld), its col_steps, b_norms[c] (the zero-vector
 * InputError) and betas. */
tpl_status tpl_lanczos_pass_two_batch_multi_cut(tpl_op_t op, const double* B, int64_t b_len,
                                                size_t s, const double* alphas,
                                                const double* betas, size_t ld,
                                                const size_t* steps, const double* b_norms,
                                                const double* y, const size_t* col_steps,
                                                size_t m, double* x_out, int mem);

/* Where tpl_lanczos_two_pass evaluates the built-in f(T_k): mode 0 = host (two graphs
 * around the host call), 1 = device (the whole solve one graph), 2 = auto (default).
 *   inv: device for k <= 1365 in mode 1, k <= 500 in mode 2: the host solver's exact
 *        operations, its elimination done during pass one and its back substitution with
 *        correctly rounded (Markstein) divisions — bitwise the host result. Auto mode
 *        stops at k = 500, the largest k measured no slower than the host round trip it
 *        removes; at k = 1000-1365 the serial back substitution is slower.
 *   exp: device for k <= 1800 (modes 1 and 2): a Chebyshev expansion of exp over the
 *        Sturm-bracketed spectrum, parallel over the rows of T_k, within
 *        a small multiple of eps * exp(lambda_max) of the host QL result — the accuracy
 *        class of the reference's EVD (src/bin/stability.rs:175-193), not its bits. A
 *        T_k that is not finite or whose spectrum is too wide for the expansion is handed
 *        back to the host solver inside the same call.                              */
tpl_status tpl_op_set_device_ftk(tpl_op_t op, int mode);
/* The long-row cache of tpl_lanczos_two_pass (single-GPU operators).
 * Pass two regenerates pass one's basis bit for bit, so the sum (A v_j)_r of a long row r
 * is the one pass one formed at its step j: pass one keeps these sums (n_long doubles per
 * step) and pass two's steps read them back instead of gathering the long rows again.
 * Results are bitwise the same with the cache on or off.
 *   mode 0: off; 1: on, at most budget_bytes of device memory; 2 (default): on with the
 *   default budget, two vectors' bytes (tpl_long_cache_default_budget), which keeps the
 *   two-pass footprint O(n).
 * The cache holds rows = min(kcap, budget / (8 n_long)) steps (tpl_long_cache_rows), kcap
 * the solver state's capacity; pass-two steps past `rows` run the full step kernel. It is
 * allocated with the solver state (a refused allocation leaves the operator as it was),
 * counted by tpl_op_device_bytes (rows x n_long x 8 bytes; plus 4 n_long for the long rows'
 * indices unless they are the operator's last rows, as the locality order puts them), and
 * not kept when the operator has no long rows. By default only tpl_lanczos_two_pass uses
 * it; tpl_op_set_long_cache_solvers (below) adds the multi-function and batch two-pass
 * solves. The stand-alone passes and partitioned operators never do.
 * Changing the mode or budget drops the cached graphs; the buffer is resized at the next
 * solve. tpl_op_flags bit 8 tells whether the last pass two read the cache.            */
tpl_status tpl_op_set_long_cache(tpl_op_t op, int mode, uint64_t budget_bytes);
/* Which two-pass solvers use the long-row cache while its mode is not 0: a mask of the bits
 * below, default TPL_LONG_CACHE_TWO_PASS. A mask with any other bit is
 * TPL_ERR_INVALID_ARGUMENT and leaves the operator unchanged. Results are bitwise the same
 * whatever the mask.
 *   A remainder column follows the bit of the entry point that was called (the single column
 * after the groups of a batch call, the multi-function solve of a last column in a
 * batch-multi call; a batch-multi call with m = 1 is a batch-multi call): one call is cached
 * throughout or not at all. Partitioned operators, operators without long rows and the
 * stand-alone passes (tpl_lanczos_pass_one[_batch], tpl_lanczos_pass_two[_multi | _batch |
 * _batch_multi]) never cache, whatever the mask.
 *   The multi-function solve uses the single solve's buffer. The batch solves keep a cache of
 * the group's own beside the group's buffers while bit 4 or bit 8 is set: rows_b x n_long x
 * NB doubles for groups of up to NB columns (plus the row-index table, as above), where
 * rows_b = tpl_long_cache_rows(2, 0, n, n_long, kcap) in mode 2 (the budget is two group
 * vectors' bytes, so a group caches as many steps as a single solve) and
 * tpl_long_cache_rows(1, budget_bytes, n, n_long NB, kcap) in mode 1. It is counted by
 * tpl_op_device_bytes, allocated by the next batch solve (a refused allocation leaves the
 * operator as it was) and freed by the next batch solve after both bits are cleared.
 * Changing the mask drops the cached graphs. tpl_op_flags bit 8 after a call with several
 * groups tells of the last group's pass two, or the remainder's.
 *   Measured at the 500k-arc headline, k = 500, every bit is faster in every
 * run: batch s = 4 28.0 -> 24.9 ms (without bit 4 a batch call no longer beats s single
 * solves), s = 2 14.8 -> 12.8, multi m = 4 9.33 -> 8.28, batch-multi s = 4, m = 4 32.7 ->
 * 29.5. None met the project's condition for a recommendation by its letter (the protocol's
 * single warm-up leaves one slow repetition that sets the spread; with two warm-ups all do),
 * so none is recommended here.                                                           */
#define TPL_LONG_CACHE_TWO_PASS 1u             /* tpl_lanczos_two_pass (default) */
#define TPL_LONG_CACHE_TWO_PASS_MULTI 2u       /* tpl_lanczos_two_pass_multi */
#define TPL_LONG_CACHE_TWO_PASS_BATCH 4u       /* tpl_lanczos_two_pass_batch */
#define TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI 8u /* tpl_lanczos_two_pass_batch_multi */
tpl_status tpl_op_set_long_cache_solvers(tpl_op_t op, unsigned mask);
/* The fused pass two of tpl_lanczos_two_pass (single-GPU operators). With the
 * long-row cache holding every step's sums, a long row's whole pass-two history follows from
 * its own cache column, and so does that of a closed short row (every column a long row or
 * the row itself) once the long rows' v_j are known; the open short rows and the long rows
 * they reference (the hub set H) step together in one workgroup. Pass two is then two
 * launches (k_p2_hub, k_p2_rows) instead of steps - 1 step launches, bitwise the same x.
 *   mode 0: off; 2 (default): whenever all of these hold — the long rows are the operator's
 *   last rows (the locality order puts them there), 1 to 2048 of them, no short row wider
 *   than 4 entries, |H| <= 256 with every column of an open row in H, the call is
 *   tpl_lanczos_two_pass without re-orthogonalisation on a single GPU, and the long-row
 *   cache is on for it and holds every step the call asked for (rows >= k).
 * Otherwise, and in every other entry point, the step launches run as before. The path
 * allocates nothing: its small tables (the open rows' entries, H's rows) come with the
 * layout in every mode, and the cache rows hold the long rows' v_j after the solve (the next
 * solve's pass one rewrites them). With live timing on, pass2_spmv_us of tpl_op_pass_timing
 * stays the bracketed time over pass2_launches = steps - 1: on this path the pass-two time
 * per regenerated step, not per launch. Changing the mode drops the cached graphs.
 * tpl_op_flags bit 9 tells whether the last pass two ran fused.                          */
tpl_status tpl_op_set_fused_pass_two(tpl_op_t op, int mode);
/* The layout's verdict without a GPU, for a CSR matrix (columns ascending per row) and a
 * short-row threshold as tpl_op_set_schedule takes it (<= 0: auto): *eligible = 1 when the
 * row classes allow the fused pass two (the placement of the long rows is the operator's
 * matter), *n_open = the open short rows, *n_hub = |H| (n_open itself when more than 256
 * rows are open). Returns 0, or -1 for NULL / negative arguments.                       */
int tpl_fused_pass_two_rows(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                            int short_row_max, int* eligible, int64_t* n_open, int64_t* n_hub);
/* Host arithmetic of the above: the default budget for n rows (2 x 8 x n padded to the
 * vector stride, a multiple of 64), and the steps cached under (mode, budget_bytes) for an
 * n-row operator with n_long long rows and a state capacity of kcap steps.              */
uint64_t tpl_long_cache_default_budget(int64_t n);
uint64_t tpl_long_cache_rows(int mode, uint64_t budget_bytes, int64_t n, int64_t n_long,
                             uint64_t kcap);
/* Test / introspection: evaluate the device f(T_k) kernel alone on a given T_k (which 0:
 * inv, 1: exp; n alphas, n - 1 betas) into y_out (n host doubles, y' = f(T_k) e_1).
 * *on_device = 0 when the exp kernel handed the case back to the host (y_out then 0).  */
tpl_status tpl_op_ftk_device(tpl_op_t op, int which, const double* alphas, size_t n,
                             const double* betas, double* y_out, int* on_device);
/* The same for k_ftk_exp_times alone: exp(t_i T_k) e_1 for the m times ts[0..m) (1 <= m <=
 * TPL_MULTI_MAX, 1 <= n <= 1800) into y_out (host, column-major n x m, leading dimension
 * n, unscaled); on_device[i] = 0 where the kernel handed time i back (that column then 0).
 * Column i and on_device[i] are bitwise tpl_op_ftk_device(op, 1, ...) on t_i * alphas,
 * t_i * betas.                                                                       */
tpl_status tpl_op_ftk_exp_times_device(tpl_op_t op, const double* alphas, size_t n,
                                       const double* betas, const double* ts, size_t m,
                                       double* y_out, int32_t* on_device);
/* The same for k_ftk_inv_shifts alone, nothing eliminated beforehand: (T_n + sigma_i I)^{-1}
 * e_1 for the m shifts sigmas[0..m) (1 <= m <= TPL_MULTI_MAX, 1 <= n <= 1365; above:
 * TPL_ERR_UNSUPPORTED) into y_out (host, column-major n x m, leading dimension n, unscaled).
 * Column i is bitwise tpl_ftk_inv on (alphas + sigma_i, betas), non-finite entries included. */
tpl_status tpl_op_ftk_inv_shifts_device(tpl_op_t op, const double* alphas, size_t n,
                                        const double* betas, const double* sigmas, size_t m,
                                        double* y_out);
/* The same for k_ftk_exp_times_batch alone, on a group of nb (2 or 4) tridiagonals: column c
 * of alphas / betas at c ld, steps[c] rows of it in use (1 <= steps[c] <= min(ld, 1800); 0 or
 * above ld: TPL_ERR_INVALID_ARGUMENT, above 1800: TPL_ERR_UNSUPPORTED), the m times
 * ts[0..m) (1 <= m <= TPL_MULTI_MAX). Loads a group state as pass one leaves it
 * (||b_c|| = 1, no error), runs the one launch and copies back: y_out (host, column-major
 * ld x (nb m)) holds in column (c m + i) the steps[c] unscaled entries of exp(t_i T_c) e_1
 * and zeros behind them; on_device[c m + i] = 0 where the kernel handed (c, i) back (that
 * column then 0). Column (c m + i) and its entry are bitwise tpl_op_ftk_device(op, 1, ...)
 * on t_i * alphas_c, t_i * betas_c.                                                    */
tpl_status tpl_op_ftk_exp_times_batch_device(tpl_op_t op, const double* alphas,
                                             const double* betas, size_t ld, const size_t* steps,
                                             size_t nb, const double* ts, size_t m, double* y_out,
                                             int32_t* on_device);

/* ---- low-level API: src/algorithms/ -------------------------------------- */
/* Per-step callback of lanczos_standard (LanczosCallback, src/algorithms/mod.rs:82-86):
 * called after every step with k = steps so far (1-based), the DEVICE pointer of
 * V_k (column-major, ld = n, k valid columns) and the host T_k scalars
 * (k alphas, k-1 betas... exactly the reference's TridiagonalSystemView, i.e.
 * betas holds the betas pushed so far). Return non-zero to continue, 0 to stop.
 * The host polls in batches (1, 2, 4, ... up to 32 steps run ahead on the device, then
 * the callback for each of them in order): a stop at step j returns exactly the
 * j-step result (later steps never change earlier coefficients or columns), with one
 * host synchronisation per batch. Columns past k may already hold later basis
 * vectors while the callback runs; only the first k are the view.               */
typedef int (*tpl_step_cb)(size_t k, const double* v_k_device, int64_t n,
                           const double* alphas, size_t n_alphas, const double* betas,
                           size_t n_betas, void* user);

/* algorithms::lanczos::lanczos_standard (src/algorithms/lanczos.rs:55-156).
 * alphas: capacity k; betas: capacity k (k-1 used); v_out: n x k capacity or NULL.
 * On return *steps = steps_taken, *b_norm = ||b||, alphas[0..steps), betas[0..steps-1),
 * v_out columns [0, steps) filled. reorth enables full re-orthogonalisation against
 * the stored V_k (an extension with no reference counterpart): 1 = CGS2 (classical
 * Gram-Schmidt, two passes every step), 2 = selective (Kahan–Parlett "twice is
 * enough": the second pass only when the first removed more than half of ||r||^2;
 * tpl_op_reorth_second_passes reports how many ran), 0 = none.                  */
tpl_status tpl_lanczos_standard(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                double* alphas, double* betas, size_t* steps,
                                double* b_norm, double* v_out, int mem, int reorth,
                                tpl_step_cb cb, void* cb_user);

/* algorithms::lanczos_two_pass::lanczos_pass_one (src/algorithms/lanczos_two_pass.rs:65-110). */
tpl_status tpl_lanczos_pass_one(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                double* alphas, double* betas, size_t* steps,
                                double* b_norm, int mem);

/* algorithms::lanczos_two_pass::lanczos_pass_two (:128-140) and, with v_out != NULL,
 * lanczos_pass_two_with_basis (:149-166). The decomposition is passed as its
 * fields (LanczosDecomposition, src/algorithms/mod.rs:94-108); y = y_k (already
 * scaled by ||b||) with y_len entries. x_out: n entries; v_out: n x steps or NULL. */
tpl_status tpl_lanczos_pass_two(tpl_op_t op, const double* b, int64_t b_len,
                                const double* alphas, size_t n_alphas, const double* betas,
                                size_t n_betas, size_t steps, double b_norm,
                                const double* y, size_t y_len, double* x_out,
                                double* v_out, int mem);

/* lanczos_pass_two for m coefficient vectors over one decomposition: y is column-major
 * y_len x m (y_len must equal steps: ParameterMismatch `y_k`), x_out column-major n x m
 * (leading dimension n); the basis is regenerated once. Column i is bitwise
 * tpl_lanczos_pass_two's x for y's column i. Single-GPU operators; 1 <= m <= TPL_MULTI_MAX. */
tpl_status tpl_lanczos_pass_two_multi(tpl_op_t op, const double* b, int64_t b_len,
                                      const double* alphas, size_t n_alphas,
                                      const double* betas, size_t n_betas, size_t steps,
                                      double b_norm, const double* y, size_t y_len, size_t m,
                                      double* x_out, int mem);
/* tpl_lanczos_pass_two_multi with a per-column cut: column i takes only the first
 * col_steps[i] steps (1 <= col_steps[i] <= steps; else TPL_ERR_INVALID_ARGUMENT), so it is
 * bitwise tpl_lanczos_pass_two at steps = col_steps[i] with the first col_steps[i] entries of
 * y's column i. y: column-major with leading dimension ldy >= steps; entries of column i at
 * or past col_steps[i] are never used. The basis is regenerated once, to `steps`.       */
tpl_status tpl_lanczos_pass_two_multi_cut(tpl_op_t op, const double* b, int64_t b_len,
                                          const double* alphas, size_t n_alphas,
                                          const double* betas, size_t n_betas, size_t steps,
                                          double b_norm, const double* y, size_t ldy,
                                          const size_t* col_steps, size_t m, double* x_out,
                                          int mem);

/* ---- data loader: src/utils/data_loader.rs:211-259 (load_kkt_system) ----- */
typedef struct tpl_csr_host {
  int64_t n, nnz;
  int64_t num_nodes, num_arcs; /* KKTSystem::num_nodes / num_arcs */
  int64_t* row_ptr;            /* n + 1 */
  int32_t* col_idx;            /* nnz, ascending within each row  */
  double* vals;                /* nnz */
} tpl_csr_host;
/* Parse a DIMACS .dmx + .qfc pair with the reference's exact semantics
 * (node-index 0 rejected; .qfc read as line 1 = m, then `skip(m).take(m)`
 * one-float-per-line — so the 3-line qfcgen format yields D = empty) and
 * assemble A = [[D, E^T],[E, 0]] as CSR. Free with tpl_csr_host_free.          */
tpl_status tpl_load_kkt_system(const char* dmx_path, const char* qfc_path, tpl_csr_host* out);
void tpl_csr_host_free(tpl_csr_host* csr);
/* Synthetic KKT instance for the scale-out config (BASELINE.json configs[4]; the
 * reference's netgen stops at 1.1M arcs, data/netgen/src/netgen.h:69-70): num_arcs arcs
 * (u, v), u != v, from a splitmix64 stream seeded by `seed`, with the netgen instances'
 * degree spread: each node draws an integer out-weight in [100, 1900]
 * and in-weight in [800, 1200]; tails are drawn in proportion to out-weight, heads to
 * in-weight (total degree / mean ~0.44 .. 1.58 at 5M arcs, like netgen's 0.5 .. 1.57 at
 * 500k). Ordered by (tail, head) like netgen output, D empty (the 3-line qfc case),
 * assembled exactly as tpl_load_kkt_system assembles a parsed .dmx; the same on every
 * platform (integer arithmetic only). num_nodes for a given m follows
 * data/qcnd/pargen.c:41-50: floor((1 + sqrt(1 + 8m/0.75)) / 2).              */
tpl_status tpl_generate_kkt(int64_t num_arcs, int64_t num_nodes, uint64_t seed,
                            tpl_csr_host* out);

/* ---- introspection / measurement ---------------------------------------- */
/* SpMV layout of the operator (DESIGN.md "SpMV layout"): rows with at most
 * short_row_max nnz ("short", ascending) are stored as sliced ELL, 512 rows per
 * chunk, one workgroup each; the n_long longer rows (ascending) are cut into S column
 * slices (tpl_op_slices) handled by XCD-local workgroups and summed by the last
 * arriver.
 * G2 workgroups of E elements run the element-wise kernels (= #norm partials).
 * short_rows_out: n_short int32 or NULL; long_rows_out: n_long int32 or NULL.
 * The CPU oracle uses this to reproduce the device reduction order bit for bit.   */
tpl_status tpl_op_schedule(tpl_op_t op, int32_t* n_short, int32_t* n_long, int32_t* G2,
                           int64_t* E, int32_t* short_rows_out, int32_t* long_rows_out);
/* Layout tuning (rebuilds the layout; 0 = keep): short_row_max (> 0: explicit,
 * -1: the default auto rule T = clamp(2 * median row nnz, 4, 32)), max_g2
 * (default 1024).                                                                */
tpl_status tpl_op_set_schedule(tpl_op_t op, int32_t short_row_max, int32_t max_g2);
/* Column slices S of the long rows (1, 2, 4 or 8; part of the canonical reduction
 * order). tpl_op_set_slices rebuilds the layout with an explicit S
 * (0 = the auto rule: the fewest slices whose share of the vector fits an eighth of an L2,
 * more if a (row, slice) piece would not fit one bin).                          */
tpl_status tpl_op_slices(tpl_op_t op, int32_t* slices);
tpl_status tpl_op_set_slices(tpl_op_t op, int32_t slices);
/* The variant flag F of the layout: which instance of the SpMV-shaped kernels (k_spmv<F>,
 * k_p1_spmv<F> and its siblings, k_p2_spmv<F>) the launchers dispatch to. F = uniform
 * chunk width 1..4 (0: the generic, per-chunk width) | 8 int8 values | 16 uint16 chunk
 * columns | 32 uint16 bin columns | 64 chunk column window in LDS. Every instance
 * computes the same bits; the tests use this to know which one they ran.             */
tpl_status tpl_op_kernel_variant(tpl_op_t op, int32_t* variant);

/* Second Gram-Schmidt passes of the last re-orthogonalised tpl_lanczos_standard call
 * (steps - 1 for CGS2; the count the selective mode actually ran).                */
tpl_status tpl_op_reorth_second_passes(tpl_op_t op, int64_t* count);
/* Device memory the operator holds now, in bytes: its layout (matrix in the engine's
 * format), the ten n-vectors of the recurrence, the solver state and — once a one-pass
 * solve (tpl_lanczos / tpl_lanczos_standard) has run — the basis V_k (8 n k bytes).
 * This is the device-side counterpart of the reference's peak-memory column
 * (src/utils/perf.rs:16-31, results/scalability_*.csv rss_kb): the two-pass variant
 * never allocates V_k.                                                            */
tpl_status tpl_op_device_bytes(tpl_op_t op, uint64_t* bytes);

/* Live timing of the solver's own launches: with timing on, HIP events on the
 * operator's stream bracket pass one's graph and the graph of pass two's step
 * launches (its prologue then runs as a separate launch), so the numbers come from
 * the very launches of the last solve, inside the caller's timed region.
 * pass2_spmv_us / pass2_launches is the average duration of one pass-two step
 * launch (k_p2_spmv), launch gaps included.                                      */
tpl_status tpl_op_enable_timing(tpl_op_t op, int on);
tpl_status tpl_op_pass_timing(tpl_op_t op, double* pass1_us, double* pass2_spmv_us,
                              int64_t* pass2_launches);
/* Live in-graph durations of pass one's two kernels: with timing on, the pass-one graph
 * of a single-GPU two-pass solve with a device f (k >= 11) has workgroup 0 of the
 * k_p1_spmv and k_p1_axpy launches of 8 consecutive middle steps record its start on the
 * GPU's 100 MHz real-time clock; this returns the average start-to-start interval of each
 * kernel (its launch plus the boundary after it, like pass2_spmv_us) over those steps of
 * the last timed solve, and the number of steps.                                   */
tpl_status tpl_op_step_samples(tpl_op_t op, double* p1_spmv_us, double* p1_axpy_us,
                               int32_t* samples);

/* ---- row-partitioned operator over several GPUs ----------
 * One process per GPU. Rank r holds the rows [starts[r], starts[r+1]) of A; every
 * SpMV gathers the full vector with an in-place all-gather (RCCL over xGMI) — or only
 * its halo (tpl_dist_op_create_halo), or, with replicated long rows, their partials
 * (tpl_dist_op_create_replicated) — and alpha / beta combine the ranks' totals (each rank reduces its own partials in the
 * single-GPU canonical order; the R totals are all-gathered and reduced in rank
 * order), so all ranks hold bitwise identical alpha, beta and steps. The solver
 * entry points above take a partitioned operator unchanged; b, x_out and v_out are
 * then this rank's block of rows. All ranks must make the same calls in the same
 * order (collective semantics). Re-orthogonalisation is not supported here.      */
typedef struct tpl_dist_s* tpl_dist_t;
enum { TPL_DIST_ID_BYTES = 128 };
/* Contiguous row blocks balanced by algorithmic bytes (12 per nonzero + 40 per row);
 * host only. starts: nranks + 1 entries.                                           */
tpl_status tpl_dist_partition(int64_t n, const int64_t* row_ptr, int nranks, int64_t* starts);
/* RCCL unique id (rank 0 creates it; the caller broadcasts the bytes).            */
tpl_status tpl_dist_unique_id(uint8_t* id);
tpl_status tpl_dist_create(int device, int rank, int nranks, const uint8_t* id, tpl_dist_t* out);
/* Test transport: all-gathers go through a host callback (recv = the ranks' send
 * buffers concatenated in rank order); synchronous, no graphs.                     */
typedef int (*tpl_allgather_fn)(const void* send, void* recv, size_t bytes_per_rank, void* user);
tpl_status tpl_dist_create_host(int device, int rank, int nranks, tpl_allgather_fn fn, void* user,
                                tpl_dist_t* out);
tpl_status tpl_dist_destroy(tpl_dist_t d);
/* This rank's block: row_ptr (n_local + 1, 0-based), global column indices.
 * Every SpMV all-gathers the whole vector (8n bytes moved per SpMV).              */
tpl_status tpl_dist_op_create_csr(tpl_dist_t d, int64_t n_global, const int64_t* starts,
                                  const int64_t* row_ptr, const int32_t* col_idx,
                                  const double* vals, tpl_op_t* out);
/* Replicated-long-row partition (the structure-aware split of SURVEY.md §8(e)), from
 * the WHOLE matrix (every rank passes the same CSR): the short rows are split into
 * contiguous byte-balanced blocks; the long rows are replicated — each rank sums the
 * entries in the columns it owns, the n_long partials are all-gathered (8 n_long
 * bytes per rank per SpMV) and every rank finishes them in rank order. Needs no halo:
 * a short row may only reference its own block and the long rows (true for the KKT
 * matrices: arc rows reference node rows only), else TPL_ERR_UNSUPPORTED.
 * This rank's vector is [its short rows | all long rows] (tpl_op_local_rows).        */
tpl_status tpl_dist_op_create_replicated(tpl_dist_t d, int64_t n, const int64_t* row_ptr,
                                         const int32_t* col_idx, const double* vals,
                                         tpl_op_t* out);
/* Halo-exchange row blocks (the general form of SURVEY.md §8(e) for matrices without
 * the KKT structure), from the WHOLE matrix (every rank passes the same CSR): rank r
 * holds the rows [starts[r], starts[r+1]) (starts NULL: the tpl_dist_partition split),
 * exactly as tpl_dist_op_create_csr, but an SpMV moves only the halo — the rows of each
 * block that another rank's rows reference (B_q for rank q, H = max_q |B_q|): each
 * rank packs its B_r into its slot and the slots are all-gathered (8 H bytes per rank
 * instead of 8 n / nranks; a banded matrix of half-bandwidth w has H <= 2w). Same
 * rows, layout and reduction order as tpl_dist_op_create_csr over the same split, so
 * alpha, beta, steps and x are bitwise those of the plain row blocks.
 * Like the two partitions above, it spreads the reference's one sequential
 * operator.apply (src/algorithms/mod.rs:177) over the ranks.                          */
tpl_status tpl_dist_op_create_halo(tpl_dist_t d, int64_t n, const int64_t* starts,
                                   const int64_t* row_ptr, const int32_t* col_idx,
                                   const double* vals, tpl_op_t* out);
/* The partition every binding's "auto" takes (Python mode="auto", C++ / Rust
 * Partition::Auto), decided on the host from the WHOLE matrix for `nranks` ranks, the same
 * on every rank: TPL_PLAN_REPLICATED when the replicated-long-row split applies (no short
 * row references another rank's short rows — the KKT case), else TPL_PLAN_HALO when the
 * halo width H is at most half the widest row block (banded, mesh-like matrices), else
 * TPL_PLAN_ROWS (the whole vector all-gathered; the three hold the same bits as their
 * partition oracles, and halo and rows the same bits as each other).                */
tpl_status tpl_dist_choose_partition(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                                     int nranks, int* mode);
/* This rank's part of the WHOLE matrix in the partition tpl_dist_choose_partition picks
 * (collective: every rank passes the same CSR); *mode (may be NULL) receives it.    */
tpl_status tpl_dist_op_create_auto(tpl_dist_t d, int64_t n, const int64_t* row_ptr,
                                   const int32_t* col_idx, const double* vals, tpl_op_t* out,
                                   int* mode);
/* Global row index of each entry of this operator's vectors (tpl_op_nrows entries). */
tpl_status tpl_op_local_rows(tpl_op_t op, int64_t* rows);

/* Identity key of a caller's compressed-sparse matrix (host only, no device call), for
 * bindings that accept the caller's own matrix per call and keep its upload (the Rust
 * shim's `HipOperand for SparseColMatRef`, integration/rust/hip.rs): key[0] hashes the
 * three arrays' addresses and lengths and n; key[1] an FNV-1a checksum of the first and
 * last 8 words of each array and `samples` evenly spaced ones. The cost is O(samples),
 * not O(nnz): a change of addresses, sizes or any sampled word is seen, a change of an
 * unsampled word is not (callers that mutate a matrix in place re-upload explicitly).
 * ptr_elem / idx_elem: 4 or 8 (bytes per index).                                      */
tpl_status tpl_operand_key(int64_t n, const void* ptr_arr, size_t ptr_len, size_t ptr_elem,
                           const void* idx_arr, size_t idx_len, size_t idx_elem,
                           const double* vals, size_t nnz, size_t samples, uint64_t* key);

/* ---- host-only plans (no GPU): the reduction order an operator would hold --------
 * The host half of tpl_op_create_csr (mode TPL_PLAN_SINGLE: auto locality order, its
 * group count pinned by order_groups > 0 as tpl_op_set_order_groups does; nranks 1,
 * rank 0), of tpl_dist_op_create_replicated (TPL_PLAN_REPLICATED) or of a row-block
 * rank with the tpl_dist_partition split (TPL_PLAN_ROWS; TPL_PLAN_HALO: of
 * tpl_dist_op_create_halo, whose tpl_kernel_algo_bytes of the exchange ids then give
 * the halo's bytes without a GPU), run by the same code: rank
 * `rank` of `nranks`, its rows, order and SpMV layout, and nothing on a device. Only
 * the host introspection calls accept the returned handle — tpl_op_nrows, tpl_op_nnz,
 * tpl_op_flags, tpl_op_schedule, tpl_op_slices, tpl_op_kernel_variant, tpl_op_permutation,
 * tpl_op_local_rows, tpl_op_order_groups, tpl_kernel_algo_bytes — every other call returns
 * TPL_ERR_INVALID_ARGUMENT; free it with tpl_op_destroy. The parity fixtures use it to
 * restate a run's reduction order on a host without a GPU (tests/golden/make_parity.py). */
enum { TPL_PLAN_SINGLE = 0, TPL_PLAN_REPLICATED = 1, TPL_PLAN_ROWS = 2, TPL_PLAN_HALO = 3 };
tpl_status tpl_plan_create(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                           const double* vals, int mode, int nranks, int rank,
                           int32_t order_groups, tpl_op_t* out);

/* Kernel ids for tpl_profile_kernel */
enum {
  TPL_KERNEL_PASS1_SPMV = 0, /* pass one: SpMV + beta-AXPY + alpha partials             */
  TPL_KERNEL_PASS1_AXPY = 1, /* pass one: alpha-AXPY + ||w||^2 partials                 */
  TPL_KERNEL_PASS2_SPMV = 2, /* pass two: SpMV + both AXPYs + scale + x += y v          */
  TPL_KERNEL_SPMV = 3,       /* plain y = A x                                           */
  /* partitioned operators only (SURVEY.md §8(e) "comm fraction"): the exchanges one
   * step issues, exactly as the pass graphs issue them (rank totals + all-gathers)  */
  TPL_KERNEL_EXCHANGE_P1 = 4, /* a pass-one step's exchanges                           */
  TPL_KERNEL_EXCHANGE_P2 = 5, /* a pass-two step's exchange                            */
  TPL_KERNEL_PASS1_STEP = 6   /* k_p1_spmv then k_p1_axpy (one pass-one step, fixed j)  */
};
/* Time `iters` back-to-back launches of one kernel on the operator's stream with
 * HIP events (a warm-up launch first). Returns the average per launch in
 * microseconds (event-to-event, so it includes the launch gap) and the
 * algorithmic bytes one launch moves ("Algorithmic bytes"). The
 * exchange ids are collective: every rank calls with the same arguments; their
 * bytes are those one rank receives.                                            */
tpl_status tpl_profile_kernel(tpl_op_t op, int kernel, int iters, double* avg_us,
                              double* algo_bytes);
/* Algorithmic bytes of one launch of `kernel` (no GPU work). */
double tpl_kernel_algo_bytes(tpl_op_t op, int kernel);

/* Blocking copy of `bytes` from device memory to host memory (used by callbacks
 * that receive device views, e.g. tpl_step_cb's V_k). */
tpl_status tpl_copy_to_host(void* dst, const void* src_device, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* TPL_H_ */
