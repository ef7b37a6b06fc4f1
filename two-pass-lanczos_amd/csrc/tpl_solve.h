// tpl_solve.h — the steps the solver units share: argument checks, the zero cases, the host
// half of a solve, the uploads of a decomposition, the tolerance solves' stop rule and
// reporter, and the single-column solves the batch solves run for a remainder column.
// Internal: tpl_solvers.cpp (the single-column solves; defines what is declared here unless
// noted), tpl_solvers_multi.cpp (m functions of one b), tpl_solvers_batch.cpp (s right-hand
// sides) and tpl_ftk_device.cpp (the device f(T_k) probes) include it.
#pragma once
#include <cmath>

#include "tpl_op.h"

namespace tpl {

// One-graph solves keep the device f(T_k)'s working rows in LDS (k_ftk_inv: 11 k doubles,
// 120 KB at this k; gfx950 has 160 KiB of LDS per workgroup).
constexpr size_t kDevFtkMaxK = 1365;
// Auto mode: the device inv up to k = 500, the largest k at which it was measured no
// slower than the host round trip it replaces. Its elimination runs during pass one
// (k_p1_axpy's extra workgroup) and its back substitution with Markstein divisions (round
// 4, same box, profiles/r04_ftk_timing.txt: 0.574 vs 0.583 ms at 5k arcs k = 50, 2.390 vs
// 2.412 at 50k k = 200, 9.312 vs 9.315 ms at the 500k headline k = 500); past that the
// serial back substitution grows longer than the round trip (round 5, same box,
// profiles/r05_ftk_timing.txt: 10.36 vs 10.24 ms at 5k arcs k = 1000, 14.16 vs 13.84 at
// k = 1365; 11.18 vs 10.99 and 15.62 vs 15.05 ms at 50k arcs). Mode 1 still takes the
// device inv up to kDevFtkMaxK.
constexpr size_t kDevFtkAutoK = 500;
// The device exp (k_ftk_exp, a Chebyshev expansion: parallel over the rows of T_k) keeps
// 4 k + 4 doubles of dynamic LDS plus 8.2 KB of static arrays: 65.8 KB at this k, which
// gfx950's 160 KiB of LDS per workgroup holds (a 64 KiB part would need k <= 1790).
constexpr size_t kDevExpMaxK = 1800;

// ---- argument checks: one fault each; an entry point composes them in its own order ----
inline void need(bool have) { if (!have) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument"); }
inline void check_count(size_t v, size_t max, const char* msg) {
  if (v == 0 || v > max) fail(TPL_ERR_INVALID_ARGUMENT, msg);
}
inline void check_m(size_t m) {
  check_count(m, TPL_MULTI_MAX, "m must be between 1 and TPL_MULTI_MAX");
}
inline void check_s(size_t s) {
  check_count(s, TPL_BATCH_MAX, "s must be between 1 and TPL_BATCH_MAX");
}
inline void check_tol(double tol) {
  if (!(tol >= 0.0)) fail(TPL_ERR_INVALID_ARGUMENT, "tol must be a number >= 0");
}
inline void check_finite(const double* v, size_t m, const char* msg) {
  for (size_t i = 0; i < m; ++i)
    if (!std::isfinite(v[i])) fail(TPL_ERR_INVALID_ARGUMENT, msg);
}
constexpr const char* kTimesFinite = "every time t_i must be finite";
constexpr const char* kShiftsFinite = "every shift sigma_i must be finite";
// what: the kind of solve a partitioned operator does not run
constexpr const char* kMultiSolve = "multi-function solve";
constexpr const char* kBatchSolve = "batch solve";
constexpr const char* kBatchMultiSolve = "batch-multi solve";
inline void refuse_partitioned(const tpl_op_s* op, const char* what) {
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, std::string(what) + " of a partitioned operator");
}
// What most multi-function and batch entry points check first; the device is current after.
inline void check_multi(tpl_op_s* op, bool have_args, size_t m) {
  need(op && have_args), check_m(m), set_device(op), refuse_partitioned(op, kMultiSolve);
}
inline void check_batch_args(tpl_op_s* op, bool have_args, size_t s) {
  need(op && have_args), refuse_dense(op, kBatchSolve);
  check_s(s), set_device(op), refuse_partitioned(op, kBatchSolve);
}
inline void check_batch_multi_args(tpl_op_s* op, bool have_args, size_t s, size_t m) {
  need(op && have_args), refuse_dense(op, kBatchMultiSolve);
  check_s(s), check_m(m), set_device(op);
  refuse_partitioned(op, kBatchMultiSolve);
}
void check_k(size_t k);

// The zero-b failure in the reference's two wordings: of the solves and pass one
// (src/solvers.rs), and of a stand-alone pass two (src/algorithms/lanczos_two_pass.rs:229-235).
constexpr const char* kZeroInput = "Input vector `b` must not be a zero vector.";
constexpr const char* kZeroInitial = "The initial vector `b` must not be a zero vector.";
// The decomposition a stand-alone pass two is handed: ||b||, and arrays that hold `steps` steps.
inline void check_b_norm(double b_norm) { if (b_norm <= kBreakdownTol) fail_input(kZeroInitial); }
[[noreturn]] inline void fail_short_decomp() {
  fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
}
inline void check_decomp_arrays(const double* alphas, size_t n_alphas, const double* betas,
                                size_t n_betas, size_t steps, bool have_y) {
  if (n_alphas < steps || n_betas + 1 < steps || !alphas || (steps > 1 && !betas) || !have_y)
    fail_short_decomp();
}
inline void check_steps_fit(size_t steps) {
  if (steps > (size_t)INT32_MAX / 2) fail(TPL_ERR_INVALID_ARGUMENT, "steps too large");
}

// ---- scopes ----------------------------------------------------------------------------
// For the length of a two-pass solve whose bit (TPL_LONG_CACHE_*) is in the operator's
// solver mask: every pass one of the call stores the long rows' sums in the long-row cache
// and the pass two that follows it reads them (tpl_passes.cpp cache_row, batch_cache_row) —
// a batch call's groups in the group's cache, its remainder column in the single solve's,
// so one call is cached throughout or not at all. Only the four two-pass solvers open one,
// so every other pass runs the full kernels and never reads a row another solve wrote.
struct LongCacheScope {
  tpl_op_s* op;
  // k: the steps a tpl_lanczos_two_pass call asked for (its pass two may run fused:
  // tpl_op.h fused_p2); 0 from every other solver
  LongCacheScope(tpl_op_s* o, unsigned bit, size_t k = 0) : op(o) {
    op->use_long_cache = (op->long_cache_solvers & bit) != 0;
    op->last_long_cache = false;
    op->last_fused_p2 = false;
    op->fused_call_k = k;
  }
  ~LongCacheScope() {
    op->use_long_cache = false;
    op->fused_call_k = 0;
  }
};
// The multi solves record no live timing: tpl_op_pass_timing keeps the last single
// solve's events.
struct TimingOff {
  tpl_op_s* op;
  bool was;
  explicit TimingOff(tpl_op_s* o) : op(o), was(o->timing) { op->timing = false; }
  ~TimingOff() { op->timing = was; }
};

// ---- the host half of a solve ------------------------------------------------------------
void call_ftk(tpl_ftk_fn f, void* user, const HostDecomp& d, std::vector<double>& y);
// m result columns of zeros (a device x_out: synchronises per column).
void zero_out(tpl_op_s* op, double* x_out, int mem, size_t m = 1);
// What a pass's flags decide before any f(T_k): a zero b is an error (kZeroInput), and a pass
// that took no step leaves the zero result (true: the m columns of x_out hold it).
bool zero_result(tpl_op_s* op, const int32_t* flags, double* x_out, int mem, size_t m = 1);
// The zero cases (zero_result), then y' = f(T_k) e_1 by the caller's solver (src/solvers.rs:71-85,
// :155-165), times ||b|| for the two-pass y_k (scale, :169), into the device state. Returns the
// steps taken; 0: the solve is over and x_out holds its zero result (:64-66, :150-152).
size_t host_ftk(tpl_op_s* op, const HostDecomp& d, tpl_ftk_fn f, void* f_user, bool scale,
                double* x_out, int mem);
// A decomposition out to the caller's arrays (a zero b is an error).
void write_decomp(const HostDecomp& d, double* alphas, double* betas, size_t* steps,
                  double* b_norm);
// Where a k-step solve evaluates f(T_k): on the device for the built-in inv / exp of an
// operator that is not partitioned, up to the mode's k (tpl_op_set_device_ftk).
DevF device_f(const tpl_op_s* op, tpl_ftk_fn f, size_t k);
// The exp-times solves evaluate their exp(t_i T_k) e_1 on the device.
inline bool exp_on_device(const tpl_op_s* op, size_t k) {
  return op->device_ftk != 0 && k <= kDevExpMaxK;
}
// A time the device handed back (without the device: every time): y = ||b|| exp(t T_k) e_1 by
// the host solver (scratch y) into `col`, which lives until the caller's next synchronisation,
// and from there to `dst` on the device. No step: the solver is still called, nothing uploaded.
void exp_col_on_host(tpl_op_s* op, const HostDecomp& d, double t, std::vector<double>& y,
                     double* col, double* dst);

// ---- a decomposition into the device state -----------------------------------------------
// norms[0], alphas, betas -> S.norms, S.alphas, S.betas on the stream (ensure_state first). The
// copies are async: every source, b_norm included, lives until the caller's next synchronisation.
void upload_decomp(tpl_op_s* op, const double& b_norm, const double* alphas, const double* betas,
                   size_t steps);
// The solver state as pass one leaves it after n steps, for the probes: no error, no row
// eliminated, no shift stopped (`flags`: filled here, alive until the next sync), ||b|| = 1.
void seed_state(tpl_op_s* op, int32_t (&flags)[kFlagBytes / 4], const double* alphas,
                const double* betas, size_t n);

// Host mirror of a group's state head: flags | norms | alphas | betas (| y), laid out as
// ensure_batch laid out the device block.
struct GroupHead {
  std::vector<double> h;
  size_t w, kc;
  explicit GroupHead(const tpl_op_s* op) : w((size_t)op->bat.nb), kc(op->bat.kcap) {
    h.assign(w * (kFlagBytes / sizeof(double)) + w * (4 * kc + 1), 0.0);
  }
  int32_t* flags(size_t c) { return reinterpret_cast<int32_t*>(h.data()) + 8 * c; }
  double* norms(size_t c) { return h.data() + w * (kFlagBytes / sizeof(double)) + c * (kc + 1); }
  double* alphas(size_t c) { return norms(0) + w * (kc + 1) + c * kc; }
  double* betas(size_t c) { return alphas(0) + w * kc + c * kc; }
  double* y(size_t c) { return betas(0) + w * kc + c * kc; }
  size_t bytes() const { return h.size() * sizeof(double); }
  size_t decomp_bytes() const { return (h.size() - w * kc) * sizeof(double); }
  HostDecomp decomp(size_t c) {
    HostDecomp d;
    std::memcpy(d.flags, flags(c), kFlagBytes);
    d.b_norm = norms(c)[0];
    d.alphas = alphas(c);
    d.betas = betas(c);
    d.steps = (size_t)d.flags[2];
    return d;
  }
  // Column c as pass one leaves it after `steps` steps (al, be: not read where no step needs them).
  void set_column(size_t c, size_t steps, double b_norm, const double* al, const double* be) {
    flags(c)[2] = (int32_t)steps;
    norms(c)[0] = b_norm;
    if (steps > 0) std::memcpy(alphas(c), al, steps * sizeof(double));
    if (steps > 1) std::memcpy(betas(c), be, (steps - 1) * sizeof(double));
  }
  // The first `bytes` of the mirror (decomp_bytes(): without y) to the group's device state; the
  // mirror lives until the caller's next synchronisation.
  void upload(tpl_op_s* op, size_t bytes) {
    HIPCHK(hipMemcpyAsync(op->bat.d_state, h.data(), bytes, hipMemcpyHostToDevice, op->stream));
  }
};

// ---- the inverse solves that stop at a residual tolerance ---------------------------------
// What the definition gives on one decomposition: the residual history of its leading blocks
// (tpl_ftk_inv_residuals), the stop rule — the smallest m in 1 .. steps - 1 with res[m - 1] <=
// tol, else steps — and y = ||b|| tpl_ftk_inv on the first m* rows: the device paths' oracle.
struct TolCol {
  size_t steps = 0;
  bool converged = false;
  std::vector<double> res, y;
};
TolCol tol_col(const double* alphas, const double* betas, size_t steps, double b_norm, double tol);
// The same for one shift: the shifted diagonal (alphas[j] + sigma, one addition per entry).
TolCol shifted_col(const HostDecomp& d, double sigma, double tol);
// Where a tolerance solve reports result e: steps[e], converged[e], res_len[e] and the history
// at res_out + e kmax. Every output may be NULL.
struct TolReport {
  size_t* steps;
  int32_t* converged;
  double* res_out;
  size_t* res_len;
  size_t kmax;
  // the reporter of the results from e0 on
  TolReport at(size_t e0) const {
    return {steps ? steps + e0 : nullptr, converged ? converged + e0 : nullptr,
            res_out ? res_out + e0 * kmax : nullptr, res_len ? res_len + e0 : nullptr, kmax};
  }
  void set(size_t e, size_t m_star, bool hit, size_t n_res) const {
    if (steps) steps[e] = m_star;
    if (converged) converged[e] = hit ? 1 : 0;
    if (res_len) res_len[e] = res_out ? n_res : 0;
  }
  void none(size_t e, size_t count = 1) const {
    for (size_t i = 0; i < count; ++i) set(e + i, 0, false, 0);
  }
  void put(size_t e, size_t m_star, bool hit, const double* res, size_t n_res) const {
    if (res_out && n_res) std::memcpy(res_out + e * kmax, res, n_res * sizeof(double));
    set(e, m_star, hit, n_res);
  }
  void put(size_t e, const TolCol& c) const {
    put(e, c.steps, c.converged, c.res.data(), c.res.size());
  }
  // A device column's m results into e0 .. e0 + m: `taken` its steps_taken, hits[i] the step
  // shift i stopped at (0: never), nres[i] the entries of its history, row r of which is at
  // res[r m + i].
  void decode(size_t e0, size_t m, int32_t taken, const int32_t* hits, const int32_t* nres,
              const double* res) const {
    if (taken == 0) return none(e0, m);
    for (size_t i = 0; i < m; ++i) {
      const size_t formed = std::min<size_t>((size_t)nres[i], kmax - 1);
      if (res_out)
        for (size_t r = 0; r < formed; ++r) res_out[(e0 + i) * kmax + r] = res[r * m + i];
      set(e0 + i, hits[i] ? (size_t)hits[i] : (size_t)taken, hits[i] != 0, formed);
    }
  }
};

// ---- the single-column solves a batch solve runs for its remainder column, after the argument
// checks and inside the caller's scopes. tpl_lanczos_two_pass with f(T_k) on the host (have_p1:
// pass one already ran), and tpl_lanczos_pass_two:
void two_pass_host_f(tpl_op_s* op, const double* b, size_t k, tpl_ftk_fn f, void* f_user,
                     double* x_out, int mem, bool have_p1);
void pass_two_one(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                  const double* betas, size_t n_betas, size_t steps, double b_norm,
                  const double* y, size_t y_len, double* x_out, double* v_out, int mem);
// tpl_solvers_multi.cpp: its entry points of these names (pass_two_multi: y's columns ldy apart;
// two_pass_exp_times: on_device m entries or NULL; pass_two_multi_cut_run: the cuts cs[0..m)).
void two_pass_multi(tpl_op_s* op, const double* b, size_t k, const tpl_ftk_fn* fs, void** f_users,
                    size_t m, double* x_out, int mem);
void pass_two_multi(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                    const double* betas, size_t n_betas, size_t steps, double b_norm,
                    const double* y, size_t ldy, size_t m, double* x_out, int mem);
void two_pass_exp_times(tpl_op_s* op, const double* b, size_t k, const double* ts, size_t m,
                        double* x_out, int mem, int32_t* on_device);
void shifted_inv_tol_one(tpl_op_s* op, const double* b, size_t kmax, const double* sigmas,
                         size_t m, double tol, double* x_out, int mem, const TolReport& rep);
void pass_two_multi_cut_run(tpl_op_s* op, const double* b, const double* alphas,
                            const double* betas, size_t steps, double b_norm, const double* y,
                            size_t ldy, const int32_t* cs, size_t m, double* x_out, int mem);

} // namespace tpl
