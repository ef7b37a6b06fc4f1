// tpl_solvers.cpp — the solver entry points of the C ABI (include/tpl.h): the SpMV, the
// passes on their own, and the one- and two-pass solves with their f(T_k) on the host or
// on the device.
#include <cmath>

#include "tpl_op.h"

using namespace tpl;

namespace {
// Callback polling (tpl_lanczos_standard with a step callback): largest batch of steps
// run ahead of the host callback.
constexpr int kCbBatchMax = 32;
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

void check_k(size_t k) {
  // The reference panics at k = 0 (Vec::with_capacity(k - 1) underflow,
  // src/algorithms/lanczos.rs:75); the C ABI reports it instead.
  if (k == 0) fail_input("The number of iterations `k` must be at least 1.");
  if (k > (size_t)INT32_MAX / 2) fail(TPL_ERR_INVALID_ARGUMENT, "k too large");
}

void call_ftk(tpl_ftk_fn f, void* user, const HostDecomp& d, std::vector<double>& y) {
  if (!f) fail(TPL_ERR_INVALID_ARGUMENT, "f_tk_solver is NULL");
  y.assign(d.steps, 0.0);
  size_t ylen = d.steps;
  char err[1024];
  err[0] = '\0';
  const int rc = f(d.alphas, d.steps, d.betas, d.steps > 0 ? d.steps - 1 : 0, y.data(), d.steps,
                   &ylen, err, sizeof(err), user);
  err[sizeof(err) - 1] = '\0';
  if (rc != 0) fail_solver(err);
  if (ylen != d.steps)
    fail_param_mismatch("y_k_prime", d.steps, ylen);
}

void zero_out(tpl_op_s* op, double* x_out, int mem) {
  if (op->part.n == 0) return;
  if (mem == TPL_MEM_DEVICE) {
    HIPCHK(hipMemsetAsync(x_out, 0, op->part.n * sizeof(double), op->stream));
    sync_checked(op);
  } else {
    std::memset(x_out, 0, op->part.n * sizeof(double));
  }
}

// What a pass's flags decide before any f(T_k): a zero b is an error, and a pass that
// took no step leaves the zero result (true: x_out holds it).
bool zero_result(tpl_op_s* op, const int32_t* flags, double* x_out, int mem) {
  if (flags[1]) fail_input("Input vector `b` must not be a zero vector.");
  if (flags[2] != 0) return false;
  zero_out(op, x_out, mem);
  return true;
}

// The host half of a solve, between the passes: the zero cases (zero_result), then
// y' = f(T_k) e_1 by the caller's solver (src/solvers.rs:71-85, :155-165), times ||b|| for
// the two-pass y_k (scale, :169), into the device state. Returns the steps taken; 0: the
// solve is over and x_out holds its zero result (:64-66, :150-152).
size_t host_ftk(tpl_op_s* op, const HostDecomp& d, tpl_ftk_fn f, void* f_user, bool scale,
                double* x_out, int mem) {
  if (zero_result(op, d.flags, x_out, mem)) return 0;
  std::vector<double> y;
  call_ftk(f, f_user, d, y);
  if (scale)
    for (auto& v : y) v = v * d.b_norm;
  HIPCHK(hipMemcpyAsync(op->st.S.y, y.data(), d.steps * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  return d.steps;
}

// A decomposition out to the caller's arrays (a zero b is an error).
void write_decomp(const HostDecomp& d, double* alphas, double* betas, size_t* steps,
                  double* b_norm) {
  if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
  std::memcpy(alphas, d.alphas, d.steps * sizeof(double));
  if (d.steps > 1) std::memcpy(betas, d.betas, (d.steps - 1) * sizeof(double));
  *steps = d.steps;
  *b_norm = d.b_norm;
}

// The two-pass solve with f(T_k) on the host (have_p1: pass one already ran).
void two_pass_host_f(tpl_op_s* op, const double* b, size_t k, tpl_ftk_fn f, void* f_user,
                     double* x_out, int mem, bool have_p1) {
  // 1. pass one (src/solvers.rs:148)
  op->last_one_graph = false;
  if (!have_p1) run_pass_one(op, b, k, mem, false, false);
  // 2. f(T_k) e_1 on the host (:155-165), 3. y = y' * ||b|| (:169)
  const size_t steps = host_ftk(op, fetch_decomp(op), f, f_user, true, x_out, mem);
  if (steps == 0) return;
  // 4. pass two (:174)
  run_pass2(op, steps);
  download_vec(op, x_out, op->x, 1, mem);
  sync_checked(op);
}

// Pass two for one decomposition (tpl_lanczos_pass_two after its argument checks).
void pass_two_one(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                  const double* betas, size_t n_betas, size_t steps, double b_norm,
                  const double* y, size_t y_len, double* x_out, double* v_out, int mem) {
  // src/algorithms/lanczos_two_pass.rs:220-227
  if (steps != y_len) fail_param_mismatch("y_k", steps, y_len);
  // :229-235
  if (b_norm <= kBreakdownTol)
    fail_input("The initial vector `b` must not be a zero vector.");
  if (steps == 0) { // :237-244
    zero_out(op, x_out, mem);
    return;
  }
  if (n_alphas < steps || n_betas + 1 < steps || !alphas || (steps > 1 && !betas) || !y)
    fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
  ensure_state(op, steps);
  // decomposition -> device: norms[0], alphas, betas, y
  const DevState& S = op->st.S;
  HIPCHK(hipMemcpyAsync(S.norms, &b_norm, sizeof(double), hipMemcpyHostToDevice, op->stream));
  HIPCHK(hipMemcpyAsync(S.alphas, alphas, steps * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  if (steps > 1)
    HIPCHK(hipMemcpyAsync(S.betas, betas, (steps - 1) * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
  HIPCHK(hipMemcpyAsync(S.y, y, steps * sizeof(double), hipMemcpyHostToDevice, op->stream));
  upload_vec(op, op->b, b, mem);
  if (v_out) {
    ensure_basis(op, steps);
    enqueue_pass2(op, steps, op->d_V);
  } else {
    run_pass2(op, steps);
  }
  download_vec(op, x_out, op->x, 1, mem);
  if (v_out) download_vec(op, v_out, op->d_V, (int64_t)steps, mem);
  sync_checked(op);
}

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

// Where a k-step solve evaluates f(T_k): on the device for the built-in inv / exp of an
// operator that is not partitioned, up to the mode's k (tpl_op_set_device_ftk).
DevF device_f(const tpl_op_s* op, tpl_ftk_fn f, size_t k) {
  const bool is_inv = f == &tpl_ftk_inv, is_exp = f == &tpl_ftk_exp;
  const size_t kmax = !op->device_ftk ? 0
                      : is_inv ? (op->device_ftk == 1 ? kDevFtkMaxK : kDevFtkAutoK)
                      : is_exp ? kDevExpMaxK : 0;
  if ((!is_inv && !is_exp) || op->dist || k > kmax) return kDevHost;
  return is_exp ? kDevExp : kDevInv;
}

} // namespace

extern "C" {

tpl_status tpl_op_apply(tpl_op_t op, const double* x, double* y, int mem) {
  return guarded([&] {
    if (!op || ((!x || !y) && op->part.n > 0)) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    if (op->part.n == 0) return;
    upload_vec(op, op->tmp, x, mem);
    if (op->dist && !op->part.hybrid) {
      halo_pack(op, op->tmpG);
      gather_vec(op, op->tmpG);
    }
    const CsrDev A = csr_dev(op);
    HIPCHK(launch::spmv(A, op->tmpG, op->W, op->stream));
    if (op->part.hybrid && A.n_long > 0) {
      dist_allgather(op, op->d_yall, (size_t)A.y_ld);
      HIPCHK(launch::long_epi_y(A, op->d_yall, op->dist->nranks, op->W, op->stream));
    }
    download_vec(op, y, op->W, 1, mem);
    sync_checked(op);
  });
}

tpl_status tpl_lanczos_pass_one(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                double* alphas, double* betas, size_t* steps, double* b_norm,
                                int mem) {
  return guarded([&] {
    if (!op || !alphas || !betas || !steps || !b_norm)
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    check_b(op, b, b_len);
    check_k(k);
    run_pass_one(op, b, k, mem, false, false);
    write_decomp(fetch_decomp(op), alphas, betas, steps, b_norm);
  });
}

tpl_status tpl_lanczos_standard(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                double* alphas, double* betas, size_t* steps, double* b_norm,
                                double* v_out, int mem, int reorth, tpl_step_cb cb,
                                void* cb_user) {
  return guarded([&] {
    if (!op || !alphas || !betas || !steps || !b_norm)
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    check_b(op, b, b_len);
    check_k(k);
    HostDecomp d;
    if (!cb) {
      if (reorth < 0 || reorth > 2) fail(TPL_ERR_INVALID_ARGUMENT, "reorth must be 0, 1 or 2");
      run_pass_one(op, b, k, mem, true, reorth);
      d = fetch_decomp(op);
    } else {
      // src/algorithms/lanczos.rs:86-128 with the host callback after every step, polled
      // in batches: the device runs a batch of steps ahead (1, 2, 4, ... up to
      // kCbBatchMax steps: at most as many speculative steps as were already confirmed),
      // then the callback sees steps j = first .. last of the batch in order, each with
      // the T_j view of that step (alphas[0..j), betas[0..j-1)) and V's first j columns.
      // A stop at step j truncates the decomposition to j steps: later steps never change
      // earlier alphas, betas or columns, so the result is exactly the one-step-at-a-time
      // result, with one host synchronisation per batch instead of per step.
      ensure_state(op, k, reorth != 0);
      ensure_basis(op, k);
      // the callback's view in the caller's row order: each batch's new columns are
      // gathered into it (reordered operators only)
      double* Vview = ensure_view(op, k);
      upload_vec(op, op->b, b, mem);
      enqueue_p1_prologue(op);
      size_t stop_at = k;
      int batch = 1;
      for (int j0 = 1; j0 <= (int)k;) {
        const int j1 = std::min<int>((int)k, j0 + batch - 1);
        for (int j = j0; j <= j1; ++j) {
          enqueue_p1_step(op, j, (int)k, op->d_V + (size_t)(j - 1) * op->part.n);
          if (reorth && j < (int)k) enqueue_reorth(op, j, reorth);
        }
        if (Vview != op->d_V)
          HIPCHK(launch::permute(op->part.n, j1 - j0 + 1,
                                 Vview + (size_t)(j0 - 1) * op->part.n, op->part.n,
                                 op->d_V + (size_t)(j0 - 1) * op->part.n, op->part.n,
                                 op->bufs.d_iperm, op->stream));
        d = fetch_decomp(op);
        bool go = true;
        for (int j = j0; j <= j1 && go; ++j) {
          if (d.flags[0] && d.steps < (size_t)j) {  // zero b, or breakdown before step j
            stop_at = d.steps;
            go = false;
            break;
          }
          go = cb((size_t)j, Vview, op->part.n, d.alphas, (size_t)j, d.betas, (size_t)j - 1,
                  cb_user) != 0;
          if (!go) stop_at = (size_t)j;
        }
        if (!go) break;
        j0 = j1 + 1;
        batch = std::min(2 * batch, kCbBatchMax);
      }
      d = fetch_decomp(op);
      d.steps = std::min(d.steps, stop_at);
    }
    write_decomp(d, alphas, betas, steps, b_norm);
    // second passes of the steps the caller keeps: a step callback may stop before the
    // device's last step (batched polling runs ahead), so count the kept steps' records
    op->reorth_second = reorth == 1 && d.steps > 1 ? (int64_t)d.steps - 1 : 0;
    if (reorth == 2 && d.steps > 1) {
      std::vector<int> rec(d.steps - 1);
      HIPCHK(hipMemcpy(rec.data(), reorth_records(op), rec.size() * sizeof(int),
                       hipMemcpyDeviceToHost));
      for (int r : rec) op->reorth_second += r;
    }
    if (v_out && d.steps > 0) {
      download_vec(op, v_out, op->d_V, (int64_t)d.steps, mem);
      sync_checked(op);
    }
  });
}

tpl_status tpl_lanczos_pass_two(tpl_op_t op, const double* b, int64_t b_len, const double* alphas,
                                size_t n_alphas, const double* betas, size_t n_betas,
                                size_t steps, double b_norm, const double* y, size_t y_len,
                                double* x_out, double* v_out, int mem) {
  return guarded([&] {
    if (!op || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    check_b(op, b, b_len);
    pass_two_one(op, b, alphas, n_alphas, betas, n_betas, steps, b_norm, y, y_len, x_out, v_out,
                 mem);
  });
}

tpl_status tpl_lanczos_two_pass(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                tpl_ftk_fn f, void* f_user, double* x_out, int mem) {
  return guarded([&] {
    if (!op || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    check_b(op, b, b_len);
    check_k(k);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS, k);
    // the built-in inv / exp on the device: the whole solve one graph (pass one, f(T_k)
    // from the device alpha / beta, pass two), no host round trip between the passes
    const DevF dev_f = device_f(op, f, k);
    bool have_p1 = false;  // pass one already ran (the device handed f back to the host)
    if (dev_f != kDevHost) {
      // inv: the host solver's operations in its order, bit for bit (src/solvers.rs:148-174);
      // exp: a parallel evaluation of the same function (k_ftk_exp), EVD-class accuracy
      ensure_state(op, k);
      upload_vec(op, op->b, b, mem);
      run_two_pass_dev(op, k, dev_f);
      download_vec(op, x_out, op->x, 1, mem);
      HIPCHK(hipMemcpyAsync(op->st.h_state, op->st.d_state, kFlagBytes, hipMemcpyDeviceToHost,
                            op->stream));
      sync_checked(op);
      int32_t flags[kFlagBytes / 4];
      std::memcpy(flags, op->st.h_state, kFlagBytes);
      if (zero_result(op, flags, x_out, mem) || !flags[4]) {
        op->last_one_graph = true;
        return;
      }
      // the device handed f(T_k) back (T_k not finite, or a spectrum too wide for the
      // expansion): the host solver on the same decomposition, then pass two again
      have_p1 = true;
    }
    two_pass_host_f(op, b, k, f, f_user, x_out, mem, have_p1);
  });
}

tpl_status tpl_lanczos(tpl_op_t op, const double* b, int64_t b_len, size_t k, tpl_ftk_fn f,
                       void* f_user, double* x_out, int mem) {
  return guarded([&] {
    if (!op || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    set_device(op);
    check_b(op, b, b_len);
    check_k(k);
    // the built-in inv / exp on the device after the standard pass, then the
    // reconstruction: no host round trip (the same rules as tpl_lanczos_two_pass; y'
    // unscaled, the GEMV multiplies by ||b||)
    const DevF dev_f = device_f(op, f, k);
    // 1. standard pass, V_k in HBM (src/solvers.rs:61); a device inv's LU eliminated
    //    during it
    run_pass_one(op, b, k, mem, true, false, dev_f == kDevInv);
    op->last_one_graph = false;
    if (dev_f != kDevHost) {
      enqueue_ftk_only(op, k, dev_f, 0);
      HIPCHK(launch::gemv_recon(op->part.n, -1, op->st.S, op->d_V, op->x, op->stream));
    }
    const HostDecomp d = fetch_decomp(op);
    if (dev_f != kDevHost && !d.flags[1] && d.steps > 0 && !d.flags[4]) {
      op->last_one_graph = true;  // the device's result stands
      download_vec(op, x_out, op->x, 1, mem);
      sync_checked(op);
      return;
    }
    // 2. y' = f(T_k) e_1 on the host (a device exp may hand back: the same V_k) (:71-85)
    const size_t steps = host_ftk(op, d, f, f_user, false, x_out, mem);
    if (steps == 0) return;
    // 3. x = ||b|| V_k y' (:96-104)
    HIPCHK(launch::gemv_recon(op->part.n, (int)steps, op->st.S, op->d_V, op->x, op->stream));
    download_vec(op, x_out, op->x, 1, mem);
    sync_checked(op);
  });
}

} // extern "C"

// ---- f_1(A) b ... f_m(A) b over one Krylov space ------------------------------------
namespace {
// What every multi entry point checks first; leaves the operator's device current.
void check_multi(tpl_op_s* op, bool have_args, size_t m) {
  if (!op || !have_args) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (m == 0 || m > (size_t)TPL_MULTI_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
  set_device(op);
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
}
// The multi solves record no live timing: tpl_op_pass_timing keeps the last single
// solve's events.
struct TimingOff {
  tpl_op_s* op;
  bool was;
  explicit TimingOff(tpl_op_s* o) : op(o), was(o->timing) { op->timing = false; }
  ~TimingOff() { op->timing = was; }
};
void zero_out_cols(tpl_op_s* op, double* x_out, size_t m, int mem) {
  for (size_t i = 0; i < m; ++i) zero_out(op, x_out + i * (size_t)op->part.n, mem);
}
// y'_i = f_i(T_k) e_1 for every function, in index order (the first failure throws),
// times ||b|| when `scale`: steps x m, column-major.
std::vector<double> call_ftks(const tpl_ftk_fn* fs, void** f_users, size_t m,
                              const HostDecomp& d, bool scale) {
  std::vector<double> Y(m * d.steps), y;
  for (size_t i = 0; i < m; ++i) {
    call_ftk(fs[i], f_users ? f_users[i] : nullptr, d, y);
    for (size_t j = 0; j < d.steps; ++j) Y[i * d.steps + j] = scale ? y[j] * d.b_norm : y[j];
  }
  return Y;
}
// The steps x m host table (columns ldy apart) into the device table (columns ycap apart).
void upload_y(tpl_op_s* op, const double* Y, size_t ldy, size_t steps, size_t m) {
  HIPCHK(hipMemcpy2DAsync(op->d_Y, op->ycap * sizeof(double), Y, ldy * sizeof(double),
                          steps * sizeof(double), m, hipMemcpyHostToDevice, op->stream));
}
// tpl_lanczos_two_pass_multi after its argument checks.
void two_pass_multi(tpl_op_s* op, const double* b, size_t k, const tpl_ftk_fn* fs, void** f_users,
                    size_t m, double* x_out, int mem) {
  // 1. pass one, once (the host-f path of tpl_lanczos_two_pass)
  op->last_one_graph = false;
  run_pass_one(op, b, k, mem, false, false);
  const HostDecomp d = fetch_decomp(op);
  if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
  if (d.steps == 0) {
    zero_out_cols(op, x_out, m, mem);
    return;
  }
  // 2. every f_i(T_k) e_1 on the host, 3. y_i = y'_i * ||b||
  const std::vector<double> Y = call_ftks(fs, f_users, m, d, true);
  ensure_multi(op, m);
  upload_y(op, Y.data(), d.steps, d.steps, m);
  // 4. one pass two for all of them
  run_pass2_multi(op, d.steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}
// tpl_lanczos_pass_two_multi after its argument checks (y's columns ldy apart).
void pass_two_multi(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                    const double* betas, size_t n_betas, size_t steps, double b_norm,
                    const double* y, size_t ldy, size_t m, double* x_out, int mem) {
  if (b_norm <= kBreakdownTol)
    fail_input("The initial vector `b` must not be a zero vector.");
  if (steps == 0) {
    zero_out_cols(op, x_out, m, mem);
    return;
  }
  if (n_alphas < steps || n_betas + 1 < steps || !alphas || (steps > 1 && !betas) || !y)
    fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
  if (steps > (size_t)INT32_MAX / 2) fail(TPL_ERR_INVALID_ARGUMENT, "steps too large");
  ensure_state(op, steps);
  ensure_multi(op, m);
  const DevState& S = op->st.S;
  HIPCHK(hipMemcpyAsync(S.norms, &b_norm, sizeof(double), hipMemcpyHostToDevice, op->stream));
  HIPCHK(hipMemcpyAsync(S.alphas, alphas, steps * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  if (steps > 1)
    HIPCHK(hipMemcpyAsync(S.betas, betas, (steps - 1) * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
  upload_y(op, y, ldy, steps, m);
  upload_vec(op, op->b, b, mem);
  run_pass2_multi(op, steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}
// tpl_lanczos_two_pass_exp_times after its argument checks (on_device: m entries or NULL).
void two_pass_exp_times(tpl_op_s* op, const double* b, size_t k, const double* ts, size_t m,
                        double* x_out, int mem, int32_t* on_device) {
  op->last_one_graph = false;
  if (on_device) std::fill(on_device, on_device + m, 0);
  ensure_state(op, k);
  ensure_multi(op, m);
  ensure_exp_times(op);
  // 1. pass one, once; 2. straight behind it on the stream every exp(t_i T_k) e_1 at once
  //    (steps_taken stays on the device), y_i = y'_i * ||b|| into the coefficient table
  const bool dev = op->device_ftk != 0 && k <= kDevExpMaxK;
  if (dev)
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
  run_pass_one(op, b, k, mem, false, false);
  if (dev) {
    HIPCHK(launch::ftk_exp_times(op->st.S, (int)k, op->d_exp_ts, (int)m, op->d_Y, (int)op->ycap,
                                 op->d_exp_back, 1, op->stream));
    HIPCHK(hipMemcpyAsync(op->h_exp_back, op->d_exp_back, m * sizeof(int32_t),
                          hipMemcpyDeviceToHost, op->stream));
  }
  const HostDecomp d = fetch_decomp(op);  // the call's one synchronisation before pass two
  if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
  if (d.steps == 0) {
    zero_out_cols(op, x_out, m, mem);
    return;
  }
  // 3. the times handed back (without the device: all of them) on the host, in index
  //    order; only their columns are uploaded
  std::vector<double> Y, y;
  double t = 0.0;
  for (size_t i = 0; i < m; ++i) {
    if (dev && !op->h_exp_back[i]) continue;
    if (Y.empty()) Y.resize(m * d.steps);
    t = ts[i];
    call_ftk(&tpl_ftk_exp_t, &t, d, y);
    double* col = Y.data() + i * d.steps;
    for (size_t j = 0; j < d.steps; ++j) col[j] = y[j] * d.b_norm;
    HIPCHK(hipMemcpyAsync(op->d_Y + i * op->ycap, col, d.steps * sizeof(double),
                          hipMemcpyHostToDevice, op->stream));
  }
  // 4. one pass two for all of them
  run_pass2_multi(op, d.steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
  if (on_device)
    for (size_t i = 0; i < m; ++i) on_device[i] = dev && !op->h_exp_back[i] ? 1 : 0;
}
} // namespace

extern "C" {

tpl_status tpl_lanczos_two_pass_multi(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                      const tpl_ftk_fn* fs, void** f_users, size_t m,
                                      double* x_out, int mem) {
  return guarded([&] {
    check_multi(op, fs && x_out, m);
    check_b(op, b, b_len);
    check_k(k);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_MULTI);
    two_pass_multi(op, b, k, fs, f_users, m, x_out, mem);
  });
}

tpl_status tpl_lanczos_multi(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                             const tpl_ftk_fn* fs, void** f_users, size_t m, double* x_out,
                             int mem) {
  return guarded([&] {
    check_multi(op, fs && x_out, m);
    check_b(op, b, b_len);
    check_k(k);
    const TimingOff untimed(op);
    op->last_one_graph = false;
    run_pass_one(op, b, k, mem, true, false);
    const HostDecomp d = fetch_decomp(op);
    if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
    if (d.steps == 0) {
      zero_out_cols(op, x_out, m, mem);
      return;
    }
    const std::vector<double> Y = call_ftks(fs, f_users, m, d, false);
    ensure_multi(op, m);
    // x_i = ||b|| V_k y'_i: the single solve's reconstruction, a column at a time
    for (size_t i = 0; i < m; ++i) {
      HIPCHK(hipMemcpyAsync(op->st.S.y, Y.data() + i * d.steps, d.steps * sizeof(double),
                            hipMemcpyHostToDevice, op->stream));
      HIPCHK(launch::gemv_recon(op->part.n, (int)d.steps, op->st.S, op->d_V,
                                op->d_X + i * (size_t)op->ld, op->stream));
    }
    download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
    sync_checked(op);
  });
}

tpl_status tpl_lanczos_pass_two_multi(tpl_op_t op, const double* b, int64_t b_len,
                                      const double* alphas, size_t n_alphas,
                                      const double* betas, size_t n_betas, size_t steps,
                                      double b_norm, const double* y, size_t y_len, size_t m,
                                      double* x_out, int mem) {
  return guarded([&] {
    check_multi(op, x_out != nullptr, m);  // y may be NULL with steps == 0
    check_b(op, b, b_len);
    if (steps != y_len) fail_param_mismatch("y_k", steps, y_len);
    pass_two_multi(op, b, alphas, n_alphas, betas, n_betas, steps, b_norm, y, steps, m, x_out,
                   mem);
  });
}

tpl_status tpl_lanczos_two_pass_exp_times(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                          const double* ts, size_t m, double* x_out, int mem,
                                          int32_t* on_device) {
  return guarded([&] {
    check_multi(op, ts && x_out, m);
    check_b(op, b, b_len);
    check_k(k);
    for (size_t i = 0; i < m; ++i)
      if (!std::isfinite(ts[i])) fail(TPL_ERR_INVALID_ARGUMENT, "every time t_i must be finite");
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_MULTI);
    two_pass_exp_times(op, b, k, ts, m, x_out, mem, on_device);
  });
}

tpl_status tpl_lanczos_two_pass_inv_tol(tpl_op_t op, const double* b, int64_t b_len, size_t kmax,
                                        double tol, double* x_out, int mem, size_t* steps,
                                        int32_t* converged, double* res_out, size_t* res_len) {
  return guarded([&] {
    if (!op || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(tol >= 0.0)) fail(TPL_ERR_INVALID_ARGUMENT, "tol must be a number >= 0");
    set_device(op);
    check_b(op, b, b_len);
    check_k(kmax);
    auto report = [&](size_t m, bool hit, const double* res, size_t n_res) {
      if (steps) *steps = m;
      if (converged) *converged = hit ? 1 : 0;
      if (res_out && n_res) std::memcpy(res_out, res, n_res * sizeof(double));
      if (res_len) *res_len = res_out ? n_res : 0;
    };
    // the stop rule on a history of `formed` entries after `taken` steps: the smallest m in
    // 1 .. taken - 1 with res[m - 1] <= tol, else taken
    auto first_hit = [&](const double* res, size_t formed, size_t taken) -> size_t {
      for (size_t m = 1; m < taken && m <= formed; ++m)
        if (res[m - 1] <= tol) return m;
      return 0;
    };
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS, kmax);
    const TimingOff untimed(op);
    if (device_f(op, &tpl_ftk_inv, kmax) == kDevInv) {
      // one graph: pass one watching the residual, k_ftk_inv on the m* rows, pass two
      ensure_state(op, kmax);
      ensure_tol(op);
      upload_vec(op, op->b, b, mem);
      const int32_t zero[2] = {0, 0};
      HIPCHK(hipMemcpyAsync(op->st.S.flags + 6, zero, sizeof(zero), hipMemcpyHostToDevice,
                            op->stream));
      HIPCHK(hipMemcpyAsync(op->d_tol, &tol, sizeof(double), hipMemcpyHostToDevice, op->stream));
      run_two_pass_inv_tol(op, kmax);
      download_vec(op, x_out, op->x, 1, mem);
      char* h = (char*)op->h_tol;
      HIPCHK(hipMemcpyAsync(h, op->st.d_state, kFlagBytes, hipMemcpyDeviceToHost, op->stream));
      if (kmax > 1)
        HIPCHK(hipMemcpyAsync(h + kFlagBytes, op->d_tol + 1, (kmax - 1) * sizeof(double),
                              hipMemcpyDeviceToHost, op->stream));
      sync_checked(op);
      int32_t flags[kFlagBytes / 4];
      std::memcpy(flags, h, kFlagBytes);
      const bool zero_x = zero_result(op, flags, x_out, mem);
      op->last_one_graph = true;
      const size_t formed = std::min<size_t>((size_t)flags[7], kmax - 1);
      report((size_t)flags[2], !zero_x && flags[6] != 0, (const double*)(h + kFlagBytes), formed);
      return;
    }
    // composed on the host: pass one to kmax, the history and the rule, y on the first m*
    // rows, pass two to m* (the oracle of the device path)
    op->last_one_graph = false;
    run_pass_one(op, b, kmax, mem, false, false);
    const HostDecomp d = fetch_decomp(op);
    if (zero_result(op, d.flags, x_out, mem)) {
      report(0, false, nullptr, 0);
      return;
    }
    std::vector<double> res(d.steps);
    size_t formed = 0;
    tpl_ftk_inv_residuals(d.alphas, d.steps, d.betas, d.steps - 1, res.data(), res.size(),
                          &formed);
    const size_t hit = first_hit(res.data(), formed, d.steps);
    const size_t m = hit ? hit : d.steps;
    std::vector<double> y(m);
    size_t ylen = m;
    tpl_ftk_inv(d.alphas, m, d.betas, m - 1, y.data(), m, &ylen, nullptr, 0, nullptr);
    for (auto& v : y) v = v * d.b_norm;
    HIPCHK(hipMemcpyAsync(op->st.S.y, y.data(), m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    run_pass2(op, m);
    download_vec(op, x_out, op->x, 1, mem);
    sync_checked(op);
    report(m, hit != 0, res.data(), formed);
  });
}

} // extern "C"

// ---- (A + sigma_i I)^{-1} b for m shifts, each stopped at the tolerance ------------------
namespace {
// What the definition gives for one shift on pass one's decomposition: the shifted diagonal
// (alphas[j] + sigma, one addition per entry), its residual history, the stop rule, and
// y = ||b|| tpl_ftk_inv on the first m* rows.
struct ShiftedCol {
  size_t steps = 0;
  bool converged = false;
  std::vector<double> res, y;
};
ShiftedCol shifted_col(const HostDecomp& d, double sigma, double tol) {
  ShiftedCol c;
  std::vector<double> a(d.steps);
  for (size_t j = 0; j < d.steps; ++j) a[j] = d.alphas[j] + sigma;
  c.res.resize(d.steps);
  size_t formed = 0;
  tpl_ftk_inv_residuals(a.data(), d.steps, d.betas, d.steps - 1, c.res.data(), c.res.size(),
                        &formed);
  c.res.resize(formed);
  c.steps = d.steps;
  for (size_t m = 1; m < d.steps && m <= formed; ++m)
    if (c.res[m - 1] <= tol) {
      c.steps = m;
      c.converged = true;
      break;
    }
  c.y.resize(c.steps);
  size_t ylen = c.steps;
  tpl_ftk_inv(a.data(), c.steps, d.betas, c.steps - 1, c.y.data(), c.steps, &ylen, nullptr, 0,
              nullptr);
  for (auto& v : c.y) v = v * d.b_norm;
  return c;
}
// The m column step counts into op->d_col_steps.
void upload_col_steps(tpl_op_s* op, const int32_t* cs, size_t m) {
  ensure_col_steps(op);
  HIPCHK(hipMemcpyAsync(op->d_col_steps, cs, m * sizeof(int32_t), hipMemcpyHostToDevice,
                        op->stream));
}
// Auto mode takes the one-graph path up to this kmax, the largest at which it was measured no
// slower than the host-composed path at every m (500k block with D, shifts 1 .. 100, m = 1,
// 4, 8, tol 1e-4 and 1e-8, profiles/shifted_inv_tol_timing.txt: 0.98-1.01 of it at kmax =
// 64). Past it the graph's launches after the stop — two of pass one and 4/3 of pass two per
// step not taken, 3.5 us each — cost more than the host path's pass one run to kmax: 1.04,
// 1.08 and 1.17 of the host path at kmax = 125, 250, 500 for one shift that stops at 116, and
// 1.01-1.02 at kmax = 500 for every m even where a shift never stops. Mode 1 still takes the
// graph up to the device inv's bound.
constexpr size_t kShiftedAutoK = 64;
// The one-graph path: where tpl_lanczos_two_pass_inv_tol takes its own, within the line
// above in auto mode, and only where the sequence can be captured.
bool shifted_on_device(const tpl_op_s* op, size_t kmax) {
  return device_f(op, &tpl_ftk_inv, kmax) == kDevInv &&
         (op->device_ftk == 1 || kmax <= kShiftedAutoK) && use_graphs() && !op->eager;
}
// tpl_lanczos_two_pass_shifted_inv_tol after its argument checks, inside the caller's
// LongCacheScope (the batch solve runs its remainder column through it).
void shifted_inv_tol_one(tpl_op_s* op, const double* b, size_t kmax, const double* sigmas,
                         size_t m, double tol, double* x_out, int mem, size_t* steps,
                         int32_t* converged, double* res_out, size_t* res_len) {
  auto report = [&](size_t i, size_t ms, bool hit, size_t n_res) {
    if (steps) steps[i] = ms;
    if (converged) converged[i] = hit ? 1 : 0;
    if (res_len) res_len[i] = res_out ? n_res : 0;
  };
  ensure_state(op, kmax);
  ensure_multi(op, m);
  ensure_col_steps(op);
  if (shifted_on_device(op, kmax)) {
    // one graph: pass one with a lane per shift, every y_i on its own m*_i rows, pass two
    const launch::ShiftTol t = ensure_stol(op, m);
    upload_vec(op, op->b, b, mem);
    const int32_t zero[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(op->st.S.flags + 6, zero, sizeof(zero), hipMemcpyHostToDevice,
                          op->stream));
    HIPCHK(hipMemsetAsync(t.hits, 0, 2 * op->stol_m * sizeof(int32_t), op->stream));
    HIPCHK(hipMemcpyAsync(op->d_stol, &tol, sizeof(double), hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(op->d_stol + 1, sigmas, m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    run_two_pass_shifted_inv_tol(op, kmax, t);
    download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
    char* h = (char*)op->h_stol;
    int32_t* h_hits = (int32_t*)(h + kFlagBytes);
    double* h_res = (double*)(h + kFlagBytes + 2 * op->stol_m * sizeof(int32_t));
    HIPCHK(hipMemcpyAsync(h, op->st.d_state, kFlagBytes, hipMemcpyDeviceToHost, op->stream));
    HIPCHK(hipMemcpyAsync(h_hits, t.hits, 2 * op->stol_m * sizeof(int32_t),
                          hipMemcpyDeviceToHost, op->stream));
    if (res_out && kmax > 1)
      HIPCHK(hipMemcpyAsync(h_res, t.res, (kmax - 1) * m * sizeof(double),
                            hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    int32_t flags[kFlagBytes / 4];
    std::memcpy(flags, h, kFlagBytes);
    op->last_one_graph = true;
    if (flags[1]) fail_input("Input vector `b` must not be a zero vector.");
    if (flags[2] == 0) {
      zero_out_cols(op, x_out, m, mem);
      for (size_t i = 0; i < m; ++i) report(i, 0, false, 0);
      return;
    }
    const int32_t* h_nres = h_hits + op->stol_m;
    for (size_t i = 0; i < m; ++i) {
      const size_t formed = std::min<size_t>((size_t)h_nres[i], kmax - 1);
      if (res_out)
        for (size_t r = 0; r < formed; ++r) res_out[i * kmax + r] = h_res[r * m + i];
      report(i, h_hits[i] ? (size_t)h_hits[i] : (size_t)flags[2], h_hits[i] != 0, formed);
    }
    return;
  }
  // composed on the host (the oracle of the device path): pass one to kmax, then per shift
  // the history, the rule and y on the first m*_i rows, one pass two of M = max m*_i steps
  op->last_one_graph = false;
  run_pass_one(op, b, kmax, mem, false, false);
  const HostDecomp d = fetch_decomp(op);
  if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
  if (d.steps == 0) {
    zero_out_cols(op, x_out, m, mem);
    for (size_t i = 0; i < m; ++i) report(i, 0, false, 0);
    return;
  }
  std::vector<double> Y(m * d.steps, 0.0);
  int32_t cs[TPL_MULTI_MAX];
  size_t M = 0;
  for (size_t i = 0; i < m; ++i) {
    const ShiftedCol c = shifted_col(d, sigmas[i], tol);
    std::copy(c.y.begin(), c.y.end(), Y.begin() + i * d.steps);
    cs[i] = (int32_t)c.steps;
    M = std::max(M, c.steps);
    if (res_out) std::copy(c.res.begin(), c.res.end(), res_out + i * kmax);
    report(i, c.steps, c.converged, c.res.size());
  }
  upload_y(op, Y.data(), d.steps, M, m);
  upload_col_steps(op, cs, m);
  run_pass2_multi_cut(op, M, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}
// tpl_lanczos_pass_two_multi_cut after its argument checks: the decomposition, the
// coefficient columns and the cuts cs[0..m) to the device, the pass, the result out.
void pass_two_multi_cut_run(tpl_op_s* op, const double* b, const double* alphas,
                            const double* betas, size_t steps, double b_norm, const double* y,
                            size_t ldy, const int32_t* cs, size_t m, double* x_out, int mem) {
  ensure_state(op, steps);
  ensure_multi(op, m);
  const DevState& S = op->st.S;
  HIPCHK(hipMemcpyAsync(S.norms, &b_norm, sizeof(double), hipMemcpyHostToDevice, op->stream));
  HIPCHK(hipMemcpyAsync(S.alphas, alphas, steps * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  if (steps > 1)
    HIPCHK(hipMemcpyAsync(S.betas, betas, (steps - 1) * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
  upload_y(op, y, ldy, steps, m);
  upload_col_steps(op, cs, m);
  upload_vec(op, op->b, b, mem);
  run_pass2_multi_cut(op, steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}
} // namespace

extern "C" {

tpl_status tpl_lanczos_two_pass_shifted_inv_tol(tpl_op_t op, const double* b, int64_t b_len,
                                                size_t kmax, const double* sigmas, size_t m,
                                                double tol, double* x_out, int mem,
                                                size_t* steps, int32_t* converged,
                                                double* res_out, size_t* res_len) {
  return guarded([&] {
    if (!op || !sigmas || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    if (!(tol >= 0.0)) fail(TPL_ERR_INVALID_ARGUMENT, "tol must be a number >= 0");
    for (size_t i = 0; i < m; ++i)
      if (!std::isfinite(sigmas[i]))
        fail(TPL_ERR_INVALID_ARGUMENT, "every shift sigma_i must be finite");
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
    check_b(op, b, b_len);
    check_k(kmax);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_MULTI);
    shifted_inv_tol_one(op, b, kmax, sigmas, m, tol, x_out, mem, steps, converged, res_out,
                        res_len);
  });
}

tpl_status tpl_lanczos_pass_two_multi_cut(tpl_op_t op, const double* b, int64_t b_len,
                                          const double* alphas, size_t n_alphas,
                                          const double* betas, size_t n_betas, size_t steps,
                                          double b_norm, const double* y, size_t ldy,
                                          const size_t* col_steps, size_t m, double* x_out,
                                          int mem) {
  return guarded([&] {
    check_multi(op, x_out != nullptr && col_steps != nullptr && y != nullptr, m);
    check_b(op, b, b_len);
    if (steps == 0 || ldy < steps || steps > (size_t)INT32_MAX / 2)
      fail(TPL_ERR_INVALID_ARGUMENT, "steps must be >= 1 and ldy >= steps");
    int32_t cs[TPL_MULTI_MAX];
    for (size_t i = 0; i < m; ++i) {
      if (col_steps[i] < 1 || col_steps[i] > steps)
        fail(TPL_ERR_INVALID_ARGUMENT, "every col_steps[i] must be between 1 and steps");
      cs[i] = (int32_t)col_steps[i];
    }
    if (b_norm <= kBreakdownTol)
      fail_input("The initial vector `b` must not be a zero vector.");
    if (n_alphas < steps || n_betas + 1 < steps || !alphas || (steps > 1 && !betas))
      fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
    pass_two_multi_cut_run(op, b, alphas, betas, steps, b_norm, y, ldy, cs, m, x_out, mem);
  });
}

tpl_status tpl_op_ftk_inv_shifts_device(tpl_op_t op, const double* alphas, size_t n,
                                        const double* betas, const double* sigmas, size_t m,
                                        double* y_out) {
  return guarded([&] {
    if (!op || !alphas || !sigmas || !y_out || (n > 1 && !betas))
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > kDevFtkMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
    ensure_state(op, n);
    ensure_multi(op, m);
    ensure_col_steps(op);
    const launch::ShiftTol t = ensure_stol(op, m);
    // the solver state as pass one leaves it: steps_taken = n, ||b|| = 1, no error, no row
    // eliminated, no shift stopped
    const int32_t flags[kFlagBytes / 4] = {0, 0, (int32_t)n, 0, 0, 0, 0, 0};
    const double one = 1.0;
    const DevState& S = op->st.S;
    HIPCHK(hipMemcpyAsync(S.flags, flags, kFlagBytes, hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.norms, &one, sizeof(double), hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.alphas, alphas, n * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    if (n > 1)
      HIPCHK(hipMemcpyAsync(S.betas, betas, (n - 1) * sizeof(double), hipMemcpyHostToDevice,
                            op->stream));
    HIPCHK(hipMemsetAsync(t.hits, 0, 2 * op->stol_m * sizeof(int32_t), op->stream));
    HIPCHK(hipMemcpyAsync(op->d_stol + 1, sigmas, m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    HIPCHK(launch::ftk_inv_shifts(S, (int)n, t, op->d_Y, (int)op->ycap, op->d_col_steps, 0,
                                  op->stream));
    HIPCHK(hipMemcpy2DAsync(y_out, n * sizeof(double), op->d_Y, op->ycap * sizeof(double),
                            n * sizeof(double), m, hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
  });
}

tpl_status tpl_op_reorth_second_passes(tpl_op_t op, int64_t* count) {
  return guarded([&] {
    if (!op || !count) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = op->reorth_second;
  });
}

tpl_status tpl_op_set_device_ftk(tpl_op_t op, int mode) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (mode < 0 || mode > 2) fail(TPL_ERR_INVALID_ARGUMENT, "device f(T_k) mode must be 0, 1 or 2");
    op->device_ftk = mode;
  });
}

tpl_status tpl_op_ftk_device(tpl_op_t op, int which, const double* alphas, size_t n,
                             const double* betas, double* y_out, int* on_device) {
  return guarded([&] {
    if (!op || !alphas || !y_out || !on_device || (n > 1 && !betas))
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (which != 0 && which != 1) fail(TPL_ERR_INVALID_ARGUMENT, "which must be 0 (inv) or 1 (exp)");
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > (which == 0 ? kDevFtkMaxK : kDevExpMaxK))
      fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    ensure_state(op, n);
    // the solver state as pass one leaves it: steps_taken = n, ||b|| = 1, no error
    int32_t flags[kFlagBytes / 4] = {0, 0, (int32_t)n, 0, 0, 0, 0, 0};
    const double one = 1.0;
    const DevState& S = op->st.S;
    HIPCHK(hipMemcpyAsync(S.flags, flags, kFlagBytes, hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.norms, &one, sizeof(double), hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.alphas, alphas, n * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    if (n > 1)
      HIPCHK(hipMemcpyAsync(S.betas, betas, (n - 1) * sizeof(double), hipMemcpyHostToDevice,
                            op->stream));
    enqueue_ftk_only(op, n, which == 1 ? kDevExp : kDevInv, 1);
    HIPCHK(hipMemcpyAsync(y_out, S.y, n * sizeof(double), hipMemcpyDeviceToHost, op->stream));
    HIPCHK(hipMemcpyAsync(flags, S.flags, kFlagBytes, hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    *on_device = flags[4] ? 0 : 1;
  });
}

tpl_status tpl_op_ftk_exp_times_device(tpl_op_t op, const double* alphas, size_t n,
                                       const double* betas, const double* ts, size_t m,
                                       double* y_out, int32_t* on_device) {
  return guarded([&] {
    if (!op || !alphas || !ts || !y_out || !on_device || (n > 1 && !betas))
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > kDevExpMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
    ensure_state(op, n);
    ensure_multi(op, m);
    ensure_exp_times(op);
    // the solver state as pass one leaves it: steps_taken = n, ||b|| = 1, no error
    const int32_t flags[kFlagBytes / 4] = {0, 0, (int32_t)n, 0, 0, 0, 0, 0};
    const double one = 1.0;
    const DevState& S = op->st.S;
    HIPCHK(hipMemcpyAsync(S.flags, flags, kFlagBytes, hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.norms, &one, sizeof(double), hipMemcpyHostToDevice, op->stream));
    HIPCHK(hipMemcpyAsync(S.alphas, alphas, n * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    if (n > 1)
      HIPCHK(hipMemcpyAsync(S.betas, betas, (n - 1) * sizeof(double), hipMemcpyHostToDevice,
                            op->stream));
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    HIPCHK(launch::ftk_exp_times(S, (int)n, op->d_exp_ts, (int)m, op->d_Y, (int)op->ycap,
                                 op->d_exp_back, 0, op->stream));
    HIPCHK(hipMemcpy2DAsync(y_out, n * sizeof(double), op->d_Y, op->ycap * sizeof(double),
                            n * sizeof(double), m, hipMemcpyDeviceToHost, op->stream));
    HIPCHK(hipMemcpyAsync(op->h_exp_back, op->d_exp_back, m * sizeof(int32_t),
                          hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    for (size_t i = 0; i < m; ++i) on_device[i] = op->h_exp_back[i] ? 0 : 1;
  });
}

} // extern "C"

// ---- f(A) b_1 ... f(A) b_s in one lock-step run ---------------------------------------
namespace {
// The grouping rule (DESIGN.md §2 "Several right-hand sides in lock-step", include/tpl.h):
// the columns are taken in order, four at a time while four remain, then two at a time;
// a last single column runs the single host-f solve. No group is padded: a remainder of
// three is a group of two and a single solve (a padded group of four measured slower than
// three single solves).
int group_width(size_t rem) { return rem >= 4 ? 4 : (rem >= 2 ? 2 : 1); }

void check_batch_args(tpl_op_s* op, bool have_args, size_t s) {
  if (!op || !have_args) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (s == 0 || s > (size_t)TPL_BATCH_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "s must be between 1 and TPL_BATCH_MAX");
  set_device(op);
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch solve of a partitioned operator");
}

// Host mirror of a group's state head: flags | norms | alphas | betas (| y), laid out as
// ensure_batch laid out the device block.
struct GroupHead {
  std::vector<double> h;
  size_t w, kc;
  explicit GroupHead(const tpl_op_s* op)
      : w((size_t)op->bat.nb), kc(op->bat.kcap) {
    h.assign(w * (kFlagBytes / sizeof(double)) + w * (4 * kc + 1), 0.0);
  }
  int32_t* flags(size_t c) { return reinterpret_cast<int32_t*>(h.data()) + 8 * c; }
  double* norms(size_t c) { return h.data() + w * (kFlagBytes / sizeof(double)) + c * (kc + 1); }
  double* alphas(size_t c) { return norms(0) + w * (kc + 1) + c * kc; }
  double* betas(size_t c) { return alphas(0) + w * kc + c * kc; }
  double* y(size_t c) { return betas(0) + w * kc + c * kc; }
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
};

// The nb columns of the caller's B (column-major, ld = n) into the group's
// interleaved b, in the operator's order.
void upload_group(tpl_op_s* op, const double* B, int nb, int mem) {
  const int64_t n = op->part.n;
  const double* src = B;
  if (mem != TPL_MEM_DEVICE) {
    HIPCHK(hipMemcpyAsync(op->bat.d_stage, B, (size_t)n * nb * sizeof(double),
                          hipMemcpyHostToDevice, op->stream));
    src = op->bat.d_stage;
  }
  HIPCHK(launch::b_interleave(nb, n, op->bat.b, src, op->bufs.d_perm, op->stream));
}
// The group's interleaved x out to the nb columns of the caller's X.
void download_group(tpl_op_s* op, double* X, int nb, int mem) {
  const int64_t n = op->part.n;
  double* dst = mem == TPL_MEM_DEVICE ? X : op->bat.d_stage;
  HIPCHK(launch::b_deinterleave(nb, n, dst, op->bat.x, op->bufs.d_iperm, op->stream));
  if (mem != TPL_MEM_DEVICE)
    HIPCHK(hipMemcpyAsync(X, op->bat.d_stage, (size_t)n * nb * sizeof(double),
                          hipMemcpyDeviceToHost, op->stream));
}
// Pass one of a group on the stream (ensure_batch first): the group's b, the lock-step steps.
void enqueue_pass_one_group(tpl_op_s* op, const double* B, size_t k, int nb, int mem) {
  upload_group(op, B, nb, mem);
  run_pass1_batch(op, k, nb);
}
// The decompositions' host mirror of the group on the stream (synchronises).
GroupHead fetch_group(tpl_op_s* op) {
  GroupHead g(op);
  HIPCHK(hipMemcpyAsync(g.h.data(), op->bat.d_state, g.decomp_bytes(), hipMemcpyDeviceToHost,
                        op->stream));
  sync_checked(op);
  return g;
}
// Pass one of a group; returns the decompositions' host mirror (synchronised).
GroupHead pass_one_group(tpl_op_s* op, const double* B, size_t k, int nb, int mem) {
  ensure_batch(op, nb, k);
  enqueue_pass_one_group(op, B, k, nb, mem);
  return fetch_group(op);
}
// tpl_lanczos_two_pass_batch after its argument checks.
void two_pass_batch(tpl_op_s* op, const double* B, size_t s, size_t k, tpl_ftk_fn f, void* f_user,
                    double* x_out, int mem) {
  op->last_one_graph = false;
  const size_t n = (size_t)op->part.n;
  for (size_t c0 = 0; c0 < s;) {
    const int nb = n == 0 ? 1 : group_width(s - c0);
    if (nb == 1) {  // the single solve's host-f path
      two_pass_host_f(op, B + c0 * n, k, f, f_user, x_out + c0 * n, mem, false);
      ++c0;
      continue;
    }
    // 1. pass one for the group's columns in lock-step
    GroupHead g = pass_one_group(op, B + c0 * n, k, nb, mem);
    // 2. f(T_k) e_1 per column on the host, in column order, 3. y_c = y'_c * ||b_c||
    size_t kmax = 0;
    std::vector<double> y;
    for (int c = 0; c < nb; ++c) {
      const HostDecomp d = g.decomp((size_t)c);
      if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
      call_ftk(f, f_user, d, y);
      for (size_t j = 0; j < d.steps; ++j) g.y((size_t)c)[j] = y[j] * d.b_norm;
      kmax = std::max(kmax, d.steps);
    }
    HIPCHK(hipMemcpyAsync(op->bat.S.y, g.y(0), g.w * g.kc * sizeof(double),
                          hipMemcpyHostToDevice, op->stream));
    // 4. one pass two for all of them
    run_pass2_batch(op, kmax, nb);
    download_group(op, x_out + c0 * n, nb, mem);
    sync_checked(op);
    c0 += (size_t)nb;
  }
}
} // namespace

extern "C" {

tpl_status tpl_lanczos_two_pass_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      size_t k, tpl_ftk_fn f, void* f_user, double* x_out,
                                      int mem) {
  return guarded([&] {
    check_batch_args(op, B && x_out && f, s);
    check_b(op, B, b_len);
    check_k(k);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH);
    two_pass_batch(op, B, s, k, f, f_user, x_out, mem);
  });
}

tpl_status tpl_lanczos_pass_one_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      size_t k, double* alphas, double* betas, size_t* steps,
                                      double* b_norms, int mem) {
  return guarded([&] {
    check_batch_args(op, B && alphas && betas && steps && b_norms, s);
    check_b(op, B, b_len);
    check_k(k);
    const TimingOff untimed(op);
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {
        run_pass_one(op, B + c0 * n, k, mem, false, false);
        write_decomp(fetch_decomp(op), alphas + c0 * k, betas + c0 * k, steps + c0, b_norms + c0);
        ++c0;
        continue;
      }
      GroupHead g = pass_one_group(op, B + c0 * n, k, nb, mem);
      for (int c = 0; c < nb; ++c)
        write_decomp(g.decomp((size_t)c), alphas + (c0 + c) * k, betas + (c0 + c) * k,
                     steps + c0 + c, b_norms + c0 + c);
      c0 += (size_t)nb;
    }
  });
}

tpl_status tpl_lanczos_pass_two_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      const double* alphas, const double* betas, size_t ld,
                                      const size_t* steps, const double* b_norms,
                                      const double* y, double* x_out, int mem) {
  return guarded([&] {
    check_batch_args(op, B && x_out && steps && b_norms, s);
    check_b(op, B, b_len);
    const TimingOff untimed(op);
    // the single call's checks, per column in ascending order
    for (size_t c = 0; c < s; ++c) {
      if (b_norms[c] <= kBreakdownTol)
        fail_input("The initial vector `b` must not be a zero vector.");
      if (steps[c] > ld || (steps[c] > 0 && (!alphas || !y)) || (steps[c] > 1 && !betas))
        fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
      if (steps[c] > (size_t)INT32_MAX / 2) fail(TPL_ERR_INVALID_ARGUMENT, "steps too large");
    }
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {
        const size_t st = steps[c0];
        // (NULL arrays are accepted when no column takes a step: no arithmetic on them)
        auto col = [&](const double* p) { return p ? p + c0 * ld : nullptr; };
        pass_two_one(op, B + c0 * n, col(alphas), st, col(betas), st > 0 ? st - 1 : 0, st,
                     b_norms[c0], col(y), st, x_out + c0 * n, nullptr, mem);
        ++c0;
        continue;
      }
      size_t kmax = 1;
      for (int c = 0; c < nb; ++c) kmax = std::max(kmax, steps[c0 + c]);
      ensure_batch(op, nb, kmax);
      // decompositions -> the group's state: steps_c, ||b_c||, alphas, betas, y
      GroupHead g(op);
      for (int c = 0; c < nb; ++c) {
        const size_t cc = c0 + (size_t)c, st = steps[cc];
        g.flags((size_t)c)[2] = (int32_t)st;
        g.norms((size_t)c)[0] = b_norms[cc];
        if (st > 0) std::memcpy(g.alphas((size_t)c), alphas + cc * ld, st * sizeof(double));
        if (st > 1) std::memcpy(g.betas((size_t)c), betas + cc * ld, (st - 1) * sizeof(double));
        if (st > 0) std::memcpy(g.y((size_t)c), y + cc * ld, st * sizeof(double));
      }
      HIPCHK(hipMemcpyAsync(op->bat.d_state, g.h.data(), g.h.size() * sizeof(double),
                            hipMemcpyHostToDevice, op->stream));
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch(op, kmax, nb);
      download_group(op, x_out + c0 * n, nb, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
  });
}

} // extern "C"

// ---- f_i(A) b_c: m functions of s right-hand sides in one run ---------------------------
namespace {
// Every group of four or two columns runs fused (lock-step pass one, one pass two for the
// group's nb x m results): both widths measured faster than nb multi-function solves and than
// m batch solves (profiles/batch_multi_timing.txt), so no width is
// routed to an existing path.
void check_batch_multi_args(tpl_op_s* op, bool have_args, size_t s, size_t m) {
  if (!op || !have_args) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (s == 0 || s > (size_t)TPL_BATCH_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "s must be between 1 and TPL_BATCH_MAX");
  if (m == 0 || m > (size_t)TPL_MULTI_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
  set_device(op);
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch-multi solve of a partitioned operator");
}
// The group's coefficient table: function f, column c at (f nb + c) kcap.
struct GroupY {
  std::vector<double> h;
  size_t nb, kc;
  GroupY(const tpl_op_s* op, int nb_, size_t m) : nb((size_t)nb_), kc(op->bat.kcap) {
    h.assign(m * nb * kc, 0.0);
  }
  double* col(size_t f, size_t c) { return h.data() + (f * nb + c) * kc; }
  void upload(tpl_op_s* op) {
    HIPCHK(hipMemcpyAsync(op->bat.d_my, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
  }
};
// The group's m interleaved result vectors out to the nb m columns (c m + f) of the caller's X.
void download_group_multi(tpl_op_s* op, double* X, int nb, size_t m, int mem) {
  const int64_t n = op->part.n;
  double* dst = mem == TPL_MEM_DEVICE ? X : op->bat.d_mstage;
  HIPCHK(launch::bm_deinterleave(nb, n, dst, op->bat.d_mx, op->ld * nb, (int)m, op->bufs.d_iperm,
                                 op->stream));
  if (mem != TPL_MEM_DEVICE && n > 0)
    HIPCHK(hipMemcpyAsync(X, dst, (size_t)n * nb * m * sizeof(double), hipMemcpyDeviceToHost,
                          op->stream));
}
} // namespace

extern "C" {

tpl_status tpl_lanczos_two_pass_batch_multi(tpl_op_t op, const double* B, int64_t b_len,
                                            size_t s, size_t k, const tpl_ftk_fn* fs,
                                            void** f_users, size_t m, double* x_out, int mem) {
  return guarded([&] {
    check_batch_multi_args(op, B && fs && x_out, s, m);
    check_b(op, B, b_len);
    check_k(k);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    if (m == 1) {  // one function: the batch solve
      two_pass_batch(op, B, s, k, fs[0], f_users ? f_users[0] : nullptr, x_out, mem);
      return;
    }
    op->last_one_graph = false;
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {  // the multi-function solve of that column
        two_pass_multi(op, B + c0 * n, k, fs, f_users, m, x_out + c0 * m * n, mem);
        ++c0;
        continue;
      }
      // 1. pass one for the group's columns in lock-step
      GroupHead g = pass_one_group(op, B + c0 * n, k, nb, mem);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      // 2. per column in order: the zero-vector check, then every f_i(T_k) e_1 on the host
      //    in index order, 3. y_{c,i} = y'_{c,i} * ||b_c||
      GroupY Y(op, nb, m);
      size_t steps[kBatchNbMax];
      std::vector<double> y;
      for (int c = 0; c < nb; ++c) {
        const HostDecomp d = g.decomp((size_t)c);
        if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
        for (size_t i = 0; i < m; ++i) {
          call_ftk(fs[i], f_users ? f_users[i] : nullptr, d, y);
          double* yc = Y.col(i, (size_t)c);
          for (size_t j = 0; j < d.steps; ++j) yc[j] = y[j] * d.b_norm;
        }
        steps[c] = d.steps;
      }
      Y.upload(op);
      // 4. one pass two for all nb x m results
      run_pass2_batch_multi(op, steps, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
  });
}

tpl_status tpl_lanczos_pass_two_batch_multi(tpl_op_t op, const double* B, int64_t b_len,
                                            size_t s, const double* alphas, const double* betas,
                                            size_t ld, const size_t* steps, const double* b_norms,
                                            const double* y, size_t m, double* x_out, int mem) {
  return guarded([&] {
    check_batch_multi_args(op, B && x_out && steps && b_norms, s, m);
    check_b(op, B, b_len);
    const TimingOff untimed(op);
    // the single call's checks, per column in ascending order
    for (size_t c = 0; c < s; ++c) {
      if (b_norms[c] <= kBreakdownTol)
        fail_input("The initial vector `b` must not be a zero vector.");
      if (steps[c] > ld || (steps[c] > 0 && (!alphas || !y)) || (steps[c] > 1 && !betas))
        fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
      if (steps[c] > (size_t)INT32_MAX / 2) fail(TPL_ERR_INVALID_ARGUMENT, "steps too large");
    }
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {  // the multi-function pass two of that column
        const size_t st = steps[c0];
        auto col = [&](const double* p) { return p ? p + c0 * ld : nullptr; };
        pass_two_multi(op, B + c0 * n, col(alphas), st, col(betas), st > 0 ? st - 1 : 0, st,
                       b_norms[c0], y ? y + c0 * m * ld : nullptr, ld, m, x_out + c0 * m * n, mem);
        ++c0;
        continue;
      }
      size_t kmax = 1;
      for (int c = 0; c < nb; ++c) kmax = std::max(kmax, steps[c0 + c]);
      ensure_batch(op, nb, kmax);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      // decompositions -> the group's state (steps_c, ||b_c||, alphas, betas), y -> the table
      GroupHead g(op);
      GroupY Y(op, nb, m);
      for (int c = 0; c < nb; ++c) {
        const size_t cc = c0 + (size_t)c, st = steps[cc];
        g.flags((size_t)c)[2] = (int32_t)st;
        g.norms((size_t)c)[0] = b_norms[cc];
        if (st > 0) std::memcpy(g.alphas((size_t)c), alphas + cc * ld, st * sizeof(double));
        if (st > 1) std::memcpy(g.betas((size_t)c), betas + cc * ld, (st - 1) * sizeof(double));
        for (size_t i = 0; i < m && st > 0; ++i)
          std::memcpy(Y.col(i, (size_t)c), y + (cc * m + i) * ld, st * sizeof(double));
      }
      HIPCHK(hipMemcpyAsync(op->bat.d_state, g.h.data(), g.h.size() * sizeof(double),
                            hipMemcpyHostToDevice, op->stream));
      Y.upload(op);
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch_multi(op, steps + c0, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
  });
}

tpl_status tpl_lanczos_two_pass_batch_exp_times(tpl_op_t op, const double* B, int64_t b_len,
                                                size_t s, size_t k, const double* ts, size_t m,
                                                double* x_out, int mem, int32_t* on_device) {
  return guarded([&] {
    check_batch_multi_args(op, B && ts && x_out, s, m);
    check_b(op, B, b_len);
    check_k(k);
    for (size_t i = 0; i < m; ++i)
      if (!std::isfinite(ts[i])) fail(TPL_ERR_INVALID_ARGUMENT, "every time t_i must be finite");
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    op->last_one_graph = false;
    if (on_device) std::fill(on_device, on_device + s * m, 0);
    const bool dev = op->device_ftk != 0 && k <= kDevExpMaxK;
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {  // the single-b exp-times solve of that column
        two_pass_exp_times(op, B + c0 * n, k, ts, m, x_out + c0 * m * n, mem,
                           on_device ? on_device + c0 * m : nullptr);
        ++c0;
        continue;
      }
      ensure_batch(op, nb, k);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_exp_times_batch(op);
      BatchBufs& bb = op->bat;
      // 1. pass one for the group's columns in lock-step; 2. straight behind it on the stream
      //    every exp(t_i T_k) e_1 of every column at once (each steps_c stays on the device),
      //    y_{c,i} = y'_{c,i} * ||b_c|| into the group's coefficient table
      if (dev)
        HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice,
                              op->stream));
      enqueue_pass_one_group(op, B + c0 * n, k, nb, mem);
      if (dev) {
        HIPCHK(launch::ftk_exp_times_batch(nb, bb.S, (int)k, op->d_exp_ts, (int)m, bb.d_my,
                                           op->d_expb_back, 1, op->stream));
        HIPCHK(hipMemcpyAsync(op->h_expb_back, op->d_expb_back, (size_t)nb * m * sizeof(int32_t),
                              hipMemcpyDeviceToHost, op->stream));
      }
      GroupHead g = fetch_group(op);  // the group's one synchronisation before pass two
      // 3. per column in order: the zero-vector check, then the times handed back (without
      //    the device: all of them) on the host in index order; only their columns are
      //    uploaded (host table: function i, column c at (i nb + c) k, alive until the sync)
      std::vector<double> Yh, y;
      size_t steps[kBatchNbMax];
      double t = 0.0;
      for (int c = 0; c < nb; ++c) {
        const HostDecomp d = g.decomp((size_t)c);
        if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
        steps[c] = d.steps;
        for (size_t i = 0; i < m; ++i) {
          const bool kept = dev && d.steps > 0 && !op->h_expb_back[(size_t)c * m + i];
          if (on_device) on_device[(c0 + (size_t)c) * m + i] = kept ? 1 : 0;
          if (kept) continue;
          t = ts[i];
          call_ftk(&tpl_ftk_exp_t, &t, d, y);
          if (d.steps == 0) continue;
          if (Yh.empty()) Yh.resize(m * (size_t)nb * k);
          double* col = Yh.data() + (i * (size_t)nb + (size_t)c) * k;
          for (size_t j = 0; j < d.steps; ++j) col[j] = y[j] * d.b_norm;
          HIPCHK(hipMemcpyAsync(bb.d_my + (i * (size_t)nb + (size_t)c) * bb.kcap, col,
                                d.steps * sizeof(double), hipMemcpyHostToDevice, op->stream));
        }
      }
      // 4. one pass two for all nb x m results
      run_pass2_batch_multi(op, steps, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
  });
}

tpl_status tpl_op_ftk_exp_times_batch_device(tpl_op_t op, const double* alphas,
                                             const double* betas, size_t ld, const size_t* steps,
                                             size_t nb, const double* ts, size_t m, double* y_out,
                                             int32_t* on_device) {
  return guarded([&] {
    if (!op || !alphas || !steps || !ts || !y_out || !on_device)
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nb != 2 && nb != 4) fail(TPL_ERR_INVALID_ARGUMENT, "nb must be 2 or 4");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    size_t kmax = 0;
    for (size_t c = 0; c < nb; ++c) {
      if (steps[c] == 0 || steps[c] > ld)
        fail(TPL_ERR_INVALID_ARGUMENT, "steps[c] must be between 1 and ld");
      if (steps[c] > 1 && !betas) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
      kmax = std::max(kmax, steps[c]);
    }
    if (kmax > kDevExpMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch-multi solve of a partitioned operator");
    ensure_batch(op, (int)nb, kmax);
    ensure_batch_multi(op, m, false);
    ensure_exp_times_batch(op);
    BatchBufs& bb = op->bat;
    // the group's state as pass one leaves it: steps_c, ||b_c|| = 1, no error
    GroupHead g(op);
    for (size_t c = 0; c < nb; ++c) {
      g.flags(c)[2] = (int32_t)steps[c];
      g.norms(c)[0] = 1.0;
      std::memcpy(g.alphas(c), alphas + c * ld, steps[c] * sizeof(double));
      if (steps[c] > 1) std::memcpy(g.betas(c), betas + c * ld, (steps[c] - 1) * sizeof(double));
    }
    HIPCHK(hipMemcpyAsync(bb.d_state, g.h.data(), g.decomp_bytes(), hipMemcpyHostToDevice,
                          op->stream));
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    HIPCHK(launch::ftk_exp_times_batch((int)nb, bb.S, (int)kmax, op->d_exp_ts, (int)m, bb.d_my,
                                       op->d_expb_back, 0, op->stream));
    // column (c m + i) of y_out <- function i, column c of the table: steps_c entries, zeros
    // behind them
    std::memset(y_out, 0, ld * nb * m * sizeof(double));
    for (size_t c = 0; c < nb; ++c)
      HIPCHK(hipMemcpy2DAsync(y_out + c * m * ld, ld * sizeof(double), bb.d_my + c * bb.kcap,
                              nb * bb.kcap * sizeof(double), steps[c] * sizeof(double), m,
                              hipMemcpyDeviceToHost, op->stream));
    HIPCHK(hipMemcpyAsync(op->h_expb_back, op->d_expb_back, nb * m * sizeof(int32_t),
                          hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    for (size_t e = 0; e < nb * m; ++e) on_device[e] = op->h_expb_back[e] ? 0 : 1;
  });
}

} // extern "C"

// ---- (A + sigma_i I)^{-1} b_c for s right-hand sides, every (c, i) stopped at the tolerance
namespace {
// Auto mode takes the one-graph path for a group up to this kmax: the largest measured kmax at
// which the graph was no slower than the host-composed path at every measured (s, m), beyond
// the repetitions' noise (scripts/batch_shifted_inv_tol_timing.py's rule, in both of its passes:
// profiles/batch_shifted_inv_tol_timing.txt). 500k block with D, shifts 1 .. 100,
// (s, m) = (2, 1), (4, 1), (4, 4), (4, 8), tol 1e-4 and 1e-8, graph over host path: 0.96 - 1.01
// at kmax = 250, every difference within the noise. At 500 it is 0.93 - 0.95 where the four
// columns stop (a lock-step step of four columns is worth far more than the 3.5 us an empty
// launch costs, unlike the single solve's: kShiftedAutoK) but 1.01 where a shift never stops
// (+0.24 to +0.37 ms: the nb k_ftk_inv_shifts launches in series, 85 us of chain each at 500
// rows), and the routing cannot know which it will be. Below the line nothing stops and the
// graph is 0.99 - 1.02 of the host path at kmax = 125 and 64 (+0.10 ms at most): the line's
// cost. Against s single-b calls either path is 0.78 - 0.95 at every measured shape. Mode 1
// takes the graph up to the device inv's bound.
constexpr size_t kBatchShiftedAutoK = 250;
// A group of four or two runs as one graph where the single shifted solve may (the device
// inv's bounds, graphs in use), within the line above in auto mode.
bool batch_shifted_on_device(const tpl_op_s* op, size_t kmax) {
  return device_f(op, &tpl_ftk_inv, kmax) == kDevInv &&
         (op->device_ftk == 1 || kmax <= kBatchShiftedAutoK) && use_graphs() && !op->eager;
}
// Column c's device-held step count (its flag word 2) := v, from a host word that lives
// until the next synchronisation.
void upload_col_count(tpl_op_s* op, int c, const int32_t* v) {
  HIPCHK(hipMemcpyAsync(op->bat.S.flags + 8 * c + 2, v, sizeof(int32_t), hipMemcpyHostToDevice,
                        op->stream));
}
} // namespace

extern "C" {

size_t tpl_batch_shifted_inv_tol_auto_k(void) { return kBatchShiftedAutoK; }

tpl_status tpl_lanczos_two_pass_batch_shifted_inv_tol(
    tpl_op_t op, const double* B, int64_t b_len, size_t s, size_t kmax, const double* sigmas,
    size_t m, double tol, double* x_out, int mem, size_t* steps, int32_t* converged,
    double* res_out, size_t* res_len) {
  return guarded([&] {
    if (!op || !B || !sigmas || !x_out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s == 0 || s > (size_t)TPL_BATCH_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "s must be between 1 and TPL_BATCH_MAX");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    if (!(tol >= 0.0)) fail(TPL_ERR_INVALID_ARGUMENT, "tol must be a number >= 0");
    for (size_t i = 0; i < m; ++i)
      if (!std::isfinite(sigmas[i]))
        fail(TPL_ERR_INVALID_ARGUMENT, "every shift sigma_i must be finite");
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch-multi solve of a partitioned operator");
    check_b(op, B, b_len);
    check_k(kmax);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    const size_t n = (size_t)op->part.n;
    // result (c, i): entry e = c m + i of every output
    auto report = [&](size_t e, size_t ms, bool hit, size_t n_res) {
      if (steps) steps[e] = ms;
      if (converged) converged[e] = hit ? 1 : 0;
      if (res_len) res_len[e] = res_out ? n_res : 0;
    };
    const bool dev = batch_shifted_on_device(op, kmax);
    bool groups_one_graph = true, any_group = false;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {  // the single-b solve of that column, with its own routing
        auto at = [&](auto* p) { return p ? p + c0 * m : nullptr; };
        shifted_inv_tol_one(op, B + c0 * n, kmax, sigmas, m, tol, x_out + c0 * m * n, mem,
                            at(steps), at(converged), res_out ? res_out + c0 * m * kmax : nullptr,
                            at(res_len));
        ++c0;
        continue;
      }
      any_group = true;
      ensure_batch(op, nb, kmax);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_batch_cut(op);
      BatchBufs& bb = op->bat;
      if (dev) {
        // one graph: pass one with a lane per (column, shift), every y_{c,i} on its own
        // m*_{c,i} rows, the cut pass two
        const launch::BatchShiftTol t = ensure_batch_stol(op, m);
        const size_t mc = bb.stol_m, kc = bb.kcap, w = (size_t)kBatchNbMax;
        upload_group(op, B + c0 * n, nb, mem);
        HIPCHK(hipMemsetAsync(t.t0.hits, 0, w * 2 * mc * sizeof(int32_t), op->stream));
        HIPCHK(hipMemcpyAsync(bb.d_stol, &tol, sizeof(double), hipMemcpyHostToDevice, op->stream));
        HIPCHK(hipMemcpyAsync(bb.d_stol + 1, sigmas, m * sizeof(double), hipMemcpyHostToDevice,
                              op->stream));
        run_two_pass_batch_shifted_inv_tol(op, kmax, nb, t);
        download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
        char* h = (char*)bb.h_stol;
        int32_t* h_flags = (int32_t*)h;
        int32_t* h_ints = (int32_t*)(h + w * kFlagBytes);
        double* h_res = (double*)(h + w * kFlagBytes + w * 2 * mc * sizeof(int32_t));
        HIPCHK(hipMemcpyAsync(h_flags, bb.S.flags, (size_t)nb * kFlagBytes, hipMemcpyDeviceToHost,
                              op->stream));
        HIPCHK(hipMemcpyAsync(h_ints, t.t0.hits, w * 2 * mc * sizeof(int32_t),
                              hipMemcpyDeviceToHost, op->stream));
        if (res_out && kmax > 1)
          for (int c = 0; c < nb; ++c)
            HIPCHK(hipMemcpyAsync(h_res + (size_t)c * kc * mc, t.col(c).res,
                                  (kmax - 1) * m * sizeof(double), hipMemcpyDeviceToHost,
                                  op->stream));
        sync_checked(op);
        for (int c = 0; c < nb; ++c) {
          const int32_t* fl = h_flags + 8 * c;
          if (fl[1]) fail_input("Input vector `b` must not be a zero vector.");
          const int32_t* hits = h_ints + (size_t)c * 2 * mc;
          const int32_t* nres = hits + mc;
          const double* res = h_res + (size_t)c * kc * mc;
          for (size_t i = 0; i < m; ++i) {
            const size_t e = (c0 + (size_t)c) * m + i;
            if (fl[2] == 0) {
              report(e, 0, false, 0);
              continue;
            }
            const size_t formed = std::min<size_t>((size_t)nres[i], kmax - 1);
            if (res_out)
              for (size_t r = 0; r < formed; ++r) res_out[e * kmax + r] = res[r * m + i];
            report(e, hits[i] ? (size_t)hits[i] : (size_t)fl[2], hits[i] != 0, formed);
          }
        }
        c0 += (size_t)nb;
        continue;
      }
      // composed on the host (the oracle of the device path): the group's pass one to kmax,
      // then per column in order the zero check and per shift the history, the rule and y on
      // the first m*_{c,i} rows; M_c = max_i m*_{c,i} becomes column c's device-held step
      // count, and one pass two of max_c M_c steps cuts every result at its own step
      groups_one_graph = false;
      enqueue_pass_one_group(op, B + c0 * n, kmax, nb, mem);
      GroupHead g = fetch_group(op);
      GroupY Y(op, nb, m);
      std::vector<int32_t> cut((size_t)kBatchNbMax * TPL_MULTI_MAX, 0);
      int32_t Mc[kBatchNbMax] = {0, 0, 0, 0};
      size_t Mmax = 0;
      for (int c = 0; c < nb; ++c) {
        const HostDecomp d = g.decomp((size_t)c);
        if (d.flags[1]) fail_input("Input vector `b` must not be a zero vector.");
        for (size_t i = 0; i < m; ++i) {
          const size_t e = (c0 + (size_t)c) * m + i;
          if (d.steps == 0) {
            report(e, 0, false, 0);
            continue;
          }
          const ShiftedCol sc = shifted_col(d, sigmas[i], tol);
          std::copy(sc.y.begin(), sc.y.end(), Y.col(i, (size_t)c));
          cut[(size_t)c * TPL_MULTI_MAX + i] = (int32_t)sc.steps;
          Mc[c] = std::max(Mc[c], (int32_t)sc.steps);
          if (res_out) std::copy(sc.res.begin(), sc.res.end(), res_out + e * kmax);
          report(e, sc.steps, sc.converged, sc.res.size());
        }
        Mmax = std::max(Mmax, (size_t)Mc[c]);
      }
      for (int c = 0; c < nb; ++c) upload_col_count(op, c, &Mc[c]);
      Y.upload(op);
      HIPCHK(hipMemcpyAsync(op->d_bcut, cut.data(), cut.size() * sizeof(int32_t),
                            hipMemcpyHostToDevice, op->stream));
      run_pass2_batch_multi_cut(op, std::max<size_t>(Mmax, 1), nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
    // bit 5: every group of four or two ran as one graph; a lone column reports its own
    if (any_group) op->last_one_graph = groups_one_graph;
  });
}

tpl_status tpl_lanczos_pass_two_batch_multi_cut(tpl_op_t op, const double* B, int64_t b_len,
                                                size_t s, const double* alphas,
                                                const double* betas, size_t ld,
                                                const size_t* steps, const double* b_norms,
                                                const double* y, const size_t* col_steps,
                                                size_t m, double* x_out, int mem) {
  return guarded([&] {
    if (!op || !B || !x_out || !steps || !b_norms || !col_steps || !y || !alphas)
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s == 0 || s > (size_t)TPL_BATCH_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "s must be between 1 and TPL_BATCH_MAX");
    if (m == 0 || m > (size_t)TPL_MULTI_MAX)
      fail(TPL_ERR_INVALID_ARGUMENT, "m must be between 1 and TPL_MULTI_MAX");
    // the single call's checks of the counts and the decomposition, per column in ascending
    // order, before anything touches a device
    for (size_t c = 0; c < s; ++c) {
      if (steps[c] == 0 || steps[c] > ld || steps[c] > (size_t)INT32_MAX / 2)
        fail(TPL_ERR_INVALID_ARGUMENT, "steps[c] must be >= 1 and ld >= steps[c]");
      for (size_t i = 0; i < m; ++i)
        if (col_steps[c * m + i] < 1 || col_steps[c * m + i] > steps[c])
          fail(TPL_ERR_INVALID_ARGUMENT,
               "every col_steps[c m + i] must be between 1 and steps[c]");
      if (b_norms[c] <= kBreakdownTol)
        fail_input("The initial vector `b` must not be a zero vector.");
      if (steps[c] > 1 && !betas)
        fail(TPL_ERR_INVALID_ARGUMENT, "decomposition arrays shorter than steps_taken");
    }
    set_device(op);
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch-multi solve of a partitioned operator");
    check_b(op, B, b_len);
    const TimingOff untimed(op);
    const size_t n = (size_t)op->part.n;
    for (size_t c0 = 0; c0 < s;) {
      const int nb = n == 0 ? 1 : group_width(s - c0);
      if (nb == 1) {  // the single pass two with a cut per column
        const size_t st = steps[c0];
        int32_t cs[TPL_MULTI_MAX];
        for (size_t i = 0; i < m; ++i) cs[i] = (int32_t)col_steps[c0 * m + i];
        pass_two_multi_cut_run(op, B + c0 * n, alphas + c0 * ld, betas ? betas + c0 * ld : nullptr,
                               st, b_norms[c0], y + c0 * m * ld, ld, cs, m, x_out + c0 * m * n,
                               mem);
        ++c0;
        continue;
      }
      size_t kmax = 1;
      for (int c = 0; c < nb; ++c) kmax = std::max(kmax, steps[c0 + c]);
      ensure_batch(op, nb, kmax);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_batch_cut(op);
      // decompositions -> the group's state (steps_c, ||b_c||, alphas, betas), y -> the
      // table, the cuts -> the cut table
      GroupHead g(op);
      GroupY Y(op, nb, m);
      std::vector<int32_t> cut((size_t)kBatchNbMax * TPL_MULTI_MAX, 0);
      for (int c = 0; c < nb; ++c) {
        const size_t cc = c0 + (size_t)c, st = steps[cc];
        g.flags((size_t)c)[2] = (int32_t)st;
        g.norms((size_t)c)[0] = b_norms[cc];
        std::memcpy(g.alphas((size_t)c), alphas + cc * ld, st * sizeof(double));
        if (st > 1) std::memcpy(g.betas((size_t)c), betas + cc * ld, (st - 1) * sizeof(double));
        for (size_t i = 0; i < m; ++i) {
          std::memcpy(Y.col(i, (size_t)c), y + (cc * m + i) * ld, st * sizeof(double));
          cut[(size_t)c * TPL_MULTI_MAX + i] = (int32_t)col_steps[cc * m + i];
        }
      }
      HIPCHK(hipMemcpyAsync(op->bat.d_state, g.h.data(), g.h.size() * sizeof(double),
                            hipMemcpyHostToDevice, op->stream));
      Y.upload(op);
      HIPCHK(hipMemcpyAsync(op->d_bcut, cut.data(), cut.size() * sizeof(int32_t),
                            hipMemcpyHostToDevice, op->stream));
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch_multi_cut(op, kmax, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
      c0 += (size_t)nb;
    }
  });
}

} // extern "C"
