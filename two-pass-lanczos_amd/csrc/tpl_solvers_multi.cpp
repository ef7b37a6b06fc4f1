// tpl_solvers_multi.cpp — m functions of one b over one Krylov space (include/tpl.h):
// f_1(A) b ... f_m(A) b by two passes or by the standard pass, exp(t_i A) b at m times,
// (A + sigma_i I)^{-1} b for m shifts each stopped at a tolerance, and the passes two on their
// own for m coefficient columns, uncut and cut.
#include "tpl_solve.h"

using namespace tpl;

namespace {
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
} // namespace

namespace tpl {

void two_pass_multi(tpl_op_s* op, const double* b, size_t k, const tpl_ftk_fn* fs, void** f_users,
                    size_t m, double* x_out, int mem) {
  // 1. pass one, once (the host-f path of tpl_lanczos_two_pass)
  op->last_one_graph = false;
  run_pass_one(op, b, k, mem, false, false);
  const HostDecomp d = fetch_decomp(op);
  if (zero_result(op, d.flags, x_out, mem, m)) return;
  // 2. every f_i(T_k) e_1 on the host, 3. y_i = y'_i * ||b||
  const std::vector<double> Y = call_ftks(fs, f_users, m, d, true);
  ensure_multi(op, m);
  upload_y(op, Y.data(), d.steps, d.steps, m);
  // 4. one pass two for all of them
  run_pass2_multi(op, d.steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}

void pass_two_multi(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                    const double* betas, size_t n_betas, size_t steps, double b_norm,
                    const double* y, size_t ldy, size_t m, double* x_out, int mem) {
  check_b_norm(b_norm);
  if (steps == 0) {
    zero_out(op, x_out, mem, m);
    return;
  }
  check_decomp_arrays(alphas, n_alphas, betas, n_betas, steps, y != nullptr);
  check_steps_fit(steps);
  ensure_state(op, steps);
  ensure_multi(op, m);
  upload_decomp(op, b_norm, alphas, betas, steps);
  upload_y(op, y, ldy, steps, m);
  upload_vec(op, op->b, b, mem);
  run_pass2_multi(op, steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}

void two_pass_exp_times(tpl_op_s* op, const double* b, size_t k, const double* ts, size_t m,
                        double* x_out, int mem, int32_t* on_device) {
  op->last_one_graph = false;
  if (on_device) std::fill(on_device, on_device + m, 0);
  ensure_state(op, k);
  ensure_multi(op, m);
  ensure_exp_times(op);
  // 1. pass one, once; 2. straight behind it on the stream every exp(t_i T_k) e_1 at once
  //    (steps_taken stays on the device), y_i = y'_i * ||b|| into the coefficient table
  const bool dev = exp_on_device(op, k);
  if (dev)
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice, op->stream));
  run_pass_one(op, b, k, mem, false, false);
  if (dev) {
    HIPCHK(launch::ftk_exp_times(op->st.S, (int)k, op->d_exp_ts, (int)m, op->d_Y, (int)op->ycap,
                                 op->d_exp_back, 1, op->stream));
    HIPCHK(hipMemcpyAsync(op->h_exp_back, op->d_exp_back, m * sizeof(int32_t),
                          hipMemcpyDeviceToHost, op->stream));
  }
  const HostDecomp d = fetch_decomp(op);  // the call's one synchronisation before pass two
  if (zero_result(op, d.flags, x_out, mem, m)) return;
  // 3. the times handed back (without the device: all of them) on the host, in index
  //    order; only their columns are uploaded (Y lives until the synchronisation below)
  std::vector<double> Y, y;
  for (size_t i = 0; i < m; ++i) {
    if (dev && !op->h_exp_back[i]) continue;
    if (Y.empty()) Y.resize(m * d.steps);
    exp_col_on_host(op, d, ts[i], y, Y.data() + i * d.steps, op->d_Y + i * op->ycap);
  }
  // 4. one pass two for all of them
  run_pass2_multi(op, d.steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
  if (on_device)
    for (size_t i = 0; i < m; ++i) on_device[i] = dev && !op->h_exp_back[i] ? 1 : 0;
}

void shifted_inv_tol_one(tpl_op_s* op, const double* b, size_t kmax, const double* sigmas,
                         size_t m, double tol, double* x_out, int mem, const TolReport& rep) {
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
    if (rep.res_out && kmax > 1)
      HIPCHK(hipMemcpyAsync(h_res, t.res, (kmax - 1) * m * sizeof(double),
                            hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    int32_t flags[kFlagBytes / 4];
    std::memcpy(flags, h, kFlagBytes);
    op->last_one_graph = true;
    if (zero_result(op, flags, x_out, mem, m)) return rep.none(0, m);
    rep.decode(0, m, flags[2], h_hits, h_hits + op->stol_m, h_res);
    return;
  }
  // composed on the host (the oracle of the device path): pass one to kmax, then per shift
  // the history, the rule and y on the first m*_i rows, one pass two of M = max m*_i steps
  op->last_one_graph = false;
  run_pass_one(op, b, kmax, mem, false, false);
  const HostDecomp d = fetch_decomp(op);
  if (zero_result(op, d.flags, x_out, mem, m)) return rep.none(0, m);
  std::vector<double> Y(m * d.steps, 0.0);
  int32_t cs[TPL_MULTI_MAX];
  size_t M = 0;
  for (size_t i = 0; i < m; ++i) {
    const TolCol c = shifted_col(d, sigmas[i], tol);
    std::copy(c.y.begin(), c.y.end(), Y.begin() + i * d.steps);
    cs[i] = (int32_t)c.steps;
    M = std::max(M, c.steps);
    rep.put(i, c);
  }
  upload_y(op, Y.data(), d.steps, M, m);
  upload_col_steps(op, cs, m);
  run_pass2_multi_cut(op, M, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}

void pass_two_multi_cut_run(tpl_op_s* op, const double* b, const double* alphas,
                            const double* betas, size_t steps, double b_norm, const double* y,
                            size_t ldy, const int32_t* cs, size_t m, double* x_out, int mem) {
  ensure_state(op, steps);
  ensure_multi(op, m);
  upload_decomp(op, b_norm, alphas, betas, steps);
  upload_y(op, y, ldy, steps, m);
  upload_col_steps(op, cs, m);
  upload_vec(op, op->b, b, mem);
  run_pass2_multi_cut(op, steps, m);
  download_cols(op, x_out, op->d_X, op->ld, (int64_t)m, mem);
  sync_checked(op);
}

} // namespace tpl

extern "C" {
tpl_status tpl_lanczos_two_pass_multi(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                      const tpl_ftk_fn* fs, void** f_users, size_t m,
                                      double* x_out, int mem) {
  return guarded([&] {
    check_multi(op, fs && x_out, m);
    check_b(op, b, b_len), check_k(k);
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
    check_b(op, b, b_len), check_k(k);
    const TimingOff untimed(op);
    op->last_one_graph = false;
    run_pass_one(op, b, k, mem, true, false);
    const HostDecomp d = fetch_decomp(op);
    if (zero_result(op, d.flags, x_out, mem, m)) return;
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
    pass_two_multi(op, b, alphas, n_alphas, betas, n_betas, steps, b_norm, y, steps, m, x_out, mem);
  });
}

tpl_status tpl_lanczos_two_pass_exp_times(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                          const double* ts, size_t m, double* x_out, int mem,
                                          int32_t* on_device) {
  return guarded([&] {
    check_multi(op, ts && x_out, m);
    check_b(op, b, b_len), check_k(k);
    check_finite(ts, m, kTimesFinite);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_MULTI);
    two_pass_exp_times(op, b, k, ts, m, x_out, mem, on_device);
  });
}

tpl_status tpl_lanczos_two_pass_shifted_inv_tol(tpl_op_t op, const double* b, int64_t b_len,
                                                size_t kmax, const double* sigmas, size_t m,
                                                double tol, double* x_out, int mem,
                                                size_t* steps, int32_t* converged,
                                                double* res_out, size_t* res_len) {
  return guarded([&] {
    need(op && sigmas && x_out), check_m(m), check_tol(tol);
    check_finite(sigmas, m, kShiftsFinite);
    set_device(op);
    refuse_partitioned(op, kMultiSolve);
    check_b(op, b, b_len), check_k(kmax);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_MULTI);
    shifted_inv_tol_one(op, b, kmax, sigmas, m, tol, x_out, mem,
                        TolReport{steps, converged, res_out, res_len, kmax});
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
    check_b_norm(b_norm);
    check_decomp_arrays(alphas, n_alphas, betas, n_betas, steps, true);
    pass_two_multi_cut_run(op, b, alphas, betas, steps, b_norm, y, ldy, cs, m, x_out, mem);
  });
}
} // extern "C"
