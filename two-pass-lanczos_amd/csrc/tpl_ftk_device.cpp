// tpl_ftk_device.cpp — the device f(T_k) kernels on a decomposition the caller hands in, without
// a solve around them (include/tpl.h: the tests' and the oracle's way to the kernels' bits), and
// the two small accessors of the solver state that are no solves.
#include "tpl_solve.h"

using namespace tpl;

extern "C" {
tpl_status tpl_op_reorth_second_passes(tpl_op_t op, int64_t* count) {
  return guarded([&] {
    need(op && count);
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
    need(op && alphas && y_out && on_device && (n <= 1 || betas));
    if (which != 0 && which != 1) fail(TPL_ERR_INVALID_ARGUMENT, "which must be 0 (inv) or 1 (exp)");
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > (which == 0 ? kDevFtkMaxK : kDevExpMaxK))
      fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    ensure_state(op, n);
    // the solver state as pass one leaves it: steps_taken = n, ||b|| = 1, no error
    int32_t flags[kFlagBytes / 4];
    seed_state(op, flags, alphas, betas, n);
    const DevState& S = op->st.S;
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
    need(op && alphas && ts && y_out && on_device && (n <= 1 || betas));
    check_m(m);
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > kDevExpMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    refuse_partitioned(op, kMultiSolve);
    ensure_state(op, n);
    ensure_multi(op, m);
    ensure_exp_times(op);
    int32_t flags[kFlagBytes / 4];
    seed_state(op, flags, alphas, betas, n);
    const DevState& S = op->st.S;
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice, op->stream));
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

tpl_status tpl_op_ftk_inv_shifts_device(tpl_op_t op, const double* alphas, size_t n,
                                        const double* betas, const double* sigmas, size_t m,
                                        double* y_out) {
  return guarded([&] {
    need(op && alphas && sigmas && y_out && (n <= 1 || betas));
    check_m(m);
    if (n == 0) fail(TPL_ERR_INVALID_ARGUMENT, "n must be >= 1");
    if (n > kDevFtkMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    set_device(op);
    refuse_partitioned(op, kMultiSolve);
    ensure_state(op, n);
    ensure_multi(op, m);
    ensure_col_steps(op);
    const launch::ShiftTol t = ensure_stol(op, m);
    // the state as pass one leaves it, and no shift stopped
    int32_t flags[kFlagBytes / 4];
    seed_state(op, flags, alphas, betas, n);
    const DevState& S = op->st.S;
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

tpl_status tpl_op_ftk_exp_times_batch_device(tpl_op_t op, const double* alphas,
                                             const double* betas, size_t ld, const size_t* steps,
                                             size_t nb, const double* ts, size_t m, double* y_out,
                                             int32_t* on_device) {
  return guarded([&] {
    need(op && alphas && steps && ts && y_out && on_device);
    if (nb != 2 && nb != 4) fail(TPL_ERR_INVALID_ARGUMENT, "nb must be 2 or 4");
    check_m(m);
    size_t kmax = 0;
    for (size_t c = 0; c < nb; ++c) {
      if (steps[c] == 0 || steps[c] > ld)
        fail(TPL_ERR_INVALID_ARGUMENT, "steps[c] must be between 1 and ld");
      need(steps[c] <= 1 || betas);
      kmax = std::max(kmax, steps[c]);
    }
    if (kmax > kDevExpMaxK) fail(TPL_ERR_UNSUPPORTED, "k above the device f(T_k) bound");
    refuse_dense(op, kBatchMultiSolve);
    set_device(op);
    refuse_partitioned(op, kBatchMultiSolve);
    ensure_batch(op, (int)nb, kmax);
    ensure_batch_multi(op, m, false);
    ensure_exp_times_batch(op);
    BatchBufs& bb = op->bat;
    // the group's state as pass one leaves it: steps_c, ||b_c|| = 1, no error; without y
    GroupHead g(op);
    for (size_t c = 0; c < nb; ++c)
      g.set_column(c, steps[c], 1.0, alphas + c * ld, betas ? betas + c * ld : nullptr);
    g.upload(op, g.decomp_bytes());
    HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice, op->stream));
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
