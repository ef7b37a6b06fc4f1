// tpl_solvers.cpp — the single-column solver entry points of the C ABI (include/tpl.h): the
// SpMV, the passes on their own, the one- and two-pass solves with their f(T_k) on the host or
// on the device, the inverse solve that stops at a tolerance — and the definitions of the steps
// every solver unit shares (tpl_solve.h).
#include "tpl_solve.h"

using namespace tpl;

// Callback polling (tpl_lanczos_standard with a step callback): largest batch of steps
// run ahead of the host callback.
constexpr int kCbBatchMax = 32;

namespace tpl {

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

void zero_out(tpl_op_s* op, double* x_out, int mem, size_t m) {
  const size_t n = (size_t)op->part.n;
  if (n == 0) return;
  for (size_t i = 0; i < m; ++i) {
    if (mem == TPL_MEM_DEVICE) {
      HIPCHK(hipMemsetAsync(x_out + i * n, 0, n * sizeof(double), op->stream));
      sync_checked(op);
    } else {
      std::memset(x_out + i * n, 0, n * sizeof(double));
    }
  }
}

bool zero_result(tpl_op_s* op, const int32_t* flags, double* x_out, int mem, size_t m) {
  if (flags[1]) fail_input(kZeroInput);
  if (flags[2] != 0) return false;
  zero_out(op, x_out, mem, m);
  return true;
}

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

void write_decomp(const HostDecomp& d, double* alphas, double* betas, size_t* steps,
                  double* b_norm) {
  if (d.flags[1]) fail_input(kZeroInput);
  std::memcpy(alphas, d.alphas, d.steps * sizeof(double));
  if (d.steps > 1) std::memcpy(betas, d.betas, (d.steps - 1) * sizeof(double));
  *steps = d.steps;
  *b_norm = d.b_norm;
}

void exp_col_on_host(tpl_op_s* op, const HostDecomp& d, double t, std::vector<double>& y,
                     double* col, double* dst) {
  call_ftk(&tpl_ftk_exp_t, &t, d, y);
  if (d.steps == 0) return;
  for (size_t j = 0; j < d.steps; ++j) col[j] = y[j] * d.b_norm;
  HIPCHK(hipMemcpyAsync(dst, col, d.steps * sizeof(double), hipMemcpyHostToDevice, op->stream));
}

void upload_decomp(tpl_op_s* op, const double& b_norm, const double* alphas, const double* betas,
                   size_t steps) {
  const DevState& S = op->st.S;
  HIPCHK(hipMemcpyAsync(S.norms, &b_norm, sizeof(double), hipMemcpyHostToDevice, op->stream));
  HIPCHK(hipMemcpyAsync(S.alphas, alphas, steps * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  if (steps > 1)
    HIPCHK(hipMemcpyAsync(S.betas, betas, (steps - 1) * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
}

void seed_state(tpl_op_s* op, int32_t (&flags)[kFlagBytes / 4], const double* alphas,
                const double* betas, size_t n) {
  static const double one = 1.0;
  std::memset(flags, 0, kFlagBytes);
  flags[2] = (int32_t)n;
  HIPCHK(hipMemcpyAsync(op->st.S.flags, flags, kFlagBytes, hipMemcpyHostToDevice, op->stream));
  upload_decomp(op, one, alphas, betas, n);
}

TolCol tol_col(const double* alphas, const double* betas, size_t steps, double b_norm, double tol) {
  TolCol c;
  c.res.resize(steps);
  size_t formed = 0;
  tpl_ftk_inv_residuals(alphas, steps, betas, steps - 1, c.res.data(), c.res.size(), &formed);
  c.res.resize(formed);
  c.steps = steps;
  for (size_t m = 1; m < steps && m <= formed; ++m)
    if (c.res[m - 1] <= tol) {
      c.steps = m;
      c.converged = true;
      break;
    }
  c.y.resize(c.steps);
  size_t ylen = c.steps;
  tpl_ftk_inv(alphas, c.steps, betas, c.steps - 1, c.y.data(), c.steps, &ylen, nullptr, 0, nullptr);
  for (auto& v : c.y) v = v * b_norm;
  return c;
}

TolCol shifted_col(const HostDecomp& d, double sigma, double tol) {
  std::vector<double> a(d.steps);
  for (size_t j = 0; j < d.steps; ++j) a[j] = d.alphas[j] + sigma;
  return tol_col(a.data(), d.betas, d.steps, d.b_norm, tol);
}

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

void pass_two_one(tpl_op_s* op, const double* b, const double* alphas, size_t n_alphas,
                  const double* betas, size_t n_betas, size_t steps, double b_norm,
                  const double* y, size_t y_len, double* x_out, double* v_out, int mem) {
  // src/algorithms/lanczos_two_pass.rs:220-227
  if (steps != y_len) fail_param_mismatch("y_k", steps, y_len);
  check_b_norm(b_norm);  // :229-235
  if (steps == 0) { // :237-244
    zero_out(op, x_out, mem);
    return;
  }
  check_decomp_arrays(alphas, n_alphas, betas, n_betas, steps, y != nullptr);
  ensure_state(op, steps);
  // decomposition -> device: norms[0], alphas, betas, y
  upload_decomp(op, b_norm, alphas, betas, steps);
  HIPCHK(hipMemcpyAsync(op->st.S.y, y, steps * sizeof(double), hipMemcpyHostToDevice, op->stream));
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

DevF device_f(const tpl_op_s* op, tpl_ftk_fn f, size_t k) {
  const bool is_inv = f == &tpl_ftk_inv, is_exp = f == &tpl_ftk_exp;
  const size_t kmax = !op->device_ftk ? 0
                      : is_inv ? (op->device_ftk == 1 ? kDevFtkMaxK : kDevFtkAutoK)
                      : is_exp ? kDevExpMaxK : 0;
  if ((!is_inv && !is_exp) || op->dist || k > kmax) return kDevHost;
  return is_exp ? kDevExp : kDevInv;
}

} // namespace tpl

extern "C" {
tpl_status tpl_op_apply(tpl_op_t op, const double* x, double* y, int mem) {
  return guarded([&] {
    need(op && ((x && y) || op->part.n == 0));
    set_device(op);
    if (op->part.n == 0) return;
    upload_vec(op, op->tmp, x, mem);
    if (op->dist && !op->part.hybrid) {
      halo_pack(op, op->tmpG);
      gather_vec(op, op->tmpG);
    }
    const CsrDev A = csr_dev(op);
    if (op->dense)
      HIPCHK(launch::dense_spmv(dense_dev(op), op->tmpG, op->W, op->stream));
    else
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
    need(op && alphas && betas && steps && b_norm);
    set_device(op);
    check_b(op, b, b_len), check_k(k);
    run_pass_one(op, b, k, mem, false, false);
    write_decomp(fetch_decomp(op), alphas, betas, steps, b_norm);
  });
}

tpl_status tpl_lanczos_standard(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                double* alphas, double* betas, size_t* steps, double* b_norm,
                                double* v_out, int mem, int reorth, tpl_step_cb cb,
                                void* cb_user) {
  return guarded([&] {
    need(op && alphas && betas && steps && b_norm);
    set_device(op);
    check_b(op, b, b_len), check_k(k);
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
    need(op && x_out);
    set_device(op);
    check_b(op, b, b_len);
    pass_two_one(op, b, alphas, n_alphas, betas, n_betas, steps, b_norm, y, y_len, x_out, v_out,
                 mem);
  });
}

tpl_status tpl_lanczos_two_pass(tpl_op_t op, const double* b, int64_t b_len, size_t k,
                                tpl_ftk_fn f, void* f_user, double* x_out, int mem) {
  return guarded([&] {
    need(op && x_out);
    set_device(op);
    check_b(op, b, b_len), check_k(k);
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
    need(op && x_out);
    set_device(op);
    check_b(op, b, b_len), check_k(k);
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

tpl_status tpl_lanczos_two_pass_inv_tol(tpl_op_t op, const double* b, int64_t b_len, size_t kmax,
                                        double tol, double* x_out, int mem, size_t* steps,
                                        int32_t* converged, double* res_out, size_t* res_len) {
  return guarded([&] {
    need(op && x_out), check_tol(tol);
    set_device(op);
    check_b(op, b, b_len), check_k(kmax);
    const TolReport rep{steps, converged, res_out, res_len, kmax};
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
      rep.put(0, (size_t)flags[2], !zero_x && flags[6] != 0, (const double*)(h + kFlagBytes),
              formed);
      return;
    }
    // composed on the host: pass one to kmax, the history and the rule, y on the first m*
    // rows, pass two to m* (the oracle of the device path)
    op->last_one_graph = false;
    run_pass_one(op, b, kmax, mem, false, false);
    const HostDecomp d = fetch_decomp(op);
    if (zero_result(op, d.flags, x_out, mem)) {
      rep.none(0);
      return;
    }
    // d.alphas as they are, not shifted by 0.0: alpha + 0.0 loses the sign of a -0.0
    const TolCol c = tol_col(d.alphas, d.betas, d.steps, d.b_norm, tol);
    HIPCHK(hipMemcpyAsync(op->st.S.y, c.y.data(), c.steps * sizeof(double), hipMemcpyHostToDevice,
                          op->stream));
    run_pass2(op, c.steps);
    download_vec(op, x_out, op->x, 1, mem);
    sync_checked(op);
    rep.put(0, c);
  });
}
} // extern "C"
