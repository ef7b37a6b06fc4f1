// tpl_solvers_batch.cpp — s right-hand sides in lock-step groups (include/tpl.h): f(A) b_c, the
// passes on their own, m functions or m times per column, and (A + sigma_i I)^{-1} b_c with every
// (c, i) stopped at a tolerance. Every entry point walks its columns as Groups: a
// group of four or two runs here, a single remainder column runs the single-column solve of
// tpl_solve.h.
#include "tpl_solve.h"

using namespace tpl;

namespace {
// The grouping rule (DESIGN.md §2 "Several right-hand sides in lock-step", include/tpl.h):
// the columns are taken in order, four at a time while four remain, then two at a time;
// a last single column runs the single host-f solve. No group is padded: a remainder of
// three is a group of two and a single solve (a padded group of four measured slower than
// three single solves).
int group_width(size_t rem) { return rem >= 4 ? 4 : (rem >= 2 ? 2 : 1); }
// The columns of a call in that order, as (c0, nb): a group of nb = 4 or 2 from column c0, or a
// lone column (nb = 1). An operator of no rows runs every column alone.
struct Groups {  // the range is its own iterator
  size_t s, c0 = 0;
  bool alone;
  struct Group { size_t c0; int nb; };
  Groups(const tpl_op_s* op, size_t s_) : s(s_), alone(op->part.n == 0) {}
  Group operator*() const { return {c0, alone ? 1 : group_width(s - c0)}; }
  void operator++() { c0 += (size_t)(**this).nb; }
  bool operator!=(const Groups&) const { return c0 < s; }
  Groups begin() const { return *this; }
  Groups end() const { return *this; }
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
// What tpl_lanczos_pass_two_batch and _batch_multi check of their decompositions: the single
// call's checks, per column in ascending order. (NULL arrays are accepted when no column takes
// a step that needs them.)
void check_decomp_cols(size_t s, const size_t* steps, size_t ld, const double* b_norms,
                       const double* alphas, const double* betas, const double* y) {
  for (size_t c = 0; c < s; ++c) {
    check_b_norm(b_norms[c]);
    if (steps[c] > ld || (steps[c] > 0 && (!alphas || !y)) || (steps[c] > 1 && !betas))
      fail_short_decomp();
    check_steps_fit(steps[c]);
  }
}
// Column c of a column-major array, columns ld apart (NULL stays NULL: no arithmetic on it).
const double* col_of(const double* p, size_t c, size_t ld) { return p ? p + c * ld : nullptr; }
// The largest steps_c of columns c0 .. c0 + nb (at least 1): what ensure_batch sizes a group
// for. set_columns: those columns' decompositions into the group's host mirror.
size_t max_steps(const size_t* steps, size_t c0, int nb) {
  size_t kmax = 1;
  for (int c = 0; c < nb; ++c) kmax = std::max(kmax, steps[c0 + c]);
  return kmax;
}
void set_columns(GroupHead& g, size_t c0, int nb, const size_t* steps, const double* b_norms,
                 const double* alphas, const double* betas, size_t ld) {
  for (int c = 0; c < nb; ++c) {
    const size_t cc = c0 + (size_t)c;
    g.set_column((size_t)c, steps[cc], b_norms[cc], col_of(alphas, cc, ld), col_of(betas, cc, ld));
  }
}

// tpl_lanczos_two_pass_batch after its argument checks.
void two_pass_batch(tpl_op_s* op, const double* B, size_t s, size_t k, tpl_ftk_fn f, void* f_user,
                    double* x_out, int mem) {
  op->last_one_graph = false;
  const size_t n = (size_t)op->part.n;
  for (const auto [c0, nb] : Groups(op, s)) {
    if (nb == 1) {  // the single solve's host-f path
      two_pass_host_f(op, B + c0 * n, k, f, f_user, x_out + c0 * n, mem, false);
      continue;
    }
    // 1. pass one for the group's columns in lock-step
    GroupHead g = pass_one_group(op, B + c0 * n, k, nb, mem);
    // 2. f(T_k) e_1 per column on the host, in column order, 3. y_c = y'_c * ||b_c||
    size_t kmax = 0;
    std::vector<double> y;
    for (int c = 0; c < nb; ++c) {
      const HostDecomp d = g.decomp((size_t)c);
      if (d.flags[1]) fail_input(kZeroInput);
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
  }
}

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

// One group of the batch shifted solve as one graph: pass one with a lane per (column, shift),
// every y_{c,i} on its own m*_{c,i} rows, the cut pass two; X: the group's nb m result columns,
// rep: the reporter of the group's first result. (ensure_batch, _batch_multi, _batch_cut first.)
void shifted_group_on_device(tpl_op_s* op, const double* B, size_t kmax, int nb,
                             const double* sigmas, size_t m, double tol, double* X, int mem,
                             const TolReport& rep) {
  BatchBufs& bb = op->bat;
  const launch::BatchShiftTol t = ensure_batch_stol(op, m);
  const size_t mc = bb.stol_m, kc = bb.kcap, w = (size_t)kBatchNbMax;
  upload_group(op, B, nb, mem);
  HIPCHK(hipMemsetAsync(t.t0.hits, 0, w * 2 * mc * sizeof(int32_t), op->stream));
  HIPCHK(hipMemcpyAsync(bb.d_stol, &tol, sizeof(double), hipMemcpyHostToDevice, op->stream));
  HIPCHK(hipMemcpyAsync(bb.d_stol + 1, sigmas, m * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  run_two_pass_batch_shifted_inv_tol(op, kmax, nb, t);
  download_group_multi(op, X, nb, m, mem);
  char* h = (char*)bb.h_stol;
  int32_t* h_flags = (int32_t*)h;
  int32_t* h_ints = (int32_t*)(h + w * kFlagBytes);
  double* h_res = (double*)(h + w * kFlagBytes + w * 2 * mc * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(h_flags, bb.S.flags, (size_t)nb * kFlagBytes, hipMemcpyDeviceToHost,
                        op->stream));
  HIPCHK(hipMemcpyAsync(h_ints, t.t0.hits, w * 2 * mc * sizeof(int32_t), hipMemcpyDeviceToHost,
                        op->stream));
  if (rep.res_out && kmax > 1)
    for (int c = 0; c < nb; ++c)
      HIPCHK(hipMemcpyAsync(h_res + (size_t)c * kc * mc, t.col(c).res,
                            (kmax - 1) * m * sizeof(double), hipMemcpyDeviceToHost, op->stream));
  sync_checked(op);
  for (int c = 0; c < nb; ++c) {
    const int32_t* fl = h_flags + 8 * c;
    if (fl[1]) fail_input(kZeroInput);
    const int32_t* hits = h_ints + (size_t)c * 2 * mc;
    rep.decode((size_t)c * m, m, fl[2], hits, hits + mc, h_res + (size_t)c * kc * mc);
  }
}
// The same group composed on the host (the oracle of the device path): the group's pass one to
// kmax, then per column in order the zero check and per shift the history, the rule and y on
// the first m*_{c,i} rows; M_c = max_i m*_{c,i} becomes column c's device-held step count, and
// one pass two of max_c M_c steps cuts every result at its own step.
void shifted_group_on_host(tpl_op_s* op, const double* B, size_t kmax, int nb,
                           const double* sigmas, size_t m, double tol, double* X, int mem,
                           const TolReport& rep) {
  enqueue_pass_one_group(op, B, kmax, nb, mem);
  GroupHead g = fetch_group(op);
  GroupY Y(op, nb, m);
  std::vector<int32_t> cut((size_t)kBatchNbMax * TPL_MULTI_MAX, 0);
  int32_t Mc[kBatchNbMax] = {0, 0, 0, 0};
  size_t Mmax = 0;
  for (int c = 0; c < nb; ++c) {
    const HostDecomp d = g.decomp((size_t)c);
    if (d.flags[1]) fail_input(kZeroInput);
    for (size_t i = 0; i < m; ++i) {
      const size_t e = (size_t)c * m + i;
      if (d.steps == 0) {
        rep.none(e);
        continue;
      }
      const TolCol sc = shifted_col(d, sigmas[i], tol);
      std::copy(sc.y.begin(), sc.y.end(), Y.col(i, (size_t)c));
      cut[(size_t)c * TPL_MULTI_MAX + i] = (int32_t)sc.steps;
      Mc[c] = std::max(Mc[c], (int32_t)sc.steps);
      rep.put(e, sc);
    }
    Mmax = std::max(Mmax, (size_t)Mc[c]);
  }
  for (int c = 0; c < nb; ++c) upload_col_count(op, c, &Mc[c]);
  Y.upload(op);
  HIPCHK(hipMemcpyAsync(op->d_bcut, cut.data(), cut.size() * sizeof(int32_t),
                        hipMemcpyHostToDevice, op->stream));
  run_pass2_batch_multi_cut(op, std::max<size_t>(Mmax, 1), nb, m);
  download_group_multi(op, X, nb, m, mem);
  sync_checked(op);
}
} // namespace

extern "C" {
tpl_status tpl_lanczos_two_pass_batch(tpl_op_t op, const double* B, int64_t b_len, size_t s,
                                      size_t k, tpl_ftk_fn f, void* f_user, double* x_out,
                                      int mem) {
  return guarded([&] {
    check_batch_args(op, B && x_out && f, s);
    check_b(op, B, b_len), check_k(k);
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
    check_b(op, B, b_len), check_k(k);
    const TimingOff untimed(op);
    const size_t n = (size_t)op->part.n;
    auto write = [&](const HostDecomp& d, size_t c) {
      write_decomp(d, alphas + c * k, betas + c * k, steps + c, b_norms + c);
    };
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {
        run_pass_one(op, B + c0 * n, k, mem, false, false);
        write(fetch_decomp(op), c0);
        continue;
      }
      GroupHead g = pass_one_group(op, B + c0 * n, k, nb, mem);
      for (int c = 0; c < nb; ++c) write(g.decomp((size_t)c), c0 + (size_t)c);
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
    check_decomp_cols(s, steps, ld, b_norms, alphas, betas, y);
    const size_t n = (size_t)op->part.n;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {
        const size_t st = steps[c0];
        pass_two_one(op, B + c0 * n, col_of(alphas, c0, ld), st, col_of(betas, c0, ld),
                     st > 0 ? st - 1 : 0, st, b_norms[c0], col_of(y, c0, ld), st, x_out + c0 * n,
                     nullptr, mem);
        continue;
      }
      const size_t kmax = max_steps(steps, c0, nb);
      ensure_batch(op, nb, kmax);
      // decompositions -> the group's state: steps_c, ||b_c||, alphas, betas, y
      GroupHead g(op);
      set_columns(g, c0, nb, steps, b_norms, alphas, betas, ld);
      for (int c = 0; c < nb; ++c)
        if (const size_t st = steps[c0 + c])
          std::memcpy(g.y((size_t)c), y + (c0 + c) * ld, st * sizeof(double));
      g.upload(op, g.bytes());
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch(op, kmax, nb);
      download_group(op, x_out + c0 * n, nb, mem);
      sync_checked(op);
    }
  });
}

// Every group of four or two columns runs fused (lock-step pass one, one pass two for the
// group's nb x m results): both widths measured faster than nb multi-function solves and than
// m batch solves (profiles/batch_multi_timing.txt), so no width is
// routed to an existing path.
tpl_status tpl_lanczos_two_pass_batch_multi(tpl_op_t op, const double* B, int64_t b_len,
                                            size_t s, size_t k, const tpl_ftk_fn* fs,
                                            void** f_users, size_t m, double* x_out, int mem) {
  return guarded([&] {
    check_batch_multi_args(op, B && fs && x_out, s, m);
    check_b(op, B, b_len), check_k(k);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    if (m == 1) {  // one function: the batch solve
      two_pass_batch(op, B, s, k, fs[0], f_users ? f_users[0] : nullptr, x_out, mem);
      return;
    }
    op->last_one_graph = false;
    const size_t n = (size_t)op->part.n;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {  // the multi-function solve of that column
        two_pass_multi(op, B + c0 * n, k, fs, f_users, m, x_out + c0 * m * n, mem);
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
        if (d.flags[1]) fail_input(kZeroInput);
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
    check_decomp_cols(s, steps, ld, b_norms, alphas, betas, y);
    const size_t n = (size_t)op->part.n;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {  // the multi-function pass two of that column
        const size_t st = steps[c0];
        pass_two_multi(op, B + c0 * n, col_of(alphas, c0, ld), st, col_of(betas, c0, ld),
                       st > 0 ? st - 1 : 0, st, b_norms[c0], col_of(y, c0 * m, ld), ld, m,
                       x_out + c0 * m * n, mem);
        continue;
      }
      ensure_batch(op, nb, max_steps(steps, c0, nb));
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      // decompositions -> the group's state (steps_c, ||b_c||, alphas, betas), y -> the table
      GroupHead g(op);
      GroupY Y(op, nb, m);
      set_columns(g, c0, nb, steps, b_norms, alphas, betas, ld);
      for (int c = 0; c < nb; ++c)
        for (size_t i = 0, cc = c0 + (size_t)c; i < m && steps[cc] > 0; ++i)
          std::memcpy(Y.col(i, (size_t)c), y + (cc * m + i) * ld, steps[cc] * sizeof(double));
      g.upload(op, g.bytes());
      Y.upload(op);
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch_multi(op, steps + c0, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
    }
  });
}

tpl_status tpl_lanczos_two_pass_batch_exp_times(tpl_op_t op, const double* B, int64_t b_len,
                                                size_t s, size_t k, const double* ts, size_t m,
                                                double* x_out, int mem, int32_t* on_device) {
  return guarded([&] {
    check_batch_multi_args(op, B && ts && x_out, s, m);
    check_b(op, B, b_len), check_k(k);
    check_finite(ts, m, kTimesFinite);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    op->last_one_graph = false;
    if (on_device) std::fill(on_device, on_device + s * m, 0);
    const bool dev = exp_on_device(op, k);
    const size_t n = (size_t)op->part.n;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {  // the single-b exp-times solve of that column
        two_pass_exp_times(op, B + c0 * n, k, ts, m, x_out + c0 * m * n, mem,
                           on_device ? on_device + c0 * m : nullptr);
        continue;
      }
      ensure_batch(op, nb, k);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_exp_times_batch(op);
      BatchBufs& bb = op->bat;
      // 1. pass one for the group's columns in lock-step; 2. straight behind it on the
      //    stream every exp(t_i T_k) e_1 of every column at once (each steps_c stays on the
      //    device), y_{c,i} = y'_{c,i} * ||b_c|| into the group's coefficient table
      if (dev)
        HIPCHK(hipMemcpyAsync(op->d_exp_ts, ts, m * sizeof(double), hipMemcpyHostToDevice,
                              op->stream));
      enqueue_pass_one_group(op, B + c0 * n, k, nb, mem);
      if (dev) {
        HIPCHK(launch::ftk_exp_times_batch(nb, bb.S, (int)k, op->d_exp_ts, (int)m, bb.d_my,
                                           op->d_expb_back, 1, op->stream));
        HIPCHK(hipMemcpyAsync(op->h_expb_back, op->d_expb_back,
                              (size_t)nb * m * sizeof(int32_t), hipMemcpyDeviceToHost,
                              op->stream));
      }
      GroupHead g = fetch_group(op);  // the group's one synchronisation before pass two
      // 3. per column in order: the zero-vector check, then the times handed back (without
      //    the device: all of them) on the host in index order; only their columns are
      //    uploaded (host table: function i, column c at (i nb + c) k, alive until the sync)
      std::vector<double> Yh, y;
      size_t steps[kBatchNbMax];
      for (int c = 0; c < nb; ++c) {
        const HostDecomp d = g.decomp((size_t)c);
        if (d.flags[1]) fail_input(kZeroInput);
        steps[c] = d.steps;
        for (size_t i = 0; i < m; ++i) {
          const bool kept = dev && d.steps > 0 && !op->h_expb_back[(size_t)c * m + i];
          if (on_device) on_device[(c0 + (size_t)c) * m + i] = kept ? 1 : 0;
          if (kept) continue;
          if (Yh.empty() && d.steps > 0) Yh.resize(m * (size_t)nb * k);
          const size_t at = i * (size_t)nb + (size_t)c;
          exp_col_on_host(op, d, ts[i], y, Yh.empty() ? nullptr : Yh.data() + at * k,
                          bb.d_my + at * bb.kcap);
        }
      }
      // 4. one pass two for all nb x m results
      run_pass2_batch_multi(op, steps, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
    }
  });
}

size_t tpl_batch_shifted_inv_tol_auto_k(void) { return kBatchShiftedAutoK; }

tpl_status tpl_lanczos_two_pass_batch_shifted_inv_tol(
    tpl_op_t op, const double* B, int64_t b_len, size_t s, size_t kmax, const double* sigmas,
    size_t m, double tol, double* x_out, int mem, size_t* steps, int32_t* converged,
    double* res_out, size_t* res_len) {
  return guarded([&] {
    need(op && B && sigmas && x_out), check_s(s), check_m(m), check_tol(tol);
    check_finite(sigmas, m, kShiftsFinite);
    refuse_dense(op, kBatchMultiSolve);
    set_device(op);
    refuse_partitioned(op, kBatchMultiSolve);
    check_b(op, B, b_len), check_k(kmax);
    const TimingOff untimed(op);
    const LongCacheScope cache(op, TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI);
    const size_t n = (size_t)op->part.n;
    // result (c, i): entry e = c m + i of every output
    const TolReport rep{steps, converged, res_out, res_len, kmax};
    const bool dev = batch_shifted_on_device(op, kmax);
    bool groups_one_graph = true, any_group = false;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {  // the single-b solve of that column, with its own routing
        shifted_inv_tol_one(op, B + c0 * n, kmax, sigmas, m, tol, x_out + c0 * m * n, mem,
                            rep.at(c0 * m));
        continue;
      }
      any_group = true;
      ensure_batch(op, nb, kmax);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_batch_cut(op);
      double* X = x_out + c0 * m * n;
      const TolReport r = rep.at(c0 * m);
      if (dev) {
        shifted_group_on_device(op, B + c0 * n, kmax, nb, sigmas, m, tol, X, mem, r);
      } else {
        groups_one_graph = false;
        shifted_group_on_host(op, B + c0 * n, kmax, nb, sigmas, m, tol, X, mem, r);
      }
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
    need(op && B && x_out && steps && b_norms && col_steps && y && alphas);
    check_s(s), check_m(m);
    // its own rule, unlike the other batch passes two (check_decomp_cols): every column takes
    // at least one step, and the counts and the decomposition are checked per column in
    // ascending order before anything touches a device
    for (size_t c = 0; c < s; ++c) {
      if (steps[c] == 0 || steps[c] > ld || steps[c] > (size_t)INT32_MAX / 2)
        fail(TPL_ERR_INVALID_ARGUMENT, "steps[c] must be >= 1 and ld >= steps[c]");
      for (size_t i = 0; i < m; ++i)
        if (col_steps[c * m + i] < 1 || col_steps[c * m + i] > steps[c])
          fail(TPL_ERR_INVALID_ARGUMENT, "every col_steps[c m + i] must be between 1 and steps[c]");
      check_b_norm(b_norms[c]);
      if (steps[c] > 1 && !betas) fail_short_decomp();
    }
    refuse_dense(op, kBatchMultiSolve);
    set_device(op);
    refuse_partitioned(op, kBatchMultiSolve);
    check_b(op, B, b_len);
    const TimingOff untimed(op);
    const size_t n = (size_t)op->part.n;
    for (const auto [c0, nb] : Groups(op, s)) {
      if (nb == 1) {  // the single pass two with a cut per column
        int32_t cs[TPL_MULTI_MAX];
        for (size_t i = 0; i < m; ++i) cs[i] = (int32_t)col_steps[c0 * m + i];
        pass_two_multi_cut_run(op, B + c0 * n, alphas + c0 * ld, col_of(betas, c0, ld),
                               steps[c0], b_norms[c0], y + c0 * m * ld, ld, cs, m,
                               x_out + c0 * m * n, mem);
        continue;
      }
      const size_t kmax = max_steps(steps, c0, nb);
      ensure_batch(op, nb, kmax);
      ensure_batch_multi(op, m, mem != TPL_MEM_DEVICE);
      ensure_batch_cut(op);
      // decompositions -> the group's state (steps_c, ||b_c||, alphas, betas), y -> the
      // table, the cuts -> the cut table
      GroupHead g(op);
      GroupY Y(op, nb, m);
      std::vector<int32_t> cut((size_t)kBatchNbMax * TPL_MULTI_MAX, 0);
      set_columns(g, c0, nb, steps, b_norms, alphas, betas, ld);
      for (int c = 0; c < nb; ++c) {
        const size_t cc = c0 + (size_t)c;
        for (size_t i = 0; i < m; ++i) {
          std::memcpy(Y.col(i, (size_t)c), y + (cc * m + i) * ld, steps[cc] * sizeof(double));
          cut[(size_t)c * TPL_MULTI_MAX + i] = (int32_t)col_steps[cc * m + i];
        }
      }
      g.upload(op, g.bytes());
      Y.upload(op);
      HIPCHK(hipMemcpyAsync(op->d_bcut, cut.data(), cut.size() * sizeof(int32_t),
                        hipMemcpyHostToDevice, op->stream));
      upload_group(op, B + c0 * n, nb, mem);
      run_pass2_batch_multi_cut(op, kmax, nb, m);
      download_group_multi(op, x_out + c0 * m * n, nb, m, mem);
      sync_checked(op);
    }
  });
}
} // extern "C"
