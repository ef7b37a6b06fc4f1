// The inverse solve that stops at a residual tolerance through the C++ host API
// (include/tpl.hpp: tpl::ftk::inv_residuals, tpl::solvers::lanczos_two_pass_inv_tol).
//   inv_tol_test --cpu   the history of a 2 x 2 T by hand
//   inv_tol_test --gpu   tridiag(-1, 2.5, -1), n = 600: the stop at 1e-6 against the fixed-k
//                        solve (bits) and against the true residual
// Built and run by tests/test_inv_tol_cpu.py and tests/test_gpu_inv_tol.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "tpl.hpp"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf("FAIL: ");        \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

using Vec = std::vector<double>;

static void history_by_hand() {
  // T = [[2, 1], [1, 2]], beta_2 = 1: res[0] = |1 * (1 / 2)|; row 0 eliminated without a
  // pivot: fact = 1 / 2, d = 2 - fact * 1, b = 0 - fact * 1, res[1] = |1 * (b / d)|
  const Vec res = tpl::ftk::inv_residuals({2.0, 2.0}, {1.0, 1.0});
  CHECK(res.size() == 2, "2 entries, got %zu", res.size());
  const double fact = 1.0 / 2.0, d = 2.0 - fact * 1.0, b = 0.0 - fact * 1.0;
  CHECK(res[0] == 0.5 && res[1] == std::fabs(1.0 * (b / d)), "res = %g, %g", res[0], res[1]);
  CHECK(tpl::ftk::inv_residuals({2.0, 2.0}, {1.0}).size() == 1, "k - 1 betas: k - 1 entries");
  CHECK(tpl::ftk::inv_residuals({}, {}).empty(), "empty T: empty history");
}

static void solve_to_tolerance() {
  const int64_t n = 600;
  std::vector<int64_t> rp(1, 0);
  std::vector<int32_t> ci;
  Vec v;
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0) ci.push_back((int32_t)(i - 1)), v.push_back(-1.0);
    ci.push_back((int32_t)i), v.push_back(2.5);
    if (i + 1 < n) ci.push_back((int32_t)(i + 1)), v.push_back(-1.0);
    rp.push_back((int64_t)ci.size());
  }
  tpl::Context ctx(0);
  tpl::HipCsrOp op(ctx, n, rp, ci, v);
  Vec b((size_t)n);
  for (int64_t i = 0; i < n; ++i) b[(size_t)i] = std::sin(1.0 + 0.37 * (double)i);
  const double tol = 1e-6;
  tpl::solvers::InvTolInfo info;
  const Vec x = tpl::solvers::lanczos_two_pass_inv_tol(op, b, 64, tol, &info);
  CHECK(info.converged && info.steps >= 2 && info.steps < 64, "steps %zu converged %d",
        info.steps, (int)info.converged);
  CHECK(info.residuals.size() >= info.steps, "history of %zu entries", info.residuals.size());
  if (failures) return;
  CHECK(info.residuals[info.steps - 1] <= tol && info.residuals[info.steps - 2] > tol,
        "first met at m*: %g then %g", info.residuals[info.steps - 2],
        info.residuals[info.steps - 1]);
  const Vec xk = tpl::solvers::lanczos_two_pass(op, b, info.steps, tpl::ftk::inv());
  CHECK(std::memcmp(x.data(), xk.data(), x.size() * sizeof(double)) == 0,
        "x is the fixed-k solve at k = m*");
  double rr = 0.0, bb = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double ax = 2.5 * x[(size_t)i];
    if (i > 0) ax -= x[(size_t)i - 1];
    if (i + 1 < n) ax -= x[(size_t)i + 1];
    rr += (b[(size_t)i] - ax) * (b[(size_t)i] - ax);
    bb += b[(size_t)i] * b[(size_t)i];
  }
  const double truth = std::sqrt(rr / bb), est = info.residuals[info.steps - 1];
  // the estimate follows the true residual to 1e-10 relative at 1e-6 (tests/test_inv_tol_cpu.py)
  CHECK(std::fabs(truth - est) <= 1e-6 * est, "true residual %.12e, estimate %.12e", truth, est);
  tpl::solvers::InvTolInfo none;
  const Vec x0 = tpl::solvers::lanczos_two_pass_inv_tol(op, b, 16, 0.0, &none);
  CHECK(!none.converged && none.steps == 16 && none.residuals.size() == 15, "tol = 0: kmax");
  bool threw = false;
  try {
    tpl::solvers::lanczos_two_pass_inv_tol(op, b, 16, -1.0);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a negative tolerance is an error");
}

int main(int argc, char** argv) {
  history_by_hand();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) solve_to_tolerance();
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
