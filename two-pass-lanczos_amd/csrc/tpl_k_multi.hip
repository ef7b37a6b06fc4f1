// tpl_k_multi.hip — the element-wise kernels of the multi-function pass two
// (tpl_lanczos_two_pass_multi, run_pass2_multi in tpl_passes.cpp): k_p2_minit, k_p2_xacc.
//
// m functions over one Krylov space share pass one and the basis pass two regenerates;
// only y_i = ||b|| f_i(T_k) e_1 differs, and it feeds one line of pass two, x += y_j v_{j+1}.
// So the step kernel runs with nflush = 0 (k_p2_spmv regenerates v_{j+1} and leaves x alone)
// and these kernels apply the x updates of every column from the three live ring vectors:
// the operations of k_p2_init and of EpiPass2R::apply's grouped flush, one for one
// (-ffp-contract=off: every product rounded on its own), so column i holds the bits of the
// single solve with f_i.
//
// Both run on the element grid (elem_block): row block rb stays on the XCD whose chunks and
// bins wrote its v entries. Y is the uploaded coefficient table, column i at Y + i * ldy.
#include "tpl_klaunch.h"

namespace tpl {

// Prologue: v_1 = b * (1/||b||) into the ring; X_i = v_1 * y_i[0] for the m columns
// (k_p2_init's two operations per column).
__global__ __launch_bounds__(kTPB) void k_p2_minit(int64_t n, int64_t E, int G2,
                                                   const double* __restrict__ norms,
                                                   const double* __restrict__ Y, int ldy,
                                                   const double* __restrict__ b,
                                                   double* __restrict__ v1,
                                                   double* __restrict__ X, int64_t ldx, int m) {
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  const double invN = 1.0 / norms[0];
  const int64_t beg = (int64_t)rb * E;
  const int64_t end = beg + E < n ? beg + E : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const double v = b[i] * invN;
    v1[i] = v;
    for (int c = 0; c < m; ++c) X[(size_t)c * ldx + i] = v * Y[(size_t)c * ldy];
  }
}

// Grouped flush after step j for M columns: the last nflush (1..3) terms, oldest first,
//   X_i = ((X_i + y_i[j-2] v_{j-1}) + y_i[j-1] v_j) + y_i[j] v_{j+1}
// with the terms beyond nflush skipped. vp / vc / vn: v_{j-1}, v_j, v_{j+1} (the ring after
// step j's launch; vp is loaded but unused below nflush = 3). The 3 M coefficients are
// loads at uniform addresses issued before the element loop; per element the three v's and
// the M x's are all loaded before the first use.
template <int M>
__global__ __launch_bounds__(kTPB) void k_p2_xacc(int64_t n, int64_t E, int G2,
                                                  const double* __restrict__ Y, int ldy, int j,
                                                  int nflush, const double* __restrict__ vp,
                                                  const double* __restrict__ vc,
                                                  const double* __restrict__ vn,
                                                  double* __restrict__ X, int64_t ldx) {
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  const int j1 = j >= 1 ? j - 1 : 0, j2 = j >= 2 ? j - 2 : 0;  // clamped: read, never used
  double y0[M], y1[M], y2[M];
#pragma unroll
  for (int c = 0; c < M; ++c) {
    const double* yc = Y + (size_t)c * ldy;
    y0[c] = yc[j];
    y1[c] = yc[j1];
    y2[c] = yc[j2];
  }
  const int64_t beg = (int64_t)rb * E;
  const int64_t end = beg + E < n ? beg + E : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const double p = vp[i], c0 = vc[i], nx = vn[i];
    double x[M];
#pragma unroll
    for (int c = 0; c < M; ++c) x[c] = X[(size_t)c * ldx + i];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double xv = x[c];
      if (nflush >= 3) xv = xv + y2[c] * p;
      if (nflush >= 2) xv = xv + y1[c] * c0;
      st_out(X + (size_t)c * ldx + i, xv + y0[c] * nx);
    }
  }
}

} // namespace tpl

// ------------------------------------------------------------ host launchers
namespace tpl {
namespace launch {

hipError_t p2_minit(const CsrDev& A, const DevState& S, const double* Y, int ldy, const double* b,
                    double* v1, double* X, int64_t ldx, int m, hipStream_t s) {
  hipLaunchKernelGGL(k_p2_minit, dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n, A.E, A.G2, S.norms, Y,
                     ldy, b, v1, X, ldx, m);
  return hipGetLastError();
}

template <int M>
static void xacc_launch(const CsrDev& A, const double* Y, int ldy, int j, int nflush,
                        const double* vp, const double* vc, const double* vn, double* X,
                        int64_t ldx, hipStream_t s) {
  hipLaunchKernelGGL(k_p2_xacc<M>, dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n, A.E, A.G2, Y, ldy, j,
                     nflush, vp, vc, vn, X, ldx);
}

hipError_t p2_xacc(const CsrDev& A, const double* Y, int ldy, int j, int nflush, const double* vp,
                   const double* vc, const double* vn, double* X, int64_t ldx, int m,
                   hipStream_t s) {
  if (nflush < 1 || nflush > 3 || j < nflush) return hipErrorInvalidValue;
  switch (m) {
    case 1: xacc_launch<1>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 2: xacc_launch<2>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 3: xacc_launch<3>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 4: xacc_launch<4>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 5: xacc_launch<5>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 6: xacc_launch<6>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 7: xacc_launch<7>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    case 8: xacc_launch<8>(A, Y, ldy, j, nflush, vp, vc, vn, X, ldx, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
