// tpl_k_batch_multi.hip — the element-wise kernels of the batch-multi pass two
// (tpl_lanczos_two_pass_batch_multi, run_pass2_batch_multi in tpl_passes.cpp): m functions
// of every column of a lock-step group of NB right-hand sides.
//
// The two mechanisms compose as they stand. The group's step kernel k_bp2_spmv<NB, FMT>
// (tpl_k_batch_p2.hip, unchanged) runs with step records whose nflush field is 0 for every
// column (k_bp2_coefs0): it regenerates v_{j+1} for the live columns and leaves x alone.
// After each step at which some column flushes, k_bp2_xacc<NB, M> applies that step's
// grouped flush to M functions of all NB columns from the three live ring vectors: per
// (function, column) the operations of BEpiPass2::apply's x update and of k_p2_xacc, one
// for one (-ffp-contract=off: every product rounded on its own), under the column's own
// count bp2_flush(j, steps_c - 1). So result (c, i) holds the bits of the single solve of
// b_c with f_i.
//
// Function f's result is an interleaved group vector of its own (entry i of column c at
// X + f xstride + i NB + c), so the X loads and stores are as wide as the ring's.
// Coefficients: (f, c, j) at Y[(f NB + c) kcap + j]. A launch stages its 3 M NB
// coefficients in LDS (one load per thread, one barrier); the element loop reads them at
// uniform LDS addresses (broadcast reads), so they hold neither 3 M NB scalar register
// pairs (96 at NB = M = 4: more than there are) nor vector registers across the loop.
//
// All three kernels of the pass run on the element grid (elem_block): row block rb stays
// on the XCD whose chunks and bins wrote its v entries.
#include "tpl_kbatch.h"

namespace tpl {

// Prologue (k_bp2_init's two operations per column, for m functions): v_1 = b_c (1/||b_c||)
// into the ring; X_f(c) = v_1 y_{c,f}[0]. A column that took no step gets zeros.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp2_minit(int64_t n, int64_t E, int G2, BatchDev B,
                                                    const double* __restrict__ Y, int m,
                                                    const double* __restrict__ b,
                                                    double* __restrict__ v1,
                                                    double* __restrict__ X, int64_t xstride) {
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  double invN[NB];
  bool on[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    on[c] = B.flags[8 * c + 2] >= 1;
    invN[c] = 1.0 / B.norms[(size_t)c * (B.kcap + 1)];
  }
  const int64_t beg = (int64_t)rb * E;
  const int64_t end = beg + E < n ? beg + E : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const VecNB<NB> bv = ld_nb<NB>(b, i);
    double v[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      v[c] = bv.v[c] * invN[c];
      v1[i * NB + c] = on[c] ? v[c] : 0.0;
    }
    for (int f = 0; f < m; ++f) {
      double* Xf = X + (size_t)f * xstride;
#pragma unroll
      for (int c = 0; c < NB; ++c)
        Xf[i * NB + c] = on[c] ? v[c] * Y[((size_t)f * NB + c) * B.kcap] : 0.0;
    }
  }
}

// k_bp2_coefs with every column's nflush written as 0 (and no y: the step kernel then never
// reads or writes x). The records of steps 1 .. kmax-1.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp2_coefs0(BatchDev B, int kmax) {
  const int j = blockIdx.x * kTPB + threadIdx.x;
  if (j < 1 || j >= kmax) return;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const int steps = B.flags[8 * c + 2];
    const double* al = B.alphas + (size_t)c * B.kcap;
    const double* be = B.betas + (size_t)c * B.kcap;
    double* r = B.p2c + 8 * ((size_t)j * NB + c);
    r[0] = j >= 2 ? be[j - 2] : 0.0;
    r[1] = al[j - 1];
    r[2] = 1.0 / be[j - 1];
    r[3] = 0.0;
    r[4] = 0.0;
    r[5] = 0.0;
    r[6] = j < steps ? 1.0 : 0.0;
    r[7] = 0.0;
  }
}

// Grouped flush after step j for M functions of the NB columns: per (f, c), with column c's
// count n_c = bp2_flush(j, steps_c - 1) (0 once j >= steps_c), the last n_c terms, oldest
// first,
//   X_f(c) = ((X_f(c) + y[j-2] v_{j-1}) + y[j-1] v_j) + y[j] v_{j+1}
// with the terms beyond n_c skipped. vp / vc / vn: v_{j-1}, v_j, v_{j+1} (the ring after
// step j's launch), read once per launch for all M functions. A column with n_c == 0 loads
// whatever is there and stores nothing; when no column flushes the launch returns at once
// (the same decision in every workgroup).
template <int NB, int M>
__global__ __launch_bounds__(kTPB) void k_bp2_xacc(int64_t n, int64_t E, int G2,
                                                   const int32_t* __restrict__ flags,
                                                   const double* __restrict__ Y, int kcap, int j,
                                                   const double* __restrict__ vp,
                                                   const double* __restrict__ vc,
                                                   const double* __restrict__ vn,
                                                   double* __restrict__ X, int64_t xstride) {
  __shared__ double co[3 * M * NB];  // [q][f][c]: y_{c,f}[j - q]
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  int cnt[NB];
  bool flush[NB];
  bool all_flush = true, any_flush = false;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const int steps = flags[8 * c + 2];
    cnt[c] = j < steps ? bp2_flush(j, steps - 1) : 0;
    flush[c] = cnt[c] > 0;
    all_flush = all_flush && flush[c];
    any_flush = any_flush || flush[c];
  }
  if (!any_flush) return;
  if (threadIdx.x < 3 * M * NB) {
    const int q = threadIdx.x / (M * NB), fc = threadIdx.x % (M * NB);
    const int jq = j - q;  // clamped: read, never used (n_c <= j)
    co[threadIdx.x] = Y[(size_t)fc * kcap + (jq > 0 ? jq : 0)];
  }
  __syncthreads();
  const int64_t beg = (int64_t)rb * E;
  const int64_t end = beg + E < n ? beg + E : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const VecNB<NB> p = ld_nb<NB>(vp, i), c0 = ld_nb<NB>(vc, i), nx = ld_nb<NB>(vn, i);
    VecNB<NB> x[M];
#pragma unroll
    for (int f = 0; f < M; ++f) x[f] = ld_nb<NB>(X + (size_t)f * xstride, i);
#pragma unroll
    for (int f = 0; f < M; ++f) {
      double out[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        double xv = x[f].v[c];
        if (cnt[c] >= 3) xv = xv + co[(2 * M + f) * NB + c] * p.v[c];
        if (cnt[c] >= 2) xv = xv + co[(M + f) * NB + c] * c0.v[c];
        out[c] = xv + co[f * NB + c] * nx.v[c];
      }
      st_nb<NB>(X + (size_t)f * xstride, i, out, flush, all_flush);
    }
  }
}

// The m result vectors of a group out to the caller's columns (c m + f), locality
// permutation included: X[(c m + f) n + i] = in_f[idx[i] NB + c] (k_b_deinterleave with
// the column stride m n, all functions in one launch).
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bm_deinterleave(int64_t n, double* __restrict__ X,
                                                          const double* __restrict__ in,
                                                          int64_t xstride, int m,
                                                          const int32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    const int64_t src = idx ? idx[i] : i;
    for (int f = 0; f < m; ++f) {
      const VecNB<NB> v = ld_nb<NB>(in + (size_t)f * xstride, src);
#pragma unroll
      for (int c = 0; c < NB; ++c) X[((int64_t)c * m + f) * n + i] = v.v[c];
    }
  }
}

namespace launch {

hipError_t bp2_minit(int nb, const CsrDev& A, const BatchDev& B, const double* Y, int m,
                     const double* b, double* v1, double* X, int64_t xstride, hipStream_t s) {
  if (A.n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp2_minit<NB>, dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n,
                                       A.E, A.G2, B, Y, m, b, v1, X, xstride));
  return hipGetLastError();
}
hipError_t bp2_coefs0(int nb, const BatchDev& B, int kmax, hipStream_t s) {
  if (kmax <= 1) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp2_coefs0<NB>, dim3((kmax + kTPB - 1) / kTPB),
                                       dim3(kTPB), 0, s, B, kmax));
  return hipGetLastError();
}

template <int NB, int M>
static void bxacc_launch(const CsrDev& A, const BatchDev& B, const double* Y, int j,
                         const double* vp, const double* vc, const double* vn, double* X,
                         int64_t xstride, hipStream_t s) {
  hipLaunchKernelGGL((k_bp2_xacc<NB, M>), dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n, A.E, A.G2,
                     B.flags, Y, B.kcap, j, vp, vc, vn, X, xstride);
}
template <int NB>
static void bxacc_funcs(int m, const CsrDev& A, const BatchDev& B, const double* Y, int j,
                        const double* vp, const double* vc, const double* vn, double* X,
                        int64_t xstride, hipStream_t s) {
  static_assert(kBatchMultiFuncs == 4, "one instance per function count");
  switch (m) {
    case 1: bxacc_launch<NB, 1>(A, B, Y, j, vp, vc, vn, X, xstride, s); break;
    case 2: bxacc_launch<NB, 2>(A, B, Y, j, vp, vc, vn, X, xstride, s); break;
    case 3: bxacc_launch<NB, 3>(A, B, Y, j, vp, vc, vn, X, xstride, s); break;
    default: bxacc_launch<NB, 4>(A, B, Y, j, vp, vc, vn, X, xstride, s); break;
  }
}
hipError_t bp2_xacc(int nb, const CsrDev& A, const BatchDev& B, const double* Y, int j,
                    const double* vp, const double* vc, const double* vn, double* X,
                    int64_t xstride, int m, hipStream_t s) {
  if (j < 1 || m < 1 || m > kBatchMultiFuncs) return hipErrorInvalidValue;
  if (A.n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, bxacc_funcs<NB>(m, A, B, Y, j, vp, vc, vn, X, xstride, s));
  return hipGetLastError();
}
hipError_t bm_deinterleave(int nb, int64_t n, double* X, const double* in, int64_t xstride,
                           int m, const int32_t* idx, hipStream_t s) {
  if (n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bm_deinterleave<NB>, dim3(elem_grid(n)), dim3(kTPB), 0,
                                       s, n, X, in, xstride, m, idx));
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
