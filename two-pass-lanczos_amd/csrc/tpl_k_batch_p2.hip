// tpl_k_batch_p2.hip — pass two of the lock-step batch solve: the batch siblings of
// k_p2_init, k_p2_coefs and k_p2_spmv for NB = 2 and NB = 4 columns per launch. A column
// whose steps_c is below the group's maximum applies, through its own step records, exactly
// the flushes the single solve applies for steps_c (at multiples of 3 and at steps_c - 1),
// and stores nothing afterwards. Building blocks: tpl_kbatch.h.
#include "tpl_kbatch.h"

namespace tpl {

// Pass-two prologue (k_p2_init per column): v_1 = b_c * (1/||b_c||); x_c = v_1 * y_1. A
// column that took no step gets the zero result.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp2_init(int64_t n, BatchDev B,
                                                   const double* __restrict__ b,
                                                   double* __restrict__ v1,
                                                   double* __restrict__ x) {
  double invN[NB], y0[NB];
  bool on[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    on[c] = B.flags[8 * c + 2] >= 1;
    invN[c] = 1.0 / B.norms[(size_t)c * (B.kcap + 1)];
    y0[c] = B.y[(size_t)c * B.kcap];
  }
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    const VecNB<NB> bv = ld_nb<NB>(b, i);
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const double v = bv.v[c] * invN[c];
      v1[i * NB + c] = on[c] ? v : 0.0;
      x[i * NB + c] = on[c] ? v * y0[c] : 0.0;
    }
  }
}

// Pass-two step records (k_p2_coefs per column) for steps 1 .. kmax-1 from the device-held
// steps_c: active = j < steps_c, nflush = p2_flush(j, steps_c - 1).
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp2_coefs(BatchDev B, int kmax) {
  const int j = blockIdx.x * kTPB + threadIdx.x;
  if (j < 1 || j >= kmax) return;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const int steps = B.flags[8 * c + 2];
    const bool active = j < steps;
    const double* al = B.alphas + (size_t)c * B.kcap;
    const double* be = B.betas + (size_t)c * B.kcap;
    const double* y = B.y + (size_t)c * B.kcap;
    double* r = B.p2c + 8 * ((size_t)j * NB + c);
    r[0] = j >= 2 ? be[j - 2] : 0.0;
    r[1] = al[j - 1];
    r[2] = 1.0 / be[j - 1];
    r[3] = y[j];
    r[4] = y[j - 1];
    r[5] = j >= 2 ? y[j - 2] : 0.0;
    r[6] = active ? 1.0 : 0.0;
    r[7] = active ? (double)bp2_flush(j, steps - 1) : 0.0;
  }
}

// Pass two, step j (k_p2_spmv per column): regenerate v_{j+1}, accumulate x.
template <int NB, int FMT>
__global__ __launch_bounds__(kTPB) void k_bp2_spmv(CsrDev A, BatchDev B,
                                                   const double* __restrict__ v_cur,
                                                   const double* __restrict__ v_prev,
                                                   double* __restrict__ v_next,
                                                   double* __restrict__ x, int j) {
  extern __shared__ double lds[];
  BEpiPass2<NB> epi;
  epi.v_cur = v_cur;
  epi.v_prev = (j >= 2) ? v_prev : v_cur;
  epi.has_prev = j >= 2;
  epi.v_next = v_next;
  epi.x = x;
  const double* rec = B.p2c + 8 * (size_t)j * NB;
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int f = 0; f < 8; ++f) epi.rec[c][f] = rec[8 * c + f];
  epi.set_masks();
  auto unit = [](double (&sc)[NB]) -> bool {
#pragma unroll
    for (int c = 0; c < NB; ++c) sc[c] = 1.0;
    return true;
  };
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  b_spmv_block<NB, FMT>(A, B, v_cur, unit, epi, acc, lds);
}

namespace launch {

hipError_t bp2_init(int nb, const CsrDev& A, const BatchDev& B, const double* b, double* v1,
                    double* x, hipStream_t s) {
  if (A.n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp2_init<NB>, dim3(elem_grid(A.n)), dim3(kTPB), 0, s, A.n,
                                       B, b, v1, x));
  return hipGetLastError();
}
hipError_t bp2_coefs(int nb, const BatchDev& B, int kmax, hipStream_t s) {
  if (kmax <= 1) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp2_coefs<NB>, dim3((kmax + kTPB - 1) / kTPB), dim3(kTPB),
                                       0, s, B, kmax));
  return hipGetLastError();
}
hipError_t bp2_spmv(int nb, const CsrDev& A, const BatchDev& B, const double* v_cur,
                    const double* v_prev, double* v_next, double* x, int j, hipStream_t s) {
  if (spmv_grid(A) <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, return dispatch_fmt(
                        batch_fmt_of(A),
                        [&](auto F) {
                          hipLaunchKernelGGL((k_bp2_spmv<NB, decltype(F)::value>),
                                             dim3(spmv_grid(A)), dim3(kTPB), batch_lds_bytes(A), s,
                                             A, B, v_cur, v_prev, v_next, x, j);
                        },
                        std::make_integer_sequence<int, kBFmtEnd>{}));
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
