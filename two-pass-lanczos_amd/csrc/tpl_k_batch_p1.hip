// tpl_k_batch_p1.hip — pass one of the lock-step batch solve (tpl_lanczos_two_pass_batch):
// the boundary kernels k_b_interleave / k_b_deinterleave and the batch siblings of
// k_p1_init, k_p1_spmv and k_p1_axpy for NB = 2 and NB = 4 columns per launch. Building
// blocks: tpl_kbatch.h. Map of the device sources: tpl_kernels.hip.
#include "tpl_kbatch.h"

namespace tpl {

// The boundary: permute (locality order) and interleave in one pass, so the caller's
// column-major B and X never need a second copy.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_b_interleave(int64_t n,
                                                       double* __restrict__ out,
                                                       const double* __restrict__ B,
                                                       const int32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    const int64_t src = idx ? idx[i] : i;
#pragma unroll
    for (int c = 0; c < NB; ++c) out[i * NB + c] = B[(int64_t)c * n + src];
  }
}
template <int NB>
__global__ __launch_bounds__(kTPB) void k_b_deinterleave(int64_t n,
                                                         double* __restrict__ X,
                                                         const double* __restrict__ in,
                                                         const int32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    const int64_t src = idx ? idx[i] : i;
#pragma unroll
    for (int c = 0; c < NB; ++c) X[(int64_t)c * n + i] = in[src * NB + c];
  }
}

// Pass-one prologue (k_p1_init per column): ||b_c||^2 partials; reset the flags.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp1_init(CsrDev A, BatchDev B,
                                                   const double* __restrict__ b) {
  __shared__ double red[4 * NB];
  if (blockIdx.x == 0 && threadIdx.x < 8 * NB)
    B.flags[threadIdx.x] = 0;
  const int rb = elem_block(A, blockIdx.x);
  if (rb < 0) return;
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  for (int64_t i0 = beg + 2 * threadIdx.x; i0 < end; i0 += 2 * kTPB) {
    const VecNB<NB> v0 = ld_nb<NB>(b, i0);
#pragma unroll
    for (int c = 0; c < NB; ++c) acc[c] = fma(v0.v[c], v0.v[c], acc[c]);
    if (i0 + 1 < end) {
      const VecNB<NB> v1 = ld_nb<NB>(b, i0 + 1);
#pragma unroll
      for (int c = 0; c < NB; ++c) acc[c] = fma(v1.v[c], v1.v[c], acc[c]);
    }
  }
  block_sum_nb<NB>(acc, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < NB; ++c) B.Pb[(size_t)c * B.g2_ld + rb] = acc[c];
}

// The pass-one step's SpMV (p1_spmv_body per column), step j >= 1: beta_{j-1} of every
// column from its norm partials (any count: the canonical partials() order, which is what
// k_p1_spmv and k_p1_spmv_wide both compute), the breakdown test per column, the SpMV
// gathering r_j * (1 / beta_{j-1}), w = y - beta_{j-1} v_{j-1}, the alpha partials.
// ycrow: the step's row of the group's long-row cache (BatchBufs::d_ycache), where the long
// rows' sums are kept for the same solve's pass two (k_bp2_cached), or nullptr.
template <int NB, int FMT>
__global__ __launch_bounds__(kTPB) void k_bp1_spmv(CsrDev A, BatchDev B,
                                                   const double* __restrict__ r_cur,
                                                   const double* __restrict__ r_prev,
                                                   double* __restrict__ W, int j,
                                                   double* __restrict__ ycrow) {
  __shared__ double red[4 * NB], redb[4 * NB];
  extern __shared__ double lds[];
  // the norm partials, the stop flags and beta_{j-2} ahead of the entries and gathers
  ColPartialRegs<NB, 1> pr;
  load_col_partials<NB, 1>(B.Pb, B.g2_ld, A.G2, pr);
  // beta_{j-2} of every column. NB = 2: loaded with the stop flags, ahead of the entries and
  // gathers. NB = 4: held across those loads the 8 SGPRs are what tipped the instance into
  // spilling SGPRs to VGPR lanes (up to 56 of them), so they are loaded at the start of the
  // prologue instead, ahead of the reduction that hides them (measured not slower: DESIGN §6.1)
  constexpr bool kLateNorms = NB > 2;
  double norm_prev[NB];
  auto load_norms = [&] {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      norm_prev[c] = (j >= 2) ? B.norms[(size_t)c * (B.kcap + 1) + j - 2] : 1.0;
  };
  if constexpr (!kLateNorms) load_norms();
  int stop0[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    stop0[c] = B.flags[8 * c];
  }
  BEpiPass1<NB> epi;
  epi.r_cur = r_cur;
  epi.r_prev = (j >= 2) ? r_prev : r_cur;
  epi.has_prev = j >= 2;
  epi.W = W;
  epi.Pa_long = B.Pa + A.n_chunks;
  epi.na_ld = B.na_ld;
  epi.ycrow = ycrow;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    epi.invN_cur[c] = epi.invN_prev[c] = epi.beta_sub[c] = 0.0;
  }
  epi.all_alive = false;
  epi.alive = 0u;
  auto scale_fn = [&](double (&sc)[NB]) -> bool {
    if constexpr (kLateNorms) load_norms();
    double sq[NB];
    finish_col_partials<NB, 1>(B.Pb, B.g2_ld, A.G2, pr, sq, redb);
    bool any = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      sc[c] = 0.0;
      if (stop0[c]) continue;
      epi.invN_prev[c] = (j >= 2) ? 1.0 / norm_prev[c] : 0.0;
      const double beta = sqrt(sq[c]);
      if (beta <= kBreakdownTol) {
        // j == 1: zero b_c; j > 1: breakdown, steps_c = j - 1, beta not pushed
        if (blockIdx.x == 0 && threadIdx.x == 0) {
          B.flags[8 * c] = 1;
          if (j == 1) B.flags[8 * c + 1] = 1;
        }
        continue;
      }
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        B.norms[(size_t)c * (B.kcap + 1) + j - 1] = beta;
        if (j >= 2) B.betas[(size_t)c * B.kcap + j - 2] = beta;
      }
      epi.invN_cur[c] = 1.0 / beta;
      epi.beta_sub[c] = (j >= 2) ? beta : 0.0;
      epi.alive |= 1u << c;
      sc[c] = epi.invN_cur[c];
      any = true;
    }
    epi.all_alive = epi.alive == (1u << NB) - 1u;
    return any;
  };
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  const int slot = b_spmv_block<NB, FMT>(A, B, r_cur, scale_fn, epi, acc, lds);
  if (slot < 0) return;  // uniform per workgroup
  block_sum_nb<NB>(acc, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (epi.is_alive(c)) st_out(B.Pa + (size_t)c * B.na_ld + slot, acc[c]);
}

// Pass one, step j (k_p1_axpy per column): alpha_j; r_{j+1} = w - alpha_j v_j; the
// ||r_{j+1}||^2 partials.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp1_axpy(CsrDev A, BatchDev B,
                                                   const double* __restrict__ W,
                                                   const double* __restrict__ r_cur,
                                                   double* __restrict__ r_next, int j, int k) {
  __shared__ double red[4 * NB];
  const int rb = elem_block(A.G2, blockIdx.x);
  if (rb < 0) return;
  int stop[NB];
  bool on[NB];
  double normj[NB];
  bool any = false, all = true;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    stop[c] = B.flags[8 * c];
    normj[c] = B.norms[(size_t)c * (B.kcap + 1) + j - 1];
    on[c] = !stop[c];
    any = any || on[c];
    all = all && on[c];
  }
  // the alpha partials first: their reduction waits for nothing else
  ColPartialRegs<NB, 4> pr;
  load_col_partials<NB, 4>(B.Pa, B.na_ld, A.NA, pr);
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  const int64_t i00 = beg + 2 * threadIdx.x;
  double alpha[NB];
  finish_col_partials<NB, 4>(B.Pa, B.na_ld, A.NA, pr, alpha, red);
  if (!any) return;  // every column stopped (uniform)
  if (rb == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (!stop[c]) {
        B.alphas[(size_t)c * B.kcap + j - 1] = alpha[c];
        B.flags[8 * c + 2] = j;
      }
  }
  if (j == k) return;  // beta_k is never used
  double invN[NB], acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    invN[c] = 1.0 / normj[c];
    acc[c] = 0.0;
  }
  auto step = [&](int64_t i0, const VecNB<NB>& w0, const VecNB<NB>& c0, const VecNB<NB>& w1,
                  const VecNB<NB>& c1) {
    const bool two = i0 + 1 < end;
    double rx[NB], ry[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      rx[c] = w0.v[c] - alpha[c] * (c0.v[c] * invN[c]);
      ry[c] = w1.v[c] - alpha[c] * (c1.v[c] * invN[c]);
      acc[c] = fma(rx[c], rx[c], acc[c]);
      acc[c] = two ? fma(ry[c], ry[c], acc[c]) : acc[c];
    }
    st_nb<NB>(r_next, i0, rx, on, all);
    if (two) st_nb<NB>(r_next, i0 + 1, ry, on, all);
  };
  // (rows preloaded ahead of the reduction, as k_p1_axpy's kAxPairs, measured slower here:
  // DESIGN.md §6.3)
  for (int64_t i0 = i00; i0 < end; i0 += 2 * kTPB) {
    const int64_t i1 = i0 + 1 < end ? i0 + 1 : i0;
    step(i0, ld_nb<NB>(W, i0), ld_nb<NB>(r_cur, i0), ld_nb<NB>(W, i1), ld_nb<NB>(r_cur, i1));
  }
  block_sum_nb<NB>(acc, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (!stop[c]) B.Pb[(size_t)c * B.g2_ld + rb] = acc[c];
}

namespace launch {

hipError_t b_interleave(int nb, int64_t n, double* out, const double* B,
                        const int32_t* idx, hipStream_t s) {
  if (n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_b_interleave<NB>, dim3(elem_grid(n)), dim3(kTPB), 0, s, n,
                                       out, B, idx));
  return hipGetLastError();
}
hipError_t b_deinterleave(int nb, int64_t n, double* X, const double* in,
                          const int32_t* idx, hipStream_t s) {
  if (n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_b_deinterleave<NB>, dim3(elem_grid(n)), dim3(kTPB), 0, s,
                                       n, X, in, idx));
  return hipGetLastError();
}
hipError_t bp1_init(int nb, const CsrDev& A, const BatchDev& B, const double* b, hipStream_t s) {
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp1_init<NB>, dim3(g2_grid(A)), dim3(kTPB), 0, s, A, B, b));
  return hipGetLastError();
}
hipError_t bp1_spmv(int nb, const CsrDev& A, const BatchDev& B, const double* r_cur,
                    const double* r_prev, double* W, int j, double* ycrow, hipStream_t s) {
  if (spmv_grid(A) <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, return dispatch_fmt(
                        batch_fmt_of(A),
                        [&](auto F) {
                          hipLaunchKernelGGL((k_bp1_spmv<NB, decltype(F)::value>),
                                             dim3(spmv_grid(A)), dim3(kTPB), batch_lds_bytes(A), s,
                                             A, B, r_cur, r_prev, W, j, ycrow);
                        },
                        std::make_integer_sequence<int, kBFmtEnd>{}));
  return hipGetLastError();
}
hipError_t bp1_axpy(int nb, const CsrDev& A, const BatchDev& B, const double* W,
                    const double* r_cur, double* r_next, int j, int k, hipStream_t s) {
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp1_axpy<NB>, dim3(g2_grid(A)), dim3(kTPB), 0, s, A, B, W,
                                       r_cur, r_next, j, k));
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
