// tpl_k_batch_stol.hip — the kernels of the batch shifted inverse solve that stops every
// (column, shift) at a residual tolerance (tpl_lanczos_two_pass_batch_shifted_inv_tol):
// (A + sigma_i I)^{-1} b_c for s right-hand sides in lock-step groups and m shifts, the
// tridiagonal of (c, i) being column c's T_k + sigma_i I.
//   k_bp1_axpy_stol  the batch pass-one AXPY step with one elimination workgroup after the
//                    element grid: wave c serves column c, lane i of it shift i, each doing
//                    what lane i of k_p1_axpy_stol (tpl_k_p1_stol.hip) does on column c's
//                    alphas and betas and its own ShiftTol block; column c stops when every
//                    lane of its wave has
//   k_bp1_stol_fin   one wave per column between pass one and the y's: k_p1_stol_fin's two
//                    cases per lane
//   k_bp2_xacc_cut   k_bp2_xacc (tpl_k_batch_multi.hip) with a device-resident cut per
//                    (function, column): term t of result (f, c) only where t < cs[(f, c)]
// The y of every (c, i) is k_ftk_inv_shifts as it stands, one launch per column on column
// c's view of the group state (tpl_passes.cpp).
//
// Words 5, 6 and 7 of a column's eight flags (BatchDev::flags + 8 c) are the stop's
// kFlagDone, kFlagHit and kFlagRes (tpl_kstop.h).
//
// Shared (tpl_kstop.h) with the one-column solve (tpl_k_p1_stol.hip): those words, the rule
// and the vote of the stop, the elimination lane (stol_elim_wave) and the fin wave
// (stol_fin_wave); a column's view of the group's per-shift state is
// launch::BatchShiftTol::col, on the host and here.
// Still repeated: k_bp1_axpy_stol's element part is k_bp1_axpy's text (tpl_k_batch_p1.hip),
// as k_p1_axpy_tol's is k_p1_axpy's (tpl_k_p1_tol.hip gives the reason): the existing
// instances must keep their instructions. The additions are marked "stol:". A change to
// k_bp1_axpy's element part belongs here too.
#include "../../include/tpl.h"
#include "tpl_kbatch.h"
#include "tpl_kstop.h"
#include "tpl_launch.h"

namespace tpl {

// k_bp1_axpy with NB waves of elimination lanes in one more workgroup (blockIdx.x ==
// elim_block, the block after the element grid). Wave c runs stol_elim_wave on column c's
// alphas, betas, flags and block of the per-shift state. When every lane of wave c has
// stopped, its lane 0 writes M_c = max_i m*_{c,i} into column c's kFlagHit; from launch
// max(M_c + 1, 3) + 1 on the element blocks count column c as stopped (flags[8c] = 1,
// flags[8c + 2] = M_c) and store nothing for it. No LDS and no barrier between the waves: a
// column's lanes read and write that column's state only.
template <int NB>
__global__ __launch_bounds__(kTPB) void k_bp1_axpy_stol(CsrDev A, BatchDev B,
                                                        const double* __restrict__ W,
                                                        const double* __restrict__ r_cur,
                                                        double* __restrict__ r_next, int j, int k,
                                                        int elim_block, launch::BatchShiftTol bt) {
  __shared__ double red[4 * NB];
  if ((int)blockIdx.x == elim_block) {  // stol: the elimination workgroup
    const int c = threadIdx.x >> 6;
    if (c >= NB || j < 3) return;
    stol_elim_wave(bt.col(c), threadIdx.x & 63, j, B.flags + 8 * c,
                   B.alphas + (size_t)c * B.kcap, B.betas + (size_t)c * B.kcap);
    return;
  }
  const int rb = elem_block(A.G2, blockIdx.x);
  if (rb < 0) return;
  int stop[NB], hit[NB];
  bool on[NB];
  double normj[NB];
  bool any = false, all = true;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    stop[c] = B.flags[8 * c];
    hit[c] = B.flags[8 * c + kFlagHit];  // stol: M_c; the stop flag's 32-byte line
    normj[c] = B.norms[(size_t)c * (B.kcap + 1) + j - 1];
  }
  // stol: ahead of the stop test, so that a breakdown in the step after the hit keeps M_c
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    if (hit_before(hit[c], j)) {
      if (rb == 0 && threadIdx.x == 0) {
        B.flags[8 * c] = 1;
        B.flags[8 * c + 2] = hit[c];
      }
      stop[c] = 1;
    }
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

// After the last step launch, one wave per column: stol_fin_wave (tpl_kstop.h) on column c
// unless its b was zero; steps_c becomes M_c there.
template <int NB>
__global__ void k_bp1_stol_fin(BatchDev B, launch::BatchShiftTol bt) {
  const int c = threadIdx.x >> 6;
  if (blockIdx.x != 0 || c >= NB) return;
  int32_t* fl = B.flags + 8 * c;
  if (fl[1]) return;
  stol_fin_wave(bt.col(c), threadIdx.x & 63, fl, B.alphas + (size_t)c * B.kcap,
                B.betas + (size_t)c * B.kcap);
}

// k_bp2_xacc with a cut per (function, column): after step j, of the last nflush (1..3)
// terms t = j - nflush + 1 .. j, oldest first, result (f, c) gets X_f(c) += y_{c,f}[t] v_{t+1}
// only where t < cs[c cld + f] — the terms of tpl_lanczos_pass_two at that many steps, in its
// order, each product rounded on its own, however the terms are grouped into launches
// (k_p2_xacc_cut's rules: a skipped term is a predicate, never a product with zero; a (f, c)
// with no live term is neither loaded nor stored; a launch with none returns at once). cs is
// read from the device: the counts may be known there only. Entries of Y at or past a cut
// and ring entries of a column past its steps_c are loaded and never used.
template <int NB, int M>
__global__ __launch_bounds__(kTPB) void k_bp2_xacc_cut(int64_t n, int64_t E, int G2,
                                                       const int32_t* __restrict__ cs, int cld,
                                                       const double* __restrict__ Y, int kcap,
                                                       int j, int nflush,
                                                       const double* __restrict__ vp,
                                                       const double* __restrict__ vc,
                                                       const double* __restrict__ vn,
                                                       double* __restrict__ X, int64_t xstride) {
  __shared__ double co[3 * M * NB];  // [q][f][c]: y_{c,f}[j - q]
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  const int first = j - nflush + 1;  // the oldest term of this flush
  int lim[M][NB];
  bool live[M][NB], all_live[M], any_live[M];
  bool any = false;
#pragma unroll
  for (int f = 0; f < M; ++f) {
    all_live[f] = true;
    any_live[f] = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      lim[f][c] = cs[(size_t)c * cld + f];
      live[f][c] = first < lim[f][c];
      all_live[f] = all_live[f] && live[f][c];
      any_live[f] = any_live[f] || live[f][c];
    }
    any = any || any_live[f];
  }
  if (!any) return;
  if (threadIdx.x < 3 * M * NB) {
    const int q = threadIdx.x / (M * NB), fc = threadIdx.x % (M * NB);
    const int jq = j - q;  // clamped: read, never used
    co[threadIdx.x] = Y[(size_t)fc * kcap + (jq > 0 ? jq : 0)];
  }
  __syncthreads();
  const int64_t beg = (int64_t)rb * E;
  const int64_t end = beg + E < n ? beg + E : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const VecNB<NB> p = ld_nb<NB>(vp, i), c0 = ld_nb<NB>(vc, i), nx = ld_nb<NB>(vn, i);
#pragma unroll
    for (int f = 0; f < M; ++f) {
      if (!any_live[f]) continue;
      double* Xf = X + (size_t)f * xstride;
      double out[NB];
      if (all_live[f]) {
        const VecNB<NB> x = ld_nb<NB>(Xf, i);
#pragma unroll
        for (int c = 0; c < NB; ++c) out[c] = x.v[c];
      } else {
#pragma unroll
        for (int c = 0; c < NB; ++c) out[c] = live[f][c] ? Xf[i * NB + c] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        if (!live[f][c]) continue;
        double xv = out[c];
        if (nflush >= 3 && j - 2 < lim[f][c]) xv = xv + co[(2 * M + f) * NB + c] * p.v[c];
        if (nflush >= 2 && j - 1 < lim[f][c]) xv = xv + co[(M + f) * NB + c] * c0.v[c];
        if (j < lim[f][c]) xv = xv + co[f * NB + c] * nx.v[c];
        out[c] = xv;
      }
      st_nb<NB>(Xf, i, out, live[f], all_live[f]);
    }
  }
}

} // namespace tpl

// ------------------------------------------------------------ host launchers
namespace tpl {
namespace launch {

static bool bstol_ok(const BatchShiftTol& t, const BatchDev& B, int k) {
  return t.t0.m >= 1 && t.t0.m <= 64 && t.t0.kcap >= k && t.t0.kcap == B.kcap;
}
hipError_t bp1_axpy_stol(int nb, const CsrDev& A, const BatchDev& B, const double* W,
                         const double* r_cur, double* r_next, int j, int k,
                         const BatchShiftTol& t, hipStream_t s) {
  if (!bstol_ok(t, B, k)) return hipErrorInvalidValue;
  const int elim_block = g2_grid(A);  // the block after the element grid, padding included
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp1_axpy_stol<NB>, dim3(g2_grid(A) + 1), dim3(kTPB), 0, s,
                                       A, B, W, r_cur, r_next, j, k, elim_block, t));
  return hipGetLastError();
}
hipError_t bp1_stol_fin(int nb, const BatchDev& B, const BatchShiftTol& t, hipStream_t s) {
  if (!bstol_ok(t, B, 1)) return hipErrorInvalidValue;
  TPL_NB_SWITCH(nb, hipLaunchKernelGGL(k_bp1_stol_fin<NB>, dim3(1), dim3(64 * NB), 0, s, B, t));
  return hipGetLastError();
}

template <int NB, int M>
static void bxacc_cut_launch(const CsrDev& A, const BatchDev& B, const int32_t* cs, int cld,
                             const double* Y, int j, int nflush, const double* vp,
                             const double* vc, const double* vn, double* X, int64_t xstride,
                             hipStream_t s) {
  hipLaunchKernelGGL((k_bp2_xacc_cut<NB, M>), dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n, A.E, A.G2,
                     cs, cld, Y, B.kcap, j, nflush, vp, vc, vn, X, xstride);
}
template <int NB>
static void bxacc_cut_funcs(int m, const CsrDev& A, const BatchDev& B, const int32_t* cs, int cld,
                            const double* Y, int j, int nflush, const double* vp,
                            const double* vc, const double* vn, double* X, int64_t xstride,
                            hipStream_t s) {
  static_assert(kBatchMultiFuncs == 4, "one instance per function count");
  switch (m) {
    case 1: bxacc_cut_launch<NB, 1>(A, B, cs, cld, Y, j, nflush, vp, vc, vn, X, xstride, s); break;
    case 2: bxacc_cut_launch<NB, 2>(A, B, cs, cld, Y, j, nflush, vp, vc, vn, X, xstride, s); break;
    case 3: bxacc_cut_launch<NB, 3>(A, B, cs, cld, Y, j, nflush, vp, vc, vn, X, xstride, s); break;
    default: bxacc_cut_launch<NB, 4>(A, B, cs, cld, Y, j, nflush, vp, vc, vn, X, xstride, s); break;
  }
}
hipError_t bp2_xacc_cut(int nb, const CsrDev& A, const BatchDev& B, const int32_t* cs, int cld,
                        const double* Y, int j, int nflush, const double* vp, const double* vc,
                        const double* vn, double* X, int64_t xstride, int m, hipStream_t s) {
  if (nflush < 1 || nflush > 3 || j < nflush || j >= B.kcap || m < 1 || m > kBatchMultiFuncs)
    return hipErrorInvalidValue;
  if (A.n <= 0) return hipGetLastError();
  TPL_NB_SWITCH(nb, bxacc_cut_funcs<NB>(m, A, B, cs, cld, Y, j, nflush, vp, vc, vn, X, xstride, s));
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
