// tpl_k_p1_stol.hip — the kernels of the shifted inverse solve that stops each shift at a
// residual tolerance (tpl_lanczos_two_pass_shifted_inv_tol): (A + sigma_s I)^{-1} b for m
// shifts over the one Krylov space of A, whose tridiagonal for shift s is T_k + sigma_s I.
//   k_p1_axpy_stol    the pass-one AXPY step whose elimination workgroup runs one lane per
//                     shift: lane s eliminates T_k + sigma_s I, keeps shift s's residual
//                     history and records its own stop; the pass stops when every lane has
//   k_p1_stol_fin     one wave between pass one and k_ftk_inv_shifts: what no later step
//                     launch is left to do (k_p1_tol_fin's cases, per lane)
//   k_ftk_inv_shifts  one workgroup per shift: k_ftk_inv's body on shift s's rows, cut at
//                     that shift's own step count m*_s
//   k_p2_xacc_cut     k_p2_xacc with a per-column cut: term t of column c only where
//                     t < m*_c
// Every entry of a shifted tridiagonal is alphas[j] + sigma_s, one IEEE addition, here as on
// the host (tpl_solvers.cpp shifted_col); nothing else ever forms it.
//
// Shared (tpl_kstop.h), written once for this unit and the batch solve's
// (tpl_k_batch_stol.hip): the flag words and rule of the stop, the wave's vote, the
// elimination lane (stol_elim_wave), the fin wave (stol_fin_wave), and div_rn with its range
// test, which k_ftk_inv (tpl_kernels.hip) takes from there too.
// Still repeated: k_p1_axpy_stol's element part is k_p1_axpy_tol's text (tpl_k_p1_tol.hip),
// which repeats k_p1_axpy's (tpl_kernels.hip), for the reason given there: one function
// inlined into both moves instructions of the existing instances. The additions are marked
// "stol:". A change to k_p1_axpy's element part belongs here too. k_ftk_inv_shifts repeats
// k_ftk_inv's text: with only the back substitution as one function inlined into both, 106
// lines of k_ftk_inv's assembly changed, and tpl_kernels.hip's bytes are the ones the
// committed headline profile is tied to.
#include "../../include/tpl.h"
#include "tpl_klaunch.h"
#include "tpl_klu.h"
#include "tpl_kstop.h"

namespace tpl {

// k_p1_axpy_tol with m lanes in the elimination workgroup's first wave: lane s eliminates
// T_k + sig[s] I and keeps shift s's history and stop (stol_elim_wave, tpl_kstop.h). Once
// flags[kFlagHit] holds M = max m*_s the element blocks stop the pass as k_p1_axpy_tol's do.
template <int NP>
__global__ __launch_bounds__(kTPB) void k_p1_axpy_stol(P1AxpyArgs a, launch::ShiftTol t) {
  __shared__ double red[4];
  struct {
    int64_t E, n, norm_n; int NA_r, G2;
  } A{a.E, a.n, a.norm_n, a.NA_r, a.G2};
  struct {
    const double* Pa_r; int32_t* flags; double* norms; double* alphas; double* Pb;
  } S{a.Pa_r, a.flags, a.norms, a.alphas, a.Pb};
  const double* __restrict__ W = a.W;
  const double* __restrict__ r_cur = a.r_cur;
  double* __restrict__ r_next = a.r_next;
  const int j = a.j, k = a.k, elim_block = a.elim_block;
  asm volatile("" ::"s"(A.E), "s"(A.n), "s"(A.norm_n), "s"(A.NA_r), "s"(A.G2), "s"(S.Pa_r),
               "s"(S.flags), "s"(S.norms), "s"(S.alphas), "s"(S.Pb));
  asm volatile("" ::"s"(W), "s"(r_cur), "s"(r_next), "s"(j), "s"(k), "s"(elim_block));
  if ((int)blockIdx.x == elim_block) {
    if (threadIdx.x >= 64 || j < 3) return;  // stol: the first wave, one lane per shift
    stol_elim_wave(t, threadIdx.x, j, S.flags, S.alphas, a.betas);
    return;
  }
  const int rb = elem_block(A.G2, blockIdx.x);
  if (rb < 0) return;
  const int stop = S.flags[0];
  const int hit = S.flags[kFlagHit];  // stol: M; the stop flag's 32-byte line
  const double normj = S.norms[j - 1];
  __builtin_amdgcn_sched_barrier(0);
  PartialRegs<NP> pr;
  const int na_ = A.NA_r;
  load_partials(S.Pa_r, na_, pr);
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  constexpr int kAxPairs = 4;
  const int64_t i00 = beg + 2 * threadIdx.x;
  double2 w0[kAxPairs], rc0[kAxPairs];
#pragma unroll
  for (int q = 0; q < kAxPairs; ++q) {
    const int64_t i0 = i00 + (int64_t)q * 2 * kTPB;
    const int64_t ic = i0 < end ? i0 : beg;
    w0[q] = *reinterpret_cast<const double2*>(W + ic);
    rc0[q] = *reinterpret_cast<const double2*>(r_cur + ic);
  }
  __builtin_amdgcn_sched_barrier(0);
  double invN = 1.0 / normj;
  keep(invN);
  __builtin_amdgcn_sched_barrier(0);
  const double alpha = finish_partials(S.Pa_r, na_, pr, red);
  // ahead of the stop test, so that a breakdown in the step after the hit keeps M
  if (hit_before(hit, j)) {
    if (rb == 0 && threadIdx.x == 0) {
      S.flags[0] = 1;
      S.flags[2] = hit;
    }
    return;
  }
  if (stop) return;
  if (rb == 0 && threadIdx.x == 0) {
    S.alphas[j - 1] = alpha;
    S.flags[2] = j;
  }
  if (j == k) return; // beta_k is never used
  double acc = 0.0;
  auto step = [&](int64_t i0, double2 w, double2 rc) {
    double2 r;
    r.x = w.x - alpha * (rc.x * invN);
    r.y = w.y - alpha * (rc.y * invN);
    if (i0 + 1 < end) {
      typedef double d2v __attribute__((ext_vector_type(2)));
      d2v rv = {r.x, r.y};
      __builtin_nontemporal_store(rv, reinterpret_cast<d2v*>(r_next + i0));
    } else {
      __builtin_nontemporal_store(r.x, r_next + i0);
    }
    acc = i0 < A.norm_n ? fma(r.x, r.x, acc) : acc;
    acc = i0 + 1 < end && i0 + 1 < A.norm_n ? fma(r.y, r.y, acc) : acc;
  };
#pragma unroll
  for (int q = 0; q < kAxPairs; ++q) {
    const int64_t i0 = i00 + (int64_t)q * 2 * kTPB;
    if (i0 < end) step(i0, w0[q], rc0[q]);
  }
  for (int64_t i0 = i00 + (int64_t)kAxPairs * 2 * kTPB; i0 < end; i0 += 2 * kTPB) // E > 2048
    step(i0, *reinterpret_cast<const double2*>(W + i0),
         *reinterpret_cast<const double2*>(r_cur + i0));
  const double p = block_sum_tail(acc, red);
  if (threadIdx.x == 0) S.Pb[rb] = p;
}

// After the last step launch, one wave: stol_fin_wave (tpl_kstop.h) unless b was zero.
__global__ void k_p1_stol_fin(DevState S, launch::ShiftTol t) {
  if (blockIdx.x != 0 || threadIdx.x >= 64 || S.flags[1]) return;
  stol_fin_wave(t, threadIdx.x, S.flags, S.alphas, S.betas);
}

// Workgroup s: y_s = (T_n + sig[s] I)^{-1} e_1 with n = m*_s — t.hits[s], or steps_taken for
// a shift that never stopped — bit for bit tpl_ftk_inv on (alphas[0..n) + sig[s],
// betas[0..n-1)): k_ftk_inv's body (tpl_kernels.hip: its comments hold) on shift s's rows of
// t.lu and its running row in t.st. The rows lane s eliminated during pass one are the first
// min(flags[5], n - 1): a lane that stopped at m* had done m* - 1 rows (one, which a single
// step does not use, when m* = 1), one that never stopped all of flags[5]. Column s of Y
// (columns ldy apart) gets y_s, times ||b|| when `scale`; cs[s] gets n (0 after a zero b or
// no step: no term of that column is live in k_p2_xacc_cut). Dynamic LDS: 11 k doubles.
__global__ __launch_bounds__(kTPB) void k_ftk_inv_shifts(DevState S, launch::ShiftTol t,
                                                         double* __restrict__ Yout, int ldy,
                                                         int32_t* __restrict__ cs, int scale) {
  extern __shared__ double sh[];
  __shared__ double last[3];
  const int s = blockIdx.x, m = t.m;
  const int own = t.hits[s];
  const int n = S.flags[1] ? 0 : (own ? own : S.flags[2]);
  if (threadIdx.x == 0) cs[s] = n < 1 ? 0 : n;
  if (n < 1) return;
  const size_t am = (size_t)t.kcap * (size_t)m;
  const double sg = t.sig[s];
  const int done = min(S.flags[5], max(n - 1, 0));  // rows eliminated during pass one
  double* D = sh;
  double* DU = sh + n;
  double* DU2 = sh + 2 * n;
  double* B = sh + 3 * n;
  double* R = sh + 4 * n;   // reciprocals of the pivots
  double* al = sh + 5 * n;  // alpha + sigma, beta of the rows still to eliminate
  double* be = sh + 6 * n;
  for (int i = threadIdx.x; i < n; i += kTPB) {
    if (i < done) {
      const size_t e = (size_t)i * m + s;
      D[i] = t.lu[e];
      DU[i] = t.lu[am + e];
      DU2[i] = t.lu[2 * am + e];
      B[i] = t.lu[3 * am + e];
    }
    al[i] = S.alphas[i] + sg;
    be[i] = i + 1 < n ? S.betas[i] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    LuRow cur = done == 0 ? LuRow{al[0], n > 1 ? be[0] : 0.0, 1.0}
                          : LuRow{t.st[s], t.st[m + s], t.st[2 * m + s]};
    for (int i = done; i + 1 < n; ++i)
      lu_row(i, i + 2 < n, be[i], al[i + 1], i + 2 < n ? be[i + 1] : 0.0, cur, D, DU, DU2, B);
    last[0] = cur.d;
    last[1] = cur.b;
  }
  __syncthreads();
  double* P = sh + ((7 * n + 1) & ~1);
  bool pbad = false;
  for (int i = threadIdx.x; i + 1 < n; i += kTPB) {
    const double d = D[i], r = 1.0 / d;
    R[i] = r;
    typedef double d2v __attribute__((ext_vector_type(2)));
    reinterpret_cast<d2v*>(P)[2 * i] = d2v{B[i], DU[i]};
    reinterpret_cast<d2v*>(P)[2 * i + 1] = d2v{DU2[i], d};
    pbad = pbad || !(exp_in_range(d) && exp_in_range(r));
  }
  const bool any_pbad = __syncthreads_or(pbad);
  double* Y = D;   // x' of every row (D is read only through P from here on)
  double* T = DU;  // the numerator t of every row, for the deferred range test
  if (threadIdx.x == 0) {
    const double xl = last[1] / last[0];  // b[n-1] / d[n-1]
    Y[n - 1] = xl;
    if (n >= 2) {
      double x1 = xl, x0;
      {
        const double tn = B[n - 2] - DU[n - 2] * x1;
        x0 = div_rn(tn, D[n - 2], R[n - 2], !any_pbad);
        Y[n - 2] = x0;
        T[n - 2] = 0.0;  // row n - 2 took div_rn's own checks
      }
      typedef double d2v __attribute__((ext_vector_type(2)));
      const d2v* PR = reinterpret_cast<const d2v*>(P);
      d2v p0 = {0.0, 0.0}, p1 = {0.0, 1.0};
      double r_n = 1.0;
      if (n >= 3) {
        p0 = PR[2 * (n - 3)]; p1 = PR[2 * (n - 3) + 1]; r_n = R[n - 3];
      }
      for (int ii = n - 3; ii >= 0; --ii) {
        const double bi = p0.x, dui = p0.y, du2i = p1.x, di = p1.y, ri = r_n;
        if (ii > 0) {
          p0 = PR[2 * (ii - 1)]; p1 = PR[2 * (ii - 1) + 1]; r_n = R[ii - 1];
        }
        const double tn = bi - dui * x0 - du2i * x1;
        const double q0 = tn * ri;
        const double qm = fma(fma(-di, q0, tn), ri, q0);
        const double xi = tn == 0.0 ? q0 : qm;  // +-0: q0 carries the quotient's sign
        Y[ii] = xi;
        T[ii] = tn;
        x1 = x0;
        x0 = xi;
      }
    }
  }
  __syncthreads();
  // deferred: a row whose numerator or quotient left div_rn's range (t == 0 is exact)
  bool bad = any_pbad && n >= 2;
  for (int i = threadIdx.x; i + 2 < n; i += kTPB) {
    const double tn = T[i];
    bad = bad || !(tn == 0.0 || (exp_in_range(tn) && exp_in_range(Y[i])));
  }
  if (__syncthreads_or(bad)) {
    // an operand outside div_rn's range (singular or badly scaled T_n): IEEE divisions
    if (threadIdx.x == 0) {
      const double* PD = P;
      double x1 = Y[n - 1];
      double x0 = (PD[4 * (n - 2)] - PD[4 * (n - 2) + 1] * x1) / PD[4 * (n - 2) + 3];
      Y[n - 2] = x0;
      for (int ii = n - 3; ii >= 0; --ii) {
        const double xi = (PD[4 * ii] - PD[4 * ii + 1] * x0 - PD[4 * ii + 2] * x1) / PD[4 * ii + 3];
        Y[ii] = xi;
        x1 = x0;
        x0 = xi;
      }
    }
    __syncthreads();
  }
  const double bnorm = scale ? S.norms[0] : 1.0;
  double* yc = Yout + (size_t)s * (size_t)ldy;
  for (int i = threadIdx.x; i < n; i += kTPB) yc[i] = Y[i] * bnorm;
}

// k_p2_xacc (tpl_k_multi.hip) with a per-column cut: after step j, of the last nflush
// (1..3) terms t = j - nflush + 1 .. j, oldest first, column c gets X_c += y_c[t] v_{t+1}
// only where t < cs[c] — the terms of tpl_lanczos_pass_two at steps = cs[c], in its order,
// each product rounded on its own, so column c holds that solve's bits however the terms
// are grouped into launches. A skipped term is a predicate, never a product with zero
// (which would turn -0 into +0 and spread a non-finite v). A column with no live term is
// neither loaded nor stored; a launch whose columns have none returns at once. cs is read
// from the device: the counts may be known there only (k_ftk_inv_shifts). Entries of Y at
// or past cs[c] are loaded and never used.
template <int M>
__global__ __launch_bounds__(kTPB) void k_p2_xacc_cut(int64_t n, int64_t E, int G2,
                                                      const double* __restrict__ Y, int ldy,
                                                      int j, int nflush,
                                                      const int32_t* __restrict__ cs,
                                                      const double* __restrict__ vp,
                                                      const double* __restrict__ vc,
                                                      const double* __restrict__ vn,
                                                      double* __restrict__ X, int64_t ldx) {
  const int rb = elem_block(G2, blockIdx.x);
  if (rb < 0) return;
  const int first = j - nflush + 1;  // the oldest term of this flush
  int lim[M];
  bool any = false;
#pragma unroll
  for (int c = 0; c < M; ++c) {
    lim[c] = cs[c];
    any = any || first < lim[c];
  }
  if (!any) return;
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
#pragma unroll
    for (int c = 0; c < M; ++c) {
      if (!(first < lim[c])) continue;
      double xv = X[(size_t)c * ldx + i];
      if (nflush >= 3 && j - 2 < lim[c]) xv = xv + y2[c] * p;
      if (nflush >= 2 && j - 1 < lim[c]) xv = xv + y1[c] * c0;
      if (j < lim[c]) xv = xv + y0[c] * nx;
      st_out(X + (size_t)c * ldx + i, xv);
    }
  }
}

} // namespace tpl

// ------------------------------------------------------------ host launchers
namespace tpl {
namespace launch {

hipError_t p1_axpy_stol(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                        double* r_next, int j, int k, const ShiftTol& t, hipStream_t s) {
  if (t.m < 1 || t.m > 64 || t.kcap < k) return hipErrorInvalidValue;
  const P1AxpyArgs a = p1_axpy_args(A, S, W, r_cur, r_next, j, k, g2_grid(A), nullptr);
  const dim3 g(g2_grid(A) + 1), b(kTPB);
  TPL_NP_SWITCH(A.NA_r, hipLaunchKernelGGL(k_p1_axpy_stol<NP>, g, b, 0, s, a, t));
  return hipGetLastError();
}
hipError_t p1_stol_fin(const DevState& S, const ShiftTol& t, hipStream_t s) {
  if (t.m < 1 || t.m > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_p1_stol_fin, dim3(1), dim3(64), 0, s, S, t);
  return hipGetLastError();
}
hipError_t ftk_inv_shifts(const DevState& S, int k, const ShiftTol& t, double* Y, int ldy,
                          int32_t* cs, int scale, hipStream_t s) {
  if (t.m < 1 || t.m > TPL_MULTI_MAX || k < 1 || k > ldy || k > t.kcap || k > S.kcap)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ftk_inv_shifts, dim3(t.m), dim3(kTPB), (size_t)11 * k * sizeof(double), s,
                     S, t, Y, ldy, cs, scale);
  return hipGetLastError();
}

template <int M>
static void xacc_cut_launch(const CsrDev& A, const double* Y, int ldy, int j, int nflush,
                            const int32_t* cs, const double* vp, const double* vc,
                            const double* vn, double* X, int64_t ldx, hipStream_t s) {
  hipLaunchKernelGGL(k_p2_xacc_cut<M>, dim3(g2_grid(A)), dim3(kTPB), 0, s, A.n, A.E, A.G2, Y,
                     ldy, j, nflush, cs, vp, vc, vn, X, ldx);
}

hipError_t p2_xacc_cut(const CsrDev& A, const double* Y, int ldy, int j, int nflush,
                       const int32_t* cs, const double* vp, const double* vc, const double* vn,
                       double* X, int64_t ldx, int m, hipStream_t s) {
  if (nflush < 1 || nflush > 3 || j < nflush || j >= ldy) return hipErrorInvalidValue;
  switch (m) {
    case 1: xacc_cut_launch<1>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 2: xacc_cut_launch<2>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 3: xacc_cut_launch<3>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 4: xacc_cut_launch<4>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 5: xacc_cut_launch<5>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 6: xacc_cut_launch<6>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 7: xacc_cut_launch<7>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    case 8: xacc_cut_launch<8>(A, Y, ldy, j, nflush, cs, vp, vc, vn, X, ldx, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
