// tpl_kexp.h — the body of the device exp(T) e_1, shared by k_ftk_exp (tpl_k_ftk_exp.hip:
// T = T_k), k_ftk_exp_times (tpl_k_ftk_exp_times.hip: T = t_i T_k, one workgroup per time)
// and k_ftk_exp_times_batch (tpl_k_ftk_exp_times_batch.hip: one workgroup per time and
// column of a batch group). Included only by those three units.
#pragma once
#include "tpl_klaunch.h"

namespace tpl {

// f(T_k) = exp(T_k) on the device: y = ||b|| exp(T_k) e_1 (src/bin/stability.rs:175-193
// forms Q exp(Lambda) Q^T e_1 from a dense EVD; the host built-in tpl_ftk_exp runs QL).
// A QL sweep is one long chain of dependent rotations (1.2 ms at k = 200 on the host, worse
// on one GPU lane), so the device evaluates the same function with a parallel method: the
// Chebyshev expansion of exp on an interval [a, b] holding the spectrum,
//   exp(c + r x) = e^c (I_0(r) + 2 sum_m I_m(r) T_m(x)),  c = (a+b)/2, r = (b-a)/2,
// applied to e_1 with x = (T - c)/r by Clenshaw's recurrence (every row of the tridiagonal
// product on its own thread, one LDS exchange and barrier per term), the modified Bessel
// coefficients generated alongside by Miller's backward recurrence I_{m-1} = I_{m+1} +
// (2m/r) I_m and normalised by e^r = I_0 + 2 sum I_m — no coefficient table, no EVD, and
// no clusters to resolve (eigenvectors never appear). [a, b]: one round of 512-shift Sturm
// multisection of the Gershgorin interval (a count is exact for a matrix within a few ulps
// of T, so the bracket holds the spectrum up to the added margin; the bracket's excess,
// at most 1/513 of the Gershgorin width, only scales the error bound by its exponential). Accuracy is the
// EVD's class: the error is a small multiple of eps * exp(lambda_max) (the coefficients sum
// to e^b), against the tolerance the host QL itself meets; the terms run until the
// coefficients fall below 1e-22 of e^b (Debye asymptotics of I_m(r)). Falls back to the host
// (y = 0 and the caller's hand-back mark: k_ftk_exp's flags[4] = 1) when T is not finite, when the expansion needs more than
// kExpMaxTerms terms (|lambda_max - lambda_min| above ~2e4), or when ||y|| < 1e-3 e^b
// (the absolute error bound would not be small against ||y||). Dynamic LDS: 4 kcap + 4 doubles
// and 256 ints.
constexpr int kExpRows = 8;          // rows per thread: n <= 2048 (the LDS bound is lower)
constexpr int kExpMaxTerms = 16384;
constexpr double kExpMinRatio = 1e-3;  // ||exp(T - b I) e_1|| below this: host (see the end)
constexpr int kExpShifts = 2 * kTPB;   // Sturm shifts per end of the spectrum (one round)
// Reciprocal for the Sturm pivots: v_rcp_f64 and one Newton step (a Sturm count tolerates
// the last-bit difference from a division; the bracket carries a margin far above it)
__device__ __forceinline__ double rcp_nr(double q) {
  const double r = __builtin_amdgcn_rcp(q);
  return fma(fma(-q, r, 1.0), r, r);
}
// ln(e^-r I_m(r)), uniform asymptotic (Debye) form; used only to size the expansion
__device__ __forceinline__ double log_scaled_bessel_i(double m, double r) {
  const double s = sqrt(m * m + r * r);
  return -r + s - m * asinh(m / r) - 0.9189385332046727 - 0.25 * log(s * s);
}
// One workgroup of kTPB threads: y = ||b|| exp(T) e_1 (||b|| = S.norms[0] when `scale`) for
// the n = S.flags[2] rows of the tridiagonal `src` hands out — src.alpha(i), src.beta(i):
// the same value at every call, each use reads it through them — into dst.y(i, v). Handing
// the case back is dst.hand_back() after a zero y; dst.kept() marks a y that stands (both
// from thread 0). Returns at once after a zero b (S.flags[1]) or no step.
template <class Src, class Dst>
__device__ __forceinline__ void ftk_exp_body(DevState S, int scale, Src src, Dst dst) {
  extern __shared__ double sh[];
  __shared__ double red[2][kTPB];
  __shared__ int cnt[2 * kExpShifts];  // Sturm counts: [min end | max end]
  __shared__ int first[2];
  TPL_MARK(0);
  const int n = S.flags[2];
  if (S.flags[1] || n < 1) return;
  const int t = threadIdx.x;
  double* al = sh;            // alpha (n)
  double* b2 = sh + n;        // beta^2 (n - 1), b2[n-1] = 0
  double* buf0 = sh + 2 * n;  // Clenshaw exchange buffers: row i at [i + 1], zeros at both ends
  double* buf1 = buf0 + (n + 2);
  const double bnorm = scale ? S.norms[0] : 1.0;
  // this thread's rows: alpha, the betas on both sides (registers for the whole expansion)
  const int R = (n + kTPB - 1) / kTPB;
  double ra[kExpRows], rbl[kExpRows], rbr[kExpRows];
  double glo = INFINITY, ghi = -INFINITY, bmax = 0.0;
  bool finite = true;
#pragma unroll
  for (int u = 0; u < kExpRows; ++u) {
    const int i = t + u * kTPB;
    ra[u] = rbl[u] = rbr[u] = 0.0;
    if (u < R && i < n) {
      ra[u] = src.alpha(i);
      rbl[u] = i > 0 ? src.beta(i - 1) : 0.0;
      rbr[u] = i + 1 < n ? src.beta(i) : 0.0;
      al[i] = ra[u];
      b2[i] = rbr[u] * rbr[u];
      finite = finite && isfinite(ra[u]) && isfinite(rbr[u]);
      const double rad = fabs(rbl[u]) + fabs(rbr[u]);
      glo = fmin(glo, ra[u] - rad);
      ghi = fmax(ghi, ra[u] + rad);
      bmax = fmax(bmax, rbr[u] * rbr[u]);
    }
  }
  for (int i = t; i < n + 2; i += kTPB) buf0[i] = buf1[i] = 0.0;
  red[0][t] = glo;
  red[1][t] = ghi;
  cnt[t] = finite ? 0 : 1;
  if (t < 2) first[t] = kExpShifts;
  __syncthreads();
  for (int h = kTPB / 2; h > 0; h >>= 1) {
    if (t < h) {
      red[0][t] = fmin(red[0][t], red[0][t + h]);
      red[1][t] = fmax(red[1][t], red[1][t + h]);
      cnt[t] |= cnt[t + h];
    }
    __syncthreads();
  }
  glo = red[0][0];
  ghi = red[1][0];
  const bool bad = cnt[0] != 0;
  __syncthreads();
  red[0][t] = bmax;
  __syncthreads();
  for (int h = kTPB / 2; h > 0; h >>= 1) {
    if (t < h) red[0][t] = fmax(red[0][t], red[0][t + h]);
    __syncthreads();
  }
  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, red[0][0]);
  auto fallback = [&]() {
    for (int i = t; i < n; i += kTPB) dst.y(i, 0.0);
    if (t == 0) dst.hand_back();
  };
  if (bad) {
    fallback();
    return;
  }
  if (n == 1) {
    if (t == 0) {
      dst.y(0, exp(al[0]) * bnorm);
      dst.kept();
    }
    return;
  }
  TPL_MARK(1);
  // One round of Sturm multisection over the Gershgorin interval [glo, ghi]: 512 shifts
  // serve both ends, two independent LDL^T pivot chains per thread (ILP: each chain is a
  // dependent sequence of n reciprocals). lambda_min lies in the bracket ending at the
  // first shift with a count >= 1, lambda_max in the one ending at the first count == n.
  {
    const double w = (ghi - glo) / (double)(kExpShifts + 1);
    double sg[2], q[2];
    int c[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sg[u] = glo + w * (double)(u * kTPB + t + 1);  // shift s = u * 256 + t
      q[u] = al[0] - sg[u];
      if (fabs(q[u]) < pivmin) q[u] = -pivmin;
      c[u] = q[u] < 0.0;
    }
    for (int i = 1; i < n; ++i) {
      const double ai = al[i], bb = b2[i - 1];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        q[u] = (ai - sg[u]) - bb * rcp_nr(q[u]);
        if (fabs(q[u]) < pivmin) q[u] = -pivmin;
        c[u] += q[u] < 0.0;
      }
    }
    cnt[t] = c[0];
    cnt[t + kTPB] = c[1];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int sidx = u * kTPB + t;
      if (cnt[sidx] >= 1) atomicMin(&first[0], sidx);
      if (cnt[sidx] >= n) atomicMin(&first[1], sidx);
    }
    __syncthreads();
  }
  TPL_MARK(2);
  // [a, b] holds the spectrum: below the shift before lambda_min's first count, above the
  // first shift counting all n, widened by a margin far above a count's backward error
  const double wsh = (ghi - glo) / (double)(kExpShifts + 1);
  const double gmag = fmax(fabs(glo), fabs(ghi));
  const double a = (first[0] > 0 ? glo + wsh * (double)first[0] : glo) - 1e-9 * (1.0 + gmag);
  const double b = (first[1] < kExpShifts ? glo + wsh * (double)(first[1] + 1) : ghi) +
                   1e-9 * (1.0 + gmag);
  const double c = 0.5 * (a + b);
  const double r = fmax(0.5 * (b - a), 1e-30 * (1.0 + fabs(c)));
  const double inv_r = 1.0 / r;
  // terms: the smallest m with e^-r I_m(r) < 1e-22 (asymptotic form, decreasing in m),
  // found in two parallel passes: every thread tests m = 64 t, then the 64 candidates
  // below the first passing one
  {
    __syncthreads();  // every thread has read the brackets out of first[]
    if (t < 2) first[t] = kExpMaxTerms + 1;
    __syncthreads();
    const int m0 = 64 * t;
    if (m0 <= kExpMaxTerms && log_scaled_bessel_i((double)m0, r) < -50.66) atomicMin(&first[0], m0);
    __syncthreads();
    const int hi = first[0];
    if (hi <= kExpMaxTerms && t < 64) {
      const int m1 = hi - 63 + t;
      if (m1 >= 0 && log_scaled_bessel_i((double)m1, r) < -50.66) atomicMin(&first[1], m1);
    }
    __syncthreads();
  }
  if (first[0] > kExpMaxTerms) {
    fallback();
    return;
  }
  const int N = min(first[0], first[1]) + 8;
  TPL_MARK(3);
  // Clenshaw: b_m = a_m e_1 + 2 x b_{m+1} - b_{m+2} (m = N .. 1), x = (T - c I) / r; the
  // result is a_0 e_1 + x b_1 - b_2 with a_0 = I_0, a_m = 2 I_m (unnormalised Miller values)
  double b1[kExpRows], b2v[kExpRows], dia[kExpRows];
#pragma unroll
  for (int u = 0; u < kExpRows; ++u) {
    b1[u] = b2v[u] = 0.0;
    dia[u] = ra[u] - c;
  }
  double Ip1 = 0.0, Im = 1.0, Ssum = 0.0;  // I_{m+1}, I_m (Miller seed), 2 sum_{m'>=m} I_m'
  double* cur = buf0;
  double* nxt = buf1;
  if (n <= 4 * 64) {
    // T_k of at most 256 rows (configs[1]: k = 200): ONE wave runs the recurrence, four
    // consecutive rows per lane, the neighbour rows across lanes by DPP wave shifts — no
    // LDS exchange and no barrier per term. The same operations on the same operands as
    // the general loop below, row by row (zero neighbours at both ends), so the same bits.
    if (t < 64) {
      double f1[4], f2[4], fd[4], fl[4], fr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * t + j;
        const bool ok = i < n;
        fd[j] = ok ? al[i] - c : 0.0;
        fl[j] = (ok && i > 0) ? src.beta(i - 1) : 0.0;
        fr[j] = (ok && i + 1 < n) ? src.beta(i) : 0.0;
        f1[j] = f2[j] = 0.0;
      }
      for (int m = N; m >= 1; --m) {
        const double left = dpp_f64<0x138>(f1[3]);   // wave_shr:1 -> row 4t - 1 (0 at lane 0)
        const double right = dpp_f64<0x130>(f1[0]);  // wave_shl:1 -> row 4t + 4 (0 at lane 63)
        const double am = 2.0 * Im;
        double nv[4];
        nv[0] = ((fl[0] * left + fd[0] * f1[0]) + fr[0] * f1[1]) * inv_r;
        nv[1] = ((fl[1] * f1[0] + fd[1] * f1[1]) + fr[1] * f1[2]) * inv_r;
        nv[2] = ((fl[2] * f1[1] + fd[2] * f1[2]) + fr[2] * f1[3]) * inv_r;
        nv[3] = ((fl[3] * f1[2] + fd[3] * f1[3]) + fr[3] * right) * inv_r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double v = 2.0 * nv[j] - f2[j];
          if (t == 0 && j == 0) v = v + am;
          f2[j] = f1[j];
          f1[j] = v;
        }
        Ssum = Ssum + am;
        const double Inext = Ip1 + (2.0 * (double)m * inv_r) * Im;
        Ip1 = Im;
        Im = Inext;
        if (fabs(Im) > 1e200) {
          Im *= 1e-200; Ip1 *= 1e-200; Ssum *= 1e-200;
#pragma unroll
          for (int j = 0; j < 4; ++j) { f1[j] *= 1e-200; f2[j] *= 1e-200; }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * t + j;
        if (i < n) {
          cur[i + 1] = f1[j];
          nxt[i + 1] = f2[j];
        }
      }
      if (t == 0) {
        red[1][0] = Im;
        red[1][1] = Ssum;
      }
    }
    __syncthreads();
    Im = red[1][0];
    Ssum = red[1][1];
#pragma unroll
    for (int u = 0; u < kExpRows; ++u) {
      const int i = t + u * kTPB;
      if (u < R && i < n) {
        b1[u] = cur[i + 1];
        b2v[u] = nxt[i + 1];
      }
    }
    __syncthreads();  // every lane has its rows before the tail rewrites cur
  } else
  for (int m = N; m >= 1; --m) {
    // publish b_{m+1}, then every row forms b_m from its neighbours
#pragma unroll
    for (int u = 0; u < kExpRows; ++u) {
      const int i = t + u * kTPB;
      if (u < R && i < n) cur[i + 1] = b1[u];
    }
    __syncthreads();
    const double am = 2.0 * Im;
#pragma unroll
    for (int u = 0; u < kExpRows; ++u) {
      const int i = t + u * kTPB;
      if (u < R && i < n) {
        const double xb = ((rbl[u] * cur[i] + dia[u] * cur[i + 1]) + rbr[u] * cur[i + 2]) * inv_r;
        double v = 2.0 * xb - b2v[u];
        if (i == 0) v = v + am;
        b2v[u] = b1[u];
        b1[u] = v;
      }
    }
    Ssum = Ssum + am;
    const double Inext = Ip1 + (2.0 * (double)m * inv_r) * Im;
    Ip1 = Im;
    Im = Inext;
    if (fabs(Im) > 1e200) {  // Miller's values grow towards m = 0: rescale the whole state
      Im *= 1e-200; Ip1 *= 1e-200; Ssum *= 1e-200;
#pragma unroll
      for (int u = 0; u < kExpRows; ++u) { b1[u] *= 1e-200; b2v[u] *= 1e-200; }
    }
    double* sw = cur; cur = nxt; nxt = sw;  // double buffer: one barrier per term
  }
  TPL_MARK(4);
  // y' = e^b (I_0 e_1 + x b_1 - b_2) / (I_0 + 2 sum I_m)
#pragma unroll
  for (int u = 0; u < kExpRows; ++u) {
    const int i = t + u * kTPB;
    if (u < R && i < n) cur[i + 1] = b1[u];
  }
  __syncthreads();
  const double norm = Ssum + Im;
  const double eb = exp(b);
  double yv[kExpRows];
  double sq = 0.0;
#pragma unroll
  for (int u = 0; u < kExpRows; ++u) {
    const int i = t + u * kTPB;
    yv[u] = 0.0;
    if (u < R && i < n) {
      const double xb = ((rbl[u] * cur[i] + dia[u] * cur[i + 1]) + rbr[u] * cur[i + 2]) * inv_r;
      double v = xb - b2v[u];
      if (i == 0) v = v + Im;
      yv[u] = v / norm;  // exp(T - b I) e_1
      sq = fma(yv[u], yv[u], sq);
    }
  }
  // The expansion's error is a few eps * (terms) in units of e^b; when ||exp(T - bI) e_1||
  // is far below 1 (e_1 nearly orthogonal to the top of the spectrum) that is no longer
  // small against ||y||, while the EVD keeps its relative accuracy: hand such cases back.
  __syncthreads();
  red[0][t] = sq;
  __syncthreads();
  for (int h = kTPB / 2; h > 0; h >>= 1) {
    if (t < h) red[0][t] = red[0][t] + red[0][t + h];
    __syncthreads();
  }
  if (!(red[0][0] >= kExpMinRatio * kExpMinRatio)) {
    fallback();
    return;
  }
#pragma unroll
  for (int u = 0; u < kExpRows; ++u) {
    const int i = t + u * kTPB;
    if (u < R && i < n) dst.y(i, (eb * yv[u]) * bnorm);
  }
  if (t == 0) dst.kept();
  TPL_MARK(5);
  TPL_STAMP_TERMS(N);
}
// The source and destination of the kernels that evaluate exp at a list of times.
// t T_k: every entry times t, one rounding (RN(t alpha_j), RN(t beta_j) — the arrays the host
// built-in tpl_ftk_exp_t forms), before anything else uses it. The build's -ffp-contract=off
// keeps the product out of the subtractions that follow (t alpha - c stays two roundings).
struct ExpSrcTimes {
  const double *al, *be;
  double t;
  __device__ __forceinline__ double alpha(int i) const { return t * al[i]; }
  __device__ __forceinline__ double beta(int i) const { return t * be[i]; }
};
struct ExpDstTimes {  // a column of the coefficient table and its hand-back entry
  double* y_;
  int32_t* back;
  __device__ __forceinline__ void y(int i, double v) const { y_[i] = v; }
  __device__ __forceinline__ void hand_back() const { *back = 1; }
  __device__ __forceinline__ void kept() const { *back = 0; }
};
// Dynamic LDS of a workgroup that runs ftk_exp_body on up to kcap rows.
static inline size_t ftk_exp_lds_bytes(int kcap) { return (size_t)(4 * kcap + 4) * sizeof(double); }

} // namespace tpl
