// tpl_k_dist_reorth.hip — the kernels only the partitioned solve and the one-pass variant's
// re-orthogonalisation launch: the long-row epilogues run after the exchange of the ranks'
// partials (k_long_epi_p1 / _y / _p2), and full / selective re-orthogonalisation
// (k_reorth_dot / _reduce / _update / _decide). One unit: compiled apart from
// k_reorth_reduce, k_long_epi_p1's rank-total branch (the same load_partials /
// finish_partials over 8 partials per thread) schedules its loads differently. Map of the
// device sources: tpl_kernels.hip.
#include "tpl_klaunch.h"

namespace tpl {

// ---------------------------------------- replicated long rows (partitioned solve)
// Long row l = sum over ranks, in rank order, of the R partials all-gathered into
// yall[r * y_ld + l]; every rank then runs the row's epilogue (identical bits on all
// ranks). Local index of long row l: A.n - A.n_long + l. Alpha partial (pass one):
// thread t accumulates fma(v, w) over rows t + 256q of its workgroup's range, tree256.
// One row per thread (kLongEpiRows = kTPB). Every load of the launch — the row's own
// vector entries, its R partials (8 in flight at a time, at clamped rows, so every lane
// loads and the adds keep rank order) — is issued before the DevState scalars are read:
// one round trip behind the boundary instead of a scalar one first (round 3).
struct LongSum {
  double t[8];
};
// the first 8 ranks' partials of long row lc (clamped: every lane loads) ...
__device__ __forceinline__ void long_sum_issue(const CsrDev& A, const double* __restrict__ yall,
                                               int R, int lc, LongSum& q) {
#pragma unroll
  for (int u = 0; u < 8; ++u) q.t[u] = yall[(size_t)clampi(u, R - 1) * A.y_ld + lc];
}
// ... summed in rank order; more ranks in batches of 8 loads in flight
__device__ __forceinline__ double long_sum_finish(const CsrDev& A, const double* __restrict__ yall,
                                                  int R, int lc, const LongSum& q) {
  double y = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (u < R) y = y + q.t[u];
  for (int r0 = 8; r0 < R; r0 += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = yall[(size_t)clampi(r0 + u, R - 1) * A.y_ld + lc];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r0 + u < R) y = y + t[u];
  }
  return y;
}

// Pass one after the exchange: the long rows' epilogue (w, alpha partials) and, in R more
// workgroups, each rank's short-chunk alpha total from its all-gathered chunk partials —
// finish_partials over yall[r * y_ld + n_long ..], the tree k_reorth_reduce applies, so
// the totals are bitwise those a separate rank-total launch before the all-gather made
// (r02/r03; that launch is gone). Pa_long[-R .. -1]: the R totals; Pa_long[b]: block b.
__global__ __launch_bounds__(kTPB) void k_long_epi_p1(CsrDev A, DevState S,
                                                      const double* __restrict__ yall, int R,
                                                      const double* __restrict__ r_cur,
                                                      const double* __restrict__ r_prev,
                                                      double* __restrict__ W,
                                                      double* __restrict__ Vcol,
                                                      double* __restrict__ Pa_long, int j) {
  __shared__ double red[4];
  const int nbl = (A.n_long + kLongEpiRows - 1) / kLongEpiRows;
  if ((int)blockIdx.x >= nbl) {  // rank total (uniform per workgroup)
    const int r = blockIdx.x - nbl;
    const double* P = yall + (size_t)r * A.y_ld + A.n_long;
    const int N = A.nch[r];
    double tot = 0.0;  // a rank without short rows (N == 0, uniform): nothing to load
    if (N > 0) {
      PartialRegs<8> pr;
      load_partials(P, N, pr);
      tot = finish_partials(P, N, pr, red);
    }
    if (threadIdx.x == 0) Pa_long[r - R] = tot;
    return;
  }
  EpiPass1 epi;
  epi.r_cur = r_cur;
  epi.r_prev = (j >= 2) ? r_prev : r_cur;
  epi.has_prev = j >= 2;
  epi.W = W;
  epi.Vcol = Vcol;
  epi.Pa_long = nullptr;
  const int l = blockIdx.x * kLongEpiRows + threadIdx.x;
  const int lc = l < A.n_long ? l : A.n_long - 1;
  const int row = (int)(A.n - A.n_long) + lc;
  const Pre1 pre = epi.pre(row);
  LongSum q;
  long_sum_issue(A, yall, R, lc, q);
  __builtin_amdgcn_sched_barrier(0);
  const int stop = S.flags[0];
  const double beta = S.norms[j - 1];
  const double beta_prev = S.norms[j >= 2 ? j - 2 : 0];
  const double y = long_sum_finish(A, yall, R, lc, q);
  if (stop) return;  // stopped / breakdown (uniform)
  epi.invN_cur = 1.0 / beta;
  epi.invN_prev = (j >= 2) ? 1.0 / beta_prev : 0.0;
  epi.beta_sub = (j >= 2) ? beta : 0.0;
  double acc = 0.0;
  if (l < A.n_long) epi.apply(row, y, pre, acc);
  const double p = block_sum_tail(acc, red);
  if (threadIdx.x == 0) Pa_long[blockIdx.x] = p;
}

__global__ __launch_bounds__(kTPB) void k_long_epi_y(CsrDev A, const double* __restrict__ yall,
                                                     int R, double* __restrict__ y) {
  const int l = blockIdx.x * kLongEpiRows + threadIdx.x;
  const int lc = l < A.n_long ? l : A.n_long - 1;
  LongSum q;
  long_sum_issue(A, yall, R, lc, q);
  const double s = long_sum_finish(A, yall, R, lc, q);
  if (l < A.n_long) st_out(y + (A.n - A.n_long) + l, s);
}

// Pass two after the exchange: the coefficients come from the step's record, loaded
// lane-wise with the row's own entries (EpiPass2R), so nothing waits for a scalar load.
__global__ __launch_bounds__(kTPB) void k_long_epi_p2(CsrDev A, const double* __restrict__ rec,
                                                      const double* __restrict__ yall, int R,
                                                      const double* __restrict__ v_cur,
                                                      const double* __restrict__ v_prev,
                                                      double* __restrict__ v_next,
                                                      double* __restrict__ x,
                                                      double* __restrict__ Vcol, int j,
                                                      int nflush) {
  const EpiPass2R epi = EpiPass2R::of(rec, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  const int l = blockIdx.x * kLongEpiRows + threadIdx.x;
  const int lc = l < A.n_long ? l : A.n_long - 1;
  const int row = (int)(A.n - A.n_long) + lc;
  const Pre2R pre = epi.pre(row);
  LongSum q;
  long_sum_issue(A, yall, R, lc, q);
  const double y = long_sum_finish(A, yall, R, lc, q);
  double acc = 0.0;
  if (l < A.n_long) epi.apply(row, y, pre, acc);
}

namespace launch {

int long_epi_blocks(const CsrDev& A) { return (A.n_long + kLongEpiRows - 1) / kLongEpiRows; }
hipError_t long_epi_p1(const CsrDev& A, const DevState& S, const double* yall, int R,
                       const double* r_cur, const double* r_prev, double* W, double* Vcol,
                       double* Pa_long, int j, hipStream_t s) {
  // the long rows' blocks, then one workgroup per rank for the short-chunk alpha totals
  hipLaunchKernelGGL(k_long_epi_p1, dim3(long_epi_blocks(A) + R), dim3(kTPB), 0, s, A, S, yall,
                     R, r_cur, r_prev, W, Vcol, Pa_long, j);
  return hipGetLastError();
}
hipError_t long_epi_y(const CsrDev& A, const double* yall, int R, double* y, hipStream_t s) {
  if (A.n_long > 0)
    hipLaunchKernelGGL(k_long_epi_y, dim3(long_epi_blocks(A)), dim3(kTPB), 0, s, A, yall, R, y);
  return hipGetLastError();
}
hipError_t long_epi_p2(const CsrDev& A, const DevState& S, const double* yall, int R,
                       const double* v_cur, const double* v_prev, double* v_next, double* x,
                       double* Vcol, int j, int nflush, hipStream_t s) {
  if (A.n_long > 0)
    hipLaunchKernelGGL(k_long_epi_p2, dim3(long_epi_blocks(A)), dim3(kTPB), 0, s, A,
                       S.p2c + 8 * (size_t)j, yall, R, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  return hipGetLastError();
}

} // namespace launch

// ---------------------------------------------------- full re-orthogonalisation
// Extension with no reference counterpart (the reference's one-pass variant runs
// only the three-term recurrence, src/algorithms/mod.rs:167-212): classical
// Gram-Schmidt applied twice (CGS2) of r_{j+1} against V_k[:, 0..cols) before
// beta_j is formed. V is column-major (ld = n): lane i of a wave reads V[c*n + i],
// so every column sweep is a coalesced stream.
constexpr int kReorthCols = 16; // columns per workgroup in the h = V^T r kernel

// h partials: grid (G2, ceil(cols/16)); workgroup (b, g) owns rows [bE, min(n,(b+1)E))
// and columns [16g, 16g+16). P[c*G2 + b] = tree256 of the thread accumulators (thread
// t: acc = fma(V[c][i], r[i], acc) over i = bE + t + 256q, q ascending). Every column's
// load is issued unconditionally (columns past cols re-read column 16g, unused) so the
// 17 loads of an iteration are all in flight; the 16 trees share one barrier.
// skip (selective variant): the second pass is not needed (k_reorth_decide).
__global__ __launch_bounds__(kTPB) void k_reorth_dot(int64_t n, int cols,
                                                     const double* __restrict__ V,
                                                     const double* __restrict__ r,
                                                     double* __restrict__ P, int G, int64_t E,
                                                     const int* __restrict__ skip) {
  __shared__ double red[kReorthCols * 4];
  if (skip && *skip) return;
  const int c0 = blockIdx.y * kReorthCols;
  const int nc = cols - c0 < kReorthCols ? cols - c0 : kReorthCols;
  const int64_t beg = (int64_t)blockIdx.x * E;
  const int64_t end = beg + E < n ? beg + E : n;
  double acc[kReorthCols];
#pragma unroll
  for (int u = 0; u < kReorthCols; ++u) acc[u] = 0.0;
#pragma unroll 2
  for (int64_t i = beg + threadIdx.x; i < end; i += kTPB) {
    const double ri = r[i];
    double v[kReorthCols];
#pragma unroll
    for (int u = 0; u < kReorthCols; ++u) v[u] = V[(int64_t)(c0 + (u < nc ? u : 0)) * n + i];
#pragma unroll
    for (int u = 0; u < kReorthCols; ++u) acc[u] = u < nc ? fma(v[u], ri, acc[u]) : acc[u];
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int u = 0; u < kReorthCols; ++u) {
    const double sw = wave_sum(acc[u]);
    if ((threadIdx.x & 63) == 0) red[u * 4 + w] = sw;
  }
  __syncthreads();
  const int u = threadIdx.x;
  if (u < nc)
    P[(int64_t)(c0 + u) * G + blockIdx.x] =
        (red[u * 4 + 0] + red[u * 4 + 1]) + (red[u * 4 + 2] + red[u * 4 + 3]);
}

// h[c] = sum of the G partials of column c (one workgroup per column).
__global__ __launch_bounds__(kTPB) void k_reorth_reduce(const double* __restrict__ P, int G,
                                                        double* __restrict__ h,
                                                        const int* __restrict__ skip) {
  __shared__ double red[4];
  if (skip && *skip) return;
  PartialRegs<8> pr;
  const double* Pc = P + (int64_t)blockIdx.x * G;
  load_partials(Pc, G, pr);
  const double s = finish_partials(Pc, G, pr, red);
  if (threadIdx.x == 0) h[blockIdx.x] = s;
}

// r -= V h ; optional ||r||^2 partials in the canonical norm order (E partition).
// Thread t owns the pairs (i0, i0 + 1), i0 = bE + 2t + 512q, as the norm order does;
// per element s = 0; s = fma(V[c][i], h[c], s) for c ascending. The columns are taken
// kUpdCols at a time with all 2 kUpdCols loads in flight before the ordered FMAs: the
// sweep is a pure HBM stream (V_j does not fit the Infinity Cache at k = 500), so bytes
// in flight per CU, not arithmetic, set its rate.
constexpr int kUpdCols = 16;
__global__ __launch_bounds__(kTPB) void k_reorth_update(int64_t n, int cols,
                                                        const double* __restrict__ V,
                                                        double* __restrict__ r,
                                                        const double* __restrict__ h,
                                                        double* __restrict__ Pnorm, int64_t E,
                                                        const int* __restrict__ skip) {
  __shared__ double red[4];
  if (skip && *skip) return;
  const int64_t beg = (int64_t)blockIdx.x * E;
  const int64_t end = beg + E < n ? beg + E : n;
  double acc = 0.0;
  for (int64_t i0 = beg + 2 * threadIdx.x; i0 < end; i0 += 2 * kTPB) {
    const bool has1 = i0 + 1 < end;
    const int64_t i1 = has1 ? i0 + 1 : i0;
    const double r0 = r[i0], r1 = r[i1];
    double s0 = 0.0, s1 = 0.0;
    int c = 0;
    for (; c + kUpdCols <= cols; c += kUpdCols) {
      double v0[kUpdCols], v1[kUpdCols];
#pragma unroll
      for (int u = 0; u < kUpdCols; ++u) {
        const double* col = V + (int64_t)(c + u) * n;
        v0[u] = col[i0];
        v1[u] = col[i1];
      }
#pragma unroll
      for (int u = 0; u < kUpdCols; ++u) {
        s0 = fma(v0[u], h[c + u], s0);
        s1 = fma(v1[u], h[c + u], s1);
      }
    }
    for (; c < cols; ++c) {
      const double* col = V + (int64_t)c * n;
      s0 = fma(col[i0], h[c], s0);
      s1 = fma(col[i1], h[c], s1);
    }
    const double q0 = r0 - s0;
    r[i0] = q0;
    acc = fma(q0, q0, acc);
    if (has1) {
      const double q1 = r1 - s1;
      r[i1] = q1;
      acc = fma(q1, q1, acc);
    }
  }
  if (Pnorm) {
    const double p = block_sum(acc, red);
    if (threadIdx.x == 0) Pnorm[blockIdx.x] = p;
  }
}

// Selective re-orthogonalisation (Kahan–Parlett "twice is enough"): after the first
// projection r' = r - V h, the second one is needed only when it removed more than half
// of r's squared norm. n0 = ||r||^2 (the partials k_p1_axpy left in S.Pb), n1 = ||r'||^2
// (Pb1, written by the first update), both reduced in the canonical norm order; if
// n1 >= n0 / 2 the second pass is skipped and r' is the result — its partials become the
// ones k_p1_spmv reduces for beta — else S.flags[3] counts a second pass. rec: this
// step's slot of the per-step record (1: a second pass ran), so the host can count only
// the steps a caller keeps (a step callback may stop before the device's last step).
// One workgroup.
__global__ __launch_bounds__(kTPB) void k_reorth_decide(DevState S, const double* __restrict__ Pb1,
                                                        int G2, int* __restrict__ skip,
                                                        int* __restrict__ rec) {
  __shared__ double red[4];
  PartialRegs<4> p0, p1;  // G2 <= 1024
  load_partials(S.Pb, G2, p0);
  load_partials(Pb1, G2, p1);
  const double n0 = finish_partials(S.Pb, G2, p0, red);
  const double n1 = finish_partials(Pb1, G2, p1, red);
  const bool sk = n1 >= 0.5 * n0;
  if (sk)
    for (int i = threadIdx.x; i < G2; i += kTPB) S.Pb[i] = Pb1[i];
  if (threadIdx.x == 0) {
    *skip = sk ? 1 : 0;
    *rec = sk ? 0 : 1;
    if (!sk) S.flags[3] = S.flags[3] + 1;
  }
}

namespace launch {

hipError_t reorth_dot(int64_t n, int cols, const double* V, const double* r, double* P, int G,
                      int64_t E, const int* skip, hipStream_t s) {
  dim3 grid(G, (cols + kReorthCols - 1) / kReorthCols);
  hipLaunchKernelGGL(k_reorth_dot, grid, dim3(kTPB), 0, s, n, cols, V, r, P, G, E, skip);
  return hipGetLastError();
}
hipError_t reorth_reduce(int cols, const double* P, int G, double* h, const int* skip,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_reorth_reduce, dim3(cols), dim3(kTPB), 0, s, P, G, h, skip);
  return hipGetLastError();
}
hipError_t reorth_update(int64_t n, int cols, const double* V, double* r, const double* h,
                         double* Pnorm, int G, int64_t E, const int* skip, hipStream_t s) {
  hipLaunchKernelGGL(k_reorth_update, dim3(G), dim3(kTPB), 0, s, n, cols, V, r, h, Pnorm, E,
                     skip);
  return hipGetLastError();
}
hipError_t reorth_decide(const DevState& S, const double* Pb1, int G2, int* skip, int* rec,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_reorth_decide, dim3(1), dim3(kTPB), 0, s, S, Pb1, G2, skip, rec);
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
