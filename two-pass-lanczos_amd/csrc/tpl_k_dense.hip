// tpl_k_dense.hip — the dense symmetric operator (tpl_op_create_dense): the three SpMV-shaped
// kernels of a matrix stored whole, row-major with a padded leading dimension. Map of the
// device sources: tpl_kernels.hip.
//   k_dense_spmv  y = A x (tpl_op_apply)
//   k_dense_p1    the pass-one step (k_p1_spmv's prologue and epilogue; k_p1_axpy follows as is)
//   k_dense_p2    the pass-two step (k_p2_spmv's records, nflush and inactive-launch rule)
// No indices, no gathers, no hand-off: the kernels stream A once per step.
//
// Arithmetic (tpl_device.h "long row", oracle/lanczos_oracle.c long_row_canon with every row
// long and every column stored): with S column slices, slice s = columns [floor(n s / S),
// floor(n (s + 1) / S)); a slice of more than kBigPiece columns is summed on L = 16 lanes, any
// other on L = 8. Lane g: p_g = +0.0; p_g += RN(A[i, c] RN(x_c scale)) for c = lo + g, lo + g + L,
// ... ascending; P_s = xor butterfly of p over the L lanes (1, 2, 4 (, 8)); y = +0.0; y += P_s,
// s ascending, empty slices included. The row's epilogue is EpiSpmv / EpiPass1 / EpiPass2R
// unchanged; its alpha partial is RN(v_i w_i) at Pa[i] (n_chunks = 0, NA = n).
//
// Work: a group of 16 consecutive threads owns a row (16 rows per workgroup) and walks its
// slices in order; thread p carries the logical lane p (L = 8: the threads p < 8 only) and the
// butterfly runs on DPP inside the group. The scaled vector is staged in LDS a tile of
// kDenseTile columns at a time (tile starts are lo + a multiple of 16, so a column keeps its
// lane), the next tile's entries prefetched into registers while the current one is summed;
// RN(x_c scale) is formed once per staged element — the product k_p1_spmv's gather makes. A
// thread's column loop is unrolled by 8: eight independent loads in flight, the adds in order
// behind them; a wave's load covers four rows' 128-B lines. (Two logical lanes per thread with
// one 16-B load per pair and the butterfly's first stage in the thread — 8 threads per row —
// measured 5 % slower at n = 10,000 and the same at 4,096: DESIGN.md §6.3.)
// Padding never enters a sum: the loops end at the slice's exact bound, the last partial
// block adds -0.0 for the entries past it (x + -0.0 is x bit for bit).
#include "tpl_klaunch.h"

namespace tpl {

constexpr int kDenseTile = 2048;            // columns of the vector staged in LDS at a time
constexpr int kDenseLanes = 16;             // threads per row: one per logical lane
constexpr int kDenseRows = kTPB / kDenseLanes;  // rows per workgroup
constexpr int kDenseXRegs = kDenseTile / kTPB;  // prefetched vector entries per thread
static_assert(kDenseTile % 16 == 0 && kDenseTile % kTPB == 0, "lane-preserving tiles");

// Kernel arguments of k_dense_p1: what P1SpmvArgs carries of the state and the step, and the
// dense view in place of the layout.
struct DenseP1Args {
  const double* Pb_r;
  int32_t* flags;
  double* norms;
  double* betas;
  double* Pa;
  const double* xsrc;
  const double* r_cur;
  const double* r_prev;
  double* W;
  double* Vcol;
  unsigned long long* stamp;
  DenseDev D;
  int32_t j;
  int32_t G2_r;
};

// One tile of one row: columns [0, cnt) of arow against the staged xs, this thread's logical
// lane p, stride L. Threads with p >= L hold no lane.
__device__ __forceinline__ void dense_tile(const double* __restrict__ arow,
                                           const double* __restrict__ xs, int cnt, int L, int p,
                                           double& acc) {
  int c = p < L ? p : cnt;
  // whole blocks of 8 entries: the loads first, then the adds in column order
  for (; c + 7 * L < cnt; c += 8 * L) {
    double a[8], x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = arow[c + u * L];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = xs[c + u * L];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = acc + a[u] * x[u];
  }
  // the last 0..8 entries, at clamped addresses (c < cnt is readable); entries past the
  // bound add -0.0
  if (c < cnt) {
    double a[8], x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int cc = c + u * L;
      const int i0 = cc < cnt ? cc : c;
      a[u] = arow[i0];
      x[u] = xs[i0];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      double p0 = a[u] * x[u];
      keep(p0);
      acc = acc + (c + u * L < cnt ? p0 : -0.0);
    }
  }
}

// The body the three kernels share. xs: kDenseTile doubles of LDS. Returns false when the
// prologue stopped the step (uniform over the grid).
template <class Epi, class ScaleFn>
__device__ __forceinline__ bool dense_block(const DenseDev& D, const double* __restrict__ xsrc,
                                            ScaleFn scale_of, const Epi& epi, double* xs) {
  const int t = threadIdx.x, p = t & (kDenseLanes - 1);
  const int n = D.n, S = D.S;
  const int row = blockIdx.x * kDenseRows + t / kDenseLanes;
  const bool live = row < n;
  const int rowc = live ? row : n - 1;
  const double* __restrict__ arow0 = D.a + (int64_t)rowc * D.ld;
  // the first tile of the vector (slice 0 starts at column 0), then the row's own entries
  double xr[kDenseXRegs];
#pragma unroll
  for (int u = 0; u < kDenseXRegs; ++u) xr[u] = xsrc[clampi(t + u * kTPB, n - 1)];
  auto pre = epi.pre(rowc);
  const Scale sc = scale_of();
  if (!sc.ok) return false;
  double y = 0.0;
  for (int s = 0; s < S; ++s) {
    const int lo = (int)((int64_t)n * s / S), hi = (int)((int64_t)n * (s + 1) / S);
    const int L = hi - lo > kBigPiece ? 16 : 8;
    double acc = 0.0;
    for (int t0 = lo; t0 < hi; t0 += kDenseTile) {
      const int cnt = hi - t0 < kDenseTile ? hi - t0 : kDenseTile;
      __syncthreads();  // the previous tile's readers are done
#pragma unroll
      for (int u = 0; u < kDenseXRegs; ++u) xs[t + u * kTPB] = xr[u] * sc.s;
      __syncthreads();
      // the next tile (of this slice, or the next non-empty slice's first) into registers
      // (the next slice starts where this one ends; empty slices stage nothing)
      const int nx = t0 + kDenseTile < hi ? t0 + kDenseTile : hi;
#pragma unroll
      for (int u = 0; u < kDenseXRegs; ++u) xr[u] = xsrc[clampi(nx + t + u * kTPB, n - 1)];
      dense_tile(arow0 + t0, xs, cnt, L, p, acc);
    }
    // the butterfly on DPP inside the 16-thread group (L = 8: the threads p < 8)
    const double v8 = group8_sum(acc);
    const double v16 = v8 + dpp_f64<0x140>(v8);
    y = y + (L == 16 ? v16 : v8);
  }
  keep_pre(pre);
  if (p == 0 && live) {
    double acc = 0.0;
    epi.apply(row, y, pre, acc);
    epi.long_alpha(row, acc);
  }
  return true;
}

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(kTPB) void k_dense_spmv(DenseDev D, const double* __restrict__ x,
                                                     double* __restrict__ y) {
  __shared__ double xs[kDenseTile];
  dense_block(D, x, UnitScale{}, EpiSpmv{y}, xs);
}

// The pass-one step of a dense operator: p1_spmv_body's prologue — beta_{j-1} from the norm
// partials k_p1_axpy left (the canonical partials() order), stored; the breakdown stop; the
// gather scale 1 / beta_{j-1} — and EpiPass1 with the alpha partials at Pa[i].
__global__ __launch_bounds__(kTPB) void k_dense_p1(DenseP1Args a) {
  __shared__ double xs[kDenseTile];
  __shared__ double redb[4];
  const int j = a.j;
  launch_stamp(a.stamp);
  PartialRegs<1> pr;
  load_partials(a.Pb_r, a.G2_r, pr);
  int stop0 = a.flags[0];
  double norm_prev = (j >= 2) ? a.norms[j - 2] : 1.0;
  __builtin_amdgcn_sched_barrier(0);
  EpiPass1 epi;
  epi.r_cur = a.r_cur;
  epi.r_prev = (j >= 2) ? a.r_prev : a.r_cur;
  epi.has_prev = j >= 2;
  epi.invN_prev = 0.0;
  epi.invN_cur = 0.0;
  epi.beta_sub = 0.0;
  epi.W = a.W;
  epi.Vcol = a.Vcol;
  epi.Pa_long = a.Pa;  // n_chunks = 0: row i's partial at Pa[i]
  auto scale_fn = [&]() -> Scale {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(stop0), "+v"(norm_prev));
    if (stop0) return Scale{0.0, false};
    epi.invN_prev = (j >= 2) ? 1.0 / norm_prev : 0.0;
    const double beta = sqrt(finish_partials(a.Pb_r, a.G2_r, pr, redb));
    if (beta <= kBreakdownTol) {
      // j == 1: zero b; j > 1: breakdown, steps_taken = j - 1 (as p1_spmv_body)
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.flags[0] = 1;
        if (j == 1) a.flags[1] = 1;
      }
      return Scale{0.0, false};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.norms[j - 1] = beta;
      if (j >= 2) a.betas[j - 2] = beta;
    }
    epi.invN_cur = 1.0 / beta;
    epi.beta_sub = (j >= 2) ? beta : 0.0;
    return Scale{epi.invN_cur, true};
  };
  dense_block(a.D, a.xsrc, scale_fn, epi, xs);
}

__global__ __launch_bounds__(kTPB) void k_dense_p2(DenseDev D, const double* __restrict__ rec,
                                                   const double* __restrict__ xsrc,
                                                   const double* __restrict__ v_cur,
                                                   const double* __restrict__ v_prev,
                                                   double* __restrict__ v_next,
                                                   double* __restrict__ x,
                                                   double* __restrict__ Vcol, int j, int nflush) {
  __shared__ double xs[kDenseTile];
  const EpiPass2R epi = EpiPass2R::of(rec, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  dense_block(D, xsrc, UnitScale{}, epi, xs);
}

// ------------------------------------------------------------ host launchers
namespace launch {

static inline int dense_grid(const DenseDev& D) { return (D.n + kDenseRows - 1) / kDenseRows; }

hipError_t dense_spmv(const DenseDev& D, const double* x, double* y, hipStream_t s) {
  if (D.n > 0)
    hipLaunchKernelGGL(k_dense_spmv, dim3(dense_grid(D)), dim3(kTPB), 0, s, D, x, y);
  return hipGetLastError();
}
hipError_t dense_p1(const DenseDev& D, const CsrDev& A, const DevState& S, const double* xsrc,
                    const double* r_cur, const double* r_prev, double* W, double* Vcol, int j,
                    hipStream_t s, unsigned long long* stamp) {
  if (D.n <= 0) return hipGetLastError();
  DenseP1Args a{};
  a.Pb_r = S.Pb_r; a.flags = S.flags; a.norms = S.norms; a.betas = S.betas; a.Pa = S.Pa;
  a.xsrc = xsrc; a.r_cur = r_cur; a.r_prev = r_prev; a.W = W; a.Vcol = Vcol; a.stamp = stamp;
  a.D = D;
  a.j = j;
  a.G2_r = A.G2_r;
  hipLaunchKernelGGL(k_dense_p1, dim3(dense_grid(D)), dim3(kTPB), 0, s, a);
  return hipGetLastError();
}
hipError_t dense_p2(const DenseDev& D, const DevState& S, const double* xsrc, const double* v_cur,
                    const double* v_prev, double* v_next, double* x, double* Vcol, int j,
                    int nflush, hipStream_t s) {
  if (D.n > 0)
    hipLaunchKernelGGL(k_dense_p2, dim3(dense_grid(D)), dim3(kTPB), 0, s, D,
                       S.p2c + 8 * (size_t)j, xsrc, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
