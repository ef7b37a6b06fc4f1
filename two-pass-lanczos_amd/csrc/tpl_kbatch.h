// tpl_kbatch.h — device building blocks of the batch kernels (tpl_k_batch_p1.hip,
// tpl_k_batch_p2.hip): NB Lanczos recurrences in lock-step over one operator. Included only
// by .hip files; the single-column blocks of tpl_kcommon.h are used as they are and none
// of them is templated on NB, so no existing kernel's code changes.
//
// Every block performs, per column, exactly the operations of its single-column sibling
// in their order (the canonical order of tpl_device.h): products a * (x * scale) with
// padding adding -0.0, row sums in entry order, piece sums by 8- / 16-lane groups with the
// fixed butterflies, slice partials summed s = 0..S-1 from +0.0, tree256 for every block
// total. What the columns share is the matrix: its entries, column indices and the bin
// table are read once per workgroup, and each column index costs one address.
//
// A column that has stopped still flows through the arithmetic, in
// registers of its own, and stores nothing: neither vectors, nor partials, nor scalars.
// A launch returns early (grid-uniformly) only when every column of the group has stopped.
//
// The instances are specialised on NB and on the storage formats (kBFmt*); the chunk
// width is chosen by a uniform branch inside the kernel (widths 1..4 unrolled, packed or
// not; any other width by the batched loop), so every layout build_layout can produce is
// served by one of 2 x 8 instances per kernel. The LDS column window (kVarWin) is not
// used: the gathers read global memory, which gives the same bits.
#pragma once
#include "tpl_batch.h"
#include "tpl_klaunch.h"

namespace tpl {

constexpr int kBFmtVal8 = 1, kBFmtSCol16 = 2, kBFmtBCol16 = 4, kBFmtEnd = 8;
inline int batch_fmt_of(const CsrDev& A) {
  return (A.val_i8 ? kBFmtVal8 : 0) | (A.s_col16 ? kBFmtSCol16 : 0) | (A.b_col16 ? kBFmtBCol16 : 0);
}

namespace launch {
// CALL with NB a constant expression equal to nb, for the group widths that have instances.
#define TPL_NB_SWITCH(nb, CALL)                       \
  switch (nb) {                                       \
    case 2: { constexpr int NB = 2; CALL; } break;    \
    case 4: { constexpr int NB = 4; CALL; } break;    \
    default: return hipErrorInvalidConfiguration;     \
  }
// launch_f(std::integral_constant<int, FMT>) for the FMT equal to f (kBFmt*);
// hipErrorInvalidConfiguration when f has no instance, else the launch's status (as
// dispatch_variant, tpl_klaunch.h).
template <class LaunchF, int... Fs>
hipError_t dispatch_fmt(int f, LaunchF launch_f, std::integer_sequence<int, Fs...>) {
  return ((f == Fs ? (launch_f(std::integral_constant<int, Fs>{}), true) : false) || ...)
             ? hipGetLastError()
             : hipErrorInvalidConfiguration;
}
} // namespace launch

template <int NB>
struct VecNB {
  double v[NB];
};
// The NB adjacent values of row i of an interleaved vector: 16-B loads.
template <int NB>
__device__ __forceinline__ VecNB<NB> ld_nb(const double* __restrict__ p, int64_t i) {
  static_assert(NB % 2 == 0, "whole 16-B loads");
  VecNB<NB> r;
  const double2* q = reinterpret_cast<const double2*>(p + i * NB);
#pragma unroll
  for (int h = 0; h < NB / 2; ++h) {
    const double2 d = q[h];
    r.v[2 * h] = d.x;
    r.v[2 * h + 1] = d.y;
  }
  return r;
}

// Row i of an interleaved vector out. Every column live (the common case): 16-B stores of
// adjacent columns; otherwise only the live columns, one 8-B store each. (The single
// kernels' write-through 8-B stores would hit every 32-B sector of a row four times here.)
template <int NB>
__device__ __forceinline__ void st_nb(double* __restrict__ p, int64_t i, const double (&v)[NB],
                                      const bool (&on)[NB], bool all_on) {
  if (all_on) {
    double2* q = reinterpret_cast<double2*>(p + i * NB);
#pragma unroll
    for (int h = 0; h < NB / 2; ++h) q[h] = double2{v[2 * h], v[2 * h + 1]};
  } else {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (on[c]) p[i * NB + c] = v[c];
  }
}

// tree256 of NB values at once: one barrier pair for all columns. red: 4 NB doubles.
template <int NB>
__device__ __forceinline__ void block_sum_nb(double (&v)[NB], double* red) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    v[c] = wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) red[4 * c + w] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NB; ++c)
    v[c] = (red[4 * c] + red[4 * c + 1]) + (red[4 * c + 2] + red[4 * c + 3]);
  __syncthreads();
}

// partials(P_c[N]) for every column (P_c = P + c ld): thread t: s = 0; s += P_c[t + 256 q],
// q ascending; tree256. In two halves, as load_partials / finish_partials: the first U
// loads per column are issued early (clamped, masked after), ahead of the loads whose
// latency the reduction should hide behind; the rest (rare) in batches of U.
template <int NB, int U>
struct ColPartialRegs {
  double t[U][NB];
};
template <int NB, int U>
__device__ __forceinline__ void load_col_partials(const double* __restrict__ P, int ld, int N,
                                                  ColPartialRegs<NB, U>& r) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int c = 0; c < NB; ++c)
      r.t[u][c] = P[(size_t)c * ld + clampi((int)threadIdx.x + u * kTPB, N - 1)];
}
template <int NB, int U>
__device__ __forceinline__ void finish_col_partials(const double* __restrict__ P, int ld, int N,
                                                    const ColPartialRegs<NB, U>& r,
                                                    double (&s)[NB], double* red) {
#pragma unroll
  for (int c = 0; c < NB; ++c) s[c] = 0.0;
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if ((int)threadIdx.x + u * kTPB < N) s[c] = s[c] + r.t[u][c];
  for (int i0 = threadIdx.x + U * kTPB; i0 - (int)threadIdx.x < N; i0 += U * kTPB) {
    double t[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NB; ++c) t[u][c] = P[(size_t)c * ld + clampi(i0 + u * kTPB, N - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (i0 + u * kTPB < N) s[c] = s[c] + t[u][c];
  }
  block_sum_nb<NB>(s, red);
}

// x terms pass-two step j (1 .. last) applies: tpl_device.h p2_flush on the device.
__device__ __forceinline__ int bp2_flush(int j, int last) {
  return (j % 3 == 0 || j == last) ? j - ((j - 1) / 3) * 3 : 0;
}

// ----------------------------------------------------------- epilogues
// Pass one (EpiPass1 per column): w = y - beta_{j-1} v_{j-1}; alpha partial += v_j . w.
template <int NB>
struct BPre1 {
  VecNB<NB> rc, rp;
};
template <int NB>
struct BEpiPass1 {
  const double* r_cur;
  const double* r_prev;  // == r_cur (never used) at j == 1
  bool has_prev;
  // bit c: column c is alive at this step. One SGPR: as NB bools the columns' lane masks
  // were 2 NB of the SGPRs k_bp1_spmv<4, FMT> spilled into VGPR lanes
  unsigned alive;
  bool all_alive;
  double invN_cur[NB], invN_prev[NB], beta_sub[NB];
  double* W;
  double* Pa_long;  // column 0's long-row alpha partials (Pa + n_chunks)
  int na_ld;
  double* ycrow;    // this step's row of the group's long-row cache (n_long x NB), or nullptr
  __device__ __forceinline__ bool is_alive(int c) const { return (alive >> c) & 1u; }
  // st_nb with the live columns as bits: 16-B stores when every column is alive, 8-B stores
  // of the alive ones otherwise
  __device__ __forceinline__ void store(double* __restrict__ p, int64_t i,
                                        const double (&v)[NB]) const {
    if (all_alive) {
      double2* q = reinterpret_cast<double2*>(p + i * NB);
#pragma unroll
      for (int h = 0; h < NB / 2; ++h) q[h] = double2{v[2 * h], v[2 * h + 1]};
    } else {
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (is_alive(c)) p[i * NB + c] = v[c];
    }
  }
  __device__ __forceinline__ BPre1<NB> pre(int i) const {
    return BPre1<NB>{ld_nb<NB>(r_cur, i), ld_nb<NB>(r_prev, i)};
  }
  // Long row ri's finished sums, before its epilogue: kept for the pass two of the same
  // solve (k_bp2_cached reads them back; EpiPass1::long_y per column). Stored as the group
  // vectors are: the alive columns only, so a stopped column leaves the row's word as it was.
  __device__ __forceinline__ void long_y(int ri, const double (&y)[NB]) const {
    if (ycrow) store(ycrow, ri, y);
  }
  __device__ __forceinline__ void apply(int i, const double (&s)[NB], const BPre1<NB>& p,
                                        double (&acc)[NB]) const {
    double w[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const double v = p.rc.v[c] * invN_cur[c];
      const double vp = has_prev ? p.rp.v[c] * invN_prev[c] : 0.0;
      w[c] = s[c] - beta_sub[c] * vp;
      acc[c] = fma(v, w[c], acc[c]);
    }
    store(W, i, w);
  }
  __device__ __forceinline__ void long_alpha(int r, const double (&acc)[NB]) const {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (is_alive(c)) st_out(Pa_long + (size_t)c * na_ld + r, acc[c]);
  }
};

// Pass two (EpiPass2R per column), the step's records in registers: rec[c] = {beta_{j-1},
// alpha_j, 1/beta_j, y_j, y_{j-1}, y_{j-2}, active, nflush}. Each column applies its own
// grouped flush: the one the single solve applies for steps_c.
template <int NB>
struct BPre2 {
  VecNB<NB> vc, vp, x;
};
template <int NB>
struct BEpiPass2 {
  const double* v_cur;
  const double* v_prev;  // == v_cur (never used) at j == 1
  bool has_prev;
  double rec[NB][8];
  bool active[NB], flush[NB];   // column c stores v_{j+1} / x at this step
  bool all_active, all_flush, any_flush;
  double* v_next;
  double* x;
  // after rec is filled
  __device__ __forceinline__ void set_masks() {
    all_active = all_flush = true;
    any_flush = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      active[c] = rec[c][6] != 0.0;
      flush[c] = active[c] && rec[c][7] != 0.0;
      all_active = all_active && active[c];
      all_flush = all_flush && flush[c];
      any_flush = any_flush || flush[c];
    }
  }
  __device__ __forceinline__ BPre2<NB> pre(int i) const {
    // x is read only by a step at which some column flushes (uniform): one step in three
    return BPre2<NB>{ld_nb<NB>(v_cur, i), ld_nb<NB>(v_prev, i),
                     any_flush ? ld_nb<NB>(x, i) : VecNB<NB>{}};
  }
  __device__ __forceinline__ void apply(int i, const double (&s)[NB], const BPre2<NB>& p,
                                        double (&)[NB]) const {
    double vn[NB], xn[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {  // a column past its steps_taken computes and stores nothing
      const double vp = has_prev ? p.vp.v[c] : 0.0;
      double w = s[c] - rec[c][0] * vp;
      w = w - rec[c][1] * p.vc.v[c];
      vn[c] = w * rec[c][2];
      const int nflush = (int)rec[c][7];
      double xv = p.x.v[c];
      if (nflush >= 3) xv = xv + rec[c][5] * p.vp.v[c];
      if (nflush >= 2) xv = xv + rec[c][4] * p.vc.v[c];
      xn[c] = xv + rec[c][3] * vn[c];
    }
    st_nb<NB>(v_next, i, vn, active, all_active);
    if (any_flush) st_nb<NB>(x, i, xn, flush, all_flush);
  }
  __device__ __forceinline__ void long_alpha(int, const double (&)[NB]) const {}
  __device__ __forceinline__ void long_y(int, const double (&)[NB]) const {}
};

// ------------------------------------------------------ short rows (sliced ELL)
// Chunk of compile-time width W (short_chunk_w per column): the entries once, one gather
// address per entry for all columns. scale_of(sc) fills the columns' gather scales and the
// epilogue, and returns whether any column is live.
template <int NB, int W, int V8, int C16, bool PK, class Epi, class ScaleFn>
__device__ __forceinline__ bool b_short_chunk_w(const CsrDev& A, int chunk, int base,
                                                const double* __restrict__ xsrc,
                                                ScaleFn scale_of, const Epi& epi,
                                                double (&acc)[NB]) {
  const int t = threadIdx.x;
  const int cbase = C16 ? A.s_cbase[chunk] : 0;
  int row[kRowsPerThread];
  bool live[kRowsPerThread];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    const int p = chunk * kChunkRows + q * kTPB + t;
    live[q] = p < A.n_short;
    const int pc = clampi(p, A.n_short - 1);
    row[q] = A.s_identity ? pc : A.srows[pc];
  }
  int c[kRowsPerThread][W];
  double a[kRowsPerThread][W];
  if constexpr (PK) {
    int cr[kRowsPerThread * W];
    double ar[kRowsPerThread * W];
    load_entry_run<kRowsPerThread * W, V8, C16>(A.s_col, A.s_val, base + t * kRowsPerThread * W,
                                                 cbase, cr, ar);
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q)
#pragma unroll
      for (int k = 0; k < W; ++k) {
        c[q][k] = cr[q * W + k];
        a[q][k] = ar[q * W + k];
      }
  } else {
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q)
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const int e = base + k * kChunkRows + q * kTPB + t;
        c[q][k] = col_at<C16>(A.s_col, e, cbase);
        a[q][k] = val_at<V8>(A.s_val, e);
      }
  }
  VecNB<NB> xv[kRowsPerThread][W];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q)
#pragma unroll
    for (int k = 0; k < W; ++k) xv[q][k] = ld_nb<NB>(xsrc, c[q][k] < 0 ? 0 : c[q][k]);
  decltype(epi.pre(0)) pre[kRowsPerThread];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) pre[q] = epi.pre(row[q]);
  double sc[NB];
  const bool any = scale_of(sc);
  if (!any) return false;  // every column stopped (uniform across the grid)
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    double sum[NB];
#pragma unroll
    for (int col = 0; col < NB; ++col) {
      sum[col] = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double prod = a[q][k] * (xv[q][k].v[col] * sc[col]);
        sum[col] = sum[col] + (c[q][k] >= 0 ? prod : -0.0);  // padding adds -0.0: exact
      }
    }
    if (live[q]) epi.apply(row[q], sum, pre[q], acc);
  }
  return true;
}

// Any width (short_chunk_any per column): one row position at a time, entries in batches
// of 4 with every load of a batch in flight.
template <int NB, int V8, int C16, class Epi, class ScaleFn>
__device__ __forceinline__ bool b_short_chunk_any(const CsrDev& A, int chunk, int base, int W,
                                                  const double* __restrict__ xsrc,
                                                  ScaleFn scale_of, const Epi& epi,
                                                  double (&acc)[NB]) {
  const int t = threadIdx.x;
  const int cbase = C16 ? A.s_cbase[chunk] : 0;
  double sc[NB];
  if (!scale_of(sc)) return false;
#pragma unroll 1
  for (int q = 0; q < kRowsPerThread; ++q) {
    const int p = chunk * kChunkRows + q * kTPB + t;
    const bool live = p < A.n_short;
    const int pc = clampi(p, A.n_short - 1);
    const int row = A.s_identity ? pc : A.srows[pc];
    const auto pre = epi.pre(row);
    double s[NB];
#pragma unroll
    for (int col = 0; col < NB; ++col) s[col] = 0.0;
#pragma unroll 1
    for (int k0 = 0; k0 < W; k0 += 4) {
      int c[4];
      double a[4];
      VecNB<NB> xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = base + clampi(k0 + u, W - 1) * kChunkRows + q * kTPB + t;
        c[u] = col_at<C16>(A.s_col, e, cbase);
        a[u] = val_at<V8>(A.s_val, e);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = ld_nb<NB>(xsrc, c[u] < 0 ? 0 : c[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int col = 0; col < NB; ++col) {
          const double prod = a[u] * (xv[u].v[col] * sc[col]);
          s[col] = s[col] + ((c[u] >= 0 && k0 + u < W) ? prod : -0.0);
        }
    }
    if (live) epi.apply(row, s, pre, acc);
  }
  return true;
}

// The chunk's width and entry order (uniform per workgroup): widths 1, 2 and 4 of a
// uniform-width layout are stored packed (tpl_device.h packed_chunk_width).
template <int NB, int V8, int C16, class Epi, class ScaleFn>
__device__ __forceinline__ bool b_short_chunk(const CsrDev& A, int chunk,
                                              const double* __restrict__ xsrc, ScaleFn scale_of,
                                              const Epi& epi, double (&acc)[NB]) {
  int W, base;
  if (A.s_width > 0) {
    W = A.s_width;
    base = chunk * kChunkRows * W;
  } else {
    W = A.c_width[chunk];
    base = A.c_base[chunk];
  }
  const bool pk = kPackedEntries && A.s_width > 0 && (W == 1 || W == 2 || W == 4);
#define TPL_BCHUNK(WW, PK) \
  b_short_chunk_w<NB, WW, V8, C16, PK>(A, chunk, base, xsrc, scale_of, epi, acc)
  switch (W) {
    case 1: return pk ? TPL_BCHUNK(1, true) : TPL_BCHUNK(1, false);
    case 2: return pk ? TPL_BCHUNK(2, true) : TPL_BCHUNK(2, false);
    case 3: return TPL_BCHUNK(3, false);
    case 4: return pk ? TPL_BCHUNK(4, true) : TPL_BCHUNK(4, false);
    default: return b_short_chunk_any<NB, V8, C16>(A, chunk, base, W, xsrc, scale_of, epi, acc);
  }
#undef TPL_BCHUNK
}

// ------------------------------------------------------ long rows (bins)
// The piece sums of one column's staged products (long_bin's wave tasks, operation for
// operation): big pieces (the first nbig) by 16-lane groups, the others by 8-lane groups.
__device__ __forceinline__ void b_piece_sums(const double* lds, const int* starts, double* psum,
                                             int npieces, int nbig) {
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tb = (nbig + 3) >> 2, ts = (npieces - nbig + 7) >> 3;
  for (int task = wv; task < tb + ts; task += kTPB / 64) {  // wave-uniform
    if (task < tb) {
      const int g16 = lane & 15;
      const int j = 4 * task + (lane >> 4);
      const bool valid = j < nbig;
      const int jc = valid ? j : 0;
      const int st = starts[jc], nx = starts[jc + 1];
      const int b0 = valid ? st : 0;
      const int en = valid ? (nx >= 0 ? nx : -1 - nx) : 0;
      int k = b0 + g16;
      const int cnt = k < en ? (en - k + 15) >> 4 : 0;
      double acc = 0.0;
      for (int q = 0; q < cnt; ++q, k += 16) acc = acc + lds[k];
      acc = group16_sum(acc);
      if (g16 == 0 && valid) psum[j] = acc;
    } else {
      const int g8 = lane & 7;
      const int j = nbig + 8 * (task - tb) + (lane >> 3);
      const int jc = j < kTPB - 2 ? j : kTPB - 2;
      const int st = starts[jc], nx = starts[jc + 1];
      const bool valid = j < npieces;
      const int b0 = valid ? st : 0;
      const int en = valid ? (nx >= 0 ? nx : -1 - nx) : 0;
      double acc = 0.0;
      for (int k0 = b0 + g8; k0 < en; k0 += 64) {  // 8 reads in flight, then the adds
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = lds[k0 + 8 * u < en ? k0 + 8 * u : k0];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + (k0 + 8 * u < en ? v[u] : -0.0);
      }
      acc = group8_sum(acc);
      if (g8 == 0 && valid) psum[j] = acc;
    }
  }
}

// Bin m of slice s for NB columns. The bin table and the first load batch's entries and
// gathers (NB values per column index) are read once and held in registers; the columns are
// then staged ONE AT A TIME through the
// bin's LDS (bin_cap products, the piece starts, kTPB piece sums: exactly the single
// kernel's allocation, whatever NB and bin_cap), each piece's NB sums ending up in the
// registers of the thread that owns the piece. The hand-off publishes the NB sums
// write-through into the batch's own slots, drains them, makes ONE arrival increment on
// the batch's own counter, and the last arriver reads the S x NB slots and finishes the row
// for every column.
template <int NB, int V8, int C16, class Epi, class ScaleFn>
__device__ __forceinline__ void b_long_bin(const CsrDev& A, const BatchDev& B, int m, int s,
                                           const double* __restrict__ xsrc, ScaleFn scale_of,
                                           const Epi& epi, double* lds) {
  const int t = threadIdx.x;
  const int bin = __builtin_amdgcn_readfirstlane(m * A.n_slices + s);
  const int base = bin * A.bin_cap;
  const int cbase = C16 ? A.b_cbase[bin] : 0;
  const int hdr = A.b_hdr[bin];
  int c[kBinBatch];
  double a[kBinBatch];
  load_bin_batch<V8, C16>(A, base, cbase, c, a);
  const int npieces = hdr & 0xFFFF, nbig = hdr >> 16;
  const BinSeg sg = A.b_seg[bin * kTPB + (t < npieces ? t : npieces)];
  VecNB<NB> xv[kBinBatch];
#pragma unroll
  for (int u = 0; u < kBinBatch; ++u) xv[u] = ld_nb<NB>(xsrc, c[u] < 0 ? 0 : c[u]);
  const auto pre = epi.pre(sg.row < 0 ? 0 : sg.row);
  double sc[NB];
  if (!scale_of(sc)) return;  // every column stopped: slots and counters untouched
  int* starts = reinterpret_cast<int*>(lds + A.bin_cap);
  double* psum = lds + A.bin_cap + kTPB / 2;  // kTPB doubles after the starts
  starts[t] = sg.ri < 0 ? -1 - sg.start : sg.start;  // < 0: no piece (value encodes the fill)
  double p[NB];
#pragma unroll
  for (int col = 0; col < NB; ++col) {
#pragma unroll
    for (int u = 0; u < kBinBatch; ++u) lds[u * kTPB + t] = a[u] * (xv[u].v[col] * sc[col]);
    // wider bins (rare): the further batches do not fit registers across the column loop, so
    // their entries are re-read per column (from cache) and gathered 8 B at a time
    for (int u0 = kBinBatch * kTPB; u0 < A.bin_cap; u0 += kBinBatch * kTPB) {
      int c2[kBinBatch];
      double a2[kBinBatch], x2[kBinBatch];
      load_bin_batch<V8, C16>(A, base + u0, cbase, c2, a2);
#pragma unroll
      for (int u = 0; u < kBinBatch; ++u)
        x2[u] = xsrc[(int64_t)(c2[u] < 0 ? 0 : c2[u]) * NB + col];
#pragma unroll
      for (int u = 0; u < kBinBatch; ++u) lds[u0 + u * kTPB + t] = a2[u] * (x2[u] * sc[col]);
    }
    __syncthreads();
    b_piece_sums(lds, starts, psum, npieces, nbig);
    __syncthreads();
    p[col] = psum[t < npieces ? t : 0];
    __syncthreads();  // the next column restages the products and the piece sums
  }
  if (sg.ri < 0) return;  // no piece for this thread
  const int ns = A.n_slices;
  double y[NB];
  if (ns == 1 || sg.pad == 0) {  // the piece is the whole row: no hand-off
#pragma unroll
    for (int col = 0; col < NB; ++col) y[col] = 0.0 + p[col];
  } else {
    unsigned long long* rowslots =
        reinterpret_cast<unsigned long long*>(B.P + (size_t)sg.ri * kSlotStride * kBatchNbMax);
#pragma unroll
    for (int col = 0; col < NB; ++col)
      __hip_atomic_store(rowslots + (size_t)s * kBatchNbMax + col,
                         (unsigned long long)__double_as_longlong(p[col]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int arrived = __builtin_amdgcn_atomic_inc32(
        B.Pcnt + (size_t)sg.ri * kCntStride, (unsigned)sg.pad, __ATOMIC_RELAXED, "agent");
    asm volatile("" ::: "memory");  // the slot loads stay behind the returned increment
    if (arrived != (unsigned)sg.pad) return;
#pragma unroll
    for (int col = 0; col < NB; ++col) y[col] = 0.0;
#pragma unroll
    for (int k = 0; k < kSlices; ++k) {
      if (k < ns) {
#pragma unroll
        for (int col = 0; col < NB; ++col)
          y[col] = y[col] + __longlong_as_double((long long)__hip_atomic_load(
                                rowslots + (size_t)k * kBatchNbMax + col, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT));
      }
    }
  }
  double acc[NB];
#pragma unroll
  for (int col = 0; col < NB; ++col) acc[col] = 0.0;
  epi.long_y(sg.ri, y);
  epi.apply(sg.row, y, pre, acc);
  epi.long_alpha(sg.ri, acc);
}

// Grid as the single kernels' (spmv_block_impl): [bins of the long rows][short chunks].
// Returns the chunk whose alpha partials this workgroup owns, or -1.
template <int NB, int FMT, class Epi, class ScaleFn>
__device__ __forceinline__ int b_spmv_block(const CsrDev& A, const BatchDev& B,
                                            const double* __restrict__ xsrc, ScaleFn scale_of,
                                            const Epi& epi, double (&acc)[NB], double* lds) {
  const int b = blockIdx.x;
  if (b < A.n_slice_blocks) {
    int m, s;
    if (A.n_slices >= 8) {
      const int T = A.n_slices >> 3, q = b >> 3;
      s = T * (b & 7) + q % T;
      m = q / T;
    } else {
      m = b / A.n_slices;
      s = b % A.n_slices;
    }
    b_long_bin<NB, (FMT & kBFmtVal8) != 0, (FMT & kBFmtBCol16) != 0>(A, B, m, s, xsrc, scale_of,
                                                                     epi, lds);
    return -1;
  }
  const int chunk = chunk_of_block(A, b - A.n_slice_blocks);
  if (chunk < 0) return -1;  // grid padding
  return b_short_chunk<NB, (FMT & kBFmtVal8) != 0, (FMT & kBFmtSCol16) != 0>(A, chunk, xsrc,
                                                                            scale_of, epi, acc)
             ? chunk : -1;
}

// Dynamic LDS of the batch SpMV-shaped kernels: a bin's staged products of ONE column,
// the piece starts and the piece sums (the columns take turns): never more than the
// single-column kernels allocate for the same layout.
static inline size_t batch_lds_bytes(const CsrDev& A) {
  return A.n_slice_blocks > 0
             ? (size_t)A.bin_cap * sizeof(double) + kTPB * sizeof(int) + kTPB * sizeof(double)
             : 0;
}

} // namespace tpl
