// tpl_k_batch_p2_cached.hip — k_bp2_cached: a pass-two step of a batch group whose long
// rows read their NB sums from the group's long-row cache (tpl_op.h BatchBufs::d_ycache)
// instead of forming them again: the batch sibling of k_p2_cached (tpl_k_p2_cached.hip).
// Building blocks: tpl_kbatch.h. The map of the device sources in tpl_kernels.hip lists the
// other units (that file's text is what bench.py's kernel-source digest ties the committed
// profiles to, so it was left as it is); this one is named in tpl_batch.h and tpl_launch.h.
//
// Pass two regenerates pass one's basis bit for bit, per column, so the sums (A v_j)_r that
// k_bp2_spmv forms for a long row r at step j are the words k_bp1_spmv formed at step j of
// the group's pass one (the same products, piece, slice and slot order). With the cache on
// for the calling solver (tpl_op_set_long_cache_solvers), that pass one keeps them
// (BEpiPass1::long_y: n_long x NB doubles per step, a row's NB sums adjacent), and the pass
// two of the same call runs this kernel for every step the cache holds: no bins, no
// gathers of the long rows' columns, no LDS staging, no per-column barrier triples, no
// hand-off — the short chunks as k_bp2_spmv runs them, plus one thread per long row.
//
// A column that stopped before step j wrote nothing into the step's row: the word it reads
// is whatever an earlier solve (or the allocation's zero fill) left, and, as everywhere in
// the batch kernels, it flows through the arithmetic and is never stored.
//
// Used by tpl_lanczos_two_pass_batch and tpl_lanczos_two_pass_batch_multi alone
// (launch_bp2_step, tpl_passes.cpp); the stand-alone batch pass twos run k_bp2_spmv.
#include "tpl_kbatch.h"
#include "tpl_launch.h"

namespace tpl {

// keep() for the NB values of a row (tpl_kcommon.h): pinned as loaded ahead of a branch
template <int NB>
__device__ __forceinline__ void keep_nb(VecNB<NB>& v) {
#pragma unroll
  for (int c = 0; c < NB; ++c) keep(v.v[c]);
}

// BEpiPass2 (tpl_kbatch.h) with the step's NB records held lane-wise, field f of column c
// on lane 8 c + f of one VGPR pair, and read with readlane where a row's epilogue uses
// them (as EpiPass2R does for the single kernels): operation for operation BEpiPass2's
// apply, so the rows get the same bits. Held as 8 NB uniform doubles the records alone take
// 64 SGPRs at NB = 4 and the compiler spills them into VGPR lanes (k_bp2_spmv<4, FMT>:
// DESIGN.md §6.1); here only the three group-wide masks stay in SGPRs.
template <int NB>
struct BEpiPass2L {
  static_assert(8 * NB <= 64, "the records fit one wave's lanes");
  const double* v_cur;
  const double* v_prev;  // == v_cur (never used) at j == 1
  bool has_prev;
  double cv;             // lane l < 8 NB: rec[l]
  bool all_active, all_flush, any_flush;
  double* v_next;
  double* x;
  // after cv is loaded (every lane of every wave: rec[lane % (8 NB)])
  __device__ __forceinline__ void set_masks() {
    all_active = all_flush = true;
    any_flush = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const bool active = readlane_f64(cv, 8 * c + 6) != 0.0;
      const bool flush = active && readlane_f64(cv, 8 * c + 7) != 0.0;
      all_active = all_active && active;
      all_flush = all_flush && flush;
      any_flush = any_flush || flush;
    }
  }
  __device__ __forceinline__ BPre2<NB> pre(int i) const {
    return BPre2<NB>{ld_nb<NB>(v_cur, i), ld_nb<NB>(v_prev, i),
                     any_flush ? ld_nb<NB>(x, i) : VecNB<NB>{}};
  }
  __device__ __forceinline__ void apply(int i, const double (&s)[NB], const BPre2<NB>& p,
                                        double (&)[NB]) const {
    double vn[NB], xn[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      // read from cv itself, which every lane loaded at the kernel's entry: apply runs under
      // the row's live mask, and a copy made here would not be written on the lanes the
      // fields are read from
      const double r = cv;
      const double vp = has_prev ? p.vp.v[c] : 0.0;
      double w = s[c] - readlane_f64(r, 8 * c) * vp;
      w = w - readlane_f64(r, 8 * c + 1) * p.vc.v[c];
      vn[c] = w * readlane_f64(r, 8 * c + 2);
      const int nflush = (int)readlane_f64(r, 8 * c + 7);
      double xv = p.x.v[c];
      if (nflush >= 3) xv = xv + readlane_f64(r, 8 * c + 5) * p.vp.v[c];
      if (nflush >= 2) xv = xv + readlane_f64(r, 8 * c + 4) * p.vc.v[c];
      xn[c] = xv + readlane_f64(r, 8 * c + 3) * vn[c];
      // one column's fields at a time: scheduled together, the four columns' fields are 48
      // SGPRs in flight beside the chunk's own
      __builtin_amdgcn_sched_barrier(0);
    }
    // st_nb's stores; the per-column masks are formed only where a column has stopped
    if (all_active) {
      double2* q = reinterpret_cast<double2*>(v_next + (int64_t)i * NB);
#pragma unroll
      for (int h = 0; h < NB / 2; ++h) q[h] = double2{vn[2 * h], vn[2 * h + 1]};
    } else {
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (readlane_f64(cv, 8 * c + 6) != 0.0) v_next[(int64_t)i * NB + c] = vn[c];
    }
    if (!any_flush) return;
    if (all_flush) {
      double2* q = reinterpret_cast<double2*>(x + (int64_t)i * NB);
#pragma unroll
      for (int h = 0; h < NB / 2; ++h) q[h] = double2{xn[2 * h], xn[2 * h + 1]};
    } else {
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (readlane_f64(cv, 8 * c + 6) != 0.0 && readlane_f64(cv, 8 * c + 7) != 0.0)
          x[(int64_t)i * NB + c] = xn[c];
    }
  }
};

// Grid: [ceil(n_long / 256) long-row workgroups][chunk part]; A.n_slice_blocks holds the
// former count (launch::bp2_cached sets it), so chunk_of_block places the chunks on the XCDs
// of their row blocks as in every other kernel. rec: the step's NB records (BatchDev::p2c).
// ycrow: the step's cache row. Long row l is row lrow[l]; lrow == nullptr: the long rows
// are the last rows (s_identity), row n - n_long + l. FMT: kBFmtVal8 | kBFmtSCol16 (the
// chunk path's formats; the bins' column format is not read). No dynamic LDS.
template <int NB, int FMT>
__global__ __launch_bounds__(kTPB) void k_bp2_cached(CsrDev A, const double* __restrict__ rec,
                                                     const double* __restrict__ v_cur,
                                                     const double* __restrict__ v_prev,
                                                     double* __restrict__ v_next,
                                                     double* __restrict__ x,
                                                     const double* __restrict__ ycrow,
                                                     const int32_t* __restrict__ lrow, int j) {
  BEpiPass2L<NB> epi;
  epi.v_cur = v_cur;
  epi.v_prev = (j >= 2) ? v_prev : v_cur;
  epi.has_prev = j >= 2;
  epi.v_next = v_next;
  epi.x = x;
  // on every lane of every wave, here, where all of them are live (pinned as loaded: the
  // fields are read with readlane from lanes that a row's live mask may have switched off)
  epi.cv = rec[threadIdx.x & (8 * NB - 1)];
  keep(epi.cv);
  epi.set_masks();
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  const int b = blockIdx.x;
  if (b < A.n_slice_blocks) {
    // one thread per long row: its sums and its own entries, clamped and masked afterwards,
    // so the last wave's loads are issued ahead of the test like every other wave's
    const int l = b * kTPB + threadIdx.x;
    const int lc = clampi(l, A.n_long - 1);
    int row = (int)(A.n - A.n_long) + lc;
    VecNB<NB> y = ld_nb<NB>(ycrow, lc);
    if (lrow) row = lrow[lc];  // uniform; one more round trip ahead of the row's own entries
    BPre2<NB> pre = epi.pre(row);
    keep_nb<NB>(y);
    keep_nb<NB>(pre.vc);
    keep_nb<NB>(pre.vp);
    keep_nb<NB>(pre.x);
    if (l < A.n_long) epi.apply(row, y.v, pre, acc);
    return;
  }
  const int chunk = chunk_of_block(A, b - A.n_slice_blocks);
  if (chunk < 0) return;  // grid padding
  auto unit = [](double (&sc)[NB]) -> bool {
#pragma unroll
    for (int c = 0; c < NB; ++c) sc[c] = 1.0;
    return true;
  };
  b_short_chunk<NB, (FMT & kBFmtVal8) != 0, (FMT & kBFmtSCol16) != 0>(A, chunk, v_cur, unit, epi,
                                                                     acc);
}

namespace launch {

hipError_t bp2_cached(int nb, const CsrDev& A0, const BatchDev& B, const double* v_cur,
                      const double* v_prev, double* v_next, double* x, const double* ycrow,
                      const int32_t* lrow, int j, hipStream_t s) {
  CsrDev A = A0;
  A.n_slice_blocks = (A.n_long + kTPB - 1) / kTPB;
  if (A.n_long <= 0 || !ycrow || (!lrow && !A.s_identity)) return hipErrorInvalidConfiguration;
  const double* rec = B.p2c + 8 * (size_t)j * nb;
  TPL_NB_SWITCH(nb, return dispatch_fmt(
                        batch_fmt_of(A) & ~kBFmtBCol16,
                        [&](auto F) {
                          hipLaunchKernelGGL((k_bp2_cached<NB, decltype(F)::value>),
                                             dim3(spmv_grid(A)), dim3(kTPB), 0, s, A, rec, v_cur,
                                             v_prev, v_next, x, ycrow, lrow, j);
                        },
                        std::make_integer_sequence<int, kBFmtBCol16>{}));
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
