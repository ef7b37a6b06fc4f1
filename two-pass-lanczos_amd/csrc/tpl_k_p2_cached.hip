// tpl_k_p2_cached.hip — k_p2_cached: a pass-two step whose long rows read their sums from
// the long-row cache (tpl_op.h SolverState::d_ycache) instead of forming them again. Map of
// the device sources: tpl_kernels.hip.
//
// Pass two regenerates pass one's basis bit for bit, so the sum y_r = (A v_j)_r k_p2_spmv
// forms for a long row r at step j has the operands, and the piece, slice and slot order,
// of the one k_p1_spmv formed at step j of pass one. The two-pass solver's pass one keeps
// those sums (EpiPass1::long_y: n_long doubles per step), and its pass two runs this kernel
// for every step the cache holds: no bins, no gathered lines, no LDS piece sums, no
// hand-off — the short chunks as k_p2_spmv runs them, plus one thread per long row.
//
// Used by the two-pass solvers in the operator's solver mask (tpl_op_set_long_cache_solvers:
// tpl_lanczos_two_pass by default; tpl_lanczos_two_pass_multi, at nflush = 0, and the
// remainder column of a batch solve on request) through launch_p2_step (tpl_passes.cpp), for
// the pass two that follows the pass one which filled the rows. Never by the stand-alone
// tpl_lanczos_pass_two (with or without _multi) or a partitioned operator: they run
// k_p2_spmv. A batch group's sibling: k_bp2_cached (tpl_k_batch_p2_cached.hip).
#include "tpl_klaunch.h"

namespace tpl {

// The instances: the format bits the chunk path reads (the bins' column format is not one).
constexpr bool cached_variant_exists(int F) { return variant_exists(F) && !(F & kVarBCol16); }

// Grid: [ceil(n_long / 256) long-row workgroups][chunk part]; A.n_slice_blocks holds the
// former count (launch::p2_cached sets it), so chunk_of_block places the chunks on the XCDs
// of their row blocks as in every other kernel. The long rows go first: they are not the
// tail. ycache: the step's cache row. Long row l is row lrow[l]; lrow == nullptr: the long
// rows are the last rows (s_identity: the locality order, the headline), row n - n_long + l.
template <int F>
__global__ __launch_bounds__(kTPB, kSpmvMinWaves) void k_p2_cached(
    CsrDev A, const double* __restrict__ rec, const double* __restrict__ xsrc,
    const double* __restrict__ v_cur, const double* __restrict__ v_prev,
    double* __restrict__ v_next, double* __restrict__ x, double* __restrict__ Vcol,
    const double* __restrict__ ycache, const int32_t* __restrict__ lrow, int j, int nflush) {
  extern __shared__ double lds[];
  // every argument either path reads, in the entry batch of scalar loads (pin_layout_args)
  asm volatile("" ::"s"(A.s_col), "s"(A.s_val), "s"(A.s_cbase), "s"(A.srows), "s"(A.n_short),
               "s"(A.n_slice_blocks), "s"(A.s_identity), "s"(A.n_chunks), "s"(A.n_long),
               "s"(A.n), "s"(A.E), "s"(A.G2));
  if constexpr ((F & kVarWidth) == 0)
    asm volatile("" ::"s"(A.c_base), "s"(A.c_width), "s"(A.s_width));
  if constexpr ((F & kVarWin) != 0) asm volatile("" ::"s"(A.s_win), "s"(A.s_win_max));
  asm volatile("" ::"s"(rec), "s"(xsrc), "s"(v_cur), "s"(v_prev), "s"(v_next), "s"(x), "s"(Vcol),
               "s"(ycache), "s"(lrow), "s"(j), "s"(nflush));
  const EpiPass2R epi = EpiPass2R::of(rec, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  double acc = 0.0;
  const int b = blockIdx.x;
  if (b < A.n_slice_blocks) {
    // as k_long_epi_p2 with the all-gathered partials: the record lane-wise with the row's
    // own entries, nothing scalar before the vector loads (clamped, masked afterwards)
    const int l = b * kTPB + threadIdx.x;
    const int lc = clampi(l, A.n_long - 1);
    int row = (int)(A.n - A.n_long) + lc;
    double y = ycache[lc];
    if (lrow) row = lrow[lc];  // uniform; one more round trip ahead of the row's own entries
    Pre2R pre = epi.pre(row);
    // pinned as loaded on every lane: apply reads the record from lanes 0-7 of the wave
    // (readlane), and in the last wave those may lie past n_long — sunk into the branch
    // below, their loads would not be made
    keep(y);
    keep_pre(pre);
    if (l < A.n_long) epi.apply(row, y, pre, acc);
    return;
  }
  const int chunk = chunk_of_block(A, b - A.n_slice_blocks);
  if (chunk < 0) return;  // grid padding
  short_chunk<(F & kVarWidth), (F & kVarVal8) != 0, (F & kVarSCol16) != 0, (F & kVarWin) != 0>(
      A, chunk, xsrc, UnitScale{}, epi, acc, lds);
}

namespace launch {

hipError_t p2_cached(const CsrDev& A0, const DevState& S, const double* xsrc, const double* v_cur,
                     const double* v_prev, double* v_next, double* x, double* Vcol,
                     const double* ycache, const int32_t* lrow, int j, int nflush,
                     hipStream_t s) {
  CsrDev A = A0;
  A.n_slice_blocks = (A.n_long + kTPB - 1) / kTPB;
  if (A.n_long <= 0 || (!lrow && !A.s_identity)) return hipErrorInvalidConfiguration;
  // dynamic LDS: what a chunk needs (its column window), not a bin's staged products
  const size_t lds = (size_t)A.s_win * sizeof(double);
  const double* rec = S.p2c + 8 * (size_t)j;
  return dispatch_variant(
      variant_of(A) & ~kVarBCol16,
      [&](auto F) {
        if constexpr (cached_variant_exists(decltype(F)::value))
          hipLaunchKernelGGL(k_p2_cached<decltype(F)::value>, dim3(spmv_grid(A)), dim3(kTPB), lds,
                             s, A, rec, xsrc, v_cur, v_prev, v_next, x, Vcol, ycache, lrow, j,
                             nflush);
      },
      std::make_integer_sequence<int, kVarEnd>{});
}

} // namespace launch
} // namespace tpl
