// tpl_kernels.hip — CDNA4 (gfx950) kernels of the two-pass Lanczos engine: the
// single-GPU solves' step kernels (the ones bench.py measures) and their launchers.
//
// Map of the device sources (one compile unit per .hip; tpl_launch.h declares every
// launcher, the unit holding a kernel defines its launcher):
//   tpl_kernels.hip     k_p1_init, k_p1_spmv, k_p1_axpy, k_ftk_inv,
//                       k_p2_init, k_p2_coefs, k_p2_spmv, k_p2_tail, k_gemv_recon.
//                       k_ftk_inv stays beside k_p1_axpy: both inline lu_row, and apart
//                       k_p1_axpy's elimination branch compiles to other registers
//   tpl_k_p1_tol.hip    k_p1_axpy_tol, k_p1_tol_fin (pass one of the inverse solve that stops
//                       at a residual tolerance)
//   tpl_k_p1_stol.hip   k_p1_axpy_stol, k_p1_stol_fin, k_ftk_inv_shifts, k_p2_xacc_cut (the
//                       same for m shifts, each stopped on its own)
//   tpl_k_batch_stol.hip  k_bp1_axpy_stol, k_bp1_stol_fin, k_bp2_xacc_cut (and for the columns
//                       of a batch group)
//   tpl_klu.h, tpl_kstop.h  what those four units share, each written once: lu_row; div_rn;
//                       the stop's flag words, rule and vote; the shifted solves' elimination
//                       lane and fin wave. Still repeated, because one inlined function moves
//                       instructions of the instances that exist (the units' headers give the
//                       figures): the element parts of k_p1_axpy, _tol and _stol and of
//                       k_bp1_axpy and _stol, and the solve of k_ftk_inv and k_ftk_inv_shifts
//   tpl_k_p2_cached.hip k_p2_cached (the two-pass solver's pass-two step whose long rows read
//                       the sums its pass one kept: the long-row cache)
//   tpl_k_spmv.hip      k_spmv (the plain product), k_permute
//   tpl_k_p1_gp.hip     k_p1_spmv_gp   } the pass-one SpMV for gathered / for more than 256
//   tpl_k_p1_wide.hip   k_p1_spmv_wide } norm partials: partitioned and very large operators
//   tpl_k_ftk_exp.hip   k_ftk_exp
//   tpl_k_multi.hip     k_p2_minit, k_p2_xacc (multi-function pass two: the x updates of
//                       every column, with k_p2_spmv run at nflush = 0)
//   tpl_k_batch_p1.hip  k_b_interleave / _deinterleave, k_bp1_init, k_bp1_spmv, k_bp1_axpy } the
//   tpl_k_batch_p2.hip  k_bp2_init, k_bp2_coefs, k_bp2_spmv } lock-step batch solve: NB = 2 / 4
//                       columns per launch (building blocks: tpl_kbatch.h, state: tpl_batch.h)
//   tpl_k_batch_multi.hip  k_bp2_minit, k_bp2_coefs0, k_bp2_xacc, k_bm_deinterleave (m functions
//                       of every column of a group: the x updates, with k_bp2_spmv run at nflush = 0)
//   tpl_k_dense.hip     k_dense_spmv, k_dense_p1, k_dense_p2 (a dense operator's plain product,
//                       pass-one step and pass-two step: the matrix whole, no layout)
//   tpl_k_dist_reorth.hip  k_long_epi_p1 / _y / _p2 (partitioned solve) and k_reorth_dot /
//                       _reduce / _update / _decide: one unit, see its header
//   tpl_kcommon.h       device building blocks: reductions, epilogues, the sliced-ELL chunk,
//                       the long-row bin, spmv_block, the variant flag F (kVar*), and
//                       p1_spmv_body, the body the three k_p1_spmv* wrappers share
//   tpl_klaunch.h       host side of the launchers: grids, LDS sizes, the dispatch on F
//   tpl_device.h        the argument structs; tpl_lab.h: diagnostic stamps
// Each of the five SpMV-shaped templates has 56 instances (variant_exists): the units
// compile in parallel, and the headline's kernels rebuild without the other 224.
//
// One Lanczos step of the reference (src/algorithms/mod.rs:167-212 + :292-340)
//     w = A v_j ; w -= beta_{j-1} v_{j-1} ; alpha_j = v_j . w ; w -= alpha_j v_j ;
//     beta_j = ||w|| ; v_{j+1} = w * (1/beta_j)
// has two grid-wide dependencies (alpha before the second AXPY, beta before the
// next SpMV). Pass one therefore runs two launches per step:
//   k_p1_spmv  [reduce beta partials -> beta_{j-1}, breakdown test]
//              fused SpMV gathering x = r_j * (1/beta_{j-1}) (the normalisation
//              v_j = w/beta folded into the gather, bit-identical to storing v_j);
//              epilogue w = y - beta_{j-1} v_{j-1}; alpha partials
//   k_p1_axpy  [reduce alpha partials -> alpha_j] r_{j+1} = w - alpha_j v_j ;
//              ||r_{j+1}||^2 partials
// Pass two (src/algorithms/lanczos_two_pass.rs:176-312) knows every coefficient, so
// each step is ONE launch (k_p2_spmv): SpMV + both AXPYs + scale + x += y v.
//
// Arithmetic follows the reference op by op (-ffp-contract=off for this file):
//   sub(w, mul(beta, v)) -> w - beta*v (two roundings), v = w * (1/beta)
//   (reciprocal then multiply), x = x + y*v. Reductions use the FIXED trees of
//   tpl_device.h, so results are run-to-run bitwise reproducible and pass two
//   regenerates pass one's basis bit for bit (reference: basis_drift_fro = 0.0,
//   results/orthogonality_*.csv).
//
// Latency structure (measured on MI355X: a graph-launched empty kernel costs 1.6 us,
// and a dependent memory round trip 1-2 us once the chip is loaded): every
// workgroup issues its independent loads (stop flag, grid partials, entries,
// epilogue vectors) before its first wait. A short-row chunk costs two round trips
// (entries -> gathers); a long-row bin the same two plus an LDS pass, and the
// slice-7 bins one more (polling the other slices' partials).
#define TPL_LAB_TABLE 1  // this unit holds the stamp build's table (tpl_lab.h)
#include "tpl_klaunch.h"
#include "tpl_klu.h"
#include "tpl_kstop.h"

namespace tpl {

// ------------------------------------------------------------------ kernels
// Pass-one prologue: ||b||^2 partials, reset flags.
__global__ __launch_bounds__(kTPB) void k_p1_init(CsrDev A, DevState S,
                                                  const double* __restrict__ b) {
  __shared__ double red[4];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S.flags[0] = 0;
    S.flags[1] = 0;
    S.flags[2] = 0;
    S.flags[3] = 0;
    S.flags[4] = 0;
    S.flags[5] = 0;
  }
  const int rb = elem_block(A, blockIdx.x);
  if (rb < 0) return;
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  double acc = 0.0;
  for (int64_t i0 = beg + 2 * threadIdx.x; i0 < end; i0 += 2 * kTPB) {
    if (i0 + 1 < end) {
      const double2 v = *reinterpret_cast<const double2*>(b + i0);
      acc = i0 < A.norm_n ? fma(v.x, v.x, acc) : acc;
      acc = i0 + 1 < A.norm_n ? fma(v.y, v.y, acc) : acc;
    } else {
      const double v = b[i0];
      acc = i0 < A.norm_n ? fma(v, v, acc) : acc;
    }
  }
  const double p = block_sum_tail(acc, red);
  if (threadIdx.x == 0) S.Pb[rb] = p;
}

// The pass-one step's SpMV (p1_spmv_body, tpl_kcommon.h) for G2_r <= 256 norm partials,
// one per thread; k_p1_spmv_gp and k_p1_spmv_wide take the other cases.
template <int F>
__global__ __launch_bounds__(kTPB, p1_min_waves(F, 1)) void k_p1_spmv(P1SpmvArgs a) {
  TPL_MARK_FIRST();
  __shared__ double red[4], redb[4];
  extern __shared__ double lds[];
  p1_spmv_body<F, 1>(a, red, redb, lds);
}

// ---- T_k^{-1} e_1 on the device (the one-graph inv): the host solver's operations
// (tpl_ftk.cpp: the LAPACK dgtsv scheme, tridiagonal elimination with partial pivoting,
// then back substitution), bit for bit.
// (LuRow, lu_row: tpl_klu.h, shared with the elimination lanes of the tolerance stops.)
// (div_rn, the back substitution's division: tpl_kstop.h, shared with k_ftk_inv_shifts.)

// Pass one / standard, step j: alpha_j; r_{j+1} = w - alpha_j v_j; ||r_{j+1}||^2 partials.
// NP: alpha partials loaded per thread up front (the launcher picks the smallest of 2, 4,
// 8, 12 with 256 NP >= NA_r; more are reduced in batches): clamped duplicate loads of a
// small partial array only cost issue slots and cache traffic.
// elim (one-graph inv): one more workgroup eliminates row j - 3 of T_k's LU
// (lu_row): its inputs beta_{j-3}, alpha_{j-2} and beta_{j-2} (0-based) are all known
// once this step's k_p1_spmv has reduced beta — the row is done off the critical path,
// so only the last rows and the back substitution remain after pass one (k_ftk_inv).
// That workgroup is block a.elim_block, the one after the element grid (its padding
// blocks included, so never one elem_block maps to a row block or to -1); -1: none.
// k_p1_axpy_tol (tpl_k_p1_tol.hip) and k_p1_axpy_stol (tpl_k_p1_stol.hip) repeat this
// kernel's text with the tolerance stop added: a change to the body below belongs there too.
template <int NP>
__global__ __launch_bounds__(kTPB) void k_p1_axpy(P1AxpyArgs a) {
  __shared__ double red[4];
  // Every kernel argument the element blocks read is fetched by the entry batch of scalar
  // loads, before any branch on one of them: a test of the stamp pointer, of gridDim.x
  // (a hidden argument) or of G2 ahead of the vector loads each cost a dependent scalar
  // round trip (ISA; scripts/entry_trips.py checks the compiled code). Only the
  // elimination workgroup's own fields (lu, kcap, betas) load later, on its branch.
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
  unsigned long long* stamp = a.stamp;
  asm volatile("" ::"s"(A.E), "s"(A.n), "s"(A.norm_n), "s"(A.NA_r), "s"(A.G2), "s"(S.Pa_r),
               "s"(S.flags), "s"(S.norms), "s"(S.alphas), "s"(S.Pb));
  asm volatile("" ::"s"(W), "s"(r_cur), "s"(r_next), "s"(j), "s"(k), "s"(elim_block),
               "s"(stamp));
  launch_stamp(stamp);
  if ((int)blockIdx.x == elim_block) {
    if (threadIdx.x != 0 || j < 3) return;
    const int i = j - 3;
    const size_t kcap = (size_t)a.kcap;
    double* D = a.lu;
    double* st = a.lu + 4 * kcap;
    // every input with the flags (one round trip): the row's coefficients and the running
    // row (the initial one at i = 0: alpha_0, beta_0, 1)
    const int stop = S.flags[0], done = S.flags[5];
    const double dli = a.betas[i], d1 = S.alphas[i + 1], du1 = a.betas[i + 1];
    LuRow cur{st[0], st[1], st[2]};
    const double a0 = S.alphas[0];
    if (stop || done != i) return;  // breakdown at this step: the tail finishes the rows
    if (i == 0) cur = LuRow{a0, dli, 1.0};
    lu_row(i, true, dli, d1, du1, cur, D, D + kcap, D + 2 * kcap, D + 3 * kcap);
    st[0] = cur.d;
    st[1] = cur.du;
    st[2] = cur.b;
    S.flags[5] = i + 1;
    return;
  }
  const int rb = elem_block(A.G2, blockIdx.x);
  if (rb < 0) return;
  TPL_MARK_AT(kAxpyMarkBase, 0);
  // The DevState scalars (stop flag, ||r_j||) are the first loads issued (vector loads at a
  // uniform address: no scalar round trip), so that 1 / ||r_j|| can be taken while the
  // alpha partials and the vectors are still in flight (below).
  const int stop = S.flags[0];
  const double normj = S.norms[j - 1];
  __builtin_amdgcn_sched_barrier(0);
  PartialRegs<NP> pr;
  const int na_ = A.NA_r;
  load_partials(S.Pa_r, na_, pr);
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  // All of this thread's pairs (up to kAxPairs) are loaded before alpha is known, at
  // clamped addresses (vectors are padded to 64 doubles, so a pair starting below
  // `end` is always readable); the loads are unconditional so none is sunk behind the
  // reduction.
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
  // 1 / ||r_j|| now, off the chain that follows alpha: the division is about ten
  // dependent FP64 operations, and its wait (vmcnt counts down in issue order) covers the
  // two loads above only, not the partials or the vectors. Same operation, same operand:
  // the same bits as dividing after the reduction (same box, alternated three times: solve
  // 8.04 vs 8.13-8.15 ms, pass one 9.99-10.03 vs 10.22-10.29 us per step).
  __builtin_amdgcn_sched_barrier(0);
  TPL_MARK_AT(kAxpyMarkBase, 1);
  double invN = 1.0 / normj;
  keep(invN);
  __builtin_amdgcn_sched_barrier(0);
#if TPL_STAMP
  // diagnostic build: when the alpha partials (issued first) have landed, the vector loads
  // (2 kAxPairs issued after them) still in flight
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  TPL_MARK_AT(kAxpyMarkBase, 4);
#endif
  // alpha while the vectors are in flight: its wait covers the partials (issued first)
  // only. The reduction's LDS stores and barrier keep the vector loads ahead of it, and
  // nothing tests the (uniform) stop flag before it: a branch there would let the compiler
  // sink the loads into it, behind the reduction.
  const double alpha = finish_partials(S.Pa_r, na_, pr, red);
  TPL_MARK_AT(kAxpyMarkBase, 2);
  if (stop) return;
  if (rb == 0 && threadIdx.x == 0) {
    S.alphas[j - 1] = alpha;
    S.flags[2] = j;
  }
  if (j == k) return; // beta_k is never used (src/algorithms/lanczos_two_pass.rs:252-254)
  double acc = 0.0;
  auto step = [&](int64_t i0, double2 w, double2 rc) {
    double2 r;
    r.x = w.x - alpha * (rc.x * invN);
    r.y = w.y - alpha * (rc.y * invN);
    // 16-B non-temporal stores: r_{j+1} leaves the L2 during the kernel instead of as
    // 4 MB of dirty lines at the boundary (same box, alternated twice: pass one 12.16-12.22
    // vs 12.33 us per step with plain 16-B stores; write-through +0.5 us)
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
  TPL_MARK_AT(kAxpyMarkBase, 3);
  const double p = block_sum_tail(acc, red);
  if (threadIdx.x == 0) S.Pb[rb] = p;  // plain: write-through measured +0.35 us here
  TPL_MARK_AT(kAxpyMarkBase, 5);
}

// Pass two prologue: v_1 = b * (1/||b||); x = v_1 * y_1 (src/algorithms/lanczos_two_pass.rs:248-252).
// dyn: steps_taken is known only on the device (one-graph solve): nothing to do after
// an error (zero b) or when pass one took no step.
__global__ __launch_bounds__(kTPB) void k_p2_init(int64_t n, DevState S,
                                                  const double* __restrict__ b,
                                                  double* __restrict__ v1,
                                                  double* __restrict__ x,
                                                  double* __restrict__ Vcol, int dyn) {
  if (dyn && (S.flags[1] || S.flags[2] < 1)) return;
  const double invN = 1.0 / S.norms[0];
  const double y0 = S.y[0];
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    const double v = b[i] * invN;
    v1[i] = v;
    x[i] = v * y0;
    if (Vcol) Vcol[i] = v;
  }
}

// Pass two, step j = 1 .. steps-1: regenerate v_{j+1}, accumulate x. rec: step j's
// coefficient record (EpiPass2R: loaded after the gathers, never waited on before the
// epilogue; the gather scale is 1).
template <int F>
__global__ __launch_bounds__(kTPB, kSpmvMinWaves) void k_p2_spmv(CsrDev A,
                                                  const double* __restrict__ rec,
                                                  const double* __restrict__ xsrc,
                                                  const double* __restrict__ v_cur,
                                                  const double* __restrict__ v_prev,
                                                  double* __restrict__ v_next,
                                                  double* __restrict__ x,
                                                  double* __restrict__ Vcol, int j,
                                                  int nflush) {
  extern __shared__ double lds[];
  pin_layout_args(A);
  asm volatile("" ::"s"(rec), "s"(xsrc), "s"(v_cur), "s"(v_prev), "s"(v_next), "s"(x), "s"(Vcol),
               "s"(j), "s"(nflush));
  const EpiPass2R epi = EpiPass2R::of(rec, v_cur, v_prev, v_next, x, Vcol, j, nflush);
  double acc = 0.0;
  spmv_block<F>(A, xsrc, UnitScale{}, epi, acc, lds);
}

// Pass-two step records (EpiPass2R): record j (1 <= j < k) = {beta_{j-1} (0 at j = 1),
// alpha_j, 1 / beta_j, y_j, y_{j-1}, y_{j-2} (0 at j = 1), active, 0}. dyn (one-graph
// solve): active = j < steps_taken (the device-held count), else 1.
__global__ __launch_bounds__(kTPB) void k_p2_coefs(DevState S, int k, int dyn) {
  const int j = blockIdx.x * kTPB + threadIdx.x;
  if (j < 1 || j >= k) return;
  double* r = S.p2c + 8 * (size_t)j;
  double2 r01, r23, r45, r67;
  r01.x = j >= 2 ? S.betas[j - 2] : 0.0;
  r01.y = S.alphas[j - 1];
  r23.x = 1.0 / S.betas[j - 1];
  r23.y = S.y[j];
  r45.x = S.y[j - 1];
  r45.y = j >= 2 ? S.y[j - 2] : 0.0;
  r67.x = dyn ? ((S.flags[1] == 0 && j < S.flags[2]) ? 1.0 : 0.0) : 1.0;
  r67.y = 0.0;
  reinterpret_cast<double2*>(r)[0] = r01;
  reinterpret_cast<double2*>(r)[1] = r23;
  reinterpret_cast<double2*>(r)[2] = r45;
  reinterpret_cast<double2*>(r)[3] = r67;
}

// One-graph solve, after the k - 1 step launches: the x terms still pending at the last
// step (last = steps_taken - 1 not a multiple of 3 — the step launches flush only at
// multiples of 3, the host-side schedule p2_flush also at `last`), added exactly as the
// last step's grouped flush would: x + y_{last-1} v_last (2 pending) + y_last v_{last+1}.
__global__ __launch_bounds__(kTPB) void k_p2_tail(int64_t n, DevState S, double* __restrict__ x,
                                                  const double* __restrict__ V0,
                                                  const double* __restrict__ V1,
                                                  const double* __restrict__ V2) {
  if (S.flags[1]) return;
  const int last = S.flags[2] - 1;
  if (last < 1) return;
  const int pending = last % 3;
  if (pending == 0) return;
  const double* ring[3] = {V0, V1, V2};
  const double* vl = ring[last % 3];
  const double* vn = ring[(last + 1) % 3];
  const double y1 = S.y[last - 1], y0 = S.y[last];
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    double xv = x[i];
    if (pending == 2) xv = xv + y1 * vl[i];
    x[i] = xv + y0 * vn[i];
  }
}

// f(T_k) = T_k^{-1} on the device: y = ||b|| * T_k^{-1} e_1, bit for bit the host solver
// tpl_ftk_inv (tpl_ftk.cpp: the LAPACK dgtsv scheme — tridiagonal elimination with partial
// pivoting, then back substitution; IEEE operations, -ffp-contract=off). Both halves are
// one dependent chain. The elimination's rows [0, flags[5]) were done during pass one by
// k_p1_axpy's extra workgroup (one row per step, one-graph inv); the rest — the last
// rows, or all of them (tpl_op_ftk_device, the one-pass solver) — run here on lane 0
// with alpha and beta staged in LDS. The back substitution divides by pivots known before
// it starts, so their reciprocals are taken first on all lanes and every division of the
// chain becomes Markstein's correction (div_rn: three dependent operations, the IEEE
// quotient's bits); a row whose operands leave div_rn's range sets a flag and the whole
// substitution is redone with IEEE divisions. The chain runs on lane 0 with nothing else
// on it: x' goes to LDS (all lanes scale and store y after), the range tests of its
// numerators and quotients are deferred to all lanes (round 4: 85.6 us at k = 500 with
// them and the global stores on the chain). Dynamic LDS: 11 k doubles.
// scale: 1 — y = ||b|| y' (two-pass: y_k, src/solvers.rs:169); 0 — y' itself (one-pass:
// the reconstruction multiplies by ||b||, src/solvers.rs:96-104); x * 1.0 is exact.
__global__ __launch_bounds__(kTPB) void k_ftk_inv(DevState S, int scale) {
  extern __shared__ double sh[];
  __shared__ double last[3];
  const int n = S.flags[2];
  if (S.flags[1] || n < 1) return;
  const size_t kc = (size_t)S.kcap;
  const int done = min(S.flags[5], max(n - 1, 0));  // rows eliminated during pass one
  double* D = sh;
  double* DU = sh + n;
  double* DU2 = sh + 2 * n;
  double* B = sh + 3 * n;
  double* R = sh + 4 * n;   // reciprocals of the pivots
  double* al = sh + 5 * n;  // alpha, beta of the rows still to eliminate
  double* be = sh + 6 * n;
  for (int i = threadIdx.x; i < n; i += kTPB) {
    if (i < done) {
      D[i] = S.lu[i];
      DU[i] = S.lu[kc + i];
      DU2[i] = S.lu[2 * kc + i];
      B[i] = S.lu[3 * kc + i];
    }
    al[i] = S.alphas[i];
    be[i] = i + 1 < n ? S.betas[i] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    LuRow cur = done == 0 ? LuRow{al[0], n > 1 ? be[0] : 0.0, 1.0}
                          : LuRow{S.lu[4 * kc], S.lu[4 * kc + 1], S.lu[4 * kc + 2]};
    for (int i = done; i + 1 < n; ++i)
      lu_row(i, i + 2 < n, be[i], al[i + 1], i + 2 < n ? be[i + 1] : 0.0, cur, D, DU, DU2, B);
    last[0] = cur.d;
    last[1] = cur.b;
  }
  __syncthreads();
  // Off the chain, on all lanes: the pivots' reciprocals, each row repacked as one
  // 32-B record {B, DU, DU2, D} (two 16-B LDS reads per row on the chain instead of four
  // 8-B ones), and div_rn's range test of every pivot and reciprocal.
  // 4 (n - 1) doubles from an even offset: 16-B aligned records for the 16-B LDS accesses
  // whatever the parity of n (at most 11 n - 3 <= 11 kcap doubles in all)
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
    // back substitution with U = (D, DU, DU2): x_i = ((B_i - DU_i x_{i+1}) - DU2_i x_{i+2}) / D_i
    const double xl = last[1] / last[0];  // b[n-1] / d[n-1]
    Y[n - 1] = xl;
    if (n >= 2) {
      double x1 = xl, x0;
      {
        const double t = B[n - 2] - DU[n - 2] * x1;
        x0 = div_rn(t, D[n - 2], R[n - 2], !any_pbad);
        Y[n - 2] = x0;
        T[n - 2] = 0.0;  // row n - 2 took div_rn's own checks
      }
      // the fast chain: Markstein's correction with every operand read one row ahead; the
      // range tests of t and the quotient are deferred to all lanes after the loop
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
        const double t = bi - dui * x0 - du2i * x1;
        const double q0 = t * ri;
        const double qm = fma(fma(-di, q0, t), ri, q0);
        const double xi = t == 0.0 ? q0 : qm;  // +-0: q0 carries the quotient's sign
        Y[ii] = xi;
        T[ii] = t;
        x1 = x0;
        x0 = xi;
      }
    }
  }
  __syncthreads();
  // deferred: a row whose numerator or quotient left div_rn's range (t == 0 is exact)
  bool bad = any_pbad && n >= 2;
  for (int i = threadIdx.x; i + 2 < n; i += kTPB) {
    const double t = T[i];
    bad = bad || !(t == 0.0 || (exp_in_range(t) && exp_in_range(Y[i])));
  }
  if (__syncthreads_or(bad)) {
    // an operand outside div_rn's range (singular or badly scaled T_k): IEEE divisions
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
  for (int i = threadIdx.x; i < n; i += kTPB) S.y[i] = Y[i] * bnorm;
}

// One-pass reconstruction x = ||b|| (V_k y') (src/solvers.rs:96-104); V column-major, ld = n.
// steps < 0: steps_taken from the device state (the device-f path, no host round trip).
__global__ __launch_bounds__(kTPB) void k_gemv_recon(int64_t n, int steps, DevState S,
                                                     const double* __restrict__ V,
                                                     double* __restrict__ x) {
  if (steps < 0) {
    if (S.flags[1] || S.flags[4]) return;  // zero b / f handed back to the host
    steps = S.flags[2];
  }
  const double bnorm = S.norms[0];
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB) {
    double s = 0.0;
    for (int c = 0; c < steps; ++c) s = fma(V[(int64_t)c * n + i], S.y[c], s);
    x[i] = bnorm * s;
  }
}

} // namespace tpl

// ------------------------------------------------------------ host launchers
namespace tpl {
namespace launch {

hipError_t p1_init(const CsrDev& A, const DevState& S, const double* b, hipStream_t s) {
  hipLaunchKernelGGL(k_p1_init, dim3(g2_grid(A)), dim3(kTPB), 0, s, A, S, b);
  return hipGetLastError();
}
hipError_t p1_spmv(const CsrDev& A, const DevState& S, const double* xsrc, const double* r_cur,
                   const double* r_prev, double* W, double* Vcol, int j, hipStream_t s,
                   unsigned long long* stamp) {
  if (spmv_grid(A) <= 0) return hipGetLastError();
  P1SpmvArgs a{};
  a.Pb_r = S.Pb_r; a.flags = S.flags; a.norms = S.norms; a.betas = S.betas; a.Pa = S.Pa;
  a.xsrc = xsrc; a.r_cur = r_cur; a.r_prev = r_prev; a.W = W; a.Vcol = Vcol; a.stamp = stamp;
  a.j = j;
#define TPL_FIELD(f) a.f = A.f;
  TPL_P1_LAYOUT_FIELDS(TPL_FIELD)
#undef TPL_FIELD
  if (A.pb_ld > 0) return p1_spmv_gp(A, a, s);
  if (A.G2_r <= kTPB) return TPL_LAUNCH_CW(k_p1_spmv, A, s, a);
  return p1_spmv_wide(A, a, s);
}
hipError_t p1_axpy(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                   double* r_next, int j, int k, int elim, hipStream_t s,
                   unsigned long long* st) {
  // the elimination workgroup: the block after the element grid, padding blocks included
  const P1AxpyArgs a = p1_axpy_args(A, S, W, r_cur, r_next, j, k, elim ? g2_grid(A) : -1, st);
  const dim3 g(g2_grid(A) + (elim ? 1 : 0)), b(kTPB);
  TPL_NP_SWITCH(A.NA_r, hipLaunchKernelGGL(k_p1_axpy<NP>, g, b, 0, s, a));
  return hipGetLastError();
}
hipError_t p2_init(int64_t n, const DevState& S, const double* b, double* v1, double* x,
                   double* Vcol, int dyn, hipStream_t s) {
  hipLaunchKernelGGL(k_p2_init, dim3(elem_grid(n)), dim3(kTPB), 0, s, n, S, b, v1, x, Vcol, dyn);
  return hipGetLastError();
}
hipError_t p2_tail(int64_t n, const DevState& S, double* x, double* const V[3], hipStream_t s) {
  hipLaunchKernelGGL(k_p2_tail, dim3(elem_grid(n)), dim3(kTPB), 0, s, n, S, x, V[0], V[1], V[2]);
  return hipGetLastError();
}
hipError_t ftk_inv(const DevState& S, int kcap, int scale, hipStream_t s) {
  hipLaunchKernelGGL(k_ftk_inv, dim3(1), dim3(kTPB), (size_t)11 * kcap * sizeof(double), s, S, scale);
  return hipGetLastError();
}
hipError_t p2_spmv(const CsrDev& A, const DevState& S, const double* xsrc, const double* v_cur,
                   const double* v_prev, double* v_next, double* x, double* Vcol, int j,
                   int nflush, hipStream_t s) {
  if (spmv_grid(A) > 0)
    return TPL_LAUNCH_CW(k_p2_spmv, A, s, A, S.p2c + 8 * (size_t)j, xsrc, v_cur, v_prev, v_next,
                         x, Vcol, j, nflush);
  return hipGetLastError();
}
hipError_t p2_coefs(const DevState& S, int k, int dyn, hipStream_t s) {
  if (k > 1)
    hipLaunchKernelGGL(k_p2_coefs, dim3((k + kTPB - 1) / kTPB), dim3(kTPB), 0, s, S, k, dyn);
  return hipGetLastError();
}
hipError_t gemv_recon(int64_t n, int steps, const DevState& S, const double* V, double* x,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_gemv_recon, dim3(elem_grid(n)), dim3(kTPB), 0, s, n, steps, S, V, x);
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
