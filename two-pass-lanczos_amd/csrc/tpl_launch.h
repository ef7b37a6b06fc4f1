// tpl_launch.h — the kernel launchers: declared here once, defined in the .hip unit that
// holds the kernel (map: tpl_kernels.hip), called by the host units. Each enqueues on `s` and returns the launch's status.
#pragma once
#include <hip/hip_runtime.h>

#include "tpl_device.h"

namespace tpl {
struct BatchDev;  // tpl_batch.h
namespace launch {
hipError_t spmv(const CsrDev& A, const double* x, double* y, hipStream_t s);
// the dense operator's SpMV-shaped kernels (tpl_k_dense.hip): the plain product, the pass-one
// step (A: the element geometry, G2_r norm partials) and the pass-two step, each in the place
// of spmv / p1_spmv / p2_spmv with the same state and vectors
hipError_t dense_spmv(const DenseDev& D, const double* x, double* y, hipStream_t s);
hipError_t dense_p1(const DenseDev& D, const CsrDev& A, const DevState& S, const double* xsrc,
                    const double* r_cur, const double* r_prev, double* W, double* Vcol, int j,
                    hipStream_t s, unsigned long long* stamp = nullptr);
hipError_t dense_p2(const DenseDev& D, const DevState& S, const double* xsrc, const double* v_cur,
                    const double* v_prev, double* v_next, double* x, double* Vcol, int j,
                    int nflush, hipStream_t s);
hipError_t p1_init(const CsrDev& A, const DevState& S, const double* b, hipStream_t s);
// stamp: workgroup 0 records the launch's start there (live timing), or nullptr
hipError_t p1_spmv(const CsrDev& A, const DevState& S, const double* xsrc, const double* r_cur,
                   const double* r_prev, double* W, double* Vcol, int j, hipStream_t s,
                   unsigned long long* stamp = nullptr);
// elim: one more workgroup eliminates row j - 3 of T_k's LU (one-graph inv)
hipError_t p1_axpy(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                   double* r_next, int j, int k, int elim, hipStream_t s,
                   unsigned long long* stamp = nullptr);
// the step of the inverse solve that stops at a residual tolerance (k_p1_axpy_tol,
// tpl_k_p1_tol.hip): p1_axpy with the elimination workgroup, which also keeps the residual
// history in tr = {tol, res[kcap]} and raises the stop; p1_tol_fin: after the last step,
// one thread settles steps_taken
hipError_t p1_axpy_tol(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                       double* r_next, int j, int k, double* tr, hipStream_t s);
hipError_t p1_tol_fin(const DevState& S, double* tr, hipStream_t s);
// ---- the shifted inverse solve that stops each shift at a tolerance (tpl_k_p1_stol.hip).
// The per-shift state of its device path, shift-interleaved: entry (row i, shift s) of an
// array sits at i m + s, so a step's m stores are adjacent.
struct ShiftTol {
  const double* tol;   // [0]: the tolerance
  const double* sig;   // the m shifts
  double* lu;          // D | DU | DU2 | B of every T_k + sig[s] I: kcap rows of m each
  double* st;          // the running rows: d | du | b, m each
  double* res;         // the residual histories: kcap rows of m
  int32_t* hits;       // m*_s, 0: shift s has not met the tolerance
  int32_t* nres;       // entries of shift s's history formed
  int32_t m, kcap;
};
// p1_axpy_tol with one elimination lane per shift (k_p1_axpy_stol): the stop is raised when
// every shift has met the tolerance, with M = max m*_s in flags[6]. p1_stol_fin: after the
// last step, one wave settles steps_taken and the history of a two-step pass.
hipError_t p1_axpy_stol(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                        double* r_next, int j, int k, const ShiftTol& t, hipStream_t s);
hipError_t p1_stol_fin(const DevState& S, const ShiftTol& t, hipStream_t s);
// (T_n + sig[s] I)^{-1} e_1 with n = m*_s (t.hits[s], or steps_taken), one workgroup per shift
// (k_ftk_inv_shifts): column s of Y (columns ldy >= k apart), times ||b|| when `scale`, and
// cs[s] = n. k: the steps asked for (it sizes the LDS). Rows [0, flags[5]) of t.lu count as
// eliminated: with flags[5] = 0 and t.hits zeroed the kernel reads neither t.lu nor t.st
hipError_t ftk_inv_shifts(const DevState& S, int k, const ShiftTol& t, double* Y, int ldy,
                          int32_t* cs, int scale, hipStream_t s);
// p2_xacc with a per-column cut (k_p2_xacc_cut): term t of column c only where t < cs[c],
// cs read on the device
hipError_t p2_xacc_cut(const CsrDev& A, const double* Y, int ldy, int j, int nflush,
                       const int32_t* cs, const double* vp, const double* vc, const double* vn,
                       double* X, int64_t ldx, int m, hipStream_t s);
// ---- the same for a batch group (tpl_k_batch_stol.hip): every column of the group has a
// ShiftTol block of its own; tol and sig are shared. t0 is column 0's view; column c's arrays
// sit c dstride doubles (st, lu, res) and c istride int32 (hits, nres) further on.
struct BatchShiftTol {
  ShiftTol t0;
  size_t dstride, istride;
  __host__ __device__ ShiftTol col(int c) const {  // the kernels' wave c calls it too
    ShiftTol v = t0;
    v.st += (size_t)c * dstride;
    v.lu += (size_t)c * dstride;
    v.res += (size_t)c * dstride;
    v.hits += (size_t)c * istride;
    v.nres += (size_t)c * istride;
    return v;
  }
};
// bp1_axpy (tpl_batch.h) with the elimination workgroup of k_bp1_axpy_stol: wave c, lane i
// eliminates column c's T_k + sig[i] I; column c stops when every shift of it has met the
// tolerance, with M_c = max_i m*_{c,i} in its flag word 6. bp1_stol_fin: after the last step,
// one wave per column settles steps_c and the history of a two-step pass.
hipError_t bp1_axpy_stol(int nb, const CsrDev& A, const BatchDev& B, const double* W,
                         const double* r_cur, double* r_next, int j, int k,
                         const BatchShiftTol& t, hipStream_t s);
hipError_t bp1_stol_fin(int nb, const BatchDev& B, const BatchShiftTol& t, hipStream_t s);
// bp2_xacc (tpl_batch.h) with a cut per (function, column), read on the device
// (k_bp2_xacc_cut): after step j, of the last nflush (1..3) terms, term t of result (f, c)
// only where t < cs[c cld + f]; m <= kBatchMultiFuncs functions per launch
hipError_t bp2_xacc_cut(int nb, const CsrDev& A, const BatchDev& B, const int32_t* cs, int cld,
                        const double* Y, int j, int nflush, const double* vp, const double* vc,
                        const double* vn, double* X, int64_t xstride, int m, hipStream_t s);
hipError_t p2_tail(int64_t n, const DevState& S, double* x, double* const V[3], hipStream_t s);
hipError_t permute(int64_t n, int cols, double* out, int64_t ldo, const double* in, int64_t ldi,
                   const int32_t* idx, hipStream_t s);
hipError_t ftk_inv(const DevState& S, int kcap, int scale, hipStream_t s);
hipError_t ftk_exp(const DevState& S, int kcap, int scale, hipStream_t s);
// exp(t_i T_k) e_1 for the m times ts[0..m), one workgroup each (k_ftk_exp_times,
// tpl_k_ftk_exp_times.hip): column i of Y (columns ldy >= kcap apart) and back[i] = 0, or a
// zero column and back[i] = 1 where k_ftk_exp would hand the case back
hipError_t ftk_exp_times(const DevState& S, int kcap, const double* ts, int m, double* Y, int ldy,
                         int32_t* back, int scale, hipStream_t s);
// the same for every column of a batch group of nb (2 or 4) columns, one workgroup per
// (time, column) (k_ftk_exp_times_batch, tpl_k_ftk_exp_times_batch.hip): column c's state is
// its part of B (steps_c from its flags; B is only read), k <= B.kcap the steps asked for
// (it sizes the LDS). Function i, column c goes to Y + (i nb + c) B.kcap — the layout
// bp2_minit / bp2_xacc read — with back[c m + i] = 0, or zeros and back[c m + i] = 1
hipError_t ftk_exp_times_batch(int nb, const BatchDev& B, int k, const double* ts, int m,
                               double* Y, int32_t* back, int scale, hipStream_t s);
hipError_t p2_init(int64_t n, const DevState& S, const double* b, double* v1, double* x,
                   double* Vcol, int dyn, hipStream_t s);
// nflush: x terms the step applies (tpl::p2_flush: every third step and the last)
hipError_t p2_spmv(const CsrDev& A, const DevState& S, const double* xsrc, const double* v_cur,
                   const double* v_prev, double* v_next, double* x, double* Vcol, int j,
                   int nflush, hipStream_t s);
// the same step with the long rows' sums read from `ycache`, the step's row of the long-row
// cache (k_p2_cached, tpl_k_p2_cached.hip); needs n_long > 0. lrow: the long rows' row
// indices, or nullptr when they are the last rows
hipError_t p2_cached(const CsrDev& A, const DevState& S, const double* xsrc, const double* v_cur,
                     const double* v_prev, double* v_next, double* x, double* Vcol,
                     const double* ycache, const int32_t* lrow, int j, int nflush,
                     hipStream_t s);
// The fused pass two (tpl_k_p2_fused.hip), after p2_init and p2_coefs: every step of pass two
// in two launches, for a layout whose rows decouple (tpl_layout.h FusedP2) with the long rows
// last. ycache holds (A v_j)_r of every long row for the steps pass one took (row j - 1:
// step j); p2_fused_hub steps the long rows (and the hub set: h_row / h_ent / h_val, n_open
// open rows of n_hub members) and leaves v_j[r] in the cache in place of the sums;
// p2_fused_rows steps the closed short rows from them. steps > 0: the steps taken; 0: read
// them (and the error flag) from the device state, as k_p2_tail does. v1, x: what p2_init
// wrote; x gets the result.
struct FusedP2Dev {
  const int32_t *h_row, *h_ent;
  const double* h_val;
  int32_t n_open, n_hub;
};
hipError_t p2_fused_hub(const CsrDev& A, const DevState& S, const FusedP2Dev& H, double* ycache,
                        const double* v1, double* x, int steps, hipStream_t s);
hipError_t p2_fused_rows(const CsrDev& A, const DevState& S, const double* ycache,
                         const double* v1, double* x, int steps, hipStream_t s);
// the batch sibling (k_bp2_cached, tpl_k_batch_p2_cached.hip): step j of a group of nb
// columns (the other batch launchers: tpl_batch.h) with the long rows' nb sums read from
// `ycrow`, the step's row of the group's long-row cache (n_long x nb, a row's sums adjacent)
hipError_t bp2_cached(int nb, const CsrDev& A, const BatchDev& B, const double* v_cur,
                      const double* v_prev, double* v_next, double* x, const double* ycrow,
                      const int32_t* lrow, int j, hipStream_t s);
// pass-two step records (EpiPass2R) for steps 1 .. k-1; dyn: activity from the device count
hipError_t p2_coefs(const DevState& S, int k, int dyn, hipStream_t s);
hipError_t gemv_recon(int64_t n, int steps, const DevState& S, const double* V, double* x,
                      hipStream_t s);
// multi-function pass two (tpl_k_multi.hip). Y: the coefficient table, column i at
// Y + i * ldy; X: the m result vectors, column i at X + i * ldx.
// p2_minit: v_1 = b / ||b||, X_i = v_1 y_i[0]. p2_xacc: after step j, the last nflush
// (1..3) x terms of m <= 8 columns from vp / vc / vn = v_{j-1}, v_j, v_{j+1}.
hipError_t p2_minit(const CsrDev& A, const DevState& S, const double* Y, int ldy, const double* b,
                    double* v1, double* X, int64_t ldx, int m, hipStream_t s);
hipError_t p2_xacc(const CsrDev& A, const double* Y, int ldy, int j, int nflush, const double* vp,
                   const double* vc, const double* vn, double* X, int64_t ldx, int m,
                   hipStream_t s);
int long_epi_blocks(const CsrDev& A);  // workgroups over the long rows (kLongEpiRows each)
hipError_t long_epi_p1(const CsrDev& A, const DevState& S, const double* yall, int R,
                       const double* r_cur, const double* r_prev, double* W, double* Vcol,
                       double* Pa_long, int j, hipStream_t s);
hipError_t long_epi_p2(const CsrDev& A, const DevState& S, const double* yall, int R,
                       const double* v_cur, const double* v_prev, double* v_next, double* x,
                       double* Vcol, int j, int nflush, hipStream_t s);
hipError_t long_epi_y(const CsrDev& A, const double* yall, int R, double* y, hipStream_t s);
hipError_t reorth_decide(const DevState& S, const double* Pb1, int G2, int* skip, int* rec,
                         hipStream_t s);
hipError_t reorth_dot(int64_t n, int cols, const double* V, const double* r, double* P, int G,
                      int64_t E, const int* skip, hipStream_t s);
hipError_t reorth_reduce(int cols, const double* P, int G, double* h, const int* skip, hipStream_t s);
hipError_t reorth_update(int64_t n, int cols, const double* V, double* r, const double* h,
                         double* Pnorm, int G, int64_t E, const int* skip, hipStream_t s);
} // namespace launch
} // namespace tpl
