// tpl_batch.h — the lock-step batch solve (tpl_lanczos_two_pass_batch): the per-column
// device state of a group of NB columns and the launchers of the batch kernels
// (tpl_k_batch_p1.hip, tpl_k_batch_p2.hip, and tpl_k_batch_p2_cached.hip, whose launcher
// tpl_launch.h declares; device building blocks: tpl_kbatch.h).
// Plain data, shared by the kernels and the host units like tpl_device.h.
//
// A group's work vectors are INTERLEAVED: entry i of column c sits at v[i * NB + c], so a
// gather of column index `col` fetches the NB values of all columns with one 16-B (NB = 2)
// or two adjacent 16-B (NB = 4) loads, and a row's own entries and stores are as wide.
#pragma once
#include <hip/hip_runtime.h>

#include "tpl_device.h"

namespace tpl {

constexpr int kBatchNbMax = 4;  // the widest group (instances: NB = 2 and NB = 4)
// Functions per k_bp2_xacc launch (tpl_k_batch_multi.hip; instances M = 1 .. 4 per NB): at
// NB = 4 the three ring vectors and M result vectors are 8 (3 + M) VGPRs of loads in flight
// per element, 56 at M = 4; more functions run as further launches.
constexpr int kBatchMultiFuncs = 4;

// Per-column solver state of a group (the batch sibling of DevState; kcap, na_ld and g2_ld
// are the column strides). Column c of the group reads and writes only its own part.
struct BatchDev {
  int32_t* flags;      // column c: flags + 8 c, fields as DevState::flags ([0] stop,
                       // [1] error, [2] steps_taken)
  double* norms;       // column c: norms + c (kcap + 1)
  double* alphas;      // column c: alphas + c kcap
  double* betas;       // column c: betas + c kcap
  double* y;           // column c: y + c kcap
  double* p2c;         // pass-two step records: step j, column c at p2c + 8 (j NB + c):
                       // the fields of EpiPass2R's record; [6] active (j < steps_c),
                       // [7] the x terms column c applies at step j (p2_flush(j, steps_c - 1))
  double* Pa;          // alpha partials, column c: Pa + c na_ld (NA each)
  double* Pb;          // norm partials, column c: Pb + c g2_ld (G2 each)
  double* P;           // long rows' hand-off slots: row ri, slice s, column c at
                       // P + (ri kSlotStride + s) kBatchNbMax + c whatever NB, so that a slot no
                       // launch writes (an empty piece) holds its +0.0 for every group width
  unsigned int* Pcnt;  // the batch's own arrival counters (kCntStride apart, never reset):
                       // ONE increment per piece per launch, whatever NB
  int32_t kcap, na_ld, g2_ld;
};

namespace launch {
// B (column-major, ld = n, the caller's order) -> the interleaved group vector in the
// operator's order: out[i NB + c] = B[c n + idx[i]] (idx == nullptr: identity). And back: X[c n + i] = in[idx[i] NB + c].
hipError_t b_interleave(int nb, int64_t n, double* out, const double* B,
                        const int32_t* idx, hipStream_t s);
hipError_t b_deinterleave(int nb, int64_t n, double* X, const double* in,
                          const int32_t* idx, hipStream_t s);
hipError_t bp1_init(int nb, const CsrDev& A, const BatchDev& B, const double* b, hipStream_t s);
// ycrow: the step's row of the group's long-row cache (the long rows' sums are stored
// there, n_long x nb), or nullptr
hipError_t bp1_spmv(int nb, const CsrDev& A, const BatchDev& B, const double* r_cur,
                    const double* r_prev, double* W, int j, double* ycrow, hipStream_t s);
hipError_t bp1_axpy(int nb, const CsrDev& A, const BatchDev& B, const double* W,
                    const double* r_cur, double* r_next, int j, int k, hipStream_t s);
hipError_t bp2_init(int nb, const CsrDev& A, const BatchDev& B, const double* b, double* v1,
                    double* x, hipStream_t s);
// records of steps 1 .. kmax-1 for every column, from the device-held steps_taken
hipError_t bp2_coefs(int nb, const BatchDev& B, int kmax, hipStream_t s);
hipError_t bp2_spmv(int nb, const CsrDev& A, const BatchDev& B, const double* v_cur,
                    const double* v_prev, double* v_next, double* x, int j, hipStream_t s);
// ---- m functions of every column of a group (tpl_k_batch_multi.hip). Function f's result
// is the interleaved group vector X + f xstride; its coefficients for column c are
// Y[(f nb + c) B.kcap + j].
hipError_t bp2_minit(int nb, const CsrDev& A, const BatchDev& B, const double* Y, int m,
                     const double* b, double* v1, double* X, int64_t xstride, hipStream_t s);
// bp2_coefs with every column's nflush 0: bp2_spmv then leaves x alone
hipError_t bp2_coefs0(int nb, const BatchDev& B, int kmax, hipStream_t s);
// the grouped flush after step j for m (1 .. kBatchMultiFuncs) functions, each column by
// its own device-held steps_c; vp / vc / vn: v_{j-1}, v_j, v_{j+1}
hipError_t bp2_xacc(int nb, const CsrDev& A, const BatchDev& B, const double* Y, int j,
                    const double* vp, const double* vc, const double* vn, double* X,
                    int64_t xstride, int m, hipStream_t s);
// X[(c m + f) n + i] = in[f xstride + idx[i] nb + c] (idx == nullptr: identity)
hipError_t bm_deinterleave(int nb, int64_t n, double* X, const double* in, int64_t xstride,
                           int m, const int32_t* idx, hipStream_t s);
} // namespace launch
} // namespace tpl
