// tpl_k_ftk_exp_times_batch.hip — exp(t_i T_k) e_1 for m times of every column of a lock-step
// group at once (k_ftk_exp_times_batch), between the passes of
// tpl_lanczos_two_pass_batch_exp_times. The body is tpl_kexp.h's, shared with k_ftk_exp and
// k_ftk_exp_times; tpl_kernels.hip's map of the device sources leaves this unit out
// (bench.py ties the committed headline profile to that file's bytes).
#include "../../include/tpl.h"
#include "tpl_batch.h"
#include "tpl_kexp.h"

namespace tpl {

// Workgroup (i, c): k_ftk_exp's evaluation on t_i T_k of column c of the group, from the
// column's part of the BatchDev (flags + 8 c, norms + c (kcap + 1), alphas / betas + c kcap;
// steps_c from the column's flags[2]) — function i, column c of the group's coefficient table,
// Y + (i nb + c) kcap with nb = gridDim.y, times ||b_c|| when `scale`, and back[c m + i] = 0;
// or, where k_ftk_exp would hand the case back, a zero column and back[c m + i] = 1. Bitwise
// k_ftk_exp on the host-scaled arrays t_i * alphas_c, t_i * betas_c. Nothing is written for
// a column with a zero b or no step. The body sees the column through a DevState view that
// holds the two pointers it reads (flags, norms); the group's state is read only.
// m nb <= 256 workgroups of 4 waves: every (time, column) has a CU of its own, so the launch
// takes what the slowest expansion takes.
__global__ __launch_bounds__(kTPB) void k_ftk_exp_times_batch(
    const int32_t* __restrict__ flags, const double* __restrict__ norms,
    const double* __restrict__ alphas, const double* __restrict__ betas, int kcap,
    const double* __restrict__ ts, double* __restrict__ Y, int32_t* __restrict__ back, int scale) {
  const int i = blockIdx.x, m = gridDim.x;
  const int c = blockIdx.y, nb = gridDim.y;
  DevState S{};
  S.flags = const_cast<int32_t*>(flags) + 8 * c;
  S.norms = const_cast<double*>(norms) + (size_t)c * (size_t)(kcap + 1);
  S.kcap = kcap;
  const size_t col = (size_t)c * (size_t)kcap;
  ftk_exp_body(S, scale, ExpSrcTimes{alphas + col, betas + col, ts[i]},
               ExpDstTimes{Y + ((size_t)i * nb + c) * (size_t)kcap, back + (c * m + i)});
}

hipError_t launch::ftk_exp_times_batch(int nb, const BatchDev& B, int k, const double* ts, int m,
                                       double* Y, int32_t* back, int scale, hipStream_t s) {
  if ((nb != 2 && nb != 4) || m < 1 || m > TPL_MULTI_MAX || k < 1 || k > B.kcap)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ftk_exp_times_batch, dim3(m, nb), dim3(kTPB), ftk_exp_lds_bytes(k), s,
                     B.flags, B.norms, B.alphas, B.betas, B.kcap, ts, Y, back, scale);
  return hipGetLastError();
}

} // namespace tpl
