// tpl_k_ftk_exp_times.hip — exp(t_i T_k) e_1 for m times at once (k_ftk_exp_times), between
// the shared passes of tpl_lanczos_two_pass_exp_times. The body is tpl_kexp.h's, shared with
// k_ftk_exp (tpl_k_ftk_exp.hip), as are the source and destination types (ExpSrcTimes,
// ExpDstTimes: every entry of T_k times t_i, rounded once); tpl_kernels.hip's map of the device sources leaves this unit
// out (bench.py ties the committed headline profile to that file's bytes).
#include "../../include/tpl.h"
#include "tpl_kexp.h"

namespace tpl {

// Workgroup i: k_ftk_exp's evaluation on t_i T_k — column i of Y (columns ldy apart), times
// ||b|| when `scale`, and back[i] = 0; or, where k_ftk_exp would hand the case back, a zero
// column and back[i] = 1. Bitwise k_ftk_exp on the host-scaled arrays t_i * alphas,
// t_i * betas. Reads the state (steps_taken from S.flags[2]; nothing is written after a zero
// b or no step) and never writes S.flags or S.y. m <= TPL_MULTI_MAX workgroups of 4 waves:
// every time has a CU of its own, so the launch takes what the slowest expansion takes.
__global__ __launch_bounds__(kTPB) void k_ftk_exp_times(DevState S, const double* __restrict__ ts,
                                                        double* __restrict__ Y, int ldy,
                                                        int32_t* __restrict__ back, int scale) {
  const int i = blockIdx.x;
  ftk_exp_body(S, scale, ExpSrcTimes{S.alphas, S.betas, ts[i]},
               ExpDstTimes{Y + (size_t)i * (size_t)ldy, back + i});
}

hipError_t launch::ftk_exp_times(const DevState& S, int kcap, const double* ts, int m, double* Y,
                                 int ldy, int32_t* back, int scale, hipStream_t s) {
  if (m < 1 || m > TPL_MULTI_MAX || kcap > ldy) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ftk_exp_times, dim3(m), dim3(kTPB), ftk_exp_lds_bytes(kcap), s, S, ts, Y,
                     ldy, back, scale);
  return hipGetLastError();
}

} // namespace tpl
