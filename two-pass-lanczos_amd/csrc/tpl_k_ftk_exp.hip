// tpl_k_ftk_exp.hip — f(T_k) = exp(T_k) on the device (k_ftk_exp): the shared body
// (tpl_kexp.h) on the state's own alpha / beta, y and hand-back flag. Map of the device
// sources: tpl_kernels.hip.
#include "tpl_kexp.h"

namespace tpl {

namespace {
struct ExpSrcState {  // T_k as pass one left it
  const double *al, *be;
  __device__ __forceinline__ double alpha(int i) const { return al[i]; }
  __device__ __forceinline__ double beta(int i) const { return be[i]; }
};
struct ExpDstState {  // S.y; handed back: S.flags[4] = 1 (a kept y leaves the flag alone)
  double* y_;
  int32_t* flags;
  __device__ __forceinline__ void y(int i, double v) const { y_[i] = v; }
  __device__ __forceinline__ void hand_back() const { flags[4] = 1; }
  __device__ __forceinline__ void kept() const {}
};
} // namespace

__global__ __launch_bounds__(kTPB) void k_ftk_exp(DevState S, int scale) {
  ftk_exp_body(S, scale, ExpSrcState{S.alphas, S.betas}, ExpDstState{S.y, S.flags});
}

hipError_t launch::ftk_exp(const DevState& S, int kcap, int scale, hipStream_t s) {
  hipLaunchKernelGGL(k_ftk_exp, dim3(1), dim3(kTPB), ftk_exp_lds_bytes(kcap), s, S, scale);
  return hipGetLastError();
}

} // namespace tpl
