// tpl_k_p1_gp.hip — k_p1_spmv_gp: the pass-one step's SpMV (p1_spmv_body, tpl_kcommon.h)
// reducing every rank's gathered norm partials itself (replicated partition:
// CsrDev::pb_ld). 56 layout variants only partitioned solves launch, in a unit of their
// own so that they compile beside the headline's. Map of the device sources: tpl_kernels.hip.
#include "tpl_klaunch.h"

namespace tpl {

template <int F>
__global__ __launch_bounds__(kTPB, p1_min_waves(F, 1)) void k_p1_spmv_gp(P1SpmvArgs a) {
  __shared__ double red[4], redb[4], redr[4 * kPbRanks];
  extern __shared__ double lds[];
  p1_spmv_body<F, -kPbRanks>(a, red, redb, lds, redr);
}

hipError_t launch::p1_spmv_gp(const CsrDev& A, const P1SpmvArgs& a, hipStream_t s) {
  return TPL_LAUNCH_CW(k_p1_spmv_gp, A, s, a);
}

} // namespace tpl
