// tpl_k_p1_wide.hip — k_p1_spmv_wide: the pass-one step's SpMV (p1_spmv_body,
// tpl_kcommon.h) for more than 256 norm partials (four per thread first, the rest in
// batches; the 5M-arc instance's 1,024 row blocks). 56 layout variants only very large
// operators launch, in a unit of their own so that they compile beside the headline's.
// Map of the device sources: tpl_kernels.hip.
#include "tpl_klaunch.h"

namespace tpl {

template <int F>
__global__ __launch_bounds__(kTPB, p1_min_waves(F, 4)) void k_p1_spmv_wide(P1SpmvArgs a) {
  __shared__ double red[4], redb[4];
  extern __shared__ double lds[];
  p1_spmv_body<F, 4>(a, red, redb, lds);
}

hipError_t launch::p1_spmv_wide(const CsrDev& A, const P1SpmvArgs& a, hipStream_t s) {
  return TPL_LAUNCH_CW(k_p1_spmv_wide, A, s, a);
}

} // namespace tpl
