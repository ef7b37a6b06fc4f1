// tpl_k_spmv.hip — the plain product y = A x (k_spmv, the 56 layout variants) and the row
// permutation at the boundary. Map of the device sources: tpl_kernels.hip.
#include "tpl_klaunch.h"

namespace tpl {

template <int F>
__global__ __launch_bounds__(kTPB, kSpmvMinWaves) void k_spmv(CsrDev A, const double* __restrict__ x,
                                               double* __restrict__ y) {
  extern __shared__ double lds[];
  pin_layout_args(A);
  asm volatile("" ::"s"(A.E), "s"(A.G2), "s"(A.srows), "s"(x), "s"(y));
  double acc = 0.0;
  spmv_block<F>(A, x, UnitScale{}, EpiSpmv{y}, acc, lds);
}

// Row permutation at the boundary (locality order, tpl_layout.h): out[i] = in[idx[i]] for
// each of `cols` columns (leading dimensions ldo / ldi).
__global__ __launch_bounds__(kTPB) void k_permute(int64_t n, int cols, double* __restrict__ out,
                                                  int64_t ldo, const double* __restrict__ in,
                                                  int64_t ldi, const int32_t* __restrict__ idx) {
  const int c = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * kTPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kTPB)
    out[(int64_t)c * ldo + i] = in[(int64_t)c * ldi + idx[i]];
}

namespace launch {

hipError_t spmv(const CsrDev& A, const double* x, double* y, hipStream_t s) {
  if (spmv_grid(A) > 0) return TPL_LAUNCH_CW(k_spmv, A, s, A, x, y);
  return hipGetLastError();
}
hipError_t permute(int64_t n, int cols, double* out, int64_t ldo, const double* in, int64_t ldi,
                   const int32_t* idx, hipStream_t s) {
  for (int c0 = 0; n > 0 && c0 < cols; c0 += 65535) {
    const int c = std::min(cols - c0, 65535);
    hipLaunchKernelGGL(k_permute, dim3(elem_grid(n), c), dim3(kTPB), 0, s, n, c,
                       out + (int64_t)c0 * ldo, ldo, in + (int64_t)c0 * ldi, ldi, idx);
  }
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
