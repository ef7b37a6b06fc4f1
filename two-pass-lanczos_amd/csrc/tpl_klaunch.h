// tpl_klaunch.h — host-side helpers of the launchers: grids, dynamic LDS, and the dispatch
// of an SpMV-shaped kernel to the instance of the layout's variant flag (tpl_kcommon.h
// kVar*). Included only by .hip files.
#pragma once
#include <utility>

#include "tpl_kcommon.h"
#include "tpl_launch.h"

namespace tpl {
namespace launch {

static inline int elem_grid(int64_t n) {
  int64_t g = (n + kTPB - 1) / kTPB;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}
// chunk part: 8 XCDs x the largest eighth of the row blocks x chunks per row block
static inline int spmv_grid(const CsrDev& A) {
  return A.n_slice_blocks + 8 * ((A.G2 + 7) / 8) * (int)(A.E / kChunkRows);
}
// element-wise kernels over the G2 row blocks (elem_block)
static inline int g2_grid(const CsrDev& A) { return 8 * ((A.G2 + 7) / 8); }
// dynamic LDS of the SpMV-shaped kernels: a bin's staged products + piece starts
static inline size_t spmv_lds_bytes(const CsrDev& A) {
  const size_t bins = A.n_slice_blocks > 0
             ? (size_t)A.bin_cap * sizeof(double) + kTPB * sizeof(int) + kTPB * sizeof(double)
             : 0;
  const size_t win = (size_t)A.s_win * sizeof(double);  // short-chunk column window
  return bins > win ? bins : win;
}
// launch_f(std::integral_constant<int, F>) for the F equal to f, over the instances that
// exist; hipErrorInvalidConfiguration when f has none, else the launch's status.
template <class LaunchF, int... Fs>
hipError_t dispatch_variant(int f, LaunchF launch_f, std::integer_sequence<int, Fs...>) {
  auto one = [&](auto F) {
    if constexpr (variant_exists(decltype(F)::value)) {
      if (f == decltype(F)::value) return launch_f(F), true;
    }
    return false;
  };
  return (one(std::integral_constant<int, Fs>{}) || ...) ? hipGetLastError()
                                                          : hipErrorInvalidConfiguration;
}
// Launch the SpMV-shaped kernel specialised for the layout A (the instance of its variant
// flag, tpl_device.h variant_of), on stream s.
#define TPL_LAUNCH_CW(KERNEL, A, s, ...)                                                    \
  dispatch_variant(                                                                         \
      variant_of(A),                                                                        \
      [&](auto F) {                                                                         \
        hipLaunchKernelGGL(KERNEL<decltype(F)::value>, dim3(spmv_grid(A)), dim3(kTPB),      \
                           spmv_lds_bytes(A), (s), __VA_ARGS__);                            \
      },                                                                                    \
      std::make_integer_sequence<int, kVarEnd>{})

// k_p1_spmv_gp / k_p1_spmv_wide (units of their own): launch::p1_spmv hands them the
// arguments it filled, for pb_ld > 0 / G2_r > kTPB.
hipError_t p1_spmv_gp(const CsrDev& A, const P1SpmvArgs& a, hipStream_t s);
hipError_t p1_spmv_wide(const CsrDev& A, const P1SpmvArgs& a, hipStream_t s);

} // namespace launch
} // namespace tpl
