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
// The arguments of a pass-one AXPY step (k_p1_axpy, k_p1_axpy_tol, k_p1_axpy_stol).
// elim_block: the elimination workgroup's block — g2_grid(A), the block after the element
// grid, padding blocks included — or -1 for none.
static inline P1AxpyArgs p1_axpy_args(const CsrDev& A, const DevState& S, const double* W,
                                      const double* r_cur, double* r_next, int j, int k,
                                      int elim_block, unsigned long long* stamp) {
  P1AxpyArgs a{};
  a.Pa_r = S.Pa_r; a.W = W; a.r_cur = r_cur; a.r_next = r_next; a.flags = S.flags;
  a.norms = S.norms; a.alphas = S.alphas; a.Pb = S.Pb; a.stamp = stamp;
  a.n = A.n; a.E = A.E; a.norm_n = A.norm_n; a.NA_r = A.NA_r; a.G2 = A.G2; a.j = j; a.k = k;
  a.elim_block = elim_block;
  a.kcap = S.kcap; a.betas = S.betas; a.lu = S.lu;
  return a;
}
// CALL with NP a constant expression: the smallest of 2, 4, 8, 12 with kTPB NP >= na_r (12
// for more: the step reduces the rest in batches), the alpha partials a thread loads up front.
#define TPL_NP_SWITCH(na_r, CALL)                                   \
  if ((na_r) <= 2 * kTPB) { constexpr int NP = 2; CALL; }           \
  else if ((na_r) <= 4 * kTPB) { constexpr int NP = 4; CALL; }      \
  else if ((na_r) <= 8 * kTPB) { constexpr int NP = 8; CALL; }      \
  else { constexpr int NP = 12; CALL; }
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
