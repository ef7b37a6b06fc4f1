// tpl_klu.h — one row of the tridiagonal elimination of T_k's LU (the dgtsv scheme of
// tpl_ftk.cpp), shared by every kernel that runs it: k_p1_axpy's elimination workgroup and
// k_ftk_inv (tpl_kernels.hip), k_p1_axpy_tol (tpl_k_p1_tol.hip), the shifted solves' lanes
// (stol_elim_wave, tpl_kstop.h) and k_ftk_inv_shifts (tpl_k_p1_stol.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace tpl {

// ---- T_k^{-1} e_1 on the device (the one-graph inv): the host solver's operations
// (tpl_ftk.cpp: the LAPACK dgtsv scheme, tridiagonal elimination with partial pivoting,
// then back substitution), bit for bit.
// Running row i of the elimination: its pivot, super-diagonal and right-hand side.
struct LuRow {
  double d, du, b;
};
// Eliminate row i (dl = beta_i, d1 = alpha_{i+1}, du1 = beta_{i+1} or 0 when row i + 1 is
// the last; more = row i + 2 exists): stores row i of U (D, DU, DU2) and of the
// transformed right-hand side (B), advances `cur` to row i + 1. The operations of the
// host loop in its order (-ffp-contract=off).
__device__ __forceinline__ void lu_row(int i, bool more, double dli, double d1, double du1,
                                       LuRow& cur, double* D, double* DU, double* DU2,
                                       double* B) {
  double dip1 = d1, duip1 = du1, bip1 = 0.0, du2i = 0.0;
  if (fabs(cur.d) >= fabs(dli)) {
    const double fact = dli / cur.d;
    dip1 = dip1 - fact * cur.du;
    bip1 = bip1 - fact * cur.b;
    D[i] = cur.d;
    DU[i] = cur.du;
    B[i] = cur.b;
  } else {
    const double fact = cur.d / dli;
    D[i] = dli;
    const double temp = dip1;
    dip1 = cur.du - fact * temp;
    if (more) {
      du2i = duip1;
      duip1 = -fact * du2i;
    }
    DU[i] = temp;
    B[i] = bip1;            // b[i] <- old b[i+1] (= 0: b[i+1] is first set at step i)
    bip1 = cur.b - fact * bip1;
  }
  DU2[i] = du2i;
  cur.d = dip1;
  cur.du = duip1;
  cur.b = bip1;
}

} // namespace tpl
