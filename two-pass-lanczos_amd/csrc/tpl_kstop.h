// tpl_kstop.h — what the solves that stop at a residual tolerance share on the device, each
// written once: the flag words and the rule of the stop, the wave's vote, the per-shift
// elimination lane and the `fin` wave of the shifted solves (k_p1_axpy_stol / k_p1_stol_fin,
// tpl_k_p1_stol.hip; k_bp1_axpy_stol / k_bp1_stol_fin, tpl_k_batch_stol.hip), and div_rn,
// the division of the back substitutions (k_ftk_inv, tpl_kernels.hip; k_ftk_inv_shifts,
// tpl_k_p1_stol.hip). k_p1_axpy_tol (tpl_k_p1_tol.hip) takes the flag words and the rule.
// Included only by .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include "tpl_klu.h"
#include "tpl_launch.h"

namespace tpl {

// a / b given y = RN(1 / b): Markstein's correction q = RN(q0 + RN(a - b q0) y), q0 =
// RN(a y), is the correctly rounded quotient — the IEEE division's bits — whenever no
// intermediate leaves the normal range; elsewhere (zeros, huge or tiny magnitudes,
// non-finite values) the IEEE division itself. Three dependent operations instead of the
// division's ten on the back substitution's chain. (Checked against IEEE division on
// 10^9 random pairs in range, exact and binade-boundary quotients included: no
// difference; tests/native/div_rn_check.c restates it on the host, tests/test_native.py)
__device__ __forceinline__ bool exp_in_range(double v) {
  const unsigned e = (unsigned)(__double2hiint(v) >> 20) & 0x7FFu;  // biased exponent
  return e - (1023u - 900u) <= 1800u;  // 2^-900 <= |v| < 2^901
}
__device__ __forceinline__ double div_rn(double a, double b, double y, bool b_ok) {
  if (b_ok && exp_in_range(a)) {
    const double q0 = a * y;
    const double q = fma(fma(-b, q0, a), y, q0);
    if (exp_in_range(q)) return q;
  } else if (b_ok && a == 0.0) {
    return a * y;  // +-0 with the quotient's sign
  }
  return a / b;
}

// The tolerance stop's words of a column's eight flags (DevState::flags, or BatchDev::flags +
// 8 c for column c of a batch group, which no other batch kernel reads or writes. k_p1_init
// zeroes the first and the host the other two before the graph; k_bp1_init zeroes all three):
// [kFlagDone] the rows of T_k's LU eliminated during pass one; [kFlagHit] the step count the
// pass stops at — the smallest m whose residual met the tolerance (k_p1_axpy_tol), or M = the
// largest m*_s once EVERY shift has met it (the shifted solves) — 0 until then; [kFlagRes] the
// entries of the residual history formed so far (by the lanes still running).
constexpr int kFlagDone = 5;
constexpr int kFlagHit = 6;
constexpr int kFlagRes = 7;
// An element block of launch j acts on a hit only when an earlier launch wrote it: the hit
// at m is written by launch m + 1 (m = 1 and 2: by launch 3, the first that eliminates); with
// several shifts the last lane to stop is the one with the largest m*, so M is written by
// launch M + 1 likewise. Launch j's own elimination workgroup may be writing the word while
// the element blocks read it; whichever value they see, this test gives every block the
// same answer.
__device__ __forceinline__ bool hit_before(int hit, int j) {
  return hit != 0 && j > (hit + 1 > 3 ? hit + 1 : 3);
}
// All 64 lanes of the wave call this. every: each lane's `hit` is non-zero; the return
// value: the largest hit of the wave.
__device__ __forceinline__ int wave_hits(int hit, bool& every) {
  every = __ballot(hit != 0) == ~0ull;
  int mx = hit;
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(mx, o);
    mx = other > mx ? other : mx;
  }
  return mx;
}

// Step j >= 3 of one column's elimination wave, all 64 lanes: lane s < t.m runs lu_row on
// (alphas + sig[s], betas). Its rows go to t.lu, its running row to t.st, its residuals to
// t.res, all shift-interleaved (a step's stores are m adjacent doubles per array), and the
// first m with res <= tol to t.hits[s]; from then on the lane eliminates nothing, so its
// running row stays row m*_s - 1's. A lane past t.m counts as stopped and touches no memory.
// When every lane has stopped, lane 0 writes M = max m*_s to flags[kFlagHit]. A shift that
// never stops keeps the pass running to k. flags, alphas, betas: the column's.
__device__ __forceinline__ void stol_elim_wave(const launch::ShiftTol& t, int lane, int j,
                                               int32_t* flags, const double* alphas,
                                               const double* betas) {
  const int i = j - 3;
  const int s = lane, m = t.m;
  const bool live = s < m;
  const size_t am = (size_t)t.kcap * (size_t)m;  // one array of t.lu
  const int stop = flags[0], done = flags[kFlagDone];
  const int every_hit = flags[kFlagHit];  // M, written by an earlier launch
  if (stop || done != i) return;  // breakdown at this step: k_ftk_inv_shifts finishes the rows
  if (every_hit) return;          // every running row stays where its lane stopped
  int hit = live ? t.hits[s] : 1;
  if (live && !hit) {
    const double tol = t.tol[0], sg = t.sig[s];
    const double dli = betas[i], d1 = alphas[i + 1] + sg, du1 = betas[i + 1];
    LuRow cur{t.st[s], t.st[m + s], t.st[2 * m + s]};
    double* D = t.lu + s;
    if (i == 0) {
      cur = LuRow{alphas[0] + sg, dli, 1.0};
      const double r0 = fabs(dli * (cur.b / cur.d));  // the one-step iterate
      t.res[s] = r0;
      if (r0 <= tol) hit = 1;
    }
    lu_row(i * m, true, dli, d1, du1, cur, D, D + am, D + 2 * am, D + 3 * am);
    t.st[s] = cur.d;
    t.st[m + s] = cur.du;
    t.st[2 * m + s] = cur.b;
    // the (i + 2)-step iterate. A zero pivot gives inf or NaN, never <= a finite tol
    const double r1 = fabs(du1 * (cur.b / cur.d));
    t.res[(size_t)(i + 1) * m + s] = r1;
    if (!hit && r1 <= tol) hit = i + 2;
    if (hit) t.hits[s] = hit;
    t.nres[s] = i + 2;
  }
  bool every;
  const int mx = wave_hits(hit, every);
  if (s == 0) {
    flags[kFlagDone] = i + 1;
    flags[kFlagRes] = i + 2;
    if (every) flags[kFlagHit] = mx;
  }
}

// After the last step launch, one column's wave, all 64 lanes (k_p1_tol_fin's two cases, per
// lane). A pass of two steps (kmax = 2, or a breakdown at step 3) never ran the elimination
// wave: lane s forms its one residual by the same expression. And when the last launch's
// stops made every lane stop (or this wave's own just did), steps_taken becomes M here.
__device__ __forceinline__ void stol_fin_wave(const launch::ShiftTol& t, int lane,
                                              int32_t* flags, const double* alphas,
                                              const double* betas) {
  const int s = lane;
  const bool live = s < t.m;
  int hit = live ? t.hits[s] : 1;
  if (flags[kFlagHit] == 0 && flags[2] == 2 && flags[kFlagRes] == 0) {
    if (live) {
      const double r0 = fabs(betas[0] * (1.0 / (alphas[0] + t.sig[s])));
      t.res[s] = r0;
      t.nres[s] = 1;
      if (r0 <= t.tol[0]) {
        hit = 1;
        t.hits[s] = 1;
      }
    }
    if (s == 0) flags[kFlagRes] = 1;
  }
  bool every;
  const int mx = wave_hits(hit, every);
  if (s == 0 && every) {
    flags[kFlagHit] = mx;
    flags[0] = 1;
    flags[2] = mx;
  }
}

} // namespace tpl
