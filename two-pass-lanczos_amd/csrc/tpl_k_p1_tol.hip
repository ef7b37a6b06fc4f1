// tpl_k_p1_tol.hip — pass one of the inverse solve that stops at a residual tolerance
// (tpl_lanczos_two_pass_inv_tol): k_p1_axpy_tol, the pass-one AXPY step whose elimination
// workgroup also keeps the residual history and raises the stop, and k_p1_tol_fin, the one
// thread that settles steps_taken between pass one and k_ftk_inv.
//
// The Lanczos residual of the m-step iterate x_m = ||b|| V_m T_m^{-1} e_1 is
//     ||b - A x_m|| / ||b|| = beta_m |e_m^T T_m^{-1} e_1|,
// and the last component of T_m^{-1} e_1 in the dgtsv scheme is b / d of the running row
// after rows 0 .. m - 2 are eliminated — the quotient k_ftk_inv starts its back
// substitution with. The elimination workgroup of the one-graph inv holds that row one
// launch after beta_m is known, so each residual costs it one division and one product,
// off the step's critical path.
// The tolerance is read from device memory (tr[0]), not passed as an argument: the graph
// is cached per kmax and replayed for any tolerance.
//
// Shared (tpl_kstop.h): the flag words of the stop and hit_before, the rule by which every
// element block of a launch decides alike; lu_row (tpl_klu.h).
// Still repeated: k_p1_axpy_tol repeats k_p1_axpy's text (tpl_kernels.hip) with the additions
// marked "tol:". The two are not one template: with the body factored out behind a
// compile-time switch, the existing k_p1_axpy instances no longer compiled to the same
// instructions (commuted operands, other registers in 227 of ~850 lines), and those are the
// headline's. Nor is its element part one inlined function with k_p1_axpy_stol's
// (tpl_k_p1_stol.hip), though the two texts are the same: tried, 148 of this unit's 4,388
// lines of assembly changed (commuted operands, moved instructions) in the element blocks,
// the part every step waits for. A change to k_p1_axpy's element part belongs here too.
#include "tpl_klaunch.h"
#include "tpl_klu.h"
#include "tpl_kstop.h"

namespace tpl {

// k_p1_axpy (tpl_kernels.hip: its comments hold for the shared text) with the tolerance
// stop. tr = {tol, res[kcap]}. The elimination thread also forms the residual of the
// iterates it can see — after rows 0 .. m - 2 the running row gives res[m - 1] =
// |beta_m (cur.b / cur.d)|, tpl_ftk_inv_residuals' expression — and records the first m
// with res <= tol in flags[kFlagHit]; from then on it eliminates nothing (the running row
// stays row m - 1's, which k_ftk_inv finishes). From the launch after the one that wrote the
// hit every element block returns before alpha, block 0 setting the stop flag and
// steps_taken = m — also when a breakdown has set the stop flag since: the hit came first.
template <int NP>
__global__ __launch_bounds__(kTPB) void k_p1_axpy_tol(P1AxpyArgs a, double* tr) {
  __shared__ double red[4];
  struct {
    int64_t E, n, norm_n; int NA_r, G2;
  } A{a.E, a.n, a.norm_n, a.NA_r, a.G2};
  struct {
    const double* Pa_r; int32_t* flags; double* norms; double* alphas; double* Pb;
  } S{a.Pa_r, a.flags, a.norms, a.alphas, a.Pb};
  const double* __restrict__ W = a.W;
  const double* __restrict__ r_cur = a.r_cur;
  double* __restrict__ r_next = a.r_next;
  const int j = a.j, k = a.k, elim_block = a.elim_block;
  asm volatile("" ::"s"(A.E), "s"(A.n), "s"(A.norm_n), "s"(A.NA_r), "s"(A.G2), "s"(S.Pa_r),
               "s"(S.flags), "s"(S.norms), "s"(S.alphas), "s"(S.Pb));
  asm volatile("" ::"s"(W), "s"(r_cur), "s"(r_next), "s"(j), "s"(k), "s"(elim_block));
  if ((int)blockIdx.x == elim_block) {
    if (threadIdx.x != 0 || j < 3) return;
    const int i = j - 3;
    const size_t kcap = (size_t)a.kcap;
    double* D = a.lu;
    double* st = a.lu + 4 * kcap;
    double* res = tr + 1;
    const int stop = S.flags[0], done = S.flags[kFlagDone];
    int hit = S.flags[kFlagHit];  // tol: written by an earlier launch of this workgroup
    const double tol = tr[0];
    const double dli = a.betas[i], d1 = S.alphas[i + 1], du1 = a.betas[i + 1];
    LuRow cur{st[0], st[1], st[2]};
    const double a0 = S.alphas[0];
    if (stop || done != i) return;  // breakdown at this step: the tail finishes the rows
    if (hit) return;                // tol: the running row stays row m - 1's
    if (i == 0) {
      cur = LuRow{a0, dli, 1.0};
      const double r0 = fabs(dli * (cur.b / cur.d));  // tol: the one-step iterate
      res[0] = r0;
      if (r0 <= tol) hit = 1;
    }
    lu_row(i, true, dli, d1, du1, cur, D, D + kcap, D + 2 * kcap, D + 3 * kcap);
    st[0] = cur.d;
    st[1] = cur.du;
    st[2] = cur.b;
    S.flags[kFlagDone] = i + 1;
    // tol: the (i + 2)-step iterate. A zero pivot gives inf or NaN, never <= a finite tol
    const double r1 = fabs(du1 * (cur.b / cur.d));
    res[i + 1] = r1;
    if (!hit && r1 <= tol) hit = i + 2;
    if (hit) S.flags[kFlagHit] = hit;
    S.flags[kFlagRes] = i + 2;
    return;
  }
  const int rb = elem_block(A.G2, blockIdx.x);
  if (rb < 0) return;
  const int stop = S.flags[0];
  const int hit = S.flags[kFlagHit];  // tol: the stop flag's 32-byte line
  const double normj = S.norms[j - 1];
  __builtin_amdgcn_sched_barrier(0);
  PartialRegs<NP> pr;
  const int na_ = A.NA_r;
  load_partials(S.Pa_r, na_, pr);
  const int64_t beg = (int64_t)rb * A.E;
  const int64_t end = beg + A.E < A.n ? beg + A.E : A.n;
  constexpr int kAxPairs = 4;
  const int64_t i00 = beg + 2 * threadIdx.x;
  double2 w0[kAxPairs], rc0[kAxPairs];
#pragma unroll
  for (int q = 0; q < kAxPairs; ++q) {
    const int64_t i0 = i00 + (int64_t)q * 2 * kTPB;
    const int64_t ic = i0 < end ? i0 : beg;
    w0[q] = *reinterpret_cast<const double2*>(W + ic);
    rc0[q] = *reinterpret_cast<const double2*>(r_cur + ic);
  }
  __builtin_amdgcn_sched_barrier(0);
  double invN = 1.0 / normj;
  keep(invN);
  __builtin_amdgcn_sched_barrier(0);
  const double alpha = finish_partials(S.Pa_r, na_, pr, red);
  // tol: ahead of the stop test, so that a breakdown in the step after the hit keeps m
  if (hit_before(hit, j)) {
    if (rb == 0 && threadIdx.x == 0) {
      S.flags[0] = 1;
      S.flags[2] = hit;
    }
    return;
  }
  if (stop) return;
  if (rb == 0 && threadIdx.x == 0) {
    S.alphas[j - 1] = alpha;
    S.flags[2] = j;
  }
  if (j == k) return; // beta_k is never used
  double acc = 0.0;
  auto step = [&](int64_t i0, double2 w, double2 rc) {
    double2 r;
    r.x = w.x - alpha * (rc.x * invN);
    r.y = w.y - alpha * (rc.y * invN);
    if (i0 + 1 < end) {
      typedef double d2v __attribute__((ext_vector_type(2)));
      d2v rv = {r.x, r.y};
      __builtin_nontemporal_store(rv, reinterpret_cast<d2v*>(r_next + i0));
    } else {
      __builtin_nontemporal_store(r.x, r_next + i0);
    }
    acc = i0 < A.norm_n ? fma(r.x, r.x, acc) : acc;
    acc = i0 + 1 < end && i0 + 1 < A.norm_n ? fma(r.y, r.y, acc) : acc;
  };
#pragma unroll
  for (int q = 0; q < kAxPairs; ++q) {
    const int64_t i0 = i00 + (int64_t)q * 2 * kTPB;
    if (i0 < end) step(i0, w0[q], rc0[q]);
  }
  for (int64_t i0 = i00 + (int64_t)kAxPairs * 2 * kTPB; i0 < end; i0 += 2 * kTPB) // E > 2048
    step(i0, *reinterpret_cast<const double2*>(W + i0),
         *reinterpret_cast<const double2*>(r_cur + i0));
  const double p = block_sum_tail(acc, red);
  if (threadIdx.x == 0) S.Pb[rb] = p;
}

// After the last step launch: what no later element block is left to do. A hit written by
// the last launch (m = kmax - 1, or any m when kmax = 3) becomes steps_taken here; and a
// pass of two steps (kmax = 2, or a breakdown at step 3) never ran the elimination
// workgroup, so its one residual, res[0], is formed here by the same expression.
__global__ void k_p1_tol_fin(DevState S, double* tr) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || S.flags[1]) return;
  int hit = S.flags[kFlagHit];
  if (!hit && S.flags[2] == 2 && S.flags[kFlagRes] == 0) {
    const double r0 = fabs(S.betas[0] * (1.0 / S.alphas[0]));
    tr[1] = r0;
    S.flags[kFlagRes] = 1;
    if (r0 <= tr[0]) {
      hit = 1;
      S.flags[kFlagHit] = 1;
    }
  }
  if (hit) {
    S.flags[0] = 1;
    S.flags[2] = hit;
  }
}

namespace launch {

hipError_t p1_axpy_tol(const CsrDev& A, const DevState& S, const double* W, const double* r_cur,
                       double* r_next, int j, int k, double* tr, hipStream_t s) {
  const P1AxpyArgs a = p1_axpy_args(A, S, W, r_cur, r_next, j, k, g2_grid(A), nullptr);
  const dim3 g(g2_grid(A) + 1), b(kTPB);
  TPL_NP_SWITCH(A.NA_r, hipLaunchKernelGGL(k_p1_axpy_tol<NP>, g, b, 0, s, a, tr));
  return hipGetLastError();
}
hipError_t p1_tol_fin(const DevState& S, double* tr, hipStream_t s) {
  hipLaunchKernelGGL(k_p1_tol_fin, dim3(1), dim3(64), 0, s, S, tr);
  return hipGetLastError();
}

} // namespace launch
} // namespace tpl
