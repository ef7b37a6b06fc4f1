// tpl_passes.cpp — the per-step launch sequences of the device-resident Lanczos passes
// and the graph cache that replays them.
//
// The Lanczos loops of the reference (src/algorithms/lanczos.rs:86-128,
// src/algorithms/lanczos_two_pass.rs:84-102 and :266-309) run entirely on the GPU:
// the per-step launches are captured once per (variant, k) into a hipGraph and
// replayed, alpha/beta never leave HBM during a pass, and breakdown is handled
// on the device (a stop flag turns the remaining launches into no-ops). The only
// host round trip of a solve is the f(T_k) call between the passes, exactly
// where the reference calls its closure (src/solvers.rs:71-75, :155-156).
#include "tpl_op.h"

namespace tpl {

namespace {
enum GraphKind {
  kGPass1 = 0,        // pass one: + the kP1* properties of the variant (kinds 0 .. 15)
  kGPass2 = 16, kGPass2Steps,
  kGTwoPassDev,       // one-graph solve: pass one, device f(T_k), pass two
  kGDevFtk,           // (timed variant) device f(T_k) + pass-two prologue
  kGPass2Dyn,         // (timed variant) the k - 1 step launches of a one-graph solve
  kGPass2Multi,       // pass two of a multi-function solve: one graph per (steps, m)
  kGPass1Batch,       // pass one of a batch group: one graph per (k, NB)
  kGPass2Batch,       // pass two of a batch group: one graph per (largest steps, NB)
  kGPass2BatchMulti,  // pass two of a batch-multi group whose columns took the same
                      // number of steps: one graph per (steps, NB, m)
  kGTwoPassInvTol,    // one-graph inverse solve that stops at a residual tolerance: one
                      // graph per kmax (the tolerance is device data, not an argument)
  kGPass2MultiCut,    // pass two of a multi-function solve with a per-column cut: one graph
                      // per (steps, m) (the columns' step counts are device data)
  kGTwoPassShiftedInvTol,  // one-graph shifted inverse solve that stops each shift at a
                      // tolerance: one graph per (kmax, m) (tolerance and shifts: device data)
  kGPass2BatchMultiCut,    // pass two of a batch-multi group with a cut per (column,
                      // function): one graph per (steps, NB, m) (the counts are device data)
  kGTwoPassBatchShiftedInvTol,  // one group of the batch shifted inverse solve that stops
                      // every (column, shift) at a tolerance: one graph per (kmax, NB, m)
  kGLongCache = 64,   // + this: the sequence stores / reads the long-row cache (a two-pass
                      // solve with the cache on for it; other kernels, other graphs)
  kGFusedP2 = 128,    // + this: pass two is the fused one (k_p2_hub, k_p2_rows) in place of
                      // the step launches (and of k_p2_tail)
};
// What tells one pass-one sequence (and its graph) from another, beside k: the basis is
// stored (the standard pass), T_k's LU is eliminated as it goes (a device inv follows:
// k_ftk_inv), kStampSteps steps carry start stamps (timed variant), the long rows' sums
// are stored in the long-row cache (tpl_lanczos_two_pass with the cache on).
enum P1Props { kP1Basis = 1, kP1Elim = 2, kP1Stamped = 4, kP1Cache = 8 };

// The long-row cache's row of step j (pass one stores it, pass two reads it), or nullptr:
// the cache is not in use (long_cache_steps) or does not reach step j.
inline double* cache_row(const tpl_op_s* op, int j) {
  return (size_t)j <= long_cache_steps(op)
             ? op->st.d_ycache + (size_t)(j - 1) * op->lay.lrows.size() : nullptr;
}
inline int graph_cache_kind(const tpl_op_s* op) {
  return long_cache_steps(op) ? kGLongCache | (fused_p2(op) ? kGFusedP2 : 0) : 0;
}
// The same for a batch group of nb columns: the row of step j in the group's own cache.
inline double* batch_cache_row(const tpl_op_s* op, int j, int nb) {
  return (size_t)j <= batch_cache_steps(op)
             ? op->bat.d_ycache + (size_t)(j - 1) * op->lay.lrows.size() * (size_t)nb : nullptr;
}
inline int batch_graph_cache_kind(const tpl_op_s* op) {
  return batch_cache_steps(op) ? kGLongCache : 0;
}

// r_j buffer of pass one: r_1 = b, then R[j % 3] (local view, and gather source).
inline double* r_of(const tpl_op_s* op, int j) { return j == 1 ? op->b : op->R[j % 3]; }
inline double* rG_of(const tpl_op_s* op, int j) { return j == 1 ? op->bG : op->RG[j % 3]; }

// Pass two's three basis buffers at position t of their rotation (a sweep's step j sits
// at t = j): the gather source and local view of v_t, v_{t-1}, and v_{t+1}'s place.
struct P2Rot {
  double *G, *cur, *prev, *next;
};
inline P2Rot p2_rot(const tpl_op_s* op, int t) {
  return {op->V2G[t % 3], op->V2[t % 3], op->V2[(t + 2) % 3], op->V2[(t + 1) % 3]};
}
// The pass-one step's SpMV launch of step j, by the operator's storage: k_dense_p1 for a dense
// operator, else k_p1_spmv (or its siblings) on the layout A.
inline void launch_p1_spmv(tpl_op_s* op, const CsrDev& A, int j, double* Vcol,
                           unsigned long long* stamp) {
  const double* prev = j >= 2 ? r_of(op, j - 1) : nullptr;
  if (op->dense)
    HIPCHK(launch::dense_p1(dense_dev(op), A, op->st.S, rG_of(op, j), r_of(op, j), prev, op->W,
                            Vcol, j, op->stream, stamp));
  else
    HIPCHK(launch::p1_spmv(A, op->st.S, rG_of(op, j), r_of(op, j), prev, op->W, Vcol, j,
                           op->stream, stamp));
}
} // namespace

bool use_graphs() {
  const char* e = std::getenv("TPL_NO_GRAPH");
  return !(e && e[0] == '1');
}

// ---- reorthogonalisation (extension, not in the reference): classical Gram-Schmidt of
// r_{j+1} against the stored columns V[:, 0..j) before beta_j. mode 1 (CGS2): two
// passes, always. mode 2 (selective, Kahan–Parlett "twice is enough"): the second pass
// runs only when the first removed more than half of ||r||^2 (k_reorth_decide; its
// kernels see the device flag and return at once otherwise).
void enqueue_reorth(tpl_op_s* op, int j, int mode) {
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "re-orthogonalisation of a partitioned operator");
  const int cols = j; // v_1 .. v_j are stored in V[:, 0..j)
  const int G2 = op->lay.G2;
  const int64_t E = op->lay.E;
  double* P = op->st.d_Pr;                             // cols x G2 partials
  double* h = op->st.d_Pr + (size_t)G2 * op->st.kcap;  // cols coefficients
  double* Pb1 = h + op->st.kcap;                       // ||r'||^2 partials (selective)
  int* skip = reinterpret_cast<int*>(Pb1 + G2);
  int* rec = reorth_records(op) + (j - 1);
  double* r = op->R[(j + 1) % 3];
  for (int pass = 0; pass < 2; ++pass) {
    const int* sk = (mode == 2 && pass == 1) ? skip : nullptr;
    HIPCHK(launch::reorth_dot(op->part.n, cols, op->d_V, r, P, G2, E, sk, op->stream));
    HIPCHK(launch::reorth_reduce(cols, P, G2, h, sk, op->stream));
    // the last update rewrites the ||r||^2 partials that k_p1_spmv(j+1) reduces; in the
    // selective mode the first one writes its own partials for the decision
    double* pn = pass == 1 ? op->st.S.Pb : (mode == 2 ? Pb1 : nullptr);
    HIPCHK(launch::reorth_update(op->part.n, cols, op->d_V, r, h, pn, G2, E, sk, op->stream));
    if (mode == 2 && pass == 0)
      HIPCHK(launch::reorth_decide(op->st.S, Pb1, G2, skip, rec, op->stream));
  }
}

// Pass one prologue: ||b||^2 partials; with a partition, b and the per-rank
// totals are all-gathered (step 1 gathers from b).
void enqueue_p1_prologue(tpl_op_s* op) {
  const CsrDev A = csr_dev(op);
  HIPCHK(launch::p1_init(A, op->st.S, op->b, op->stream));
  if (op->dist) enqueue_p1_exchange_norm(op, A, op->bG);
}

// Pass one, step j (k = requested steps). elim: also eliminate row j - 3 of T_k's LU
// (the one-graph inv, k_p1_axpy).
// st1 / st2: start stamps of the step's k_p1_spmv / k_p1_axpy launch (live timing), or nullptr.
// ycrow: the step's row of the long-row cache (one GPU: carried in the idle ypart), or nullptr.
void enqueue_p1_step(tpl_op_s* op, int j, int k, double* Vcol, bool elim, unsigned long long* st1,
                     unsigned long long* st2, double* ycrow) {
  CsrDev A = csr_dev(op, true);
  if (ycrow && !op->dist) A.ypart = ycrow;
  launch_p1_spmv(op, A, j, Vcol, st1);
  if (op->dist) enqueue_p1_exchange_a(op, A);
  if (op->part.hybrid)
    HIPCHK(launch::long_epi_p1(A, op->st.S, op->d_yall, op->dist->nranks, r_of(op, j),
                               j >= 2 ? r_of(op, j - 1) : nullptr, op->W, Vcol,
                               op->d_rsum + op->dist->nranks, j, op->stream));
  HIPCHK(launch::p1_axpy(A, op->st.S, op->W, r_of(op, j), op->R[(j + 1) % 3], j, k,
                         elim ? 1 : 0, op->stream, st2));
  if (op->dist && j < k) enqueue_p1_exchange_norm(op, A, op->RG[(j + 1) % 3]);
}

// First stamped step of a k-step pass one (steps js .. js + kStampSteps - 1, and the
// k_p1_spmv of the step after), or 0: the pass is too short to sample.
static int stamp_first(size_t k) {
  return k >= (size_t)kStampSteps + 3 ? (int)(k - kStampSteps) / 2 + 1 : 0;
}

static void enqueue_pass1(tpl_op_s* op, size_t k, int props, int reorth = 0) {
  enqueue_p1_prologue(op);
  const int js = props & kP1Stamped ? stamp_first(k) : 0;
  for (int j = 1; j <= (int)k; ++j) {
    double* Vcol = props & kP1Basis ? op->d_V + (size_t)(j - 1) * op->part.n : nullptr;
    const int i = j - js;  // stamp slots: spmv of step js + i at 2i, its axpy at 2i + 1
    unsigned long long* st1 = js && i >= 0 && i <= kStampSteps ? op->d_stamps + 2 * i : nullptr;
    unsigned long long* st2 = js && i >= 0 && i < kStampSteps ? op->d_stamps + 2 * i + 1 : nullptr;
    enqueue_p1_step(op, j, (int)k, Vcol, (props & kP1Elim) != 0, st1, st2,
                    props & kP1Cache ? cache_row(op, j) : nullptr);
    if (reorth && j < (int)k) enqueue_reorth(op, j, reorth);
  }
}

static void enqueue_pass2_init(tpl_op_s* op, size_t steps, double* Vout) {
  HIPCHK(launch::p2_init(op->part.n, op->st.S, op->b, op->V2[1], op->x, Vout, 0, op->stream));
  HIPCHK(launch::p2_coefs(op->st.S, (int)steps, 0, op->stream));
  if (op->dist && !op->part.hybrid) {
    halo_pack(op, op->V2G[1]);
    gather_vec(op, op->V2G[1]);
  }
}

// The pass-two step launch: step record j, the buffers at position t of their rotation
// (a sweep: t = j; the profiler re-runs one step's record as the buffers turn). The single
// place that picks the kernel: k_p2_cached when the running tpl_lanczos_two_pass's pass one
// stored step j's row of the long-row cache (cache_row), k_dense_p2 for a dense operator (it
// keeps no cache), else the full k_p2_spmv.
void launch_p2_step(tpl_op_s* op, const CsrDev& A, int j, int t, int nflush, double* Vcol) {
  const P2Rot v = p2_rot(op, t);
  if (const double* yc = cache_row(op, j)) {
    HIPCHK(launch::p2_cached(A, op->st.S, v.G, v.cur, j >= 2 ? v.prev : nullptr, v.next, op->x,
                             Vcol, yc, op->st.d_ylrow, j, nflush, op->stream));
    return;
  }
  if (op->dense) {
    HIPCHK(launch::dense_p2(dense_dev(op), op->st.S, v.G, v.cur, j >= 2 ? v.prev : nullptr, v.next,
                            op->x, Vcol, j, nflush, op->stream));
    return;
  }
  HIPCHK(launch::p2_spmv(A, op->st.S, v.G, v.cur, j >= 2 ? v.prev : nullptr, v.next, op->x, Vcol,
                         j, nflush, op->stream));
}

static void enqueue_pass2_steps(tpl_op_s* op, size_t steps, double* Vout) {
  const CsrDev A = csr_dev(op);
  for (int j = 1; j < (int)steps; ++j) {
    double* Vcol = Vout ? Vout + (size_t)j * op->part.n : nullptr;
    const int nflush = p2_flush(j, (int)steps - 1);
    launch_p2_step(op, A, j, j, nflush, Vcol);
    if (op->part.hybrid) {
      const P2Rot v = p2_rot(op, j);
      enqueue_p2_exchange(op, j);
      HIPCHK(launch::long_epi_p2(A, op->st.S, op->d_yall, op->dist->nranks, v.cur,
                                 j >= 2 ? v.prev : nullptr, v.next, op->x, Vcol, j, nflush,
                                 op->stream));
    } else if (op->dist && j + 1 < (int)steps) {
      enqueue_p2_exchange(op, j);
    }
  }
}
// The fused pass two (tpl_op.h fused_p2), after the prologue: every step in two launches.
// steps > 0: the steps taken (the host knows them); 0: the device-held count (one-graph
// solve), whose pending x terms need no k_p2_tail — both kernels run the host schedule.
static void enqueue_pass2_fused(tpl_op_s* op, size_t steps) {
  const CsrDev A = csr_dev(op);
  const FusedP2& f = op->lay.fp2;
  const launch::FusedP2Dev H{op->bufs.d_hrow, op->bufs.d_hent, op->bufs.d_hval, (int32_t)f.n_open,
                             (int32_t)f.n_hub};
  HIPCHK(launch::p2_fused_hub(A, op->st.S, H, op->st.d_ycache, op->V2[1], op->x, (int)steps,
                              op->stream));
  HIPCHK(launch::p2_fused_rows(A, op->st.S, op->st.d_ycache, op->V2[1], op->x, (int)steps,
                               op->stream));
}
void enqueue_pass2(tpl_op_s* op, size_t steps, double* Vout) {
  // the step launches, never fused: tpl_op_flags bits 8 and 9 tell of this pass two
  op->last_long_cache = steps >= 2 && long_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  enqueue_pass2_init(op, steps, Vout);
  enqueue_pass2_steps(op, steps, Vout);
}

// ---- one-graph two-pass solve (built-in f = inv, single GPU): steps_taken stays on the
// device. Pass one as usual; k_ftk_inv forms y = ||b|| T^{-1} e_1 from the device alpha /
// beta (bitwise the host solver's result); pass two is the k - 1 step launches, those at
// or past steps_taken doing nothing, with x flushed at multiples of 3 only and the
// pending terms of the last step added by k_p2_tail (the same sums as the host schedule).
// y = f(T_k) e_1 from the device alpha / beta, times ||b|| (scale: the two-pass y_k) or not
// (the one-pass y').
void enqueue_ftk_only(tpl_op_s* op, size_t k, int f, int scale) {
  if (f == kDevExp)
    HIPCHK(launch::ftk_exp(op->st.S, (int)k, scale, op->stream));
  else
    HIPCHK(launch::ftk_inv(op->st.S, (int)k, scale, op->stream));
}
static void enqueue_ftk_dev(tpl_op_s* op, size_t k, int f) {
  enqueue_ftk_only(op, k, f, 1);
  HIPCHK(launch::p2_init(op->part.n, op->st.S, op->b, op->V2[1], op->x, nullptr, 1, op->stream));
  HIPCHK(launch::p2_coefs(op->st.S, (int)k, 1, op->stream));
}
static void enqueue_pass2_dyn_steps(tpl_op_s* op, size_t k) {
  const CsrDev A = csr_dev(op);
  for (int j = 1; j < (int)k; ++j) launch_p2_step(op, A, j, j, j % 3 == 0 ? 3 : 0, nullptr);
}
static void enqueue_pass2_tail(tpl_op_s* op) {
  HIPCHK(launch::p2_tail(op->part.n, op->st.S, op->x, op->V2, op->stream));
}

GraphExec capture_graph(tpl_op_s* op, const std::function<void()>& enqueue) {
  auto go_eager = [&]() -> GraphExec {
    op->eager = true;  // the transport refused capture: launch eagerly from now on
    hipGetLastError();
    return nullptr;
  };
  HIPCHK(hipStreamBeginCapture(op->stream, hipStreamCaptureModeThreadLocal));
  hipGraph_t g = nullptr;
  try {
    enqueue();
  } catch (...) {
    hipStreamEndCapture(op->stream, &g);
    if (g) hipGraphDestroy(g);
    if (!op->dist) throw;
    return go_eager();
  }
  hipError_t e = hipStreamEndCapture(op->stream, &g);
  hipGraphExec_t ge = nullptr;
  if (e == hipSuccess) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  if (g) hipGraphDestroy(g);
  if (e != hipSuccess && op->dist) return go_eager();
  HIPCHK(e);
  return GraphExec(ge);
}

template <class Enq>
static void run_graph(tpl_op_s* op, int kind, size_t key, Enq&& enqueue) {
  if (!use_graphs() || op->eager) {
    enqueue();
    return;
  }
  auto it = op->graphs.find({kind, key});
  if (it == op->graphs.end()) {
    GraphExec ge = capture_graph(op, [&] { enqueue(); });
    if (!ge) {
      enqueue();
      return;
    }
    it = op->graphs.emplace(std::make_pair(kind, key), std::move(ge)).first;
  }
  HIPCHK(hipGraphLaunch(it->second.get(), op->stream));
}

static void run_pass1_graph(tpl_op_s* op, size_t k, int props) {
  if (long_cache_steps(op)) props |= kP1Cache;
  run_graph(op, kGPass1 + props, k, [&] { enqueue_pass1(op, k, props); });
}

// Pass two without a basis. With live timing on, the prologue is launched on its own
// and events bracket the graph of the steps - 1 step launches (tpl_op_pass_timing).
void run_pass2(tpl_op_s* op, size_t steps) {
  op->last_long_cache = steps >= 2 && long_cache_steps(op) > 0;
  const bool fused = fused_p2(op);
  op->last_fused_p2 = steps >= 2 && fused;
  auto enqueue_steps = [&] {
    if (fused) enqueue_pass2_fused(op, steps);
    else enqueue_pass2_steps(op, steps, nullptr);
  };
  if (!op->timing) {
    run_graph(op, kGPass2 + graph_cache_kind(op), steps, [&] {
      enqueue_pass2_init(op, steps, nullptr);
      enqueue_steps();
    });
    return;
  }
  enqueue_pass2_init(op, steps, nullptr);
  HIPCHK(hipEventRecord(op->tev[2], op->stream));
  run_graph(op, kGPass2Steps + graph_cache_kind(op), steps, enqueue_steps);
  HIPCHK(hipEventRecord(op->tev[3], op->stream));
  op->p2_launches = (int64_t)steps - 1;
}

// Pass two for m functions over one Krylov space (tpl_lanczos_two_pass_multi): the basis
// is regenerated once — every step launch runs with nflush = 0, so k_p2_spmv writes
// v_{j+1} and leaves x alone — and after each step of the single solve's flush schedule
// (p2_flush) k_p2_xacc applies that step's grouped flush to every column, up to 8 columns
// per launch, from the three live ring vectors: column i gets the single solve's bits.
static void enqueue_pass2_multi(tpl_op_s* op, size_t steps, size_t m) {
  const CsrDev A = csr_dev(op);
  const int ldy = (int)op->ycap;
  HIPCHK(launch::p2_minit(A, op->st.S, op->d_Y, ldy, op->b, op->V2[1], op->d_X, op->ld, (int)m,
                          op->stream));
  HIPCHK(launch::p2_coefs(op->st.S, (int)steps, 0, op->stream));
  for (int j = 1; j < (int)steps; ++j) {
    launch_p2_step(op, A, j, j, 0, nullptr);
    const int nflush = p2_flush(j, (int)steps - 1);
    if (!nflush) continue;
    const P2Rot v = p2_rot(op, j);
    for (size_t c0 = 0; c0 < m; c0 += 8)
      HIPCHK(launch::p2_xacc(A, op->d_Y + c0 * op->ycap, ldy, j, nflush, v.prev, v.cur, v.next,
                             op->d_X + c0 * (size_t)op->ld, op->ld, (int)std::min<size_t>(8, m - c0),
                             op->stream));
  }
}
void run_pass2_multi(tpl_op_s* op, size_t steps, size_t m) {
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
  if (m == 0 || m > op->xcols || steps > op->ycap || m > TPL_MULTI_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "run_pass2_multi: buffers smaller than the request");
  op->last_long_cache = steps >= 2 && long_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  run_graph(op, kGPass2Multi + graph_cache_kind(op), steps * (TPL_MULTI_MAX + 1) + m,
            [&] { enqueue_pass2_multi(op, steps, m); });
}

// The same with a per-column cut (tpl_lanczos_pass_two_multi_cut and the shifted inverse
// solve): k_p2_xacc_cut in place of k_p2_xacc, the columns' step counts in op->d_col_steps.
// dyn: the one-graph solve — `steps` is the count asked for, the step records take their
// activity from the device-held count, and x is flushed at multiples of 3 and once after the
// last launch (the cut covers the ragged end); else the host schedule for `steps` (p2_flush).
// The terms a column gets, and their order, are the same either way.
static void enqueue_pass2_multi_cut(tpl_op_s* op, size_t steps, size_t m, bool dyn) {
  const CsrDev A = csr_dev(op);
  const int ldy = (int)op->ycap;
  HIPCHK(launch::p2_minit(A, op->st.S, op->d_Y, ldy, op->b, op->V2[1], op->d_X, op->ld, (int)m,
                          op->stream));
  HIPCHK(launch::p2_coefs(op->st.S, (int)steps, dyn ? 1 : 0, op->stream));
  for (int j = 1; j < (int)steps; ++j) {
    launch_p2_step(op, A, j, j, 0, nullptr);
    const int nflush = p2_flush(j, (int)steps - 1);
    if (!nflush) continue;
    const P2Rot v = p2_rot(op, j);
    for (size_t c0 = 0; c0 < m; c0 += 8)
      HIPCHK(launch::p2_xacc_cut(A, op->d_Y + c0 * op->ycap, ldy, j, nflush,
                                 op->d_col_steps + c0, v.prev, v.cur, v.next,
                                 op->d_X + c0 * (size_t)op->ld, op->ld,
                                 (int)std::min<size_t>(8, m - c0), op->stream));
  }
}
static void check_multi_cut(const tpl_op_s* op, size_t steps, size_t m) {
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "multi-function solve of a partitioned operator");
  if (m == 0 || m > op->xcols || steps > op->ycap || m > TPL_MULTI_MAX || !op->d_col_steps)
    fail(TPL_ERR_INVALID_ARGUMENT, "run_pass2_multi_cut: buffers smaller than the request");
}
void run_pass2_multi_cut(tpl_op_s* op, size_t steps, size_t m) {
  check_multi_cut(op, steps, m);
  op->last_long_cache = steps >= 2 && long_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  run_graph(op, kGPass2MultiCut + graph_cache_kind(op), steps * (TPL_MULTI_MAX + 1) + m,
            [&] { enqueue_pass2_multi_cut(op, steps, m, false); });
}

// The one-graph shifted inverse solve: run_two_pass_inv_tol's pass one with k_p1_axpy_stol
// and k_p1_stol_fin, every (T + sigma_s I)^{-1} e_1 at its own m*_s by k_ftk_inv_shifts into
// the coefficient table, then the multi-function pass two with the cut. After the stop (every
// shift met the tolerance) the later launches of pass one return at their stop test, the step
// launches of pass two past M are inactive and the flush launches past M return at once.
void run_two_pass_shifted_inv_tol(tpl_op_s* op, size_t kmax, const launch::ShiftTol& t) {
  const size_t m = (size_t)t.m;
  check_multi_cut(op, kmax, m);
  const int ck = graph_cache_kind(op);
  op->last_long_cache = kmax >= 2 && ck != 0;
  op->last_fused_p2 = false;
  run_graph(op, kGTwoPassShiftedInvTol + ck, kmax * (TPL_MULTI_MAX + 1) + m, [&] {
    enqueue_p1_prologue(op);
    for (int j = 1; j <= (int)kmax; ++j) {
      CsrDev A = csr_dev(op, true);
      if (double* ycrow = ck ? cache_row(op, j) : nullptr) A.ypart = ycrow;
      launch_p1_spmv(op, A, j, nullptr, nullptr);
      HIPCHK(launch::p1_axpy_stol(A, op->st.S, op->W, r_of(op, j), op->R[(j + 1) % 3], j,
                                  (int)kmax, t, op->stream));
    }
    HIPCHK(launch::p1_stol_fin(op->st.S, t, op->stream));
    HIPCHK(launch::ftk_inv_shifts(op->st.S, (int)kmax, t, op->d_Y, (int)op->ycap,
                                  op->d_col_steps, 1, op->stream));
    enqueue_pass2_multi_cut(op, kmax, m, true);
  });
}

// ---- lock-step batch groups (tpl_lanczos_two_pass_batch): the single solve's launch
// sequences with the batch kernels, over the group's interleaved vectors. r_1 = b, then
// R[j % 3]; pass two reuses the ring for v (v_1 in R[1]).
static void enqueue_pass1_batch(tpl_op_s* op, size_t k, int nb) {
  const CsrDev A = csr_dev(op);
  BatchBufs& bb = op->bat;
  const BatchDev& S = bb.S;
  HIPCHK(launch::bp1_init(nb, A, S, bb.b, op->stream));
  auto r_of = [&](int j) { return j == 1 ? bb.b : bb.R[j % 3]; };
  for (int j = 1; j <= (int)k; ++j) {
    HIPCHK(launch::bp1_spmv(nb, A, S, r_of(j), j >= 2 ? r_of(j - 1) : nullptr, bb.W, j,
                            batch_cache_row(op, j, nb), op->stream));
    HIPCHK(launch::bp1_axpy(nb, A, S, bb.W, r_of(j), bb.R[(j + 1) % 3], j, (int)k, op->stream));
  }
}
// The batch pass-two step launch: step j of a group of nb columns over the ring (v_j in
// R[j % 3]). The single place that picks the batch step kernel: k_bp2_cached when the
// running batch solve's pass one, for this group, stored step j's row of the group's
// long-row cache (batch_cache_row), else the full k_bp2_spmv.
void launch_bp2_step(tpl_op_s* op, const CsrDev& A, int nb, int j) {
  BatchBufs& bb = op->bat;
  double *vp = j >= 2 ? bb.R[(j + 2) % 3] : nullptr, *vc = bb.R[j % 3], *vn = bb.R[(j + 1) % 3];
  if (const double* yc = batch_cache_row(op, j, nb)) {
    HIPCHK(launch::bp2_cached(nb, A, bb.S, vc, vp, vn, bb.x, yc, bb.d_ylrow, j, op->stream));
    return;
  }
  HIPCHK(launch::bp2_spmv(nb, A, bb.S, vc, vp, vn, bb.x, j, op->stream));
}
static void enqueue_pass2_batch(tpl_op_s* op, size_t kmax, int nb) {
  const CsrDev A = csr_dev(op);
  BatchBufs& bb = op->bat;
  const BatchDev& S = bb.S;
  HIPCHK(launch::bp2_init(nb, A, S, bb.b, bb.R[1], bb.x, op->stream));
  HIPCHK(launch::bp2_coefs(nb, S, (int)kmax, op->stream));
  for (int j = 1; j < (int)kmax; ++j) launch_bp2_step(op, A, nb, j);
}
static void check_batch(const tpl_op_s* op, size_t k, int nb) {
  if (op->dist) fail(TPL_ERR_UNSUPPORTED, "batch solve of a partitioned operator");
  if ((nb != 2 && nb != 4) || nb > op->bat.nb || k > op->bat.kcap)
    fail(TPL_ERR_INVALID_ARGUMENT, "batch group: buffers smaller than the request");
}
void run_pass1_batch(tpl_op_s* op, size_t k, int nb) {
  check_batch(op, k, nb);
  run_graph(op, kGPass1Batch + batch_graph_cache_kind(op), k * 8 + (size_t)nb,
            [&] { enqueue_pass1_batch(op, k, nb); });
}
void run_pass2_batch(tpl_op_s* op, size_t kmax, int nb) {
  check_batch(op, kmax, nb);
  op->last_long_cache = kmax >= 2 && batch_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  run_graph(op, kGPass2Batch + batch_graph_cache_kind(op), kmax * 8 + (size_t)nb,
            [&] { enqueue_pass2_batch(op, kmax, nb); });
}

// ---- m functions of every column of a group (tpl_lanczos_two_pass_batch_multi): the
// group's pass two with every record's nflush 0 (bp2_coefs0), so bp2_spmv regenerates
// v_{j+1} and leaves x alone, and after each step at which some column flushes bp2_xacc
// applies the grouped flush to every function's group vector, kBatchMultiFuncs functions
// per launch, from the three live ring vectors. The kernel takes each column's count from
// the device-held steps_c; the host's copy only decides which launches are worth making.
static void enqueue_pass2_batch_multi(tpl_op_s* op, const size_t* steps, int nb, size_t m) {
  const CsrDev A = csr_dev(op);
  BatchBufs& bb = op->bat;
  const BatchDev& S = bb.S;
  const int64_t xs = op->ld * nb;  // one function's group vector
  size_t kmax = 0;
  for (int c = 0; c < nb; ++c) kmax = std::max(kmax, steps[c]);
  HIPCHK(launch::bp2_minit(nb, A, S, bb.d_my, (int)m, bb.b, bb.R[1], bb.d_mx, xs, op->stream));
  HIPCHK(launch::bp2_coefs0(nb, S, (int)kmax, op->stream));
  for (int j = 1; j < (int)kmax; ++j) {
    double *vp = bb.R[(j + 2) % 3], *vc = bb.R[j % 3], *vn = bb.R[(j + 1) % 3];
    launch_bp2_step(op, A, nb, j);
    bool any = false;
    for (int c = 0; c < nb; ++c)
      any = any || (j < (int)steps[c] && p2_flush(j, (int)steps[c] - 1) > 0);
    if (!any) continue;
    for (size_t f0 = 0; f0 < m; f0 += kBatchMultiFuncs)
      HIPCHK(launch::bp2_xacc(nb, A, S, bb.d_my + f0 * (size_t)nb * bb.kcap, j, vp, vc, vn,
                              bb.d_mx + f0 * (size_t)xs, xs,
                              (int)std::min<size_t>(kBatchMultiFuncs, m - f0), op->stream));
  }
}
void run_pass2_batch_multi(tpl_op_s* op, const size_t* steps, int nb, size_t m) {
  size_t kmax = 0;
  bool even = true;
  for (int c = 0; c < nb; ++c) {
    kmax = std::max(kmax, steps[c]);
    even = even && steps[c] == steps[0];
  }
  check_batch(op, kmax, nb);
  if (m == 0 || m > op->bat.mcols || m > TPL_MULTI_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "batch-multi group: buffers smaller than the request");
  op->last_long_cache = kmax >= 2 && batch_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  if (!even) {  // the launch list depends on every steps_c: not captured
    enqueue_pass2_batch_multi(op, steps, nb, m);
    return;
  }
  run_graph(op, kGPass2BatchMulti + batch_graph_cache_kind(op),
            (kmax * 8 + (size_t)nb) * (TPL_MULTI_MAX + 1) + m,
            [&] { enqueue_pass2_batch_multi(op, steps, nb, m); });
}

// The same with a cut per (column, function) (tpl_lanczos_pass_two_batch_multi_cut and the
// batch shifted inverse solve): k_bp2_xacc_cut in place of k_bp2_xacc, the counts in
// op->d_bcut. The step launches run for `steps` (the group's largest steps_c on the
// host-composed paths, the count asked for in the one-graph solve), each column active below
// its device-held steps_c (bp2_coefs0), and x is flushed by the single schedule for `steps`
// (p2_flush: multiples of 3 and once after the last launch); the cut covers every column's
// and every function's ragged end. The terms a result gets, and their order, are the same
// whatever `steps` is.
static void enqueue_pass2_batch_multi_cut(tpl_op_s* op, size_t steps, int nb, size_t m) {
  const CsrDev A = csr_dev(op);
  BatchBufs& bb = op->bat;
  const BatchDev& S = bb.S;
  const int64_t xs = op->ld * nb;  // one function's group vector
  HIPCHK(launch::bp2_minit(nb, A, S, bb.d_my, (int)m, bb.b, bb.R[1], bb.d_mx, xs, op->stream));
  HIPCHK(launch::bp2_coefs0(nb, S, (int)steps, op->stream));
  for (int j = 1; j < (int)steps; ++j) {
    double *vp = bb.R[(j + 2) % 3], *vc = bb.R[j % 3], *vn = bb.R[(j + 1) % 3];
    launch_bp2_step(op, A, nb, j);
    const int nflush = p2_flush(j, (int)steps - 1);
    if (!nflush) continue;
    for (size_t f0 = 0; f0 < m; f0 += kBatchMultiFuncs)
      HIPCHK(launch::bp2_xacc_cut(nb, A, S, op->d_bcut + f0, TPL_MULTI_MAX,
                                  bb.d_my + f0 * (size_t)nb * bb.kcap, j, nflush, vp, vc, vn,
                                  bb.d_mx + f0 * (size_t)xs, xs,
                                  (int)std::min<size_t>(kBatchMultiFuncs, m - f0), op->stream));
  }
}
static void check_batch_multi_cut(const tpl_op_s* op, size_t steps, int nb, size_t m) {
  check_batch(op, steps, nb);
  if (m == 0 || m > op->bat.mcols || m > TPL_MULTI_MAX || !op->d_bcut)
    fail(TPL_ERR_INVALID_ARGUMENT, "batch-multi group: buffers smaller than the request");
}
void run_pass2_batch_multi_cut(tpl_op_s* op, size_t steps, int nb, size_t m) {
  check_batch_multi_cut(op, steps, nb, m);
  op->last_long_cache = steps >= 2 && batch_cache_steps(op) > 0;
  op->last_fused_p2 = false;
  run_graph(op, kGPass2BatchMultiCut + batch_graph_cache_kind(op),
            (steps * 8 + (size_t)nb) * (TPL_MULTI_MAX + 1) + m,
            [&] { enqueue_pass2_batch_multi_cut(op, steps, nb, m); });
}

// One group of the batch shifted inverse solve as one graph: run_pass1_batch's sequence with
// k_bp1_axpy_stol in place of k_bp1_axpy, k_bp1_stol_fin, every (T_c + sigma_i I)^{-1} e_1 at
// its own m*_{c,i} by k_ftk_inv_shifts — one launch per column, in series, on column c's view
// of the group state, into the batch-multi coefficient layout and column c's row of the cut
// table — then the batch-multi pass two with the cut. A column whose shifts have all met the
// tolerance stores nothing more; once every column has stopped the later launches of pass one
// return at their stop test, the step launches of pass two past every M_c are inactive and
// the flush launches past every cut return at once.
void run_two_pass_batch_shifted_inv_tol(tpl_op_s* op, size_t kmax, int nb,
                                        const launch::BatchShiftTol& t) {
  const size_t m = (size_t)t.t0.m;
  check_batch_multi_cut(op, kmax, nb, m);
  const int ck = batch_graph_cache_kind(op);
  op->last_long_cache = kmax >= 2 && ck != 0;
  op->last_fused_p2 = false;
  run_graph(op, kGTwoPassBatchShiftedInvTol + ck,
            (kmax * 8 + (size_t)nb) * (TPL_MULTI_MAX + 1) + m, [&] {
    const CsrDev A = csr_dev(op);
    BatchBufs& bb = op->bat;
    const BatchDev& S = bb.S;
    HIPCHK(launch::bp1_init(nb, A, S, bb.b, op->stream));
    auto r_of = [&](int j) { return j == 1 ? bb.b : bb.R[j % 3]; };
    for (int j = 1; j <= (int)kmax; ++j) {
      HIPCHK(launch::bp1_spmv(nb, A, S, r_of(j), j >= 2 ? r_of(j - 1) : nullptr, bb.W, j,
                              batch_cache_row(op, j, nb), op->stream));
      HIPCHK(launch::bp1_axpy_stol(nb, A, S, bb.W, r_of(j), bb.R[(j + 1) % 3], j, (int)kmax, t,
                                   op->stream));
    }
    HIPCHK(launch::bp1_stol_fin(nb, S, t, op->stream));
    for (int c = 0; c < nb; ++c) {
      DevState Sc{};  // column c's part of the group state, as k_ftk_inv_shifts reads it
      Sc.flags = S.flags + 8 * c;
      Sc.norms = S.norms + (size_t)c * (S.kcap + 1);
      Sc.alphas = S.alphas + (size_t)c * S.kcap;
      Sc.betas = S.betas + (size_t)c * S.kcap;
      Sc.kcap = S.kcap;
      HIPCHK(launch::ftk_inv_shifts(Sc, (int)kmax, t.col(c), bb.d_my + (size_t)c * bb.kcap,
                                    nb * (int)bb.kcap, op->d_bcut + (size_t)c * TPL_MULTI_MAX, 1,
                                    op->stream));
    }
    enqueue_pass2_batch_multi_cut(op, kmax, nb, m);
  });
}

// Copy flags | norms[0] | alphas | betas back (one D2H), synchronise.
HostDecomp fetch_decomp(tpl_op_s* op) {
  const size_t kc = op->st.kcap;
  char* h = (char*)op->st.h_state;
  const size_t bytes = kFlagBytes + ((kc + 1) + 2 * kc) * sizeof(double);
  HIPCHK(hipMemcpyAsync(h, op->st.d_state, bytes, hipMemcpyDeviceToHost, op->stream));
  sync_checked(op);
  HostDecomp d;
  std::memcpy(d.flags, h, kFlagBytes);
  const double* norms = (const double*)(h + kFlagBytes);
  d.b_norm = norms[0];
  d.alphas = norms + (kc + 1);
  d.betas = d.alphas + kc;
  d.steps = (size_t)d.flags[2];
  return d;
}

// The whole two-pass solve as one graph (or, with live timing on, as several graphs with
// the events between them); no host round trip between the passes.
void run_two_pass_dev(tpl_op_s* op, size_t k, int f) {
  const size_t key = 2 * k + (size_t)f;  // one graph per (k, f)
  const int elim = f == kDevInv ? kP1Elim : 0;  // T_k's LU eliminated during pass one
  const int ck = graph_cache_kind(op);
  op->last_long_cache = k >= 2 && ck != 0;
  const bool fused = fused_p2(op);
  op->last_fused_p2 = k >= 2 && fused;
  if (!op->timing) {
    op->p1_samples = 0;  // the untimed graph records no launch stamps
    run_graph(op, kGTwoPassDev + ck, key, [&] {
      enqueue_pass1(op, k, elim | (ck ? kP1Cache : 0));
      enqueue_ftk_dev(op, k, f);
      if (fused) {
        enqueue_pass2_fused(op, 0);
      } else {
        enqueue_pass2_dyn_steps(op, k);
        enqueue_pass2_tail(op);
      }
    });
    return;
  }
  HIPCHK(hipEventRecord(op->tev[0], op->stream));
  const bool stamped = !op->dist && stamp_first(k) > 0;
  if (stamped && !op->d_stamps) {
    dev_alloc(op, &op->d_stamps, 32 * sizeof(unsigned long long));
    dev_zero(op, op->d_stamps, 32 * sizeof(unsigned long long));
  }
  run_pass1_graph(op, k, elim | (stamped ? kP1Stamped : 0));
  op->p1_samples = stamped ? kStampSteps : 0;
  HIPCHK(hipEventRecord(op->tev[1], op->stream));
  run_graph(op, kGDevFtk, key, [&] { enqueue_ftk_dev(op, k, f); });
  HIPCHK(hipEventRecord(op->tev[2], op->stream));
  run_graph(op, kGPass2Dyn + ck, k, [&] {
    if (fused) enqueue_pass2_fused(op, 0);
    else enqueue_pass2_dyn_steps(op, k);
  });
  HIPCHK(hipEventRecord(op->tev[3], op->stream));
  if (!fused) enqueue_pass2_tail(op);
  op->p2_launches = (int64_t)k - 1;
}

// The one-graph inverse solve that stops at a residual tolerance: run_two_pass_dev's graph
// for inv with k_p1_axpy_tol in place of k_p1_axpy (the SpMV launches, the long-row cache
// and the choice of pass two are its own), and k_p1_tol_fin between pass one and k_ftk_inv.
// After the stop every later launch of pass one returns at its stop test, and pass two takes
// steps_taken from the device as after a breakdown. No live timing.
void run_two_pass_inv_tol(tpl_op_s* op, size_t kmax) {
  const int ck = graph_cache_kind(op);
  op->last_long_cache = kmax >= 2 && ck != 0;
  const bool fused = fused_p2(op);
  op->last_fused_p2 = kmax >= 2 && fused;
  run_graph(op, kGTwoPassInvTol + ck, kmax, [&] {
    enqueue_p1_prologue(op);
    for (int j = 1; j <= (int)kmax; ++j) {
      CsrDev A = csr_dev(op, true);
      if (double* ycrow = ck ? cache_row(op, j) : nullptr) A.ypart = ycrow;
      launch_p1_spmv(op, A, j, nullptr, nullptr);
      HIPCHK(launch::p1_axpy_tol(A, op->st.S, op->W, r_of(op, j), op->R[(j + 1) % 3], j,
                                 (int)kmax, op->d_tol, op->stream));
    }
    HIPCHK(launch::p1_tol_fin(op->st.S, op->d_tol, op->stream));
    enqueue_ftk_dev(op, kmax, kDevInv);
    if (fused) {
      enqueue_pass2_fused(op, 0);
    } else {
      enqueue_pass2_dyn_steps(op, kmax);
      enqueue_pass2_tail(op);
    }
  });
}

// elim: eliminate T_k's LU during the pass (a device inv follows: k_ftk_inv)
void run_pass_one(tpl_op_s* op, const double* b, size_t k, int mem, bool storeV, int reorth,
                  bool elim) {
  ensure_state(op, k, reorth);
  if (storeV) ensure_basis(op, k);
  upload_vec(op, op->b, b, mem);
  op->p1_samples = 0;  // no pass run here records launch stamps (tpl_op_step_samples)
  if (reorth) {
    enqueue_pass1(op, k, kP1Basis, reorth); // eager: reorth launch counts vary with j
  } else {
    if (op->timing) HIPCHK(hipEventRecord(op->tev[0], op->stream));
    run_pass1_graph(op, k, (storeV ? kP1Basis : 0) | (elim ? kP1Elim : 0));
    if (op->timing) HIPCHK(hipEventRecord(op->tev[1], op->stream));
  }
}

} // namespace tpl
