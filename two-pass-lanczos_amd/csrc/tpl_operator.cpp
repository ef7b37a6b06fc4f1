// tpl_operator.cpp — operator lifetime: what an operator owns and how it is released,
// the layout's device buffers and the schedule rebuild, the solver state and basis,
// vectors in and out, and the create / destroy / schedule entry points of the C ABI
// (include/tpl.h). The planner is tpl_partition, the layout builder tpl_layout.
#include "tpl_op.h"

#ifndef TPL_LAB
#define TPL_LAB 0  // lab builds only (scripts/build_variants.sh): runtime layout knobs
#endif

using namespace tpl;

tpl_op_s::~tpl_op_s() {
  graphs.clear();
  for (const auto& kv : allocs) hipFree(const_cast<void*>(kv.first));  // every dev_alloc
  if (st.h_state) hipHostFree(st.h_state);
  if (h_exp_back) hipHostFree(h_exp_back);
  if (h_tol) hipHostFree(h_tol);
  if (h_stol) hipHostFree(h_stol);
  if (bat.h_stol) hipHostFree(bat.h_stol);
  if (h_expb_back) hipHostFree(h_expb_back);
  if (ev0) hipEventDestroy(ev0);
  if (ev1) hipEventDestroy(ev1);
  for (hipEvent_t e : tev)
    if (e) hipEventDestroy(e);
}

namespace tpl {

int long_epi_blocks(const tpl_op_s* op) {
  return (int)((op->lay.lrows.size() + kLongEpiRows - 1) / kLongEpiRows);
}

// The layout's format fields, the ones variant_of reads (tpl_device.h): set here for the
// launchers' CsrDev and for tpl_op_kernel_variant alike.
static void format_fields(const Layout& L, CsrDev& A) {
  A.val_i8 = L.val_i8 ? 1 : 0;
  A.s_col16 = L.s_col16 ? 1 : 0;
  A.b_col16 = L.b_col16 ? 1 : 0;
  A.s_width = L.s_width;
  A.s_win = L.s_win;
}

CsrDev csr_dev(const tpl_op_s* op, bool pass1) {
  const Layout& L = op->lay;
  CsrDev A;
  format_fields(L, A);
  A.srows = op->bufs.d_srows;
  A.s_col = op->bufs.d_scol;
  A.s_val = op->bufs.d_sval;
  A.s_cbase = op->bufs.d_scbase;
  A.b_cbase = op->bufs.d_bcbase;
  A.c_base = op->bufs.d_cbase;
  A.c_width = op->bufs.d_cwidth;
  A.b_col = op->bufs.d_bcol;
  A.b_val = op->bufs.d_bval;
  A.b_seg = op->bufs.d_bseg;
  A.b_hdr = op->bufs.d_bhdr;
  A.P = op->bufs.d_P;
  A.Pcnt = op->bufs.d_Pcnt;
  A.s_identity = L.s_identity;
  A.n_short = (int32_t)L.srows.size();
  A.n_chunks = (int32_t)L.c_base.size();
  A.n_long = (int32_t)L.lrows.size();
  A.bin_cap = L.bin_cap;
  A.n_slices = L.nslices;
  A.n_slice_blocks = L.nslices * L.M;
  A.G2 = L.G2;
  A.NA = A.n_chunks + A.n_long;
  A.NA_r = op->dist ? op->dist->nranks + (op->part.hybrid ? long_epi_blocks(op) : 0) : A.NA;
  A.G2_r = op->dist ? op->dist->nranks : A.G2;
  A.pb_ld = op->pb_ld;
  A.long_defer = op->part.hybrid ? 1 : 0;
  A.y_ld = pass1 && op->part.hybrid ? op->y_ld1 : (int32_t)L.lrows.size() + 1;
  A.ypart = op->part.hybrid ? op->d_yall + (size_t)op->dist->rank * A.y_ld : nullptr;
  A.nch = op->d_nch;
  A.norm_n = op->part.hybrid && op->dist->rank != 0 ? op->part.ns_local : op->part.n;
  A.s_win_max = L.s_win_max;
  A.n = op->part.n;
  A.E = L.E;
  return A;
}

uint64_t device_bytes(const tpl_op_s* op) {
  uint64_t t = 0;
  for (const auto& kv : op->allocs) t += kv.second;
  return t;
}

void dev_alloc_bytes(tpl_op_s* op, void** p, size_t bytes) {
  if (const char* cap = std::getenv("TPL_TEST_ALLOC_CAP"))
    if (device_bytes(op) + bytes > std::strtoull(cap, nullptr, 10))
      fail(TPL_ERR_OUT_OF_MEMORY,
           std::string("hipMalloc(p, bytes): ") + hipGetErrorString(hipErrorOutOfMemory));
  HIPCHK(hipMalloc(p, bytes));
  op->allocs[*p] = bytes;
}

namespace {

template <class T>
void upload(tpl_op_s* op, T** dst, const std::vector<T>& src) {
  dev_free(op, *dst);
  if (src.empty()) return;
  dev_alloc(op, dst, src.size() * sizeof(T));
  HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
}

void free_bufs(tpl_op_s* op, LayoutBufs& b) {
  dev_free(op, b.d_scol), dev_free(op, b.d_sval), dev_free(op, b.d_bcol), dev_free(op, b.d_bval);
  dev_free(op, b.d_srows), dev_free(op, b.d_scbase), dev_free(op, b.d_cbase);
  dev_free(op, b.d_cwidth), dev_free(op, b.d_bcbase), dev_free(op, b.d_bhdr);
  dev_free(op, b.d_bseg), dev_free(op, b.d_P), dev_free(op, b.d_Pcnt);
  dev_free(op, b.d_perm), dev_free(op, b.d_iperm), dev_free(op, b.d_stage);
  dev_free(op, b.d_hrow), dev_free(op, b.d_hent), dev_free(op, b.d_hval);
}

// A layout (and its row order) into a fresh set of device buffers.
void upload_layout(tpl_op_s* op, const Layout& L, const std::vector<int32_t>& perm,
                   const std::vector<int32_t>& iperm, LayoutBufs& nb) {
  upload(op, &nb.d_perm, perm);
  upload(op, &nb.d_iperm, iperm);
  if (!perm.empty()) dev_alloc(op, &nb.d_stage, perm.size() * sizeof(double));
  upload(op, &nb.d_srows, L.srows);
  upload(op, &nb.d_hrow, L.fp2.h_row);
  upload(op, &nb.d_hent, L.fp2.h_ent);
  upload(op, &nb.d_hval, L.fp2.h_val);
  // entries in the device order (tpl_device.h kPackedEntries; positions unchanged)
  const bool pack_s = packed_chunk_width(L.s_width);
  auto sidx = [&](int64_t i) { return pack_s ? packed_chunk_index(i, L.s_width) : i; };
  auto bidx = [&](int64_t i) { return kPackedEntries ? packed_bin_index(i, L.bin_cap) : i; };
  if (L.s_col16)
    upload(op, reinterpret_cast<uint16_t**>(&nb.d_scol), to_device_order(L.s_col16v, sidx));
  else
    upload(op, reinterpret_cast<int32_t**>(&nb.d_scol), to_device_order(L.s_col, sidx));
  upload(op, &nb.d_scbase, L.s_cbase);
  if (L.val_i8)
    upload(op, reinterpret_cast<int8_t**>(&nb.d_sval), to_device_order(L.s_val8, sidx));
  else
    upload(op, reinterpret_cast<double**>(&nb.d_sval), to_device_order(L.s_val, sidx));
  upload(op, &nb.d_cbase, L.c_base);
  upload(op, &nb.d_cwidth, L.c_width);
  if (L.b_col16)
    upload(op, reinterpret_cast<uint16_t**>(&nb.d_bcol), to_device_order(L.b_col16v, bidx));
  else
    upload(op, reinterpret_cast<int32_t**>(&nb.d_bcol), to_device_order(L.b_col, bidx));
  upload(op, &nb.d_bcbase, L.b_cbase);
  if (L.val_i8)
    upload(op, reinterpret_cast<int8_t**>(&nb.d_bval), to_device_order(L.b_val8, bidx));
  else
    upload(op, reinterpret_cast<double**>(&nb.d_bval), to_device_order(L.b_val, bidx));
  upload(op, &nb.d_bseg, L.b_seg);
  upload(op, &nb.d_bhdr, L.b_hdr);
  // piece slots, and the arrival counters of the sliced long rows (zero; each wraps at
  // its row's packed-piece count, BinSeg::pad + 1, so it runs on across launches)
  upload(op, &nb.d_P, std::vector<double>(std::max<size_t>(L.lrows.size() * kSlotStride, 1), 0.0));
  upload(op, &nb.d_Pcnt,
         std::vector<unsigned int>(std::max<size_t>(L.lrows.size() * kCntStride, 1), 0u));
}

void free_state(tpl_op_s* op, SolverState& s) {
  dev_free(op, s.d_state), dev_free(op, s.d_Pr), dev_free(op, s.d_ycache);
  if (s.h_state) hipHostFree(s.h_state);
  s = SolverState{};
}

// How a partition's gathered vectors hold the ranks' parts: a row partition keeps R
// copies' worth (R = nranks; every other operator one), and plain row blocks gather whole
// blocks, so that a rank's own vector is the rank-th slice (halo blocks: the first).
struct Gathered {
  int R;
  bool blocks;
};
Gathered gather_rule(const tpl_op_s* op) {
  const bool rows = op->dist && !op->part.hybrid;
  return {rows ? op->dist->nranks : 1, rows && !op->part.halo};
}

} // namespace

// The operator's row order, Layout and their device buffers under the schedule parameters
// `cand` and the order mode `reorder`. Everything is built aside and swapped into the
// operator only once it is complete, `cand` and `reorder` with it: when anything throws
// (a layout the kernels or the partition cannot hold, device memory), the operator keeps
// its layout, buffers, graphs, state and parameters, and what was allocated on the way is
// freed. The price: while both sets exist a rebuild's peak device memory is one layout's
// worth higher (init_op's first build has no old set).
void rebuild_schedule(tpl_op_s* op, const SchedParams& cand, int reorder) {
  if (op->dense) {
    // A dense operator's schedule is a rule (tpl_dense_schedule), not a build: every row a
    // long row in the caller's order, S column slices, the element geometry of n rows. The
    // slice count only changes the kernels' loop bounds: the state and its partial arrays
    // (NA = n, G2) stay, the graphs hold the old count and go.
    Layout L;
    L.lrows.resize((size_t)op->part.n);
    for (int64_t i = 0; i < op->part.n; ++i) L.lrows[(size_t)i] = (int32_t)i;
    L.s_identity = 1;
    L.nslices = cand.slices > 0 ? cand.slices : auto_slices(op->part.n);
    elem_geometry(op->part.n, SchedParams{}, L.G2, L.E);
    op->sp = cand;
    op->reorder = reorder;
    op->lay = std::move(L);
    if (!op->plan_only) drop_graphs(op);
    return;
  }
  ColMap cmap;
  const RankPlan& part = op->part;
  if (part.halo) {
    cmap.table = &part.halo_map;
  } else if (op->dist && !part.hybrid) {
    cmap.starts = &part.starts;
    cmap.ld = op->ld;
  }
  std::vector<int32_t> perm, iperm;
  const bool want = reorder == 1 || (reorder == 2 && part.n <= kReorderAutoMaxRows);
  if (want && !op->dist) perm = locality_order(part.n, part.h_rowptr, part.h_col, cand);
  std::vector<int32_t> prp, pcol;
  std::vector<double> pval;
  const bool p = !perm.empty();
  if (p) {
    iperm.resize(part.n);
    for (int64_t i = 0; i < part.n; ++i) iperm[perm[i]] = (int32_t)i;
    permute_csr(part.n, part.h_rowptr, part.h_col, part.h_val, perm, iperm, prp, pcol, pval);
  }
  // In the locality order a chunk's rows share their hub columns, so its gathers hit
  // few lines and the LDS window costs more than it saves (measured +0.4 us per SpMV at
  // 500k): window only in the caller's order.
  SchedParams sp = cand;
  sp.window = !p && !part.local_order;
#if TPL_LAB
  // layout knobs of the lab builds (scripts/build_variants.sh -DTPL_LAB=1), never in the
  // product library: the measured alternatives of DESIGN.md §3/§4
  if (const char* e = std::getenv("TPL_WINDOW")) sp.window = std::atoi(e) != 0;
  if (const char* e = std::getenv("TPL_ELEM_ROWS")) sp.elem_rows = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_LINES")) sp.bin_lines = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_SEGS")) sp.bin_segs = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_BIG")) sp.bin_big = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_SMALL")) sp.bin_small = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_BALANCE")) sp.bin_balance = std::atoi(e);
  if (const char* e = std::getenv("TPL_BIN_CROWD")) sp.bin_crowd = std::atof(e);
  if (const char* e = std::getenv("TPL_SLICES")) {  // auto slice count only; the values
    const int s = std::atoi(e);                     // tpl_op_set_slices accepts
    if (sp.slices <= 0 && s > 0 && s <= kSlices && (s & (s - 1)) == 0) sp.slices = s;
  }
#endif
  // slice bounds over global columns — or, replicated-long-row partition, over this
  // rank's local columns (its CSR is stored in local indices)
  Layout L = build_layout(part.n, part.hybrid ? part.n : part.n_glob, p ? prp : part.h_rowptr,
                          p ? pcol : part.h_col, p ? pval : part.h_val, sp, cmap);
  // the replicated partition's ranks agree on every rank's element-wise block count (the
  // gathered norm partials, the alpha partial counts): a layout that changed it is refused
  if (part.hybrid && !part.g2s.empty() && L.G2 != part.g2s[op->dist->rank])
    fail(TPL_ERR_UNSUPPORTED, "replicated partition: the element-wise blocks must stay those "
                              "every rank computed from the split");
  LayoutBufs nb;  // the new set; after the swap below, the old one
  try {
    if (!op->plan_only) upload_layout(op, L, perm, iperm, nb);  // a plan holds the layout only
  } catch (...) {
    free_bufs(op, nb);
    throw;
  }
  // commit: nothing below throws
  op->sp = cand;
  op->reorder = reorder;
  op->lay = std::move(L);
  op->perm = std::move(perm);
  op->iperm = std::move(iperm);
  if (op->plan_only) return;
  std::swap(op->bufs, nb);
  free_bufs(op, nb);
  dev_free(op, op->d_Vext);
  op->vext_cols = 0;
  drop_graphs(op);
  // partial buffers depend on the layout: force state reallocation
  op->st.kcap = 0;
  free_batch(op);
}

// ---- long-row cache (tpl_op_set_long_cache) ----------------------------------------------
// Default budget: two vectors' bytes, so the two-pass footprint stays O(n): at most 12
// vectors instead of 10.
uint64_t long_cache_default_budget(int64_t n) { return 2 * 8 * (uint64_t)padded_stride(n); }
uint64_t long_cache_rows(int mode, uint64_t budget_bytes, int64_t n, int64_t n_long, uint64_t kcap) {
  if (mode == 0 || n_long <= 0) return 0;
  const uint64_t budget = mode == 1 ? budget_bytes : long_cache_default_budget(n);
  return std::min<uint64_t>(kcap, budget / (8 * (uint64_t)n_long));
}
namespace {
// Steps the operator's cache should hold at a state capacity of kc steps. No cache for a
// partitioned operator (its ypart is the exchange's).
size_t wanted_cache_rows(const tpl_op_s* op, size_t kc) {
  // nor for a dense one: caching every row's sum would be the standard method's memory
  if (op->dist || op->dense) return 0;
  return (size_t)long_cache_rows(op->long_cache, op->long_cache_budget, op->part.n,
                                 (int64_t)op->lay.lrows.size(), kc);
}
// A zeroed cache of `rows` steps into s (a one-graph solve's inactive launches read rows
// no pass one wrote). Unless the long rows are the last rows (s_identity: long row l is row
// n - n_long + l), their row indices follow the sums in the same allocation.
void alloc_cache(tpl_op_s* op, SolverState& s, size_t rows) {
  if (rows == 0) return;
  const std::vector<int32_t>& lr = op->lay.lrows;
  const size_t sums = rows * lr.size() * sizeof(double);
  const size_t table = op->lay.s_identity ? 0 : (lr.size() * sizeof(int32_t) + 7) / 8 * 8;
  dev_alloc(op, &s.d_ycache, sums + table);
  dev_zero(op, s.d_ycache, sums);
  if (table) {
    s.d_ylrow = reinterpret_cast<int32_t*>(s.d_ycache + rows * lr.size());
    HIPCHK(hipMemcpy(s.d_ylrow, lr.data(), lr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  s.yrows = rows;
}
} // namespace

// state layout: [flags: 8 int32 (kFlagBytes)] [norms kcap+1] [alphas kcap] [betas kcap] [y kcap]
// [Pa NA] [Pb G2] [p2c 8 kcap] [lu 4 kcap + 3]; reorthogonalisation partials separately (d_Pr).
// A larger state is built aside and swapped in once it is complete (as rebuild_schedule
// does the layout): when an allocation throws, the operator keeps its state, its kcap and
// its graphs, and what was allocated on the way is freed. The price: while both blocks
// exist the peak device memory is one state block higher (about 20 k doubles plus the
// partial arrays). The long-row cache is part of the state: sized with it, built aside with
// it, and rebuilt alone (the same way) when only its mode or budget changed.
void ensure_state(tpl_op_s* op, size_t k, bool reorth) {
  if (k <= op->st.kcap && wanted_cache_rows(op, op->st.kcap) != op->st.yrows) {
    SolverState ns;  // carries the new cache only; after the swap below, the old one
    try {
      alloc_cache(op, ns, wanted_cache_rows(op, op->st.kcap));
    } catch (...) {
      dev_free(op, ns.d_ycache);
      throw;
    }
    std::swap(op->st.d_ycache, ns.d_ycache);
    std::swap(op->st.d_ylrow, ns.d_ylrow);
    std::swap(op->st.yrows, ns.yrows);
    dev_free(op, ns.d_ycache);
    drop_graphs(op);
  }
  if (k > op->st.kcap) {
    const size_t kc = std::max<size_t>(k, 16);
    const CsrDev A = csr_dev(op);
    // [.. | Pb G2 | pad to 64 B | p2c: 8 kc step records | lu: 4 kc + 3]
    const size_t head = kFlagBytes / sizeof(double) + (kc + 1) + 3 * kc +
                        (size_t)std::max(A.NA, 1) + (size_t)A.G2;
    const size_t p2c_off = (head + 7) / 8 * 8;  // in doubles from the base (64-B aligned)
    const size_t doubles = p2c_off - kFlagBytes / sizeof(double) + 8 * kc + 4 * kc + 3;
    const size_t bytes = kFlagBytes + doubles * sizeof(double);
    SolverState ns;  // the new state; after the swap below, the old one
    try {
      dev_alloc(op, &ns.d_state, bytes);
      dev_zero(op, ns.d_state, bytes);
      HIPCHK(hipHostMalloc(&ns.h_state, kFlagBytes + (4 * kc + 1) * sizeof(double),
                           hipHostMallocDefault));
      alloc_cache(op, ns, wanted_cache_rows(op, kc));
    } catch (...) {
      free_state(op, ns);
      throw;
    }
    char* base = (char*)ns.d_state;
    DevState& S = ns.S;
    S.flags = (int32_t*)base;
    S.norms = (double*)(base + kFlagBytes);
    S.alphas = S.norms + (kc + 1);
    S.betas = S.alphas + kc;
    S.y = S.betas + kc;
    S.Pa = S.y + kc;
    S.Pb = S.Pa + std::max(A.NA, 1);
    S.p2c = reinterpret_cast<double*>(base) + p2c_off;
    S.lu = S.p2c + 8 * kc;
    S.kcap = (int32_t)kc;
    // hybrid: the chunks' alpha partials go straight into this rank's pass-one segment of
    // the all-gather (k_long_epi_p1 reduces every rank's after the exchange)
    if (op->part.hybrid)
      S.Pa = op->d_yall + (size_t)op->dist->rank * op->y_ld1 + op->lay.lrows.size();
    S.Pa_r = op->dist ? op->d_rsum : S.Pa;
    S.Pb_r = op->dist ? op->d_rsum + A.NA_r : S.Pb;
    if (op->pb_ld > 0) {  // the norm partials go straight into this rank's gathered segment
      S.Pb = op->d_pball + (size_t)op->dist->rank * op->pb_ld;
      S.Pb_r = op->d_pball;
    }
    ns.kcap = kc;
    // commit: nothing below throws; the graphs hold the old state's pointers
    std::swap(op->st, ns);
    free_state(op, ns);
    drop_graphs(op);
  }
  if (reorth && !op->st.d_Pr) {
    // [cols x G partials][cols coefficients][G norm partials after the first pass][skip flag]
    // [kcap per-step second-pass records (int)]
    dev_alloc(op, &op->st.d_Pr,
              (((size_t)op->lay.G2 + 2) * op->st.kcap + (size_t)op->lay.G2 + 1) * sizeof(double));
  }
}

// The basis and the callback's view free before they grow (n x k doubles: two copies
// would not fit where one does); the column count is zero whenever the pointer is null.
void ensure_basis(tpl_op_s* op, size_t cols) {
  if (cols <= op->vcols && op->d_V) return;
  drop_graphs(op);
  dev_free(op, op->d_V);
  op->vcols = 0;
  const size_t c = std::max<size_t>(cols, 1);
  dev_alloc(op, &op->d_V, (size_t)op->part.n * c * sizeof(double) + 64);
  op->vcols = c;
}
// Freed before they grow, as the basis is.
void ensure_multi(tpl_op_s* op, size_t m) {
  const size_t kc = op->st.kcap;
  if (m <= op->xcols && kc <= op->ycap && op->d_X) return;
  const size_t cols = std::max(m, op->xcols), cap = std::max(kc, op->ycap);
  drop_graphs(op);
  dev_free(op, op->d_X);
  dev_free(op, op->d_Y);
  op->xcols = op->ycap = 0;
  dev_alloc(op, &op->d_X, cols * (size_t)op->ld * sizeof(double));
  dev_alloc(op, &op->d_Y, cols * cap * sizeof(double));
  op->xcols = cols;
  op->ycap = cap;
}
namespace {
void ensure_exp_ts(tpl_op_s* op) {
  if (op->d_exp_ts) return;
  dev_alloc(op, &op->d_exp_ts, TPL_MULTI_MAX * sizeof(double));
  dev_zero(op, op->d_exp_ts, TPL_MULTI_MAX * sizeof(double));
}
} // namespace
void ensure_exp_times_batch(tpl_op_s* op) {
  constexpr size_t bytes = (size_t)kBatchNbMax * TPL_MULTI_MAX * sizeof(int32_t);
  ensure_exp_ts(op);
  if (!op->d_expb_back) {
    dev_alloc(op, &op->d_expb_back, bytes);
    dev_zero(op, op->d_expb_back, bytes);
  }
  if (!op->h_expb_back)
    HIPCHK(hipHostMalloc((void**)&op->h_expb_back, bytes, hipHostMallocDefault));
}
void ensure_exp_times(tpl_op_s* op) {
  ensure_exp_ts(op);
  if (!op->d_exp_back) {
    dev_alloc(op, &op->d_exp_back, TPL_MULTI_MAX * sizeof(int32_t));
    dev_zero(op, op->d_exp_back, TPL_MULTI_MAX * sizeof(int32_t));
  }
  if (!op->h_exp_back)
    HIPCHK(hipHostMalloc((void**)&op->h_exp_back, TPL_MULTI_MAX * sizeof(int32_t),
                         hipHostMallocDefault));
}
namespace {
// A tolerance-stop family's device block and its pinned mirror, replaced by a zeroed block of
// dev_bytes and a mirror of host_bytes. The graphs hold the old block's pointer and go with it
// (a first allocation drops nothing). The caller zeroes its capacities before and sets them
// after: a refused allocation leaves them zero, so the next call starts over.
void replace_stop_block(tpl_op_s* op, double*& dev, void*& host, size_t dev_bytes,
                        size_t host_bytes) {
  if (dev) drop_graphs(op);
  dev_free(op, dev);
  if (host) hipHostFree(host);
  host = nullptr;
  dev_alloc(op, &dev, dev_bytes);
  dev_zero(op, dev, dev_bytes);
  HIPCHK(hipHostMalloc(&host, host_bytes, hipHostMallocDefault));
}
} // namespace
void ensure_tol(tpl_op_s* op) {
  const size_t kc = op->st.kcap;
  if (op->d_tol && op->tol_cap == kc) return;
  op->tol_cap = 0;
  replace_stop_block(op, op->d_tol, op->h_tol, (1 + kc) * sizeof(double),
                     kFlagBytes + kc * sizeof(double));
  op->tol_cap = kc;
}
void ensure_col_steps(tpl_op_s* op) {
  if (op->d_col_steps) return;
  dev_alloc(op, &op->d_col_steps, TPL_MULTI_MAX * sizeof(int32_t));
  dev_zero(op, op->d_col_steps, TPL_MULTI_MAX * sizeof(int32_t));
}
launch::ShiftTol ensure_stol(tpl_op_s* op, size_t m) {
  const size_t kc = op->st.kcap;
  if (!op->d_stol || op->stol_cap != kc || op->stol_m < m) {
    const size_t mc = std::max(m, op->stol_m);
    op->stol_m = op->stol_cap = 0;
    const size_t doubles = 1 + mc * (4 + 5 * kc);
    replace_stop_block(op, op->d_stol, op->h_stol,
                       doubles * sizeof(double) + 2 * mc * sizeof(int32_t),
                       kFlagBytes + 2 * mc * sizeof(int32_t) + kc * mc * sizeof(double));
    op->stol_m = mc;
    op->stol_cap = kc;
  }
  // the arrays are laid out for the capacity; their inner stride is this call's m
  const size_t mc = op->stol_m;
  launch::ShiftTol t{};
  double* p = op->d_stol;
  t.tol = p;
  t.sig = p + 1;
  t.st = p + 1 + mc;
  t.lu = p + 1 + 4 * mc;
  t.res = t.lu + 4 * kc * mc;
  t.hits = reinterpret_cast<int32_t*>(t.res + kc * mc);
  t.nres = t.hits + mc;
  t.m = (int32_t)m;
  t.kcap = (int32_t)kc;
  return t;
}
void free_batch(tpl_op_s* op) {
  BatchBufs& b = op->bat;
  dev_free(op, b.d_vecs), dev_free(op, b.d_state), dev_free(op, b.d_P), dev_free(op, b.d_Pcnt);
  dev_free(op, b.d_stage);
  dev_free(op, b.d_mx), dev_free(op, b.d_my), dev_free(op, b.d_mstage);
  dev_free(op, b.d_ycache);
  dev_free(op, b.d_stol);
  if (b.h_stol) hipHostFree(b.h_stol);
  b = BatchBufs{};
}
namespace {
// Steps a batch group's long-row cache should hold for buffers of w columns and kc steps:
// none unless a batch solver is in the mask. Mode 2: a group caches as many steps as a
// single solve (the budget is two GROUP vectors' bytes); mode 1: budget_bytes over the
// w n_long doubles of a step.
size_t wanted_batch_cache_rows(const tpl_op_s* op, int w, size_t kc) {
  const unsigned batch_bits = TPL_LONG_CACHE_TWO_PASS_BATCH | TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI;
  if (op->dist || !(op->long_cache_solvers & batch_bits) || w <= 0) return 0;
  const int64_t nl = (int64_t)op->lay.lrows.size();
  return (size_t)long_cache_rows(op->long_cache, op->long_cache_budget, op->part.n,
                                 op->long_cache == 1 ? nl * w : nl, kc);
}
// A zeroed cache of `rows` steps for groups of up to w columns (alloc_cache's layout: the row
// indices behind the sums unless the long rows are the last rows).
void alloc_batch_cache(tpl_op_s* op, double** ycache, int32_t** ylrow, int w, size_t rows) {
  if (rows == 0) return;
  const std::vector<int32_t>& lr = op->lay.lrows;
  const size_t sums = rows * lr.size() * (size_t)w * sizeof(double);
  const size_t table = op->lay.s_identity ? 0 : (lr.size() * sizeof(int32_t) + 7) / 8 * 8;
  dev_alloc(op, ycache, sums + table);
  dev_zero(op, *ycache, sums);
  if (table) {
    *ylrow = reinterpret_cast<int32_t*>(*ycache + rows * lr.size() * (size_t)w);
    HIPCHK(hipMemcpy(*ylrow, lr.data(), lr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
}
} // namespace
// Freed before they grow, as the basis is; sized for the batch buffers' nb and kcap.
void ensure_batch_multi(tpl_op_s* op, size_t m, bool stage) {
  BatchBufs& b = op->bat;
  if (b.nb == 0 || m == 0)
    fail(TPL_ERR_INVALID_ARGUMENT, "ensure_batch_multi: no batch buffers to size by");
  const size_t w = (size_t)b.nb;
  if (m > b.mcols || !b.d_mx) {
    const size_t cols = std::max(m, b.mcols);
    drop_graphs(op);
    dev_free(op, b.d_mx), dev_free(op, b.d_my);
    b.mcols = 0;
    try {
      dev_alloc(op, &b.d_mx, cols * (size_t)op->ld * w * sizeof(double));
      dev_zero(op, b.d_mx, cols * (size_t)op->ld * w * sizeof(double));
      dev_alloc(op, &b.d_my, cols * w * b.kcap * sizeof(double));
      dev_zero(op, b.d_my, cols * w * b.kcap * sizeof(double));
    } catch (...) {
      dev_free(op, b.d_mx), dev_free(op, b.d_my);
      throw;
    }
    b.mcols = cols;
  }
  if (stage && (m > b.mstage_cols || !b.d_mstage)) {
    const size_t cols = std::max(m, b.mstage_cols);
    dev_free(op, b.d_mstage);
    b.mstage_cols = 0;
    dev_alloc(op, &b.d_mstage,
              std::max<size_t>((size_t)op->part.n, 1) * w * cols * sizeof(double));
    b.mstage_cols = cols;
  }
}
void ensure_batch_cut(tpl_op_s* op) {
  if (op->d_bcut) return;
  constexpr size_t bytes = (size_t)kBatchNbMax * TPL_MULTI_MAX * sizeof(int32_t);
  dev_alloc(op, &op->d_bcut, bytes);
  dev_zero(op, op->d_bcut, bytes);
}
launch::BatchShiftTol ensure_batch_stol(tpl_op_s* op, size_t m) {
  BatchBufs& b = op->bat;
  if (b.nb == 0 || m == 0)
    fail(TPL_ERR_INVALID_ARGUMENT, "ensure_batch_stol: no batch buffers to size by");
  const size_t kc = b.kcap, w = (size_t)kBatchNbMax;
  if (!b.d_stol || b.stol_m < m) {
    const size_t mc = std::max(m, b.stol_m);
    b.stol_m = 0;
    const size_t doubles = 1 + mc + w * mc * (3 + 5 * kc);
    replace_stop_block(op, b.d_stol, b.h_stol,
                       doubles * sizeof(double) + w * 2 * mc * sizeof(int32_t),
                       w * (kFlagBytes + 2 * mc * sizeof(int32_t) + kc * mc * sizeof(double)));
    b.stol_m = mc;
  }
  // the arrays are laid out for the capacity; their inner stride is this call's m
  const size_t mc = b.stol_m;
  launch::BatchShiftTol t{};
  double* p = b.d_stol;
  t.t0.tol = p;
  t.t0.sig = p + 1;
  t.t0.st = p + 1 + mc;
  t.t0.lu = t.t0.st + 3 * mc;
  t.t0.res = t.t0.lu + 4 * kc * mc;
  t.dstride = mc * (3 + 5 * kc);
  t.t0.hits = reinterpret_cast<int32_t*>(p + 1 + mc + w * t.dstride);
  t.t0.nres = t.t0.hits + mc;
  t.istride = 2 * mc;
  t.t0.m = (int32_t)m;
  t.t0.kcap = (int32_t)kc;
  return t;
}
// Freed before they grow, as the basis is. State layout, per group: [flags: 8 int32 per
// column] [norms nb (kc + 1)] [alphas nb kc] [betas nb kc] [y nb kc] | 64-B aligned:
// [p2c 8 nb kc] [Pa nb NA] [Pb nb G2].
void ensure_batch(tpl_op_s* op, int nb, size_t k) {
  BatchBufs& b = op->bat;
  if (nb <= b.nb && k <= b.kcap) {
    // the buffers do; the group's long-row cache alone when its mode, budget or solver
    // mask changed since they were sized: built aside, so a refused allocation leaves the
    // operator as it was
    const size_t rows = wanted_batch_cache_rows(op, b.nb, b.kcap);
    if (rows == b.yrows) return;
    double* yc = nullptr;
    int32_t* yl = nullptr;
    try {
      alloc_batch_cache(op, &yc, &yl, b.nb, rows);
    } catch (...) {
      dev_free(op, yc);
      throw;
    }
    std::swap(b.d_ycache, yc);
    b.d_ylrow = yl;
    b.yrows = rows;
    dev_free(op, yc);
    drop_graphs(op);
    return;
  }
  const int w = std::max(nb, b.nb);
  const size_t kc = std::max<size_t>(std::max(k, b.kcap), 16);
  drop_graphs(op);
  free_batch(op);
  const CsrDev A = csr_dev(op);
  const size_t ld = (size_t)op->ld, na = (size_t)std::max(A.NA, 1), g2 = (size_t)std::max(A.G2, 1);
  try {
    dev_alloc(op, &b.d_vecs, 6 * ld * w * sizeof(double));
    dev_zero(op, b.d_vecs, 6 * ld * w * sizeof(double));
    const size_t head = (size_t)w * (kFlagBytes / sizeof(double)) + (size_t)w * (4 * kc + 1);
    const size_t p2c_off = (head + 7) / 8 * 8;
    const size_t doubles = p2c_off + 8 * (size_t)w * kc + (size_t)w * (na + g2);
    dev_alloc(op, &b.d_state, doubles * sizeof(double));
    dev_zero(op, b.d_state, doubles * sizeof(double));
    const size_t nl = std::max<size_t>(op->lay.lrows.size(), 1);
    dev_alloc(op, &b.d_P, nl * kSlotStride * kBatchNbMax * sizeof(double));
    dev_zero(op, b.d_P, nl * kSlotStride * kBatchNbMax * sizeof(double));
    dev_alloc(op, &b.d_Pcnt, nl * kCntStride * sizeof(unsigned int));
    dev_zero(op, b.d_Pcnt, nl * kCntStride * sizeof(unsigned int));
    dev_alloc(op, &b.d_stage, std::max<size_t>((size_t)op->part.n, 1) * w * sizeof(double));
    double* p = b.d_vecs;
    b.b = p, p += ld * w;
    for (int i = 0; i < 3; ++i) b.R[i] = p, p += ld * w;
    b.W = p, p += ld * w;
    b.x = p;
    double* base = (double*)b.d_state;
    BatchDev& S = b.S;
    S.flags = (int32_t*)base;
    S.norms = base + (size_t)w * (kFlagBytes / sizeof(double));
    S.alphas = S.norms + (size_t)w * (kc + 1);
    S.betas = S.alphas + (size_t)w * kc;
    S.y = S.betas + (size_t)w * kc;
    S.p2c = base + p2c_off;
    S.Pa = S.p2c + 8 * (size_t)w * kc;
    S.Pb = S.Pa + (size_t)w * na;
    S.P = b.d_P;
    S.Pcnt = b.d_Pcnt;
    S.kcap = (int32_t)kc;
    S.na_ld = (int32_t)na;
    S.g2_ld = (int32_t)g2;
    const size_t rows = wanted_batch_cache_rows(op, w, kc);
    alloc_batch_cache(op, &b.d_ycache, &b.d_ylrow, w, rows);
    b.yrows = rows;
  } catch (...) {
    free_batch(op);
    throw;
  }
  b.nb = w;
  b.kcap = kc;
}
// The step callback's view of V_k in the caller's row order: the basis itself, or (a
// reordered operator) an n x cols buffer each batch's new columns are gathered into.
double* ensure_view(tpl_op_s* op, size_t cols) {
  if (!op->bufs.d_perm) return op->d_V;
  if (op->vext_cols < cols) {
    dev_free(op, op->d_Vext);
    op->vext_cols = 0;
    dev_alloc(op, &op->d_Vext, (size_t)op->part.n * cols * sizeof(double));
    op->vext_cols = cols;
  }
  return op->d_Vext;
}

int* reorth_records(const tpl_op_s* op) {
  return reinterpret_cast<int*>(op->st.d_Pr + ((size_t)op->lay.G2 + 1) * op->st.kcap +
                                op->lay.G2 + 1);
}

void set_device(const tpl_op_s* op) {
  if (op->plan_only)
    fail(TPL_ERR_INVALID_ARGUMENT, "a host-only plan (tpl_plan_create) holds no device data");
  HIPCHK(hipSetDevice(op->device));
}

void check_b(const tpl_op_s* op, const double* b, int64_t b_len) {
  if (!b && op->part.n > 0) fail(TPL_ERR_INVALID_ARGUMENT, "b is NULL");
  if (b_len != op->part.n) fail_dimension(op->part.n, b_len);
}

// A caller-order vector into a device vector (internal order).
void upload_vec(tpl_op_s* op, double* dst, const double* src, int mem) {
  if (op->part.n == 0) return;
  const size_t bytes = op->part.n * sizeof(double);
  if (!op->bufs.d_perm) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes,
                          mem == TPL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          op->stream));
    return;
  }
  const double* from = src;
  if (mem != TPL_MEM_DEVICE) {
    HIPCHK(hipMemcpyAsync(op->bufs.d_stage, src, bytes, hipMemcpyHostToDevice, op->stream));
    from = op->bufs.d_stage;
  }
  HIPCHK(launch::permute(op->part.n, 1, dst, op->part.n, from, op->part.n, op->bufs.d_perm,
                         op->stream));
}
// `cols` device columns (internal order, ld = n) out to the caller, in the caller's order.
void download_vec(tpl_op_s* op, double* dst, const double* src, int64_t cols, int mem) {
  const int64_t n = op->part.n;
  if (cols == 0 || n == 0) return;
  // one vector, or columns of the basis: nothing else is ever this wide
  if (cols < 0 || (cols > 1 && (src != op->d_V || (size_t)cols > op->vcols)))
    fail(TPL_ERR_INVALID_ARGUMENT, "download_vec: column count exceeds its source");
  if (!op->bufs.d_perm) {
    HIPCHK(hipMemcpyAsync(dst, src, cols * n * sizeof(double),
                          mem == TPL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          op->stream));
    return;
  }
  if (mem == TPL_MEM_DEVICE) {
    HIPCHK(launch::permute(n, (int)cols, dst, n, src, n, op->bufs.d_iperm, op->stream));
    return;
  }
  for (int64_t c = 0; c < cols; ++c) {  // through the staging vector, a column at a time
    HIPCHK(launch::permute(n, 1, op->bufs.d_stage, n, src + c * n, n, op->bufs.d_iperm,
                           op->stream));
    HIPCHK(hipMemcpyAsync(dst + c * n, op->bufs.d_stage, n * sizeof(double),
                          hipMemcpyDeviceToHost, op->stream));
  }
}

void download_cols(tpl_op_s* op, double* dst, const double* src, int64_t lds, int64_t cols,
                   int mem) {
  for (int64_t c = 0; c < cols; ++c)
    download_vec(op, dst + c * op->part.n, src + c * lds, 1, mem);
}

// Vector stride ld, common to all ranks (the gathered vector holds rank r's block at r * ld).
void set_stride(tpl_op_s* op) {
  const RankPlan& part = op->part;
  if (part.halo) {  // [own block | nranks x hH halo slots]; the row split sized and checked it
    op->ld = padded_stride(part.n);
    return;
  }
  const Gathered g = gather_rule(op);
  int64_t widest = part.n;
  if (g.blocks)
    for (int r = 0; r < g.R; ++r) widest = std::max(widest, part.starts[r + 1] - part.starts[r]);
  op->ld = padded_stride(widest);
  // gathered column indices (ColMap: r * ld + local) are int32 on the device
  if ((int64_t)g.R * op->ld >= (int64_t)INT32_MAX)
    fail(TPL_ERR_UNSUPPORTED, "row blocks too unbalanced: nranks x widest block >= 2^31");
}

// Layout, vectors and events of a freshly planned operator (single GPU or one rank
// of a partition; the vector stride ld is common to all ranks).
void init_op(tpl_op_s* op) {
  const Gathered g = gather_rule(op);
  set_stride(op);
  rebuild_schedule(op, op->sp, op->reorder);
  // gathered: b, R0..2, V2_0..2, tmp (R x ld each; halo: ld + R x hH); local: W, x (ld each)
  const size_t gl =
      op->part.halo ? (size_t)op->ld + (size_t)g.R * op->part.hH : (size_t)g.R * op->ld;
  const size_t gathered = 8 * gl, local = 2 * (size_t)op->ld;
  dev_alloc(op, &op->d_vecs, (gathered + local) * sizeof(double));
  dev_zero(op, op->d_vecs, (gathered + local) * sizeof(double));
  double* p = op->d_vecs;
  const size_t own = (size_t)(g.blocks ? op->dist->rank : 0) * op->ld;
  upload(op, &op->d_halo_send, op->part.halo_send);
  op->bG = p;
  p += gl;
  for (int i = 0; i < 3; ++i, p += gl) op->RG[i] = p;
  for (int i = 0; i < 3; ++i, p += gl) op->V2G[i] = p;
  op->tmpG = p;
  p += gl;
  op->W = p;
  p += op->ld;
  op->x = p;
  op->b = op->bG + own;
  for (int i = 0; i < 3; ++i) op->R[i] = op->RG[i] + own;
  for (int i = 0; i < 3; ++i) op->V2[i] = op->V2G[i] + own;
  op->tmp = op->tmpG + own;
  if (op->dist) {
    // [nranks alpha totals | long-row alpha partials (hybrid) | nranks norm totals]
    const size_t nr = (size_t)op->dist->nranks;
    const size_t cnt = 2 * nr + (op->part.hybrid ? (size_t)long_epi_blocks(op) : 0);
    dev_alloc(op, &op->d_rsum, cnt * sizeof(double));
    dev_zero(op, op->d_rsum, cnt * sizeof(double));
    if (op->part.hybrid) {
      // every rank's chunk count (each rank's short rows are a contiguous block of the
      // global split, chunked by kChunkRows: every rank computes all counts alike)
      if ((int)op->part.nch.size() != op->dist->nranks ||
          op->part.nch[op->dist->rank] != (int32_t)op->lay.c_base.size())
        fail(TPL_ERR_UNSUPPORTED, "replicated partition: chunk counts disagree with the layout");
      const int32_t nmax = *std::max_element(op->part.nch.begin(), op->part.nch.end());
      op->y_ld1 = (int32_t)op->lay.lrows.size() + nmax;
      upload(op, &op->d_nch, op->part.nch);
      // pass one strides the all-gather by y_ld1, pass two and tpl_op_apply by n_long + 1
      const size_t ya = nr * (size_t)std::max<int64_t>(op->y_ld1, (int64_t)op->lay.lrows.size() + 1);
      dev_alloc(op, &op->d_yall, ya * sizeof(double));
      dev_zero(op, op->d_yall, ya * sizeof(double));
      // the β stage all-gathers every rank's norm partials (each rank computes all ranks'
      // counts from the global split) and k_p1_spmv reduces each rank's with the tree the
      // rank-total launch applied — one launch less per pass-one step, the same bits —
      // while they fit one load per lane and rank (≤ kPbRanks ranks, ≤ kTPB partials)
      if ((int)op->part.g2s.size() != op->dist->nranks ||
          op->part.g2s[op->dist->rank] != op->lay.G2)
        fail(TPL_ERR_UNSUPPORTED, "replicated partition: block counts disagree with the layout");
      const int32_t g2max = *std::max_element(op->part.g2s.begin(), op->part.g2s.end());
      if (op->dist->nranks <= kPbRanks && g2max <= kTPB) {
        op->pb_ld = g2max;
        dev_alloc(op, &op->d_pball, nr * (size_t)g2max * sizeof(double));
        dev_zero(op, op->d_pball, nr * (size_t)g2max * sizeof(double));
      }
    }
  }
  HIPCHK(hipEventCreate(&op->ev0));
  HIPCHK(hipEventCreate(&op->ev1));
  for (hipEvent_t& e : op->tev) HIPCHK(hipEventCreate(&e));
  sync_checked(op);  // the zeroes above are in place when the create returns
}

// The one way to make an operator: `part` on ctx's device and stream, as a rank of `dist`
// (or nullptr: single GPU), ready for init_op. ctx == nullptr: a host-only plan
// (tpl_plan_create), which gets a stride and a layout and nothing on a device.
std::unique_ptr<tpl_op_s> make_op(tpl_ctx_s* ctx, tpl_dist_s* dist, RankPlan&& part) {
  auto op = std::make_unique<tpl_op_s>();
  op->part = std::move(part);
  op->sp.long_from = op->part.long_from;
  op->sp.elem_rows = op->part.elem_rows;
  op->dist = dist;
  op->plan_only = !ctx;
  if (ctx) {
    op->device = ctx->device;
    op->stream = ctx->stream;
    op->eager = dist && dist->comm == nullptr;
  }
  return op;
}

namespace {
// The schedule setters' common half: on the operator's device, `edit` applied to a copy
// of its parameters, the stream idle, the layout rebuilt under them (and `reorder`).
template <class Edit>
void reschedule(tpl_op_s* op, int reorder, Edit&& edit) {
  set_device(op);
  SchedParams sp = op->sp;
  edit(sp);
  sync_checked(op);
  rebuild_schedule(op, sp, reorder);
}
} // namespace

} // namespace tpl

// =========================================================== C ABI
extern "C" {

const char* tpl_version(void) { return "tpl_amd 0.1.0 gfx950"; }

int tpl_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

tpl_status tpl_ctx_create(int device, tpl_ctx_t* out) {
  return guarded([&] {
    if (!out) fail(TPL_ERR_INVALID_ARGUMENT, "out is NULL");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0)
      fail(TPL_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= cnt) fail(TPL_ERR_INVALID_ARGUMENT, "device index out of range");
    HIPCHK(hipSetDevice(device));
    auto c = std::make_unique<tpl_ctx_s>();
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    *out = c.release();
  });
}

tpl_status tpl_ctx_destroy(tpl_ctx_t ctx) {
  return guarded([&] {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    delete ctx;
  }, true);
}

tpl_status tpl_ctx_synchronize(tpl_ctx_t ctx) {
  return guarded([&] {
    if (!ctx) fail(TPL_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

tpl_status tpl_op_create_csr(tpl_ctx_t ctx, int64_t n, int64_t nnz, const int64_t* row_ptr,
                             const int32_t* col_idx, const double* vals, tpl_op_t* out) {
  return guarded([&] {
    if (!ctx || !out) fail(TPL_ERR_INVALID_ARGUMENT, "ctx/out is NULL");
    if (n < 0 || nnz < 0) fail(TPL_ERR_INVALID_ARGUMENT, "negative size");
    RankPlan part = single_plan(n, nnz, row_ptr, col_idx, vals);
    HIPCHK(hipSetDevice(ctx->device));
    auto op = make_op(ctx, nullptr, std::move(part));
    init_op(op.get());
    *out = op.release();
  });
}

// The matrix whole: n rows, dense_stride(n) apart, the padding zeroed (it is never summed).
// `a` is read during the call only.
tpl_status tpl_op_create_dense(tpl_ctx_t ctx, int64_t n, const double* a, int64_t lda, int mem,
                               tpl_op_t* out) {
  return guarded([&] {
    if (!ctx || !out || !a) fail(TPL_ERR_INVALID_ARGUMENT, "ctx/a/out is NULL");
    if (n <= 0) fail(TPL_ERR_INVALID_ARGUMENT, "a dense operator needs n >= 1");
    if (lda < n) fail(TPL_ERR_INVALID_ARGUMENT, "a dense operator needs lda >= n");
    if (mem != TPL_MEM_HOST && mem != TPL_MEM_DEVICE)
      fail(TPL_ERR_INVALID_ARGUMENT, "mem must be TPL_MEM_HOST or TPL_MEM_DEVICE");
    if (n >= (int64_t)INT32_MAX) fail(TPL_ERR_UNSUPPORTED, "a dense operator of 2^31 rows or more");
    RankPlan part;
    part.n = part.n_glob = n;
    part.nnz = n * n;
    HIPCHK(hipSetDevice(ctx->device));
    auto op = make_op(ctx, nullptr, std::move(part));
    op->dense = true;
    op->dense_ld = dense_stride(n);
    const size_t bytes = (size_t)n * (size_t)op->dense_ld * sizeof(double);
    dev_alloc(op.get(), &op->d_dense, bytes);  // first: the allocation a cap refuses
    dev_zero(op.get(), op->d_dense, bytes);
    HIPCHK(hipMemcpy2DAsync(op->d_dense, (size_t)op->dense_ld * sizeof(double), a,
                            (size_t)lda * sizeof(double), (size_t)n * sizeof(double), (size_t)n,
                            mem == TPL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            op->stream));
    init_op(op.get());  // synchronises: `a` is free again when the create returns
    *out = op.release();
  });
}

tpl_status tpl_dense_schedule(int64_t n, int32_t slices_req, int32_t* slices, int32_t* G2,
                              int64_t* E) {
  return guarded([&] {
    if (n <= 0) fail(TPL_ERR_INVALID_ARGUMENT, "a dense operator needs n >= 1");
    if (slices_req < 0 || slices_req > kSlices || (slices_req & (slices_req - 1)) != 0)
      fail(TPL_ERR_INVALID_ARGUMENT,
           "slices must be 0 (auto) or a power of two up to " + std::to_string(kSlices));
    int32_t g2 = 0;
    int64_t e = 0;
    elem_geometry(n, SchedParams{}, g2, e);
    if (slices) *slices = slices_req > 0 ? slices_req : auto_slices(n);
    if (G2) *G2 = g2;
    if (E) *E = e;
  });
}

tpl_status tpl_op_destroy(tpl_op_t op) {
  return guarded([&] {
    if (!op) return;
    if (!op->plan_only) {  // a plan holds host vectors only
      hipSetDevice(op->device);
      hipStreamSynchronize(op->stream);
    }
    delete op;
  }, true);
}

int64_t tpl_op_nrows(tpl_op_t op) { return op ? op->part.n : -1; }
int64_t tpl_op_nnz(tpl_op_t op) { return op ? op->part.nnz : -1; }
int tpl_op_flags(tpl_op_t op) {
  if (!op) return -1;
  return (op->dist ? 1 : 0) | (op->eager ? 2 : 0) | (op->lay.val_i8 ? 4 : 0) |
         (op->lay.s_col16 ? 8 : 0) | (op->lay.b_col16 ? 16 : 0) | (op->last_one_graph ? 32 : 0) |
         (!op->perm.empty() || op->part.local_order ? 64 : 0) | (op->pb_ld > 0 ? 128 : 0) |
         (op->last_long_cache ? 256 : 0) | (op->last_fused_p2 ? 512 : 0) | (op->dense ? 1024 : 0);
}

tpl_status tpl_op_set_fused_pass_two(tpl_op_t op, int mode) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (mode != 0 && mode != 2) fail(TPL_ERR_INVALID_ARGUMENT, "fused pass-two mode must be 0 or 2");
    if (!op->plan_only) {  // a host-only plan keeps the mode and has nothing to drop
      set_device(op);
      sync_checked(op);
      drop_graphs(op);
    }
    op->fused_p2 = mode;
  });
}
int tpl_fused_pass_two_rows(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                            int short_row_max, int* eligible, int64_t* n_open, int64_t* n_hub) {
  if (n < 0 || !row_ptr || (row_ptr[n] > 0 && !col_idx) || row_ptr[n] >= INT32_MAX) return -1;
  std::vector<int32_t> rp((size_t)n + 1);
  for (int64_t i = 0; i <= n; ++i) rp[i] = (int32_t)row_ptr[i];
  const tpl::FusedP2 f = tpl::classify_fused_p2(
      n, rp.data(), col_idx, nullptr, tpl::short_row_threshold(n, rp, short_row_max), -1);
  if (eligible) *eligible = f.eligible ? 1 : 0;
  if (n_open) *n_open = f.n_open;
  if (n_hub) *n_hub = f.n_hub;
  return 0;
}

tpl_status tpl_op_set_long_cache(tpl_op_t op, int mode, uint64_t budget_bytes) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (mode < 0 || mode > 2) fail(TPL_ERR_INVALID_ARGUMENT, "long-row cache mode must be 0, 1 or 2");
    if (mode == 1) refuse_dense(op, "the long-row cache");  // auto resolves to off
    set_device(op);
    sync_checked(op);
    // the buffer itself is resized by the next solve's ensure_state
    op->long_cache = mode;
    op->long_cache_budget = mode == 1 ? budget_bytes : 0;
    drop_graphs(op);
  });
}
tpl_status tpl_op_set_long_cache_solvers(tpl_op_t op, unsigned mask) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    const unsigned all = TPL_LONG_CACHE_TWO_PASS | TPL_LONG_CACHE_TWO_PASS_MULTI |
                         TPL_LONG_CACHE_TWO_PASS_BATCH | TPL_LONG_CACHE_TWO_PASS_BATCH_MULTI;
    if (mask & ~all)
      fail(TPL_ERR_INVALID_ARGUMENT, "long-row cache solver mask has bits above TPL_LONG_CACHE_*");
    if (!op->plan_only) {  // a host-only plan keeps the mask and has nothing to drop
      set_device(op);
      sync_checked(op);
      // the group's buffer is resized or freed by the next batch solve's ensure_batch
      drop_graphs(op);
    }
    op->long_cache_solvers = mask;
  });
}
uint64_t tpl_long_cache_default_budget(int64_t n) { return tpl::long_cache_default_budget(n); }
uint64_t tpl_long_cache_rows(int mode, uint64_t budget_bytes, int64_t n, int64_t n_long,
                             uint64_t kcap) {
  return tpl::long_cache_rows(mode, budget_bytes, n, n_long, kcap);
}

tpl_status tpl_op_set_reorder(tpl_op_t op, int mode) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (mode < 0 || mode > 2) fail(TPL_ERR_INVALID_ARGUMENT, "reorder mode must be 0, 1 or 2");
    if (mode == 1) refuse_dense(op, "the locality order");  // auto resolves to off
    reschedule(op, mode, [](SchedParams&) {});
  });
}

tpl_status tpl_op_permutation(tpl_op_t op, int32_t* perm) {
  return guarded([&] {
    if (!op || (!perm && op->part.n > 0)) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (op->perm.empty())
      for (int64_t i = 0; i < op->part.n; ++i) perm[i] = (int32_t)i;
    else
      std::copy(op->perm.begin(), op->perm.end(), perm);
  });
}

tpl_status tpl_op_set_value_format(tpl_op_t op, int compress) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    refuse_dense(op, "a value format");
    reschedule(op, op->reorder, [&](SchedParams& sp) {
      sp.compress_values = compress != 0;
      sp.compress_cols = compress != 0;
    });
  });
}

tpl_status tpl_op_schedule(tpl_op_t op, int32_t* n_short, int32_t* n_long, int32_t* G2,
                           int64_t* E, int32_t* short_rows_out, int32_t* long_rows_out) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    const Layout& L = op->lay;
    if (n_short) *n_short = (int32_t)L.srows.size();
    if (n_long) *n_long = (int32_t)L.lrows.size();
    if (G2) *G2 = L.G2;
    if (E) *E = L.E;
    if (short_rows_out) std::copy(L.srows.begin(), L.srows.end(), short_rows_out);
    if (long_rows_out) std::copy(L.lrows.begin(), L.lrows.end(), long_rows_out);
  });
}

tpl_status tpl_op_set_schedule(tpl_op_t op, int32_t short_row_max, int32_t max_g2) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    refuse_dense(op, "a short-row schedule");
    reschedule(op, op->reorder, [&](SchedParams& sp) {
      if (short_row_max != 0) sp.short_row_max = short_row_max < 0 ? -1 : short_row_max;
      if (max_g2 > 0) sp.max_g2 = max_g2;
    });
  });
}

tpl_status tpl_op_slices(tpl_op_t op, int32_t* slices) {
  return guarded([&] {
    if (!op || !slices) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    *slices = op->lay.nslices;
  });
}

tpl_status tpl_op_kernel_variant(tpl_op_t op, int32_t* variant) {
  return guarded([&] {
    if (!op || !variant) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    // what TPL_LAUNCH_CW dispatches on: variant_of over the fields csr_dev gives the
    // launchers, taken from the layout alone (a host plan has no device view to build)
    CsrDev A{};
    format_fields(op->lay, A);
    *variant = variant_of(A);
  });
}

tpl_status tpl_op_set_slices(tpl_op_t op, int32_t slices) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (slices < 0 || slices > kSlices || (slices & (slices - 1)) != 0)
      fail(TPL_ERR_INVALID_ARGUMENT,
           "slices must be 0 (auto) or a power of two up to " + std::to_string(kSlices));
    reschedule(op, op->reorder, [&](SchedParams& sp) { sp.slices = slices; });
  });
}

tpl_status tpl_op_set_order_groups(tpl_op_t op, int32_t groups) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (groups < 0) fail(TPL_ERR_INVALID_ARGUMENT, "group count must be >= 0 (0: default 16)");
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "the locality order is single-GPU only");
    refuse_dense(op, "the locality order");
    reschedule(op, op->reorder, [&](SchedParams& sp) {
      sp.order_groups = groups > 0 ? groups : SchedParams{}.order_groups;
    });
  });
}

int32_t tpl_op_order_groups(tpl_op_t op) {
  if (!op) return -1;
  return !op->perm.empty() ? op->sp.order_groups : 0;
}

tpl_status tpl_copy_to_host(void* dst, const void* src_device, size_t bytes) {
  return guarded([&] {
    if (bytes == 0) return;
    if (!dst || !src_device) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    HIPCHK(hipMemcpy(dst, src_device, bytes, hipMemcpyDeviceToHost));
  });
}

tpl_status tpl_op_device_bytes(tpl_op_t op, uint64_t* bytes) {
  return guarded([&] {
    if (!op || !bytes) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    *bytes = device_bytes(op);
  });
}

tpl_status tpl_operand_key(int64_t n, const void* ptr_arr, size_t ptr_len, size_t ptr_elem,
                           const void* idx_arr, size_t idx_len, size_t idx_elem,
                           const double* vals, size_t nnz, size_t samples, uint64_t* key) {
  return guarded([&] {
    if (!key) fail(TPL_ERR_INVALID_ARGUMENT, "key is NULL");
    if ((ptr_len && !ptr_arr) || (idx_len && !idx_arr) || (nnz && !vals))
      fail(TPL_ERR_INVALID_ARGUMENT, "NULL array with a nonzero length");
    if ((ptr_elem != 4 && ptr_elem != 8) || (idx_elem != 4 && idx_elem != 8))
      fail(TPL_ERR_INVALID_ARGUMENT, "index element size must be 4 or 8 bytes");
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over 64-bit words
    auto mix = [&](uint64_t w) { h = (h ^ w) * 0x100000001b3ull; };
    // identity: the arrays' addresses and lengths, the dimension
    for (uint64_t w : {(uint64_t)n, (uint64_t)(uintptr_t)ptr_arr, (uint64_t)ptr_len,
                       (uint64_t)(uintptr_t)idx_arr, (uint64_t)idx_len,
                       (uint64_t)(uintptr_t)vals, (uint64_t)nnz})
      mix(w);
    key[0] = h;
    // contents: the first and last 8 words of each array and `samples` evenly spaced
    // ones (positions i * len / samples), so the check costs O(samples), not O(nnz)
    h = 0xcbf29ce484222325ull;
    auto sample = [&](const void* a, size_t len, size_t elem) {
      auto word = [&](size_t i) {
        return elem == 8 ? ((const uint64_t*)a)[i] : (uint64_t)((const uint32_t*)a)[i];
      };
      for (size_t i = 0; i < std::min<size_t>(len, 8); ++i) mix(word(i));
      for (size_t i = len > 8 ? len - 8 : len; i < len; ++i) mix(word(i));
      if (len > 16)
        for (size_t s = 0; s < samples; ++s) mix(word((size_t)((unsigned __int128)s * len / samples)));
    };
    sample(ptr_arr, ptr_len, ptr_elem);
    sample(idx_arr, idx_len, idx_elem);
    sample(vals, nnz, 8);
    key[1] = h;
  });
}

tpl_status tpl_op_local_rows(tpl_op_t op, int64_t* rows) {
  return guarded([&] {
    if (!op || !rows) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (op->part.hybrid) {
      std::copy(op->part.local_rows.begin(), op->part.local_rows.end(), rows);
    } else {
      const int64_t r0 = op->dist ? op->part.starts[op->dist->rank] : 0;
      for (int64_t i = 0; i < op->part.n; ++i) rows[i] = r0 + i;
    }
  });
}

// ------------------------------------------------------------ host-only plans
tpl_status tpl_plan_create(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                           const double* vals, int mode, int nranks, int rank,
                           int32_t order_groups, tpl_op_t* out) {
  return guarded([&] {
    if (!row_ptr || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    if (mode < TPL_PLAN_SINGLE || mode > TPL_PLAN_HALO)
      fail(TPL_ERR_INVALID_ARGUMENT,
           "plan mode must be TPL_PLAN_SINGLE, _REPLICATED, _ROWS or _HALO");
    if (mode == TPL_PLAN_SINGLE ? (nranks != 1 || rank != 0)
                                : (nranks < 1 || rank < 0 || rank >= nranks))
      fail(TPL_ERR_INVALID_ARGUMENT, "bad rank / nranks");
    if (order_groups < 0) fail(TPL_ERR_INVALID_ARGUMENT, "group count must be >= 0 (0: default 16)");
    if (n < 0) fail(TPL_ERR_INVALID_ARGUMENT, "negative size");
    const int64_t nnz = row_ptr[n];
    if (nnz > 0 && (!vals || !col_idx)) fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
    std::unique_ptr<tpl_dist_s> pd;  // a partitioned plan's rank and rank count
    RankPlan part;
    if (mode == TPL_PLAN_SINGLE) {  // tpl_op_create_csr's host half
      part = single_plan(n, nnz, row_ptr, col_idx, vals);
    } else {
      pd = std::make_unique<tpl_dist_s>();
      pd->rank = rank;
      pd->nranks = nranks;
      if (mode == TPL_PLAN_REPLICATED) {
        const ReplicatedSplit s = split_replicated(nranks, n, row_ptr, col_idx);
        if (!s.feasible()) fail(TPL_ERR_UNSUPPORTED, s.refused);
        part = materialise(s, rank, row_ptr, col_idx, vals);
      } else {  // the block tpl_dist_partition gives this rank (tpl_dist_op_create_csr /
                // tpl_dist_op_create_halo)
        const bool halo = mode == TPL_PLAN_HALO;
        part = materialise(split_rows(nranks, n, nullptr, row_ptr, col_idx, true, halo), rank,
                           row_ptr, col_idx, vals);
      }
    }
    auto op = make_op(nullptr, pd.get(), std::move(part));
    op->plan_dist = std::move(pd);
    if (mode == TPL_PLAN_SINGLE && order_groups > 0) op->sp.order_groups = order_groups;
    set_stride(op.get());
    rebuild_schedule(op.get(), op->sp, op->reorder);  // the layout only: nothing is uploaded
    *out = op.release();
  });
}

} // extern "C"
