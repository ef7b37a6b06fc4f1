// tpl_dist.cpp — the rank-to-rank transport of a row-partitioned operator: the in-place
// all-gather (RCCL over xGMI, or the tests' host callback), the halo pack / gather, the
// per-step exchanges of the passes, and the tpl_dist_* entry points of the C ABI
// (include/tpl.h). The only unit that sees RCCL.
#include <rccl/rccl.h>

#include "tpl_op.h"

using namespace tpl;

#define NCCLCHK(expr)                                                                       \
  do {                                                                                      \
    ncclResult_t r_ = (expr);                                                               \
    if (r_ != ncclSuccess)                                                                  \
      ::tpl::fail(TPL_ERR_DEVICE, std::string(#expr) + ": " + ncclGetErrorString(r_));     \
  } while (0)

tpl_dist_s::~tpl_dist_s() {
  if (comm) ncclCommDestroy(comm);
}

namespace tpl {

// In-place all-gather of `count` doubles per rank: rank r's part sits at base + r*count.
void dist_allgather(tpl_op_s* op, double* base, size_t count) {
  tpl_dist_s* d = op->dist;
  if (d->comm && std::getenv("TPL_TEST_REFUSE_CAPTURE")) {
    // test hook: behave like a transport that cannot be captured into a graph
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(op->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) fail(TPL_ERR_DEVICE, "exchange refused stream capture (test hook)");
  }
  if (d->comm) {
    NCCLCHK(ncclAllGather(base + (size_t)d->rank * count, base, count, ncclDouble, d->comm,
                          op->stream));
    return;
  }
  // host transport (tests): stage through host memory around the callback
  std::vector<double> send(count), recv(count * (size_t)d->nranks);
  HIPCHK(hipMemcpyAsync(send.data(), base + (size_t)d->rank * count, count * sizeof(double),
                        hipMemcpyDeviceToHost, op->stream));
  HIPCHK(hipStreamSynchronize(op->stream));
  if (d->host_fn(send.data(), recv.data(), count * sizeof(double), d->host_user) != 0)
    fail(TPL_ERR_DEVICE, "host all-gather callback failed");
  HIPCHK(hipMemcpyAsync(base, recv.data(), recv.size() * sizeof(double), hipMemcpyHostToDevice,
                        op->stream));
  HIPCHK(hipStreamSynchronize(op->stream));
}
// Row blocks: complete the gather source G of this rank's SpMV. Plain row blocks
// all-gather every rank's whole block (ld doubles each, in place); halo blocks first pack
// the rows other ranks reference into this rank's halo slot (halo_pack, k_permute — issued
// before the collective group) and all-gather the slots only (hH doubles each).
void halo_pack(tpl_op_s* op, double* G) {
  if (!op->part.halo || op->part.halo_send.empty()) return;
  HIPCHK(launch::permute((int64_t)op->part.halo_send.size(), 1,
                         G + op->ld + (size_t)op->dist->rank * op->part.hH, 0, G, 0,
                         op->d_halo_send, op->stream));
}
void gather_vec(tpl_op_s* op, double* G) {
  if (!op->part.halo) dist_allgather(op, G, (size_t)op->ld);
  else if (op->part.hH > 0) dist_allgather(op, G + op->ld, (size_t)op->part.hH);
}

namespace {
void dist_group(tpl_op_s* op, bool begin) {
  if (op->dist && op->dist->comm) NCCLCHK(begin ? ncclGroupStart() : ncclGroupEnd());
}
// This rank's total of a partial array, in the single-GPU canonical order, into
// its slot of the all-gathered totals.
void dist_total(tpl_op_s* op, const double* P, int N, double* slot) {
  HIPCHK(launch::reorth_reduce(1, P, N, slot, nullptr, op->stream));
}
} // namespace

// The exchanges of a pass-one step of a partitioned operator: (a) after the SpMV launch
// (the alpha total; with replicated long rows their partials travel with it), (norm) after
// the AXPY (the beta total; with row blocks r_{j+1} travels with it).
void enqueue_p1_exchange_a(tpl_op_s* op, const CsrDev& A) {
  if (op->part.hybrid) {
    // ONE all-gather: each rank's long-row partials and its short-chunk alpha partials
    // travel in one segment (one collective's latency per SpMV); every rank then finishes
    // the long rows itself (replicated), reduces each rank's alpha partials to its total
    // and adds the long rows' alpha once (k_long_epi_p1). No rank-total launch sits
    // between the SpMV and the collective.
    dist_allgather(op, op->d_yall, (size_t)op->y_ld1);
  } else {
    dist_total(op, op->st.S.Pa, A.NA, op->d_rsum + op->dist->rank);
    dist_allgather(op, op->d_rsum, 1);
  }
}
// The norm exchange: the ||.||^2 partials of the vector whose gathered copy is G — b in
// pass one's prologue, r_{j+1} = RG[(j + 1) % 3] after step j's AXPY — and, with row
// blocks, the vector itself (the next step gathers from it).
void enqueue_p1_exchange_norm(tpl_op_s* op, const CsrDev& A, double* G) {
  if (op->part.hybrid) {  // every column this rank gathers is local: only the norm partials move
    if (op->pb_ld > 0) {
      // round 6: every rank's norm partials travel (pb_ld doubles per rank) and the next
      // k_p1_spmv reduces each rank's itself — no rank-total launch between k_p1_axpy and
      // the collective
      dist_allgather(op, op->d_pball, (size_t)op->pb_ld);
    } else {
      // the rank's beta total: its own one-workgroup launch (folding it into k_p1_axpy's
      // last arriver measured slower, round 5: DESIGN.md §6.3)
      dist_total(op, op->st.S.Pb, A.G2, const_cast<double*>(op->st.S.Pb_r) + op->dist->rank);
      dist_allgather(op, const_cast<double*>(op->st.S.Pb_r), 1);
    }
  } else {
    const int R = op->dist->nranks;
    dist_total(op, op->st.S.Pb, A.G2, op->d_rsum + R + op->dist->rank);
    halo_pack(op, G);
    dist_group(op, true);
    dist_allgather(op, op->d_rsum + R, 1);
    gather_vec(op, G);
    dist_group(op, false);
  }
}
// The exchange after pass-two step j's SpMV launch.
void enqueue_p2_exchange(tpl_op_s* op, int j) {
  if (op->part.hybrid) {
    const size_t nl = op->lay.lrows.size();
    if (nl) dist_allgather(op, op->d_yall, nl + 1);
  } else {
    halo_pack(op, op->V2G[(j + 1) % 3]);
    gather_vec(op, op->V2G[(j + 1) % 3]);
  }
}

namespace {
std::unique_ptr<tpl_dist_s> new_dist(int device, int rank, int nranks) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) fail(TPL_ERR_DEVICE, "no HIP device available");
  if (device < 0 || device >= cnt) fail(TPL_ERR_INVALID_ARGUMENT, "device index out of range");
  if (nranks < 1 || rank < 0 || rank >= nranks) fail(TPL_ERR_INVALID_ARGUMENT, "bad rank / nranks");
  HIPCHK(hipSetDevice(device));
  auto d = std::make_unique<tpl_dist_s>();
  d->ctx.device = device;
  d->rank = rank;
  d->nranks = nranks;
  HIPCHK(hipStreamCreateWithFlags(&d->ctx.stream, hipStreamNonBlocking));
  return d;
}

// An operator for `part` as a rank of d (the device is set).
void create_op(tpl_dist_s* d, RankPlan&& part, tpl_op_t* out) {
  auto op = make_op(&d->ctx, d, std::move(part));
  init_op(op.get());
  *out = op.release();
}
} // namespace

} // namespace tpl

// =========================================================== C ABI: row partition
extern "C" {

tpl_status tpl_dist_partition(int64_t n, const int64_t* row_ptr, int nranks, int64_t* starts) {
  return guarded([&] {
    if (!row_ptr || !starts || nranks < 1) fail(TPL_ERR_INVALID_ARGUMENT, "bad argument");
    if (n < nranks) fail(TPL_ERR_INVALID_ARGUMENT, "fewer rows than ranks");
    balanced_row_blocks(n, row_ptr, nranks, starts);
  });
}

tpl_status tpl_dist_unique_id(uint8_t* id) {
  return guarded([&] {
    if (!id) fail(TPL_ERR_INVALID_ARGUMENT, "id is NULL");
    static_assert(sizeof(ncclUniqueId) == TPL_DIST_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    NCCLCHK(ncclGetUniqueId(&u));
    std::memcpy(id, &u, sizeof(u));
  });
}

tpl_status tpl_dist_create(int device, int rank, int nranks, const uint8_t* id, tpl_dist_t* out) {
  return guarded([&] {
    if (!id || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    auto d = new_dist(device, rank, nranks);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    NCCLCHK(ncclCommInitRank(&d->comm, nranks, u, rank));
    *out = d.release();
  });
}

tpl_status tpl_dist_create_host(int device, int rank, int nranks, tpl_allgather_fn fn, void* user,
                                tpl_dist_t* out) {
  return guarded([&] {
    if (!fn || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    auto d = new_dist(device, rank, nranks);
    d->host_fn = fn;
    d->host_user = user;
    *out = d.release();
  });
}

tpl_status tpl_dist_destroy(tpl_dist_t d) {
  return guarded([&] {
    if (!d) return;
    hipSetDevice(d->ctx.device);
    if (d->ctx.stream) hipStreamSynchronize(d->ctx.stream);
    delete d;
  }, true);
}

tpl_status tpl_dist_op_create_csr(tpl_dist_t d, int64_t n_global, const int64_t* starts,
                                  const int64_t* row_ptr, const int32_t* col_idx,
                                  const double* vals, tpl_op_t* out) {
  return guarded([&] {
    if (!d || !starts || !row_ptr || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    RankPlan part = block_plan(d->nranks, d->rank, n_global, starts, row_ptr, col_idx, vals);
    HIPCHK(hipSetDevice(d->ctx.device));
    create_op(d, std::move(part), out);
  });
}

tpl_status tpl_dist_op_create_halo(tpl_dist_t d, int64_t n, const int64_t* starts,
                                   const int64_t* row_ptr, const int32_t* col_idx,
                                   const double* vals, tpl_op_t* out) {
  return guarded([&] {
    if (!d || !row_ptr || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    HIPCHK(hipSetDevice(d->ctx.device));
    const RowSplit s = split_rows(d->nranks, n, starts, row_ptr, col_idx, vals != nullptr, true);
    create_op(d, materialise(s, d->rank, row_ptr, col_idx, vals), out);
  });
}

tpl_status tpl_dist_op_create_replicated(tpl_dist_t d, int64_t n, const int64_t* row_ptr,
                                         const int32_t* col_idx, const double* vals,
                                         tpl_op_t* out) {
  return guarded([&] {
    if (!d || !row_ptr || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    HIPCHK(hipSetDevice(d->ctx.device));
    const ReplicatedSplit s = split_replicated(d->nranks, n, row_ptr, col_idx, vals != nullptr);
    if (!s.feasible()) fail(TPL_ERR_UNSUPPORTED, s.refused);
    create_op(d, materialise(s, d->rank, row_ptr, col_idx, vals), out);
  });
}

tpl_status tpl_dist_choose_partition(int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                                     int nranks, int* mode) {
  return guarded([&] {
    if (!mode) fail(TPL_ERR_INVALID_ARGUMENT, "mode is NULL");
    *mode = choose_partition(n, row_ptr, col_idx, nranks).mode;
  });
}

tpl_status tpl_dist_op_create_auto(tpl_dist_t d, int64_t n, const int64_t* row_ptr,
                                   const int32_t* col_idx, const double* vals, tpl_op_t* out,
                                   int* mode) {
  return guarded([&] {
    if (!d || !row_ptr || !out) fail(TPL_ERR_INVALID_ARGUMENT, "NULL argument");
    const PartitionChoice c = choose_partition(n, row_ptr, col_idx, d->nranks);
    HIPCHK(hipSetDevice(d->ctx.device));
    if (row_ptr[n] > 0 && !vals) fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
    create_op(d, c.mode == TPL_PLAN_REPLICATED
                     ? materialise(c.rep, d->rank, row_ptr, col_idx, vals)
                     : materialise(c.rows, d->rank, row_ptr, col_idx, vals), out);
    if (mode) *mode = c.mode;
  });
}

} // extern "C"
