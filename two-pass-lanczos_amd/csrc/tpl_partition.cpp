// tpl_partition.cpp — the partition planner (tpl_partition.h). Host only.
#include "tpl_partition.h"

#include <utility>

namespace tpl {
namespace {

// Contiguous blocks over items 0..m-1 with cost prefix[m+1]: cut where the prefix
// crosses r/nranks of the total; every block keeps at least one item.
void balanced_cuts(const std::vector<double>& prefix, int nranks, int64_t* starts) {
  const int64_t m = (int64_t)prefix.size() - 1;
  const double total = prefix[m];
  starts[0] = 0;
  int64_t i = 0;
  for (int r = 1; r < nranks; ++r) {
    const double target = total * r / nranks;
    while (i < m && prefix[i] < target) ++i;
    starts[r] = std::min<int64_t>(std::max<int64_t>(i, starts[r - 1] + 1), m - (nranks - r));
    i = starts[r];
  }
  starts[nranks] = m;
}

// What the device's int32 indices can hold of rank me's block.
void check_row_block(const RowSplit& s, int me, const int64_t* row_ptr) {
  const int64_t r0 = s.starts[me], r1 = s.starts[me + 1], R = (int64_t)s.starts.size() - 1;
  if (row_ptr[r1] - row_ptr[r0] >= INT32_MAX) fail(TPL_ERR_UNSUPPORTED, "nnz must be < 2^31");
  if (s.halo && padded_stride(r1 - r0) + R * s.H >= (int64_t)INT32_MAX)
    fail(TPL_ERR_UNSUPPORTED, "halo partition: own block + nranks x halo width >= 2^31");
}

// Rows [r0, r1) of a CSR, entry for entry, row_ptr rebased to 0.
void copy_rows(RankPlan& p, int64_t r0, int64_t r1, const int64_t* row_ptr, const int32_t* col_idx,
               const double* vals) {
  p.n = r1 - r0;
  p.nnz = row_ptr[r1] - row_ptr[r0];
  p.h_rowptr.resize(p.n + 1);
  for (int64_t i = 0; i <= p.n; ++i) p.h_rowptr[i] = (int32_t)(row_ptr[r0 + i] - row_ptr[r0]);
  p.h_col.assign(col_idx + row_ptr[r0], col_idx + row_ptr[r1]);
  p.h_val.assign(vals + row_ptr[r0], vals + row_ptr[r1]);
}

} // namespace

void check_starts(const int64_t* starts, int R, int64_t n) {
  if (starts[0] != 0 || starts[R] != n) fail(TPL_ERR_INVALID_ARGUMENT, "bad partition");
  for (int r = 0; r < R; ++r)
    if (starts[r + 1] <= starts[r]) fail(TPL_ERR_INVALID_ARGUMENT, "empty or unordered block");
}

// 12 bytes per nonzero (value + column) + 40 per row (pass two's vector traffic)
void balanced_row_blocks(int64_t n, const int64_t* row_ptr, int R, int64_t* starts) {
  std::vector<double> prefix(n + 1);
  for (int64_t i = 0; i <= n; ++i) prefix[i] = 12.0 * (double)row_ptr[i] + 40.0 * (double)i;
  balanced_cuts(prefix, R, starts);
}

RankPlan single_plan(int64_t n, int64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
                     const double* vals) {
  if (n >= INT32_MAX || nnz >= INT32_MAX)
    fail(TPL_ERR_UNSUPPORTED, "n and nnz must be < 2^31 (int32 device offsets)");
  if (!row_ptr) fail(TPL_ERR_INVALID_ARGUMENT, "row_ptr is NULL");
  if (nnz > 0 && !vals) fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
  if (row_ptr[n] != nnz) fail(TPL_ERR_INVALID_ARGUMENT, "row_ptr must start at 0 and end at nnz");
  check_csr(n, n, row_ptr, col_idx);
  RankPlan p;
  p.n_glob = n;
  copy_rows(p, 0, n, row_ptr, col_idx, vals);
  return p;
}

RankPlan block_plan(int R, int me, int64_t n_glob, const int64_t* starts, const int64_t* row_ptr,
                    const int32_t* col_idx, const double* vals) {
  check_starts(starts, R, n_glob);
  if (n_glob >= INT32_MAX / 2) fail(TPL_ERR_UNSUPPORTED, "n must be < 2^30");
  const int64_t n = starts[me + 1] - starts[me];
  const int64_t nnz = row_ptr[n];
  if (row_ptr[0] != 0 || nnz < 0 || nnz >= INT32_MAX)
    fail(TPL_ERR_INVALID_ARGUMENT, "row_ptr must start at 0; nnz < 2^31");
  if (nnz > 0 && !vals) fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
  check_csr(n, n_glob, row_ptr, col_idx);
  RankPlan p;
  p.n_glob = n_glob;
  p.starts.assign(starts, starts + R + 1);
  copy_rows(p, 0, n, row_ptr, col_idx, vals);
  return p;
}

ReplicatedSplit split_replicated(int R, int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                                 bool has_vals) {
  if (n < 1 || n >= INT32_MAX / 2 || row_ptr[n] >= INT32_MAX || row_ptr[0] != 0)
    fail(TPL_ERR_INVALID_ARGUMENT, "bad CSR sizes");
  if (row_ptr[n] > 0 && !has_vals) fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
  check_csr(n, n, row_ptr, col_idx);
  ReplicatedSplit s;
  s.n = n;
  std::vector<int32_t> rp32(n + 1);
  for (int64_t i = 0; i <= n; ++i) rp32[i] = (int32_t)row_ptr[i];
  // short / long rows by the global rule; long rows are replicated on every rank
  const int32_t T = short_row_threshold(n, rp32, -1);
  s.lidx.assign(n, -1);
  for (int64_t i = 0; i < n; ++i) {
    if (rp32[i + 1] - rp32[i] > T) {
      s.lidx[i] = (int32_t)s.lrows.size();
      s.lrows.push_back(i);
    } else {
      s.srows.push_back(i);
    }
  }
  if ((int64_t)s.srows.size() < R) {
    s.refused = "fewer short rows than ranks";
    return s;
  }
  // short rows in contiguous blocks balanced by bytes: the row itself plus the
  // long-row entries in its column, which the owner of that column computes
  std::vector<int32_t> longcnt(n, 0);
  for (int64_t l : s.lrows)
    for (int64_t q = row_ptr[l]; q < row_ptr[l + 1]; ++q) longcnt[col_idx[q]]++;
  std::vector<double> prefix(s.srows.size() + 1, 0.0);
  for (size_t p = 0; p < s.srows.size(); ++p) {
    const int64_t i = s.srows[p];
    prefix[p + 1] = prefix[p] + 12.0 * (double)(rp32[i + 1] - rp32[i] + longcnt[i]) + 40.0;
  }
  s.cut.resize(R + 1);
  balanced_cuts(prefix, R, s.cut.data());
  s.owner.assign(n, -1);
  for (int r = 0; r < R; ++r)
    for (int64_t p = s.cut[r]; p < s.cut[r + 1]; ++p) s.owner[s.srows[p]] = r;
  // halo-free check (all ranks decide alike: they all see the whole matrix)
  for (int64_t i : s.srows)
    for (int64_t q = row_ptr[i]; q < row_ptr[i + 1]; ++q) {
      const int32_t c = col_idx[q];
      if (s.lidx[c] < 0 && s.owner[c] != s.owner[i]) {
        s.refused = "a short row references a short row of another rank "
                    "(use the row-partitioned operator)";
        return s;
      }
    }
  // every rank's chunk and element-wise block counts (each rank's short rows are a
  // contiguous block of the split, chunked by kChunkRows: every rank computes all alike)
  const int64_t nl = (int64_t)s.lrows.size();
  SchedParams sp;
  s.nch.resize(R);
  s.g2s.resize(R);
  int64_t rows_max = 0;
  auto count_blocks = [&] {
    for (int r = 0; r < R; ++r) {
      int64_t E = 0;
      elem_geometry(s.cut[r + 1] - s.cut[r] + nl, sp, s.g2s[r], E);
    }
  };
  for (int r = 0; r < R; ++r) {
    s.nch[r] = (int32_t)((s.cut[r + 1] - s.cut[r] + kChunkRows - 1) / kChunkRows);
    rows_max = std::max<int64_t>(rows_max, s.cut[r + 1] - s.cut[r] + nl);
  }
  count_blocks();
  // Up to kPbRanks ranks: element-wise blocks wide enough that no rank holds more than kTPB
  // norm partials, so pass one's SpMV reduces every rank's gathered partials itself (one
  // load per lane and rank) and no rank-total launch remains — when that needs at most
  // 2 kElemRows rows per block. Measured on the 5M-arc instance (round 6, rank shares
  // through one RCCL rank, profiles/r06_rank_share_5m_wide.txt): N = 8, 306 -> 246
  // partials at 2,560 rows per block, slowest share 14.35 -> 13.78 ms; N = 4, 5,120 rows
  // per block, 20.69 -> 21.29 ms (k_p1_axpy's wider blocks cost more than the launch), so
  // not applied there. Every rank applies the same rule to the same split, so all agree
  // on every rank's count.
  const int64_t er_gp = (((rows_max + kTPB - 1) / kTPB) + 511) / 512 * 512;
  if (R <= kPbRanks && er_gp <= 2 * kElemRows &&
      *std::max_element(s.g2s.begin(), s.g2s.end()) > kTPB) {
    s.elem_rows = sp.elem_rows = (int)er_gp;
    count_blocks();
  }
  return s;
}

RankPlan materialise(const ReplicatedSplit& s, int me, const int64_t* row_ptr,
                     const int32_t* col_idx, const double* vals) {
  RankPlan p;
  p.hybrid = true;
  p.n_glob = s.n;
  const int64_t ns = s.cut[me + 1] - s.cut[me], nl = (int64_t)s.lrows.size();
  p.ns_local = ns;
  p.n = ns + nl;
  // this rank's short rows; in the locality order (tpl_layout.h locality_order, the
  // same key over the replicated long rows' ranks) when the rank's rows fit the auto
  // rule. The local order is the caller's to follow through tpl_op_local_rows, so no
  // vector is permuted on the device.
  std::vector<int64_t> mine(s.srows.begin() + s.cut[me], s.srows.begin() + s.cut[me + 1]);
  if (nl > 0 && p.n <= kReorderAutoMaxRows) {
    // lidx is each long row's rank among the long rows, as locality_order ranks them
    locality_sort(mine, row_ptr, col_idx, s.lidx.data(), (int32_t)nl, SchedParams{}.order_groups);
    p.local_order = true;
  }
  p.g2l.assign(s.n, -1);
  p.local_rows = std::move(mine);
  p.local_rows.insert(p.local_rows.end(), s.lrows.begin(), s.lrows.end());
  for (int64_t i = 0; i < p.n; ++i) p.g2l[p.local_rows[i]] = (int32_t)i;
  // local CSR in local column indices, each row ascending: own short rows whole; long
  // rows restricted to the columns this rank owns (long-row columns: rank 0). The
  // long rows' 8 column slices then split this rank's own columns, so every XCD
  // gets a share of the long-row work.
  p.h_rowptr.assign(1, 0);
  std::vector<std::pair<int32_t, double>> row;
  for (int64_t i = 0; i < p.n; ++i) {
    const int64_t g = p.local_rows[i];
    const bool is_long = i >= ns;
    row.clear();
    for (int64_t q = row_ptr[g]; q < row_ptr[g + 1]; ++q) {
      const int32_t c = col_idx[q];
      if (is_long && !(s.lidx[c] < 0 ? s.owner[c] == me : me == 0)) continue;
      row.emplace_back(p.g2l[c], vals[q]);
    }
    std::sort(row.begin(), row.end(),
              [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) {
                return a.first < b.first;
              });
    for (const auto& e : row) {
      p.h_col.push_back(e.first);
      p.h_val.push_back(e.second);
    }
    p.h_rowptr.push_back((int32_t)p.h_col.size());
  }
  p.nnz = (int64_t)p.h_col.size();
  p.long_from = ns;
  p.nch = s.nch;
  p.g2s = s.g2s;
  p.elem_rows = s.elem_rows;
  return p;
}

RowSplit split_rows(int R, int64_t n, const int64_t* starts, const int64_t* row_ptr,
                    const int32_t* col_idx, bool has_vals, bool halo) {
  if (n < R) fail(TPL_ERR_INVALID_ARGUMENT, "fewer rows than ranks");
  if (n >= INT32_MAX / 2) fail(TPL_ERR_UNSUPPORTED, "n must be < 2^30");
  if (row_ptr[0] != 0) fail(TPL_ERR_INVALID_ARGUMENT, "row_ptr must start at 0");
  if (row_ptr[n] > 0 && (!has_vals || !col_idx))
    fail(TPL_ERR_INVALID_ARGUMENT, "col_idx/vals is NULL");
  check_csr(n, n, row_ptr, col_idx);
  RowSplit s;
  s.n = n;
  s.starts.resize(R + 1);
  if (starts) {
    check_starts(starts, R, n);
    s.starts.assign(starts, starts + R + 1);
  } else {
    balanced_row_blocks(n, row_ptr, R, s.starts.data());
  }
  if (!halo) return s;
  const std::vector<int64_t>& st = s.starts;
  s.halo = true;
  s.need.assign(n, 0);
  for (int r = 0; r < R; ++r)
    for (int64_t q = row_ptr[st[r]]; q < row_ptr[st[r + 1]]; ++q) {
      const int32_t c = col_idx[q];
      if (c < st[r] || c >= st[r + 1]) s.need[c] = 1;
    }
  s.pos.assign(n, -1);
  for (int q = 0; q < R; ++q) {
    int32_t m = 0;
    for (int64_t c = st[q]; c < st[q + 1]; ++c)
      if (s.need[c]) s.pos[c] = m++;
    s.H = std::max<int64_t>(s.H, m);
  }
  return s;
}

// Rank me's rows with global column indices; halo: its send list (B_me in local indices)
// and the column table: own column c -> c - starts[me], remote column c in B_q ->
// ld + q H + pos[c]. The layout is built from the same CSR and global-column slices as
// plain row blocks, so the two hold the same reduction order; only the gathered positions differ.
RankPlan materialise(const RowSplit& s, int me, const int64_t* row_ptr, const int32_t* col_idx,
                     const double* vals) {
  check_row_block(s, me, row_ptr);
  const int64_t r0 = s.starts[me], r1 = s.starts[me + 1];
  RankPlan p;
  p.n_glob = s.n;
  p.starts = s.starts;
  copy_rows(p, r0, r1, row_ptr, col_idx, vals);
  if (!s.halo) return p;
  p.halo = true;
  p.hH = s.H;
  const int64_t ld = padded_stride(p.n);
  for (int64_t c = r0; c < r1; ++c)
    if (s.need[c]) p.halo_send.push_back((int32_t)(c - r0));
  p.halo_map.assign(s.n, -1);
  for (int64_t c = r0; c < r1; ++c) p.halo_map[c] = (int32_t)(c - r0);
  for (int q = 0; q + 1 < (int)s.starts.size(); ++q)
    if (q != me)
      for (int64_t c = s.starts[q]; c < s.starts[q + 1]; ++c)
        if (s.pos[c] >= 0) p.halo_map[c] = (int32_t)(ld + (int64_t)q * s.H + s.pos[c]);
  return p;
}

PartitionChoice choose_partition(int64_t n, const int64_t* row_ptr, const int32_t* col_idx, int R) {
  if (!row_ptr || R < 1) fail(TPL_ERR_INVALID_ARGUMENT, "bad argument");
  PartitionChoice c;
  c.rep = split_replicated(R, n, row_ptr, col_idx);
  if (c.rep.feasible()) {
    c.mode = TPL_PLAN_REPLICATED;
    return c;
  }
  c.rows = split_rows(R, n, nullptr, row_ptr, col_idx, true, true);
  check_row_block(c.rows, 0, row_ptr);
  const std::vector<int64_t>& st = c.rows.starts;
  int64_t widest = 0;
  for (int r = 0; r < R; ++r) widest = std::max<int64_t>(widest, st[r + 1] - st[r]);
  c.mode = 2 * c.rows.H <= widest ? TPL_PLAN_HALO : TPL_PLAN_ROWS;
  c.rows.halo = c.mode == TPL_PLAN_HALO;  // plain row blocks: the halo plan is not used
  return c;
}

} // namespace tpl
