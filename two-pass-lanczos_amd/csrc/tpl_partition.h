// tpl_partition.h — the partition planner (host side): which rows and which local CSR
// every rank of a multi-GPU solve gets. A split is decided once from the whole matrix's
// pattern (rank-independent, no values read); a rank's plan is materialised from it. Pure
// host code, built by tpl_partition.cpp; the runtime makes operators and plans from a RankPlan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "tpl_internal.h"
#include "tpl_layout.h"

namespace tpl {

// What one operator holds of the matrix: its rows, their CSR, its place in the partition.
struct RankPlan {
  int64_t n = 0, nnz = 0;           // this operator's rows (the rank's block) and nonzeros
  int64_t n_glob = 0;               // rows of the whole matrix (single GPU: n)
  std::vector<int64_t> starts;      // row blocks: rank r owns rows [starts[r], starts[r+1])
  // replicated-long-row partition ("hybrid"): local vector = [own short rows | all long
  // rows]; g2l maps global rows/columns to local indices (-1: not local), local_rows back
  bool hybrid = false;
  int64_t ns_local = 0;
  std::vector<int32_t> g2l;
  std::vector<int64_t> local_rows;
  bool local_order = false;         // own short rows in locality order
  std::vector<int32_t> nch;         // chunks (alpha partials) of every rank
  std::vector<int32_t> g2s;         // norm partials (element-wise blocks) of every rank
  // halo-exchange row blocks: the gathered vector is [own block (ld) | nranks x hH halo
  // slots]; rank q's slot holds the hH_q <= hH rows of its block that some other rank's
  // rows reference (halo_send: their local indices), packed before each all-gather;
  // halo_map: global column -> device position
  bool halo = false;
  int64_t hH = 0;
  std::vector<int32_t> halo_send, halo_map;
  std::vector<int32_t> h_rowptr, h_col;  // the local CSR (hybrid: local column indices)
  std::vector<double> h_val;
  int64_t long_from = -1;           // the SchedParams of these names, as the split sets them
  int elem_rows = 0;
};

// Vector stride of a block of `rows` rows: padded to 64 rows, at least 64.
inline int64_t padded_stride(int64_t rows) { return ((std::max<int64_t>(rows, 1) + 63) / 64) * 64; }
// Throws TPL_ERR_INVALID_ARGUMENT unless starts[0..R] is an increasing split of 0..n.
void check_starts(const int64_t* starts, int R, int64_t n);
// tpl_dist_partition: contiguous row blocks balanced by algorithmic bytes.
void balanced_row_blocks(int64_t n, const int64_t* row_ptr, int R, int64_t* starts);

// A single-GPU operator's plan (tpl_op_create_csr, TPL_PLAN_SINGLE): the whole CSR, checked.
RankPlan single_plan(int64_t n, int64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
                     const double* vals);
// A rank's plan from its own block alone (tpl_dist_op_create_csr): rows
// [starts[me], starts[me+1]) with global column indices, row_ptr starting at 0.
RankPlan block_plan(int R, int me, int64_t n_glob, const int64_t* starts, const int64_t* row_ptr,
                    const int32_t* col_idx, const double* vals);

// Replicated long rows: short rows in byte-balanced contiguous blocks (no short row may
// reference another rank's short row), long rows on every rank.
struct ReplicatedSplit {
  std::string refused;              // not feasible: the TPL_ERR_UNSUPPORTED message
  int64_t n = 0;
  std::vector<int64_t> srows, lrows;  // short / long rows by the global rule, ascending
  std::vector<int32_t> lidx;        // row -> its rank among the long rows (-1: short)
  std::vector<int64_t> cut;         // rank r owns srows[cut[r] .. cut[r+1])
  std::vector<int32_t> owner;       // short row -> rank (-1: long)
  std::vector<int32_t> nch, g2s;    // RankPlan's
  int elem_rows = 0;
  bool feasible() const { return refused.empty(); }
};
// Row blocks from the WHOLE matrix: `starts`, or nullptr for the balanced_row_blocks split.
// halo: also B_q = the rows of rank q's block that a row of another rank references (need;
// one pass over the nonzeros), pos = a row's rank in its B_q, H = max_q |B_q|.
struct RowSplit {
  int64_t n = 0;
  std::vector<int64_t> starts;
  bool halo = false;
  std::vector<uint8_t> need;
  std::vector<int32_t> pos;
  int64_t H = 0;
};
// has_vals: the caller passed values (checked where the entry points always checked it).
ReplicatedSplit split_replicated(int R, int64_t n, const int64_t* row_ptr, const int32_t* col_idx,
                                 bool has_vals = true);
RowSplit split_rows(int R, int64_t n, const int64_t* starts, const int64_t* row_ptr,
                    const int32_t* col_idx, bool has_vals, bool halo);
// Rank me's plan of a (feasible) split.
RankPlan materialise(const ReplicatedSplit& s, int me, const int64_t* row_ptr,
                     const int32_t* col_idx, const double* vals);
RankPlan materialise(const RowSplit& s, int me, const int64_t* row_ptr, const int32_t* col_idx,
                     const double* vals);

// The partition every binding's "auto" takes (tpl_dist_choose_partition): replicated long
// rows when the matrix allows them, else halo row blocks when the halo is at most half the
// widest block, else plain row blocks. The same answer on every rank, with the split it
// was decided on (mode TPL_PLAN_REPLICATED: rep, else rows).
struct PartitionChoice {
  int mode = TPL_PLAN_ROWS;
  ReplicatedSplit rep;
  RowSplit rows;
};
PartitionChoice choose_partition(int64_t n, const int64_t* row_ptr, const int32_t* col_idx, int R);

} // namespace tpl
