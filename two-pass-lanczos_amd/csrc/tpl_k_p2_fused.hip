// tpl_k_p2_fused.hip — k_p2_hub and k_p2_rows: every step of pass two in two launches, for
// a layout whose rows decouple once the long-row cache holds the long rows' sums (tpl_layout.h
// FusedP2). Map of the device sources: tpl_kernels.hip.
//
// Pass two's recurrence for row i is
//   v_{j+1}[i] = (((A v_j)_i - beta_{j-1} v_{j-1}[i]) - alpha_j v_j[i]) * (1 / beta_j),
//   x[i] += y_j v_{j+1}[i],
// and only (A v_j)_i couples rows. The cache (tpl_op.h SolverState::d_ycache) holds (A v_j)_r
// of every long row r for every step pass one took, so a long row's whole history follows
// from its own cache column and the step records; a CLOSED short row (every column a long
// row or the row itself) needs only the long rows' v_j; the few OPEN rows and the long rows
// they reference — the hub set H, at most kFusedHubMax rows — step together in one workgroup.
//   k_p2_hub   one thread per long row: v_j[r] replaces the sum in the cache row of step j;
//              one more workgroup owns H (its rows' only reader and writer in the cache) and
//              exchanges v_j inside one wave (|H| <= 64) or through LDS, one barrier per step.
//   k_p2_rows  one workgroup per four short chunks: a thread keeps its rows' entries, v and
//              x in registers; per block of S steps the workgroup stages the long rows' v_j
//              from S cache rows into LDS once for its chunks (double-buffered, the loads
//              two blocks ahead in registers), meets at one barrier, and the rows gather
//              and step S times from there.
// No workgroup waits on another: the only dependency between workgroups is the kernel
// boundary between the two launches.
//
// Bits: a row's sum is short_chunk_w's (s = 0; s += a_k x_k in entry order, padding adds
// -0.0; the gather scale is 1) or the cached long-row sum, and its epilogue is
// EpiPass2R::apply's operations in their order. x is kept in a register and takes one term per
// step — the grouped flush of the step launches (tpl::p2_flush) adds the same terms in the
// same order, so the roundings are the same. Both kernels stop at steps_taken - 1, which is
// where the host schedule (and the one-graph schedule plus k_p2_tail) ends.
#include "tpl_klaunch.h"

namespace tpl {

constexpr int kHubAhead = 8;  // steps a long row's cache and record loads run ahead of its chain

struct FusedP2Args {
  // the hub set (k_p2_hub's last workgroup)
  const int32_t* h_row;
  const int32_t* h_ent;
  const double* h_val;
  int32_t n_open, n_hub;
  // both kernels
  double* ycache;        // n_long doubles per step: sums in, v_j out (k_p2_hub); v_j (k_p2_rows)
  const double* rec;     // DevState::p2c: 8 doubles per step (EpiPass2R)
  const int32_t* flags;  // DevState::flags
  const double* v1;
  double* x;
  int64_t n;
  int32_t n_long;
  int32_t steps;         // > 0: the steps taken; 0: flags[2] (nothing after an error, flags[1],
                         // or when the device handed f(T_k) back, flags[4]: the host's pass
                         // two follows and needs the sums)
  // k_p2_rows: the short chunks (CsrDev)
  const void* s_col;
  const void* s_val;
  const int32_t* s_cbase;
  const int32_t* c_base;
  const int32_t* c_width;
  int32_t n_short, n_chunks, s_width, val_i8, s_col16;
};

__device__ __forceinline__ int fused_steps(const FusedP2Args& a) {
  if (a.steps > 0) return a.steps;
  return a.flags[1] || a.flags[4] ? 0 : a.flags[2];
}

// One step of one row (EpiPass2R::apply): s = (A v_j)_i, r = the four fields of the step's
// record that the step uses. vp is 0.0 at j = 1, where the record's beta is 0.
struct StepRec {
  double beta_sub, alpha, invb, ycoef;
};
// The fields of step j's record by scalar loads: j is uniform, and the records were
// written by an earlier launch and are not written during this one, so they may be read
// through the constant address space, whatever the kernel stores elsewhere in between.
__device__ __forceinline__ StepRec rec_scalar(const double* rec, int j) {
  typedef const double __attribute__((address_space(4))) cdouble;
  cdouble* p = (cdouble*)(uintptr_t)(rec + 8 * (size_t)j);
  return {p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void fused_step_r(double s, const StepRec& r, double& vc, double& vp,
                                             double& xv) {
  double w = s - r.beta_sub * vp;
  w = w - r.alpha * vc;
  const double vn = w * r.invb;
  xv = xv + r.ycoef * vn;
  vp = vc;
  vc = vn;
}

// k_p2_hub's store of v_j[r] into a cache row, as a raw buffer store over exactly that row
// (base `row`, n_long * 8 bytes): a lane that must not write passes kLaneOff, which the
// hardware's range check of the descriptor drops. The store is then one instruction on
// every path — no branch around it — so the compiler counts it exactly in the s_waitcnt
// vmcnt of the prefetch loads behind it (a store under `if` made it assume none was issued
// and wait for loads several steps younger than the one it needed).
constexpr uint32_t kLaneOff = 0x80000000u;  // past any row: n_long * 8 <= 16 KiB
__device__ __forceinline__ void st_cache_row(double* row, int nl, uint32_t off, double v) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  // word 3: an untyped 32-bit element, no swizzle; stride 0: `off` is a byte offset
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, 0, nl * 8, 0x00020000);
  u32x2 d;
  d.x = (uint32_t)__double2loint(v);
  d.y = (uint32_t)__double2hiint(v);
  __builtin_amdgcn_raw_buffer_store_b64(d, r, off, 0, 0);
}

// The chain of one thread of k_p2_hub over steps 1 .. last. MODE: a long-row workgroup; the
// hub workgroup exchanging v_j through LDS, one barrier per step; or, where H fits one wave
// (|H| <= 64), the hub workgroup's first wave alone — no LDS round trip and no barrier on what
// is the kernel's longest chain — its open rows reading the other lanes' v_j by a wave shuffle
// or, for the few members of a small set (|H| = NH <= kHubLanesMax: the KKT instances' 3),
// from NH lane broadcasts and selects, with no LDS permute and nothing to wait for. WM: the
// entries summed, on one wave the widest open row's own width (an entry past it is padding on
// every row and would add -0.0: no bit). The sums and records run kHubAhead steps ahead of
// the chain in yb / ra, rb: they do not depend on it. A record's four fields are loaded into
// every lane (one address for the wave: this kernel stores into the cache between them, so
// they stay vector loads, counted in order with the sums' loads), which keeps the eight lane
// reads of a record held one field per lane off the chain. The main loop takes whole blocks of
// kHubAhead steps with no exit inside a block, each step refilling its own slot (one cache
// load, two record loads), so no wait in a block asks for a load of that block; the last
// `last mod kHubAhead` steps run from the registers and load nothing.
enum HubMode { kHubLong, kHubLds, kHubWave, kHubLanes };
constexpr int kWave = 64;
constexpr int kHubLanesMax = 3;  // the largest |H| stepped by lane broadcasts
template <HubMode MODE, int WM = kFusedWidth, int NH = 0>
__device__ __forceinline__ void hub_chain(const FusedP2Args& a, double (*vh)[kTPB], int last,
                                          int lc, bool writes, bool open,
                                          const int (&ent)[kFusedWidth],
                                          const double (&av)[kFusedWidth], double& vc, double& vp,
                                          double& xv) {
  const int t = threadIdx.x;
  const int nl = a.n_long;
  double yb[kHubAhead];
  double2 ra[kHubAhead], rb[kHubAhead];  // beta_sub, alpha; invb, ycoef
  auto load_rec = [&](int u, int jj) {
    const double2* p = reinterpret_cast<const double2*>(a.rec + 8 * (size_t)jj);
    ra[u] = p[0];
    rb[u] = p[1];
  };
#pragma unroll
  for (int u = 0; u < kHubAhead; ++u) {
    const int jj = clampi(1 + u, last);
    yb[u] = a.ycache[(size_t)(jj - 1) * nl + lc];
    load_rec(u, jj);
  }
  const uint32_t soff = writes ? (uint32_t)lc * 8u : kLaneOff;
  auto step = [&](int j, double s, const StepRec& r) {
    st_cache_row(a.ycache + (size_t)(j - 1) * nl, nl, soff, vc);  // v_j[r] in the sum's place
    if (MODE == kHubLds) {
      double* vb = vh[j & 1];
      vb[t] = vc;
      __syncthreads();
      if (open) {  // short_chunk_w's sum over the row's entries
        s = 0.0;
#pragma unroll
        for (int k = 0; k < WM; ++k) {
          const double prod = av[k] * vb[ent[k] < 0 ? 0 : ent[k]];
          s = s + (ent[k] >= 0 ? prod : -0.0);
        }
      }
    }
    if (MODE == kHubWave) {  // the same sum; every lane takes part in the shuffles
      double so = 0.0;
#pragma unroll
      for (int k = 0; k < WM; ++k) {
        const double prod = av[k] * __shfl(vc, ent[k] < 0 ? 0 : ent[k], kWave);
        so = so + (ent[k] >= 0 ? prod : -0.0);
      }
      s = open ? so : s;
    }
    if (MODE == kHubLanes) {  // the same sum; member m's v_j is lane m's, read once for all
      double bm[NH > 0 ? NH : 1];
#pragma unroll
      for (int m = 0; m < NH; ++m) bm[m] = readlane_f64(vc, m);
      double so = 0.0;
#pragma unroll
      for (int k = 0; k < WM; ++k) {
        double g = bm[0];
#pragma unroll
        for (int m = 1; m < NH; ++m) g = ent[k] == m ? bm[m] : g;
        const double prod = av[k] * g;
        so = so + (ent[k] >= 0 ? prod : -0.0);
      }
      s = open ? so : s;
    }
    fused_step_r(s, r, vc, vp, xv);
  };
  auto rec_of = [&](int u) { return StepRec{ra[u].x, ra[u].y, rb[u].x, rb[u].y}; };
  const int nblk = last / kHubAhead;
  int j0 = 1;
  // every load so far has landed before the first block (s_waitcnt vmcnt(0); step 1 waits
  // for its own anyway): the compiler folds the loop's entry state into the waits of every
  // iteration, and with these loads pending it asked each block for the previous block's last
  if (nblk > 0) __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int b = 0; b < nblk; ++b, j0 += kHubAhead) {
#pragma unroll
    for (int u = 0; u < kHubAhead; ++u) {
      const int j = j0 + u;
      step(j, yb[u], rec_of(u));
      // the slot's refill comes after its last use and stays there: a load hoisted over the
      // use needs a second register and a copy at the loop's end, which waits for the load
      __builtin_amdgcn_sched_barrier(0);
      const int jn = clampi(j + kHubAhead, last);
      yb[u] = a.ycache[(size_t)(jn - 1) * nl + lc];
      load_rec(u, jn);
    }
  }
  const int rem = last - nblk * kHubAhead;  // uniform
#pragma unroll
  for (int u = 0; u < kHubAhead - 1; ++u) {
    if (u >= rem) break;
    step(j0 + u, yb[u], rec_of(u));
  }
}

// The one-wave hub set: the chain's instance for the widest open row's width wm (1 ..
// kFusedWidth; uniform) and, for a small set, its size.
template <int NH, typename... Args>
__device__ __forceinline__ void hub_wave(int wm, Args&&... args) {
  constexpr HubMode M = NH > 0 ? kHubLanes : kHubWave;
  switch (wm) {
    case 1: return hub_chain<M, 1, NH>(args...);
    case 2: return hub_chain<M, 2, NH>(args...);
    case 3: return hub_chain<M, 3, NH>(args...);
    default: return hub_chain<M, kFusedWidth, NH>(args...);
  }
}

// Grid: [ceil(n_long / 256) long-row workgroups][the hub workgroup, if n_hub > 0].
__global__ __launch_bounds__(kTPB) void k_p2_hub(FusedP2Args a) {
  __shared__ double vh[2][kTPB];
  const int steps = fused_steps(a);
  if (steps < 2) return;  // uniform over the grid
  const int last = steps - 1;
  const int t = threadIdx.x;
  const int nl = a.n_long;
  const int64_t first_long = a.n - nl;
  const int n_lb = (nl + kTPB - 1) / kTPB;
  const bool hub = (int)blockIdx.x >= n_lb;  // uniform per workgroup
  // this thread's row: a long row (its sums come from cache column lc), or an open row of H
  bool live, open = false;
  int lc;
  int64_t row;
  int ent[kFusedWidth];
  double av[kFusedWidth];
#pragma unroll
  for (int k = 0; k < kFusedWidth; ++k) {
    ent[k] = -1;
    av[k] = 0.0;
  }
  if (hub) {
    live = t < a.n_hub;
    open = t < a.n_open;
    row = a.h_row[clampi(t, a.n_hub - 1)];
    lc = open ? 0 : clampi((int)(row - first_long), nl - 1);
    if (open) {
#pragma unroll
      for (int k = 0; k < kFusedWidth; ++k) {
        ent[k] = a.h_ent[t * kFusedWidth + k];
        av[k] = a.h_val[t * kFusedWidth + k];
      }
    }
  } else {
    const int l = blockIdx.x * kTPB + t;
    lc = clampi(l, nl - 1);
    row = first_long + lc;
    live = l < nl;
    // H's long rows belong to the hub workgroup (h_row[n_open ..] ascending; a few at most)
    for (int h = a.n_open; h < a.n_hub; ++h) live = live && a.h_row[h] != (int32_t)row;
  }
  double vc = a.v1[row], vp = 0.0, xv = a.x[row];
  if (hub && a.n_hub <= kWave) {
    if (t >= kWave) return;  // whole waves without a row of H, and no barrier ahead of them
    // the widest open row's width: one past the last entry any lane holds
    int wm = 1;
#pragma unroll
    for (int k = 1; k < kFusedWidth; ++k)
      if (__builtin_amdgcn_ballot_w64(ent[k] >= 0) != 0) wm = k + 1;
    const bool wr = live && !open;
    // an open row references another row of H, so |H| >= 2 wherever this workgroup exists
    static_assert(kHubLanesMax == 3, "the cases below");
    switch (a.n_hub <= kHubLanesMax ? a.n_hub : 0) {
      case 2: hub_wave<2>(wm, a, vh, last, lc, wr, open, ent, av, vc, vp, xv); break;
      case 3: hub_wave<3>(wm, a, vh, last, lc, wr, open, ent, av, vc, vp, xv); break;
      default: hub_wave<0>(wm, a, vh, last, lc, wr, open, ent, av, vc, vp, xv); break;
    }
  } else if (hub) {
    hub_chain<kHubLds>(a, vh, last, lc, live && !open, open, ent, av, vc, vp, xv);
  } else {
    hub_chain<kHubLong>(a, vh, last, lc, live, false, ent, av, vc, vp, xv);
  }
  if (live) st_out(a.x + row, xv);
}

// Entry e of the short chunks as stored (tpl_kcommon.h col_at / val_at), formats at run time:
// the entries are read once per solve.
__device__ __forceinline__ int fused_col(const FusedP2Args& a, int e, int cbase) {
  if (a.s_col16) {
    const int off = reinterpret_cast<const uint16_t*>(a.s_col)[e];
    return off == 0xFFFF ? -1 : cbase + off;
  }
  return reinterpret_cast<const int32_t*>(a.s_col)[e];
}
__device__ __forceinline__ double fused_val(const FusedP2Args& a, int e) {
  if (a.val_i8) return (double)reinterpret_cast<const int8_t*>(a.s_val)[e];
  return reinterpret_cast<const double*>(a.s_val)[e];
}

// k_p2_rows: kRowsGroup consecutive chunks per workgroup (256 threads each, staging the cache
// rows once for all of them), one barrier per block of S steps, and the cache rows of the next
// kRowsDepth blocks in registers. Fixed choices of the measurements in DESIGN.md 6.1 / 6.3.
constexpr int kRowsGroup = 4;
constexpr int kRowsThreads = kTPB * kRowsGroup;
constexpr int kRowsDepth = 2;
constexpr int kRowsStepsMax = 3;  // the cap on S
constexpr int kRowsGatherMax = 12;  // gathers of a block a thread issues at once (24 registers)

// S, the steps per barrier of k_p2_rows<W, NL>: as many cache rows as two buffers of them fit
// the 64 KiB one workgroup may ask for at the instance's largest n_long (2 S 256 NL 8 B <=
// 65,536: S <= 16 / NL), at most kRowsStepsMax.
constexpr int rows_block_steps(int NL) {
  const int fit = (64 * 1024) / (2 * kTPB * NL * (int)sizeof(double));
  return fit < kRowsStepsMax ? fit : kRowsStepsMax;
}

// Grid: one workgroup per kRowsGroup short chunks. W: the widest chunk (1 .. kFusedWidth);
// NL: ceil(n_long / 256). Block b is the steps 1 + b S .. (b + 1) S; their cache rows are
// contiguous, S n_long doubles, and are staged as one flat run, ceil(S NL / kRowsGroup) loads
// per thread. Dynamic LDS: two buffers of S n_long doubles, the second at S 256 NL doubles.
// The waves of a chunk past the last one take every barrier and stage with the rest.
template <int W, int NL>
__global__ __launch_bounds__(kRowsThreads) void k_p2_rows(FusedP2Args a) {
  extern __shared__ double lds[];
  constexpr int S = rows_block_steps(NL);
  constexpr int NLB = (S * NL + kRowsGroup - 1) / kRowsGroup;
  constexpr int D = kRowsDepth;
  constexpr int kBuf = S * kTPB * NL;  // the second buffer's place: fixed, an immediate offset
  static_assert(S >= 1 && 2 * kBuf * sizeof(double) <= 64 * 1024, "two buffers in one workgroup's LDS");
  const int steps = fused_steps(a);
  if (steps < 2) return;  // uniform over the grid
  const int last = steps - 1;
  const int tw = threadIdx.x;  // the staging index
  const int t = tw % kTPB;     // the thread of its chunk
  const int chunk_w = blockIdx.x * kRowsGroup + tw / kTPB;
  const bool have = chunk_w < a.n_chunks;
  const int chunk = have ? chunk_w : a.n_chunks - 1;
  const int nl = a.n_long;
  const int first_long = (int)(a.n - nl);
  // the chunk's entries: width, base and order as short_chunk has them
  const int wc = a.s_width > 0 ? a.s_width : a.c_width[chunk];
  const int base = a.s_width > 0 ? chunk * kChunkRows * a.s_width : a.c_base[chunk];
  const bool packed = a.s_width > 0 && packed_chunk_width(a.s_width);
  const int cbase = a.s_col16 ? a.s_cbase[chunk] : 0;
  int row[kRowsPerThread];
  bool live[kRowsPerThread];
  int li[kRowsPerThread][W];  // >= 0: long row's index; -1: padding; -2: the row itself
  double av[kRowsPerThread][W];
  double vc[kRowsPerThread], vp[kRowsPerThread], xv[kRowsPerThread];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    const int p = chunk * kChunkRows + q * kTPB + t;
    live[q] = have && p < a.n_short;
    row[q] = clampi(p, a.n_short - 1);  // the long rows are last: position = row
#pragma unroll
    for (int k = 0; k < W; ++k) {
      // entries past the chunk's own width re-read its last one (masked below); a chunk of
      // empty rows stores nothing: entry 0
      const int kc = clampi(k, wc - 1);
      const int e = wc <= 0 ? 0
                    : packed ? base + t * (kRowsPerThread * wc) + q * wc + kc
                             : base + kc * kChunkRows + q * kTPB + t;
      const int c = fused_col(a, e, cbase);
      av[q][k] = fused_val(a, e);
      int idx = -1;
      if (k < wc && c >= 0) {
        if (c >= first_long) idx = c - first_long;
        else if (c == row[q]) idx = -2;
        else live[q] = false;  // an open row: the hub workgroup's
      }
      li[q][k] = idx;
    }
    vc[q] = a.v1[row[q]];
    vp[q] = 0.0;
    xv[q] = a.x[row[q]];
  }
  const int bw = S * nl;  // the words of a block
  // What the wave's rows need per step, decided once (uniform: a ballot). Idle: no live row —
  // the waves of a missing chunk, of the part of the last chunk past n_short, of open rows
  // only — which stages and takes the barriers and does no row arithmetic, so that the one
  // workgroup with missing chunks does not set the kernel's length. Clean: every live row's
  // entries, all wc of the chunk's own width, are long-row indices — no self column and no
  // padding, so the sum is the plain wc products (an entry past wc would add -0.0: no bit).
  // General: the selects of the self column and the padding, over the instance's W.
  bool any_live = false, lane_clean = true;
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    any_live = any_live || live[q];
#pragma unroll
    for (int k = 0; k < W; ++k) lane_clean = lane_clean && (!live[q] || k >= wc || li[q][k] >= 0);
  }
  const int wcu = __builtin_amdgcn_readfirstlane(wc);  // the chunk is the wave's
  const bool idle = __builtin_amdgcn_ballot_w64(any_live) == 0;
  const bool clean = __builtin_amdgcn_ballot_w64(!lane_clean) == 0;
  // an entry's S gathers of a block: one LDS word index (below), a non-index entry's clamped
  int lx[kRowsPerThread][W];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q)
#pragma unroll
    for (int k = 0; k < W; ++k) lx[q][k] = (li[q][k] < 0 ? 0 : li[q][k]) * S;
  // slot d: block d (this thread's NLB words of it), then every D-th block after it. Words past
  // the block re-read its last one, words past the cache row of step `last` that row's last.
  double st[D][NLB];
  // In LDS a block lies step-minor: word s n_long + c of the run (step s of the block, long
  // row c) at c S + s, so that a row entry's S gathers of a block are one address and the
  // offsets 0 .. S - 1. The same for every block: where this thread's words go.
  int wofs[NLB];
#pragma unroll
  for (int u = 0; u < NLB; ++u) {
    const int i = tw + u * kRowsThreads;
    int sb = 0;
#pragma unroll
    for (int s = 1; s < S; ++s) sb += i >= s * nl ? 1 : 0;
    wofs[u] = (i - sb * nl) * S + sb;
  }
  // the same words as byte offsets into the run; the run's base and the clamp are uniform, so
  // a load's address costs one instruction
  uint32_t cb[NLB];
#pragma unroll
  for (int u = 0; u < NLB; ++u) cb[u] = 8u * (uint32_t)clampi(tw + u * kRowsThreads, bw - 1);
  auto fill = [&](int d, int b) {
    int r0 = b * S;         // the cache row of the block's first step
    if (r0 >= last) r0 = 0;  // a block wholly past step `last` is never used: any place will do
    const int rows = clampi(last - r0, S);  // those of steps 1 .. last
    const uint32_t lim = 8u * (uint32_t)(rows * nl - 1);
    const char* run = reinterpret_cast<const char*>(a.ycache + (size_t)r0 * nl);
#pragma unroll
    for (int u = 0; u < NLB; ++u)
      st[d][u] = *reinterpret_cast<const double*>(run + (cb[u] < lim ? cb[u] : lim));
  };
#pragma unroll
  for (int d = 0; d < D; ++d) fill(d, d);
  // The record of the step at hand in scalar registers; the next step's is fetched during the
  // step, behind its gathers (a scalar load in flight turns the wait for a gather into a wait
  // for everything) and ahead of its arithmetic, which hides it.
  StepRec rn{};
  if (!idle) rn = rec_scalar(a.rec, 1);
  // `cnt` steps of a block for the wave's rows. WC: the chunk's width on a clean wave, -1 on a
  // general one.
  auto row_steps = [&](const double* vb, int b, auto cnt, auto wcc) {
    constexpr int WC = decltype(wcc)::value;
    // a clean wave of few entries gathers the whole block at once (an entry's S words are
    // neighbours), so the block waits for LDS once and not once per step
    constexpr bool kAhead = WC >= 1 && WC * S * kRowsPerThread <= kRowsGatherMax;
    double g[kAhead ? S : 1][kRowsPerThread][kAhead ? WC : 1];
    if constexpr (kAhead) {
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q)
#pragma unroll
        for (int k = 0; k < WC; ++k)
#pragma unroll
          for (int s = 0; s < S; ++s) g[s][q][k] = vb[lx[q][k] + s];
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s >= cnt) break;
      const StepRec r = rn;
      double sum[kRowsPerThread];
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) {
        sum[q] = 0.0;
        if constexpr (kAhead) {
#pragma unroll
          for (int k = 0; k < WC; ++k) sum[q] = sum[q] + av[q][k] * g[s][q][k];
        } else if constexpr (WC >= 0) {
#pragma unroll
          for (int k = 0; k < WC; ++k) sum[q] = sum[q] + av[q][k] * vb[lx[q][k] + s];
        } else {
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const double g = vb[lx[q][k] + s];
            const double prod = av[q][k] * (li[q][k] == -2 ? vc[q] : g);
            sum[q] = sum[q] + (li[q][k] != -1 ? prod : -0.0);  // padding adds -0.0: exact
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      rn = rec_scalar(a.rec, clampi(2 + b * S + s, last));
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) fused_step_r(sum[q], r, vc[q], vp[q], xv[q]);
    }
  };
  // Block b from slot d, `cnt` of its steps (uniform; S in the main loop). The buffers
  // alternate with b: the waves write block b's buffer, meet at the block's one barrier, and
  // then gather and step S times from it on their own. Block b + 2 is written into the same
  // buffer only by a wave that has passed the barrier of block b + 1, which every wave reaches
  // after its last read of block b — so no write overtakes a read. The slot's last use (the
  // LDS writes) comes before its refill, which is then in flight over this and the next
  // D - 1 blocks' barriers, gathers and arithmetic.
  auto block = [&](int b, int d, auto cnt, auto refill) {
    double* vb = lds + (b & 1) * kBuf;
#pragma unroll
    for (int u = 0; u < NLB; ++u)  // the loads that lie wholly inside the smallest block
      if ((u + 1) * kRowsThreads <= S * (kTPB * (NL - 1) + 1) || tw + u * kRowsThreads < bw)
        vb[wofs[u]] = st[d][u];
    if (decltype(refill)::value) {
      __builtin_amdgcn_sched_barrier(0);
      fill(d, b + D);
    }
    __syncthreads();
    // the branches are uniform per wave and hold no barrier
    if (idle) return;
    if (!clean) return row_steps(vb, b, cnt, std::integral_constant<int, -1>{});
    switch (wcu) {
      case 1: return row_steps(vb, b, cnt, std::integral_constant<int, 1>{});
      case 2: return row_steps(vb, b, cnt, std::integral_constant<int, W < 2 ? W : 2>{});
      case 3: return row_steps(vb, b, cnt, std::integral_constant<int, W < 3 ? W : 3>{});
      case 4: return row_steps(vb, b, cnt, std::integral_constant<int, W < 4 ? W : 4>{});
      default: return row_steps(vb, b, cnt, std::integral_constant<int, 0>{});  // empty rows
    }
  };
  // whole groups of D blocks without an exit, then the last `last mod D S` steps from the
  // registers: whole blocks and one part of a block
  constexpr int B = D * S;
  const int ngrp = last / B;
  int b0 = 0;
  if (ngrp > 0) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as in hub_chain
  for (int g = 0; g < ngrp; ++g, b0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) block(b0 + d, d, std::integral_constant<int, S>{}, std::true_type{});
  }
  const int rem = last - ngrp * B;  // uniform, < B
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int cnt = rem - d * S;
    if (cnt <= 0) break;
    block(b0 + d, d, cnt, std::false_type{});
  }
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q)
    if (live[q]) st_out(a.x + row[q], xv[q]);
}

namespace launch {

static FusedP2Args fused_args(const CsrDev& A, const DevState& S, const double* ycache,
                              const double* v1, double* x, int steps) {
  FusedP2Args a{};
  a.ycache = const_cast<double*>(ycache);
  a.rec = S.p2c;
  a.flags = S.flags;
  a.v1 = v1;
  a.x = x;
  a.n = A.n;
  a.n_long = A.n_long;
  a.steps = steps;
  a.s_col = A.s_col;
  a.s_val = A.s_val;
  a.s_cbase = A.s_cbase;
  a.c_base = A.c_base;
  a.c_width = A.c_width;
  a.n_short = A.n_short;
  a.n_chunks = A.n_chunks;
  a.s_width = A.s_width;
  a.val_i8 = A.val_i8;
  a.s_col16 = A.s_col16;
  return a;
}

hipError_t p2_fused_hub(const CsrDev& A, const DevState& S, const FusedP2Dev& H, double* ycache,
                        const double* v1, double* x, int steps, hipStream_t s) {
  if (A.n_long <= 0 || !A.s_identity || H.n_hub > kFusedHubMax || H.n_open > H.n_hub)
    return hipErrorInvalidConfiguration;
  FusedP2Args a = fused_args(A, S, ycache, v1, x, steps);
  a.h_row = H.h_row;
  a.h_ent = H.h_ent;
  a.h_val = H.h_val;
  a.n_open = H.n_open;
  a.n_hub = H.n_hub;
  const int grid = (A.n_long + kTPB - 1) / kTPB + (H.n_hub > 0 ? 1 : 0);
  hipLaunchKernelGGL(k_p2_hub, dim3(grid), dim3(kTPB), 0, s, a);
  return hipGetLastError();
}

template <int W, int... NLs>
static bool rows_nl(int nloads, const FusedP2Args& a, int grid, size_t lds, hipStream_t s,
                    std::integer_sequence<int, NLs...>) {
  auto one = [&](auto NL) {
    if (nloads != decltype(NL)::value + 1) return false;
    hipLaunchKernelGGL((k_p2_rows<W, decltype(NL)::value + 1>), dim3(grid), dim3(kRowsThreads),
                       lds, s, a);
    return true;
  };
  return (one(std::integral_constant<int, NLs>{}) || ...);
}

hipError_t p2_fused_rows(const CsrDev& A, const DevState& S, const double* ycache,
                         const double* v1, double* x, int steps, hipStream_t s) {
  if (A.n_long <= 0 || A.n_long > kFusedLongMax || !A.s_identity)
    return hipErrorInvalidConfiguration;
  if (A.n_chunks <= 0) return hipSuccess;  // no short row
  const FusedP2Args a = fused_args(A, S, ycache, v1, x, steps);
  const int nloads = (A.n_long + kTPB - 1) / kTPB;
  const size_t lds = (size_t)rows_block_steps(nloads) * (nloads * kTPB + A.n_long) * sizeof(double);
  constexpr auto nls = std::make_integer_sequence<int, kFusedLongMax / kTPB>{};
  // W: the widest chunk. A uniform layout has its width; per-chunk widths (s_width == 0)
  // run the widest instance, each chunk masking the entries past its own width
  const int w = A.s_width > 0 ? A.s_width : kFusedWidth;
  const int grid = (A.n_chunks + kRowsGroup - 1) / kRowsGroup;
  bool ok = false;
  switch (w) {
    case 1: ok = rows_nl<1>(nloads, a, grid, lds, s, nls); break;
    case 2: ok = rows_nl<2>(nloads, a, grid, lds, s, nls); break;
    case 3: ok = rows_nl<3>(nloads, a, grid, lds, s, nls); break;
    case 4: ok = rows_nl<4>(nloads, a, grid, lds, s, nls); break;
    default: break;
  }
  return ok ? hipGetLastError() : hipErrorInvalidConfiguration;
}

} // namespace launch
} // namespace tpl
