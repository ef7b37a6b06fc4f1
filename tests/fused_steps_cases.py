"""The fused pass two's block structure, as the tests see it (DESIGN.md §2;
two-pass-lanczos_amd/csrc/tpl_k_p2_fused.hip): k_p2_rows<W, NL> takes S steps per barrier and
keeps kRowsDepth blocks in registers, S a function of NL = ceil(n_long / 256); k_p2_hub steps
a hub set of at most kHubLanesMax members by lane broadcasts. The numbers are derived from the
source's constants here; tests/test_fused_pass_two_steps_cpu.py checks them against the
compiled kernels, and tests/test_gpu_fused_pass_two_steps.py takes its edges from them.
"""
import re

import numpy as np

import fused_tuned_cases as tc

LDS_PER_WG = 64 * 1024  # bytes one workgroup may ask for
CHUNK_ROWS = 512        # rows of a short chunk: 256 threads, two rows each
IDLE, CLEAN, GENERAL = 0, 1, 2


def source_constant(name):
    with open(tc.SOURCE) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


STEPS_MAX = source_constant("kRowsStepsMax")
HUB_LANES_MAX = source_constant("kHubLanesMax")


def block_steps(nl):
    """S of k_p2_rows<W, nl>: the cache rows of two buffers within LDS_PER_WG at the
    instance's largest n_long (2 S 256 nl 8 B), at most kRowsStepsMax."""
    return min(LDS_PER_WG // (2 * tc.TPB * nl * 8), STEPS_MAX)


def rows_block(n_long):
    """-> (S, B): the steps per barrier and the steps held in registers at once."""
    s = block_steps(-(-n_long // tc.TPB))
    return s, s * tc.ROWS_DEPTH


def step_edge_ks(n_long):
    """k for last = k - 1 in {1, S - 1, S, S + 1, B - 1, B, B + 1, 2 B + 1}."""
    s, b = rows_block(n_long)
    return sorted({l + 1 for l in (1, s - 1, s, s + 1, b - 1, b, b + 1, 2 * b + 1) if l >= 1})


def staging_loads(n_long):
    """-> (loads per thread the instance issues per block, words of the block's last load that
    lie inside the block; 0: that load is absent at this n_long)."""
    s, _ = rows_block(n_long)
    threads = tc.TPB * tc.ROWS_GROUP
    nlb = -(-s * -(-n_long // tc.TPB) // tc.ROWS_GROUP)
    return nlb, max(0, min(threads, s * n_long - (nlb - 1) * threads))


def wave_classes(a, sched, uniform_width):
    """What every wave of k_p2_rows does with its rows, from the matrix and the operator's
    schedule (op.schedule(); uniform_width = op.kernel_variant() & 7, 0: per-chunk widths):
    an int array [workgroup][chunk of the workgroup][wave of the chunk] of IDLE (no live row:
    a missing chunk, rows past the last, open rows), CLEAN (every live row holds exactly the
    chunk's width of entries, all of them long-row columns) or GENERAL (a self column or
    padding on a live row)."""
    perm, n = sched["perm"], a.shape[0]
    ai = a.tocsr()
    if perm is not None:
        ai = ai[perm][:, perm].tocsr()
    ai.sort_indices()
    n_short = len(sched["short_rows"])
    assert np.array_equal(sched["short_rows"], np.arange(n_short))
    assert np.array_equal(sched["long_rows"], np.arange(n_short, n))
    nnz = np.diff(ai.indptr)[:n_short]
    has_self = np.zeros(n_short, dtype=bool)
    is_open = np.zeros(n_short, dtype=bool)
    for p in range(n_short):
        cols = ai.indices[ai.indptr[p]:ai.indptr[p + 1]]
        has_self[p] = np.any(cols == p)
        is_open[p] = np.any((cols < n_short) & (cols != p))
    n_chunks = -(-n_short // CHUNK_ROWS)
    n_wg = -(-n_chunks // tc.ROWS_GROUP)
    out = np.full((n_wg, tc.ROWS_GROUP, tc.TPB // 64), IDLE)
    for c in range(n_chunks):
        rows = np.arange(c * CHUNK_ROWS, min((c + 1) * CHUNK_ROWS, n_short))
        wc = uniform_width or int(nnz[rows].max())
        live = ~is_open[rows]
        lane_clean = ~live | ((nnz[rows] == wc) & ~has_self[rows])
        wave = ((rows - c * CHUNK_ROWS) % tc.TPB) // 64
        for w in range(tc.TPB // 64):
            m = wave == w
            if live[m].any():
                out[c // tc.ROWS_GROUP, c % tc.ROWS_GROUP, w] = CLEAN if lane_clean[m].all() else GENERAL
    return out
