"""Per-chunk span of long-row indices in the fused pass two's short chunks, on the CPU (dev
tool; DESIGN.md §6.3: the per-chunk window candidate of k_p2_rows).

For each of the three KKT fixtures in the order the bench pins (HostPlan: the runtime's own
layout code, no GPU), every chunk of 512 consecutive short-row positions references long
rows lo .. hi of the n_long the workgroup stages per step; the span is hi - lo + 1. A window
per chunk in place of the whole cache row pays only where the spans are well below n_long.

usage: python scripts/fused_chunk_spans.py [CHUNKS_PER_WORKGROUP]   (default 1; 4 ships)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "two-pass-lanczos_amd"))
sys.path.insert(0, ROOT)

from bench import PINNED_ORDER_GROUPS, load_workload  # noqa: E402
from tpl_amd.operator import HostPlan  # noqa: E402

CHUNK_ROWS = 512
GROUP = int(sys.argv[1]) if len(sys.argv) > 1 else 1  # chunks per workgroup (kRowsGroup)

for arcs in (5000, 50000, 500000):
    a = load_workload(arcs)[0].a.tocsr()
    plan = HostPlan(a, order_groups=PINNED_ORDER_GROUPS.get(arcs, 0))
    s = plan.schedule()
    plan.close()
    perm = s["perm"] if s["perm"] is not None else np.arange(a.shape[0])
    pos = np.empty(a.shape[0], dtype=np.int64)
    pos[perm] = np.arange(a.shape[0])  # internal position of the caller's row
    n_short, n_long = len(s["short_rows"]), len(s["long_rows"])
    first_long = a.shape[0] - n_long
    assert np.array_equal(s["long_rows"], np.arange(first_long, a.shape[0])), "long rows last"
    spans = []
    for c0 in range(0, n_short, CHUNK_ROWS * GROUP):
        rows = perm[s["short_rows"][c0:c0 + CHUNK_ROWS * GROUP]]
        cols = np.concatenate([a.indices[a.indptr[r]:a.indptr[r + 1]] for r in rows])
        li = pos[cols] - first_long
        li = li[li >= 0]
        spans.append(int(li.max() - li.min() + 1) if li.size else 0)
    spans = np.array(spans)
    print(f"{arcs:7d} arcs: n_long {n_long:5d}, {len(spans):4d} groups of {GROUP}, span min {spans.min()} "
          f"median {int(np.median(spans))} max {spans.max()} "
          f"(median / n_long = {np.median(spans) / n_long:.2f})")
