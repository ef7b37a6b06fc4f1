"""Dev tool: f_i(A) b_c for m functions and s right-hand sides in one call against the three
ways to get the same bits without it, at the 500k-arc headline (locality order pinned at 13
groups, k = 500, B and X resident on the device, f_i = ftk.inv_shift(1 + i) on the host).

For (s, m) in (2, 2), (4, 2), (4, 4), (4, 8), (8, 4), one process per pair (each under its own
time limit) times, alternating, after one warm-up of each:
  new       one solvers.lanczos_two_pass_batch_multi call (as the entry point routes it);
  multis    s solvers.lanczos_two_pass_multi calls, one per column;
  batches   m solvers.lanczos_two_pass_batch calls, one per function;
  singles   s m solvers.lanczos_two_pass calls with f(T_k) on the host (set_device_ftk(0));
  p1batch   one algorithms.lanczos_pass_one_batch call (pass one of the groups alone);
  p2fused   one algorithms.lanczos_pass_two_batch_multi call on the decompositions and
            coefficients computed beforehand: the fused pass two of every group (the low-level
            call never routes away from it), uploads and downloads included.
Every run asserts that `new`, `multis`, `batches` and `p2fused` are bitwise the singles.
Prints per pair the medians and min-max in ms and the ratios new / multis, new / batches.

    python scripts/batch_multi_timing.py [--arcs 500000] [--k 500] [--reps 7] [--pairs 2x2 4x4]
    python scripts/batch_multi_timing.py --solve-only 4x4   # three new calls, for a profiler
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "two-pass-lanczos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_timing import setup  # noqa: E402  (the same operator and columns)

DEFAULT_PAIRS = ["2x2", "4x2", "4x4", "4x8", "8x4"]


def pair(text):
    s, m = text.split("x")
    return int(s), int(m)


def worker(arcs, k, s, m, reps, groups):
    import numpy as np
    import torch
    from tpl_amd import algorithms, ftk, solvers

    op, B, n = setup(arcs, s, groups)
    bs = [B[:, c].contiguous() for c in range(s)]
    fs = [ftk.inv_shift(1.0 + i) for i in range(m)]

    def new():
        return solvers.lanczos_two_pass_batch_multi(op, B, k, fs)

    def multis():
        return [solvers.lanczos_two_pass_multi(op, b, k, fs) for b in bs]

    def batches():
        return [solvers.lanczos_two_pass_batch(op, B, k, f) for f in fs]

    def singles():
        op.set_device_ftk(0)
        out = [[solvers.lanczos_two_pass(op, b, k, f) for f in fs] for b in bs]
        op.set_device_ftk(2)
        return out

    def p1batch():
        return algorithms.lanczos_pass_one_batch(op, B, k)

    decs = p1batch()
    Ys = [np.stack([np.asarray(f(d.alphas, d.betas)) * d.b_norm for f in fs], axis=1) for d in decs]

    def p2fused():
        return algorithms.lanczos_pass_two_batch_multi(op, B, decs, Ys)

    def bits(t):
        return t.contiguous().view(torch.int64)

    ref = singles()  # warm-up of each, and the result checks
    X, Xm, Xb, Xl = new(), multis(), batches(), p2fused()
    same = {
        "new": all(torch.equal(bits(X[:, i, c]), bits(ref[c][i])) for c in range(s) for i in range(m)),
        "multis": all(torch.equal(bits(Xm[c][:, i]), bits(ref[c][i])) for c in range(s) for i in range(m)),
        "batches": all(torch.equal(bits(Xb[i][:, c]), bits(ref[c][i])) for c in range(s) for i in range(m)),
        "p2fused": all(torch.equal(bits(Xl[:, i, c]), bits(ref[c][i])) for c in range(s) for i in range(m)),
    }
    assert all(same.values()), same
    variants = {"new": new, "multis": multis, "batches": batches, "singles": singles,
                "p1batch": p1batch, "p2fused": p2fused}
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
    med = {name: statistics.median(v) for name, v in times.items()}
    print(json.dumps({
        "arcs": arcs, "n": n, "k": k, "s": s, "m": m, "reps": reps,
        "order_groups": op.order_groups(), "steps": [d.steps_taken for d in decs],
        "bitwise_equal_singles": all(same.values()),
        **{f"{name}_ms": round(v, 4) for name, v in med.items()},
        **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
        **{f"{name}_max_ms": round(max(times[name]), 4) for name in times},
        "new_over_multis": round(med["new"] / med["multis"], 4),
        "new_over_batches": round(med["new"] / med["batches"], 4),
        "new_over_singles": round(med["new"] / med["singles"], 4)}), flush=True)


def solve_only(arcs, k, s, m, groups):
    import torch
    from tpl_amd import ftk, solvers
    op, B, _ = setup(arcs, s, groups)
    fs = [ftk.inv_shift(1.0 + i) for i in range(m)]
    for _ in range(3):
        solvers.lanczos_two_pass_batch_multi(op, B, k, fs)
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--k", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--pairs", nargs="+", default=DEFAULT_PAIRS, help="s x m pairs, e.g. 4x4")
    p.add_argument("--step-timeout", type=float, default=150.0)
    p.add_argument("--worker", default="", help="internal: time this s x m pair in-process")
    p.add_argument("--solve-only", default="",
                   help="three new calls of this s x m pair and nothing else (run under a profiler)")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.solve_only:
        solve_only(a.arcs, a.k, *pair(a.solve_only), a.groups)
        return 0
    if a.worker:
        worker(a.arcs, a.k, *pair(a.worker), a.reps, a.groups)
        return 0
    for sm in a.pairs:  # a fresh process per pair, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--k", str(a.k),
               "--reps", str(a.reps), "--groups", str(a.groups), "--worker", sm]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"{sm}: time limit of {a.step_timeout:.0f} s reached; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{sm}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
