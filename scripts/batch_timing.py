"""Dev tool: one lock-step batch two-pass solve against s single solves, at the 500k-arc
headline (locality order pinned at 13 groups, k = 500, B and X resident on the device,
f = ftk.INV evaluated on the host).

For s in {1, 2, 3, 4, 7, 8}, one process per s (each under its own time limit) times, alternating,
after one warm-up of each:
  batch     one solvers.lanczos_two_pass_batch call (the columns in groups of 4 / 2 / 1);
  singles   s solvers.lanczos_two_pass calls with f(T_k) on the host (set_device_ftk(0)):
            the code path each batch column is bitwise equal to (checked inside the run);
  split     (--split) the columns cut 4 / 2 / 1 by hand: batch calls of four and two columns
            and a single solve, i.e. what a remainder of three costs without a padded group;
  p1batch   one algorithms.lanczos_pass_one_batch call (pass one alone), from which the
            per-step figures of the two passes are derived:
            pass one = p1batch / k, pass two = (batch - p1batch) / (k - 1).
Prints per s the medians and min-max in ms and the ratio batch / singles.

    python scripts/batch_timing.py [--arcs 500000] [--k 500] [--reps 7] [--ss 1 2 3 4 7 8] [--split]
    python scripts/batch_timing.py --solve-only 4     # three batch solves, for a profiler
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


def setup(arcs, s, groups):
    import numpy as np
    import torch
    import tpl_amd
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    qfc = f"/tmp/batch_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    a = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                        qfc).a
    n = a.shape[0]
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    rng = np.random.default_rng(1)
    cols = [a @ np.full(n, 1.0 / np.sqrt(n))] + [rng.standard_normal(n) for _ in range(s - 1)]
    # (s, n) C-order, transposed: the column-major (n, s) block the binding takes as it is
    B = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=0))).cuda().t()
    return op, B, n


def worker(arcs, k, s, reps, groups, with_split=False):
    import torch
    from tpl_amd import algorithms, ftk, solvers

    op, B, n = setup(arcs, s, groups)
    bs = [B[:, c].contiguous() for c in range(s)]

    def batch():
        return solvers.lanczos_two_pass_batch(op, B, k, ftk.INV)

    def singles():
        op.set_device_ftk(0)
        out = [solvers.lanczos_two_pass(op, b, k, ftk.INV) for b in bs]
        op.set_device_ftk(2)
        return out

    def p1batch():
        return algorithms.lanczos_pass_one_batch(op, B, k)

    def split():
        # the columns cut 4 / 2 / 1 by hand (no padded group): fours, then a two, then a single
        out, c = [], 0
        while c < s:
            w = 4 if s - c >= 4 else (2 if s - c >= 2 else 1)
            if w == 1:
                op.set_device_ftk(0)
                out.append(solvers.lanczos_two_pass(op, bs[c], k, ftk.INV))
                op.set_device_ftk(2)
            else:
                out.append(solvers.lanczos_two_pass_batch(op, B[:, c:c + w], k, ftk.INV))
            c += w
        return out

    variants = {"batch": batch, "singles": singles, "p1batch": p1batch}
    if with_split:
        variants["split"] = split
        split()
    X, ref = batch(), singles()  # warm-up of each, and the result check
    same = all(torch.equal(X[:, c].contiguous().view(torch.int64), ref[c].view(torch.int64))
               for c in range(s))
    steps = [d.steps_taken for d in p1batch()]
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
        "arcs": arcs, "n": n, "k": k, "s": s, "reps": reps, "order_groups": op.order_groups(),
        "steps": steps, "columns_bitwise_equal_single": same,
        **{f"{name}_ms": round(v, 4) for name, v in med.items()},
        **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
        **{f"{name}_max_ms": round(max(times[name]), 4) for name in times},
        "batch_over_singles": round(med["batch"] / med["singles"], 4),
        **({"split_over_singles": round(med["split"] / med["singles"], 4)} if with_split else {}),
        "p1_us_per_step": round(1e3 * med["p1batch"] / k, 3),
        "p2_us_per_step": round(1e3 * (med["batch"] - med["p1batch"]) / max(k - 1, 1), 3)}),
        flush=True)


def solve_only(arcs, k, s, groups):
    import torch
    from tpl_amd import ftk, solvers
    op, B, _ = setup(arcs, s, groups)
    for _ in range(3):
        solvers.lanczos_two_pass_batch(op, B, k, ftk.INV)
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--k", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--ss", type=int, nargs="+", default=[1, 2, 3, 4, 7, 8])
    p.add_argument("--step-timeout", type=float, default=150.0)
    p.add_argument("--worker", type=int, default=0, help="internal: time this s in-process")
    p.add_argument("--split", action="store_true",
                   help="also time the columns cut 4 / 2 / 1 by hand: fours, a two, a single "
                        "solve (what a remainder of three costs without a padded group)")
    p.add_argument("--solve-only", type=int, default=0,
                   help="three batch solves of this s and nothing else (run under a profiler)")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.solve_only:
        solve_only(a.arcs, a.k, a.solve_only, a.groups)
        return 0
    if a.worker:
        worker(a.arcs, a.k, a.worker, a.reps, a.groups, a.split)
        return 0
    for s in a.ss:  # a fresh process per s, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--k", str(a.k),
               "--reps", str(a.reps), "--groups", str(a.groups), "--worker", str(s)] + (["--split"] if a.split else [])
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"s = {s}: time limit of {a.step_timeout:.0f} s reached; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"s = {s}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
