"""Dev tool: the long-row cache in the multi-function and batch two-pass solves
(tpl_op_set_long_cache_solvers) against a build without it, at the 500k-arc headline
(locality order pinned at 13 groups, k = 500, vectors resident on the device, f on the host).

Two builds of the package are compared: `--pkg` (this tree's two-pass-lanczos_amd, the
default) and `--parent-pkg` (a copy of the parent commit's two-pass-lanczos_amd directory with
its own libtpl_amd.so). The driver alternates them, `--rounds` times, and then runs the
parent once more (parent against parent: the A/A spread). One process per line, each under
its own time limit; a line is one (build, case):
  multi4    one solvers.lanczos_two_pass_multi call, m = 4 (f_i = ftk.inv_shift(1 + i));
            beside it, alternated, the 4 single host-f solves it replaces
  batch2    one solvers.lanczos_two_pass_batch call, s = 2 (f = ftk.INV); beside it the s
  batch4    single solves, and algorithms.lanczos_pass_one_batch alone (pass one of the
            group; a stand-alone pass never stores the cache: the null-pointer k_bp1_spmv)
  bm4x4     one solvers.lanczos_two_pass_batch_multi call, s = 4, m = 4
The tree's lines run with the case's bit set (2, 4, 4, 8; `--mask 0` in a worker: the setter
is never called, which is all a parent build can do). Every line, after one warm-up, checks
that the call's result is bitwise the single host-f solves', then times 7 repetitions.
Prints one JSON line per process and, at the end, per case the medians (min-max) of every
process's median, parent against tree.

    python scripts/long_cache_wide_timing.py --parent-pkg DIR [--rounds 3] [--cases batch4 ...]
    python scripts/long_cache_wide_timing.py --solve-only batch4 [--mask 4] [--pkg DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"multi4": (1, 4, 2), "batch2": (2, 1, 4), "batch4": (4, 1, 4), "bm4x4": (4, 4, 8)}  # s, m, bit


def setup(arcs, s, groups, mask):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import tpl_amd
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    cache = f"/tmp/lcw_{arcs}.npz"   # the parsed matrix, shared by the processes of one run
    if os.path.exists(cache):
        a = sp.load_npz(cache)
    else:
        qfc = f"/tmp/lcw_{arcs}.qfc"
        write_qfc_3line(qfc, arcs)
        a = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                            qfc).a
        sp.save_npz(cache + ".tmp.npz", a, compressed=False)
        os.replace(cache + ".tmp.npz", cache)
    n = a.shape[0]
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    if mask:
        op.set_long_cache_solvers(mask)
    rng = np.random.default_rng(1)
    cols = [a @ np.full(n, 1.0 / np.sqrt(n))] + [rng.standard_normal(n) for _ in range(s - 1)]
    B = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=0))).cuda().t()
    return op, B, n


def calls(op, B, k, case):
    """-> (the case's call, its single solves, pass one alone or None, result -> [columns])."""
    from tpl_amd import algorithms, ftk, solvers
    s, m, _ = CASES[case]
    bs = [B[:, c].contiguous() for c in range(s)]
    fs = [ftk.inv_shift(1.0 + i) for i in range(m)] if m > 1 else [ftk.INV]

    def singles():
        op.set_device_ftk(0)
        out = [solvers.lanczos_two_pass(op, b, k, f) for b in bs for f in fs]
        op.set_device_ftk(2)
        return out

    if case == "multi4":
        return (lambda: solvers.lanczos_two_pass_multi(op, bs[0], k, fs), singles, None,
                lambda X: [X[:, i] for i in range(m)])
    p1 = lambda: algorithms.lanczos_pass_one_batch(op, B, k)
    if case == "bm4x4":
        return (lambda: solvers.lanczos_two_pass_batch_multi(op, B, k, fs), singles, p1,
                lambda X: [X[:, i, c] for c in range(s) for i in range(m)])
    return (lambda: solvers.lanczos_two_pass_batch(op, B, k, ftk.INV), singles, p1,
            lambda X: [X[:, c] for c in range(s)])


def worker(a):
    import torch
    op, B, n = setup(a.arcs, CASES[a.worker][0], a.groups, a.mask)
    call, singles, p1, cols = calls(op, B, a.k, a.worker)
    variants = {"call": call, "singles": singles}
    if p1:
        variants["p1batch"] = p1
        p1()
    X = call()   # warm-up of each, and the result check
    flags = op.flags()
    ref = singles()
    for _ in range(a.warmups - 1):   # further warm-ups: a graph's second launch is a slow one
        for run in variants.values():
            run()
    same = all(torch.equal(x.contiguous().view(torch.int64), r.contiguous().view(torch.int64))
               for x, r in zip(cols(X), ref))
    times = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
    print(json.dumps({
        "label": a.label, "case": a.worker, "mask": a.mask, "arcs": a.arcs, "n": n, "k": a.k,
        "reps": a.reps, "warmups": a.warmups, "order_groups": op.order_groups(), "cached": bool(flags & 256),
        "bitwise_equal_singles": same, "device_bytes": op.device_bytes(),
        **{f"{name}_ms": round(statistics.median(v), 4) for name, v in times.items()},
        **{f"{name}_min_ms": round(min(v), 4) for name, v in times.items()},
        **{f"{name}_max_ms": round(max(v), 4) for name, v in times.items()},
        **{f"{name}_reps_ms": [round(t, 3) for t in v] for name, v in times.items()}}), flush=True)
    return 0 if same else 1


def solve_only(a):
    import torch
    op, B, _ = setup(a.arcs, CASES[a.solve_only][0], a.groups, a.mask)
    call = calls(op, B, a.k, a.solve_only)[0]
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    return 0


def summary(lines):
    print("# case       what      label   n  median of medians (min-max of medians), ms;"
          " widest min-max of one process's repetitions")
    for case in CASES:
        for what in ("call", "p1batch", "singles"):
            for label in ("parent", "tree"):
                v = [l[what + "_ms"] for l in lines
                     if l["case"] == case and l["label"] == label and what + "_ms" in l]
                if v:
                    w = max(l[what + "_max_ms"] - l[what + "_min_ms"] for l in lines
                            if l["case"] == case and l["label"] == label and what + "_ms" in l)
                    print("# %-10s %-9s %-6s %2d  %.3f (%.3f-%.3f); %.3f" % (
                        case, what, label, len(v), statistics.median(v), min(v), max(v), w))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--k", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmups", type=int, default=1)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--pkg", default=os.path.join(ROOT, "two-pass-lanczos_amd"))
    p.add_argument("--parent-pkg", default="")
    p.add_argument("--step-timeout", type=float, default=150.0)
    p.add_argument("--worker", default="", choices=[""] + list(CASES), help="internal")
    p.add_argument("--mask", type=int, default=0, help="worker: the solver mask (0: default)")
    p.add_argument("--label", default="tree")
    p.add_argument("--solve-only", default="", choices=[""] + list(CASES),
                   help="three calls of this case and nothing else (run under a profiler)")
    a = p.parse_args()
    if a.worker or a.solve_only:
        sys.path.insert(0, a.pkg)
        return solve_only(a) if a.solve_only else worker(a)
    if a.reps < 5 or a.rounds < 1 or not a.parent_pkg:
        p.error("--reps >= 5, --rounds >= 1 and --parent-pkg are needed")
    order = [("parent", a.parent_pkg), ("tree", a.pkg)] * a.rounds + [("parent", a.parent_pkg)]
    lines = []
    for label, pkg in order:   # a fresh process per line; stop at the first failure
        for case in a.cases:
            mask = CASES[case][2] | 1 if label == "tree" else 0
            cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--k", str(a.k),
                   "--reps", str(a.reps), "--warmups", str(a.warmups), "--groups", str(a.groups), "--worker", case,
                   "--mask", str(mask), "--label", label, "--pkg", pkg]
            try:
                r = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                print(f"{label} {case}: time limit of {a.step_timeout:.0f} s reached; stopping",
                      flush=True)
                return 124
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                print(f"{label} {case}: exit status {r.returncode}; stopping", flush=True)
                return r.returncode
            lines += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    summary(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
