"""Dev tool: exp(t_i A) b_c for m times and s right-hand sides — the new call against the
batch-multi solve with exp_t closures, at the 500k-arc headline (locality order pinned at 13
groups, k = 500, B and X resident on the device).

For (s, m) in {(2, 1), (2, 4), (4, 1), (4, 4), (4, 8)} and t_i = 0.25 (i + 1), one process per
shape (each under its own time limit) times, alternating, after one warm-up of each:
  closures  (a) solvers.lanczos_two_pass_batch_multi with ftk.exp_t(t_i): every
            exp(t_i T_k) e_1 of every column a host QL sweep behind a Python closure (today's
            way, and the baseline: none of its code changes);
  host      (b) solvers.lanczos_two_pass_batch_exp_times under set_device_ftk(0): the native
            host built-in tpl_ftk_exp_t, no Python between the passes;
  device    (c) the same call in the default mode: k_ftk_exp_times_batch, one workgroup per
            (time, column).
Prints per shape one JSON line: the medians and minima in ms, every repetition of (a) and (c)
(the shape's run-to-run spread), on_device of (c) and whether it was the same in every run,
whether (b) is bitwise (a), the ratios, and the largest relative column difference of (c)
against (b) (the device exp's tolerance class, not bits).

    python scripts/batch_exp_times_timing.py [--arcs 500000] [--k 500] [--reps 7]
                                             [--shapes 2x1 2x4 4x1 4x4 4x8]
    python scripts/batch_exp_times_timing.py --solve-only 4x4   # for a rocprofv3 run
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

    qfc = f"/tmp/batch_exp_times_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    a = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                        qfc).a
    n = a.shape[0]
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    # column 0 is the harness's b; the others are seeded and differ per column
    cols = [a @ np.full(n, 1.0 / np.sqrt(n))]
    cols += [a @ np.random.default_rng(100 + c).standard_normal(n) for c in range(1, s)]
    B = torch.from_numpy(np.stack(cols, axis=1)).cuda()
    return op, B, n


def worker(arcs, k, s, m, reps, groups):
    import torch
    from tpl_amd import ftk, solvers

    op, B, n = setup(arcs, s, groups)
    ts = [0.25 * (i + 1) for i in range(m)]
    fs = [ftk.exp_t(t) for t in ts]
    on_seen = []

    def closures():
        return solvers.lanczos_two_pass_batch_multi(op, B, k, fs)

    def host():
        op.set_device_ftk(0)
        try:
            return solvers.lanczos_two_pass_batch_exp_times(op, B, k, ts)
        finally:
            op.set_device_ftk(2)

    def device():
        x, on = solvers.lanczos_two_pass_batch_exp_times(op, B, k, ts, return_on_device=True)
        on_seen.append([[int(v) for v in row] for row in on])  # (m, s)
        return x

    variants = {"closures": closures, "host": host, "device": device}
    Xa, Xb, Xc = closures(), host(), device()  # the warm-up of each, and the result checks
    same_ab = bool(torch.equal(Xa.contiguous().view(torch.int64), Xb.contiguous().view(torch.int64)))
    rel = max(float(torch.linalg.norm(Xc[:, i, c] - Xb[:, i, c]) / torch.linalg.norm(Xb[:, i, c]))
              for i in range(m) for c in range(s))
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
        "order_groups": op.order_groups(), "ts": ts, "on_device": on_seen[-1],
        "on_device_same_every_run": all(o == on_seen[0] for o in on_seen),
        "host_bitwise_equal_closures": same_ab, "device_vs_host_max_rel": rel,
        **{f"{name}_ms": round(v, 4) for name, v in med.items()},
        **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
        "closures_all_ms": [round(v, 3) for v in times["closures"]],
        "device_all_ms": [round(v, 3) for v in times["device"]],
        "device_over_closures": round(med["device"] / med["closures"], 4),
        "device_over_host": round(med["device"] / med["host"], 4),
        "host_over_closures": round(med["host"] / med["closures"], 4)}), flush=True)


def solve_only(arcs, k, s, m, groups):
    """One warm-up and three device-mode calls, for a kernel trace of k_ftk_exp_times_batch."""
    import torch
    from tpl_amd import solvers

    op, B, _ = setup(arcs, s, groups)
    ts = [0.25 * (i + 1) for i in range(m)]
    for _ in range(4):
        solvers.lanczos_two_pass_batch_exp_times(op, B, k, ts)
    torch.cuda.synchronize()


def shape(text):
    s, m = text.lower().split("x")
    return int(s), int(m)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--k", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--shapes", type=shape, nargs="+",
                   default=[(2, 1), (2, 4), (4, 1), (4, 4), (4, 8)], metavar="SxM")
    p.add_argument("--step-timeout", type=float, default=150.0)
    p.add_argument("--worker", type=shape, default=None, help="internal: time this shape in-process")
    p.add_argument("--solve-only", type=shape, default=None, metavar="SxM")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.solve_only:
        solve_only(a.arcs, a.k, *a.solve_only, a.groups)
        return 0
    if a.worker:
        worker(a.arcs, a.k, *a.worker, a.reps, a.groups)
        return 0
    for s, m in a.shapes:  # a fresh process per shape, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--k", str(a.k),
               "--reps", str(a.reps), "--groups", str(a.groups), "--worker", f"{s}x{m}"]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"s = {s}, m = {m}: time limit of {a.step_timeout:.0f} s reached; stopping",
                  flush=True)
            return 124
        if rc != 0:
            print(f"s = {s}, m = {m}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
