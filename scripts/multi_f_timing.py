"""Dev tool: one multi-function two-pass solve against m single solves, at the 500k-arc
headline (locality order pinned at 13 groups, k = 500, b and X resident on the device).

For m in {1, 2, 4, 8} and f_i = ftk.inv_shift(sigma_i), sigma_i = 1 + i, one process per m
(each under its own time limit) times, alternating, after one warm-up of each:
  multi     one solvers.lanczos_two_pass_multi call (pass one once, one pass two);
  host      m solvers.lanczos_two_pass calls with f(T_k) on the host (set_device_ftk(0)):
            the code path each multi column is bitwise equal to;
  default   the same m calls under the default mode (set_device_ftk(2); these closures
            still run on the host, only the built-in INV / EXP move to the device);
  inv1g     m calls with the built-in INV as one device graph each: the fastest single
            solve the engine has, for scale (not the same functions).
Prints per m the medians in ms and the ratios multi / host, multi / default.

    python scripts/multi_f_timing.py [--arcs 500000] [--k 500] [--reps 7] [--ms 1 2 4 8]
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


def worker(arcs, k, m, reps, groups):
    import numpy as np
    import torch
    import tpl_amd
    from tpl_amd import ftk, solvers
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    qfc = f"/tmp/multi_f_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    a = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                        qfc).a
    n = a.shape[0]
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    b = torch.from_numpy(a @ np.full(n, 1.0 / np.sqrt(n))).cuda()
    fs = [ftk.inv_shift(1.0 + i) for i in range(m)]

    def multi():
        return solvers.lanczos_two_pass_multi(op, b, k, fs)

    def singles(mode, funcs):
        op.set_device_ftk(mode)
        out = [solvers.lanczos_two_pass(op, b, k, f) for f in funcs]
        op.set_device_ftk(2)
        return out

    variants = {"multi": multi, "host": lambda: singles(0, fs), "default": lambda: singles(2, fs),
                "inv1g": lambda: singles(1, [ftk.INV] * m)}
    X = multi()  # warm-up of each, and the result check: column i == single solve i, bitwise
    ref = singles(0, fs)
    same = all(torch.equal(X[:, i].contiguous().view(torch.int64), ref[i].view(torch.int64))
               for i in range(m))
    variants["default"](), variants["inv1g"]()
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
        "arcs": arcs, "n": n, "k": k, "m": m, "reps": reps, "order_groups": op.order_groups(),
        "columns_bitwise_equal_single": same,
        **{f"{name}_ms": round(v, 4) for name, v in med.items()},
        **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
        "multi_over_host": round(med["multi"] / med["host"], 4),
        "multi_over_default": round(med["multi"] / med["default"], 4),
        "multi_over_inv1g": round(med["multi"] / med["inv1g"], 4)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--k", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--ms", type=int, nargs="+", default=[1, 2, 4, 8])
    p.add_argument("--step-timeout", type=float, default=150.0)
    p.add_argument("--worker", type=int, default=0, help="internal: time this m in-process")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.worker:
        worker(a.arcs, a.k, a.worker, a.reps, a.groups)
        return 0
    for m in a.ms:  # a fresh process per m, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--k", str(a.k),
               "--reps", str(a.reps), "--groups", str(a.groups), "--worker", str(m)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"m = {m}: time limit of {a.step_timeout:.0f} s reached; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"m = {m}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
