"""Dev tool: exp(t_i A) b at m times — the new call against the multi-function solve with
exp_t closures, at the 500k-arc headline (locality order pinned at 13 groups, k = 500, b and
X resident on the device).

For m in {1, 2, 4, 8} and t_i = 0.25 (i + 1), one process per m (each under its own time
limit) times, alternating, after one warm-up of each:
  closures  (a) solvers.lanczos_two_pass_multi with ftk.exp_t(t_i): every exp(t_i T_k) e_1 a
            host QL sweep behind a Python closure (the path this work leaves unchanged);
  host      (b) solvers.lanczos_two_pass_exp_times under set_device_ftk(0): the native host
            built-in tpl_ftk_exp_t, no Python between the passes;
  device    (c) the same call in the default mode: k_ftk_exp_times, one workgroup per time.
Prints per m one JSON line: the medians in ms, on_device of (c), the ratios, and the largest
relative column difference of (c) against (b) (the device exp's tolerance class, not bits).

    python scripts/exp_times_timing.py [--arcs 500000] [--k 500] [--reps 7] [--ms 1 2 4 8]
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

    qfc = f"/tmp/exp_times_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    a = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                        qfc).a
    n = a.shape[0]
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    b = torch.from_numpy(a @ np.full(n, 1.0 / np.sqrt(n))).cuda()
    ts = [0.25 * (i + 1) for i in range(m)]
    fs = [ftk.exp_t(t) for t in ts]
    on_seen = []

    def closures():
        return solvers.lanczos_two_pass_multi(op, b, k, fs)

    def host():
        op.set_device_ftk(0)
        try:
            return solvers.lanczos_two_pass_exp_times(op, b, k, ts)
        finally:
            op.set_device_ftk(2)

    def device():
        x, on = solvers.lanczos_two_pass_exp_times(op, b, k, ts, return_on_device=True)
        on_seen.append([int(v) for v in on])
        return x

    variants = {"closures": closures, "host": host, "device": device}
    Xa, Xb, Xc = closures(), host(), device()  # the warm-up of each, and the result checks
    same_ab = bool(torch.equal(Xa.contiguous().view(torch.int64), Xb.contiguous().view(torch.int64)))
    rel = max(float(torch.linalg.norm(Xc[:, i] - Xb[:, i]) / torch.linalg.norm(Xb[:, i]))
              for i in range(m))
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
        "ts": ts, "on_device": on_seen[-1],
        "on_device_same_every_run": all(o == on_seen[0] for o in on_seen),
        "host_bitwise_equal_closures": same_ab, "device_vs_host_max_rel": rel,
        **{f"{name}_ms": round(v, 4) for name, v in med.items()},
        **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
        "device_over_closures": round(med["device"] / med["closures"], 4),
        "device_over_host": round(med["device"] / med["host"], 4),
        "host_over_closures": round(med["host"] / med["closures"], 4)}), flush=True)


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
