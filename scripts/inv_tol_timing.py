"""Dev tool: the inverse solve that stops at a residual tolerance, timed against the fixed-k
solve at the 500k-arc headline size (locality order pinned at 13 groups, kmax = 500, b and x
resident on the device).

The headline KKT block (D = 0) is singular, so no tolerance is ever met on it. The instance
here is that block made nonsingular: A = [[D, E^T], [E, 0]] + sigma I with D = diag(2, 3, 4,
2, ...) on the arc rows (tests/fused_cases.py with_d) and sigma = 1, b = A 1 / sqrt(n).

One process (under its own time limit) times, alternating, after one warm-up of each:
  tol_<t>    (i)   solvers.lanczos_two_pass_inv_tol(op, b, kmax, t) for each tolerance t;
  fixed_kmax (ii)  solvers.lanczos_two_pass(op, b, kmax, INV): what a caller pays without the stop;
  fixed_<m>  (iii) solvers.lanczos_two_pass(op, b, m*, INV) at the m* each tolerance reached:
                   the floor, a caller who guessed the step count exactly;
  tol_0            the tol call with tol = 0 (never met): the cost of watching the residual.
(ii) and (iii) are this tree's fixed-k solve: its kernels compile to the same instructions as
the parent commit's (make asm in both trees, scripts/kernel_asm_diff.py), its host side is this
tree's build, not the parent's library.
Prints one JSON line: m* and converged per tolerance, the medians and minima in ms, whether
each tol result is bitwise the fixed-m* solve, and the differences the issue asks about.

    python scripts/inv_tol_timing.py [--arcs 500000] [--kmax 500] [--reps 7] [--tols 1e-4 1e-8]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def worker(arcs, kmax, tols, reps, groups, sigma):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import tpl_amd
    from tpl_amd import ftk, solvers
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    import fused_cases as fc

    qfc = f"/tmp/inv_tol_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    kkt = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                          qfc)
    a = fc.with_d(kkt)
    n = a.shape[0]
    a = (a + sigma * sp.identity(n, format="csr")).tocsr()
    a.sort_indices()
    op = tpl_amd.HipCsrOp(a)
    if groups > 0:
        op.set_order_groups(groups)
    b = torch.from_numpy(a @ np.full(n, 1.0 / np.sqrt(n))).cuda()

    def bits_equal(x, y):
        return bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))

    variants, reached, same = {}, {}, {}
    for t in tols:
        x, info = solvers.lanczos_two_pass_inv_tol(op, b, kmax, t, return_info=True)  # warm-up
        flags = op.flags()
        m = info["steps"]
        reached[f"{t:g}"] = {"m": m, "converged": info["converged"],
                             "residual_at_m": float(info["residuals"][m - 1]) if m <= len(info["residuals"]) else None,
                             "one_graph": bool(flags & 32), "cached": bool(flags & 256),
                             "fused": bool(flags & 512)}
        variants[f"tol_{t:g}"] = lambda t=t: solvers.lanczos_two_pass_inv_tol(op, b, kmax, t)
        variants[f"fixed_{m}"] = lambda m=m: solvers.lanczos_two_pass(op, b, m, ftk.INV)
        same[f"{t:g}"] = bits_equal(x, variants[f"fixed_{m}"]())  # its warm-up too
    variants["fixed_kmax"] = lambda: solvers.lanczos_two_pass(op, b, kmax, ftk.INV)
    variants["tol_0"] = lambda: solvers.lanczos_two_pass_inv_tol(op, b, kmax, 0.0)
    same["0"] = bits_equal(variants["tol_0"](), variants["fixed_kmax"]())
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(v) for name, v in times.items()}
    out = {"arcs": arcs, "n": n, "sigma": sigma, "kmax": kmax, "reps": reps,
           "order_groups": op.order_groups(), "reached": reached, "tol_bitwise_equal_fixed_m": same,
           **{f"{name}_ms": round(v, 4) for name, v in med.items()},
           **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
           **{f"{name}_max_ms": round(max(times[name]), 4) for name in times},
           "tol_0_minus_fixed_kmax_ms": round(med["tol_0"] - med["fixed_kmax"], 4)}
    for t in tols:
        m = reached[f"{t:g}"]["m"]
        out[f"tol_{t:g}_minus_fixed_{m}_ms"] = round(med[f"tol_{t:g}"] - med[f"fixed_{m}"], 4)
        out[f"tol_{t:g}_over_fixed_kmax"] = round(med[f"tol_{t:g}"] / med["fixed_kmax"], 4)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--kmax", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--sigma", type=float, default=1.0)
    p.add_argument("--tols", type=float, nargs="+", default=[1e-4, 1e-8])
    p.add_argument("--step-timeout", type=float, default=240.0)
    p.add_argument("--worker", action="store_true", help="internal: time in-process")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.worker:
        worker(a.arcs, a.kmax, a.tols, a.reps, a.groups, a.sigma)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--kmax", str(a.kmax),
           "--reps", str(a.reps), "--groups", str(a.groups), "--sigma", str(a.sigma), "--worker",
           "--tols"] + [repr(t) for t in a.tols]
    try:  # a fresh process under its own limit
        rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"time limit of {a.step_timeout:.0f} s reached; stopping", flush=True)
        return 124
    if rc != 0:
        print(f"exit status {rc}; stopping", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
