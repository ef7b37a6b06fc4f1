"""Dev tool: (A + sigma_i I)^-1 b for m shifts, each stopped at a residual tolerance, timed at
the 500k-arc headline size on scripts/inv_tol_timing.py's instance and protocol (locality
order pinned at 13 groups, kmax = 500, b and x resident on the device, alternated runs after
one warm-up each, medians and minima).

A0 = [[D, E^T], [E, 0]] with D = diag(2, 3, 4, 2, ...) on the arc rows (tests/fused_cases.py
with_d); the shifts start at sigma_0 = 1 and are spread over two decades (geometrically, up
to 100); b = (A0 + I) 1 / sqrt(n). For each m in --ms and each tolerance, one process (under
its own time limit) times:
  dev_m<m>_tol<t>    solvers.lanczos_two_pass_shifted_inv_tol(op, b, kmax, sigmas, t) as one graph
                     (set_device_ftk(1): auto mode takes the graph up to kmax = 64 only, a line
                     drawn from this script's output);
  host_m<m>_tol<t>   (ii)  the same call on an operator under set_device_ftk(0): composed on the host;
  calls_m<m>_tol<t>  (i)   m calls of solvers.lanczos_two_pass_inv_tol on m operators built
                           explicitly as A0 + sigma_i I: the parent tree's way to the same answer
                           (to rounding: Lanczos on A0 + sigma I rounds alpha differently);
  multi_m<m>         (iii) solvers.lanczos_two_pass_multi with m ftk.inv_shift closures at k = kmax;
  inv_tol_tol<t>           solvers.lanczos_two_pass_inv_tol on A0 + I: against dev_m1, the cost of
                           the m-lane elimination workgroup over the one-lane one.
Prints one JSON line: the m*_i reached, whether every column is bitwise the fixed-m*_i solve
(solvers.lanczos_two_pass with ftk.inv_shift(sigma_i) on the mode-0 operator) and the
mode-0 call's, medians and minima in ms, and the ratios the routing decision reads (dev / host).

    python scripts/shifted_inv_tol_timing.py [--arcs 500000] [--kmax 500] [--reps 7]
        [--ms 1 4 8] [--tols 1e-4 1e-8]
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


def worker(arcs, kmax, ms, tols, reps, groups):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import tpl_amd
    from tpl_amd import ftk, solvers
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    import fused_cases as fc

    qfc = f"/tmp/shifted_inv_tol_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    kkt = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                          qfc)
    a0 = fc.with_d(kkt).tocsr()
    a0.sort_indices()
    n = a0.shape[0]

    def make_op(a, mode=None):
        op = tpl_amd.HipCsrOp(a)
        if groups > 0:
            op.set_order_groups(groups)
        if mode is not None:
            op.set_device_ftk(mode)
        return op

    def shifted(sigma):
        a = (a0 + sigma * sp.identity(n, format="csr")).tocsr()
        a.sort_indices()
        return a

    sig_all = sorted({float(s) for m in ms for s in np.geomspace(1.0, 100.0, m)} | {1.0})
    dev, host = make_op(a0, 1), make_op(a0, 0)  # mode 1: the graph at any kmax <= 1365
    explicit = {s: make_op(shifted(s)) for s in sig_all}
    b = torch.from_numpy(shifted(1.0) @ np.full(n, 1.0 / np.sqrt(n))).cuda()

    def bits_equal(x, y):
        return bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))

    variants, reached, same = {}, {}, {}
    for m in ms:
        sig = [float(s) for s in np.geomspace(1.0, 100.0, m)]
        for t in tols:
            key = f"m{m}_tol{t:g}"
            x, info = solvers.lanczos_two_pass_shifted_inv_tol(dev, b, kmax, sig, t,
                                                               return_info=True)  # warm-up
            flags = dev.flags()
            xh, ih = solvers.lanczos_two_pass_shifted_inv_tol(host, b, kmax, sig, t,
                                                              return_info=True)
            steps = [int(s) for s in info["steps"]]
            fixed = [bits_equal(x[:, i], solvers.lanczos_two_pass(host, b, steps[i],
                                                                  ftk.inv_shift(sig[i])))
                     for i in range(m)]
            reached[key] = {"sigmas": [round(s, 4) for s in sig], "steps": steps,
                            "converged": [bool(c) for c in info["converged"]],
                            "host_steps": [int(s) for s in ih["steps"]],
                            "explicit_steps": [], "one_graph": bool(flags & 32),
                            "cached": bool(flags & 256), "fused": bool(flags & 512)}
            for s in sig:  # warm-up of the explicit operators, and where they stop
                _, ie = solvers.lanczos_two_pass_inv_tol(explicit[s], b, kmax, t, return_info=True)
                reached[key]["explicit_steps"].append(int(ie["steps"]))
            same[key] = {"every_column_is_the_fixed_m_solve": all(fixed),
                         "device_is_host_path": bits_equal(x, xh)}
            variants[f"dev_{key}"] = lambda sig=sig, t=t: solvers.lanczos_two_pass_shifted_inv_tol(
                dev, b, kmax, sig, t)
            variants[f"host_{key}"] = lambda sig=sig, t=t: solvers.lanczos_two_pass_shifted_inv_tol(
                host, b, kmax, sig, t)
            variants[f"calls_{key}"] = lambda sig=sig, t=t: [
                solvers.lanczos_two_pass_inv_tol(explicit[s], b, kmax, t) for s in sig]
        fs = [ftk.inv_shift(s) for s in sig]
        variants[f"multi_m{m}"] = lambda fs=fs: solvers.lanczos_two_pass_multi(host, b, kmax, fs)
        variants[f"multi_m{m}"]()
    for t in tols:
        variants[f"inv_tol_tol{t:g}"] = lambda t=t: solvers.lanczos_two_pass_inv_tol(
            explicit[1.0], b, kmax, t)
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(v) for name, v in times.items()}
    out = {"arcs": arcs, "n": n, "kmax": kmax, "reps": reps, "order_groups": dev.order_groups(),
           "reached": reached, "bitwise": same,
           **{f"{name}_ms": round(v, 4) for name, v in med.items()},
           **{f"{name}_min_ms": round(min(times[name]), 4) for name in times}}
    for m in ms:
        for t in tols:
            key = f"m{m}_tol{t:g}"
            out[f"dev_over_host_{key}"] = round(med[f"dev_{key}"] / med[f"host_{key}"], 4)
            out[f"dev_over_calls_{key}"] = round(med[f"dev_{key}"] / med[f"calls_{key}"], 4)
            out[f"dev_over_multi_{key}"] = round(med[f"dev_{key}"] / med[f"multi_m{m}"], 4)
    if 1 in ms:
        for t in tols:
            out[f"dev_m1_minus_inv_tol_tol{t:g}_ms"] = round(
                med[f"dev_m1_tol{t:g}"] - med[f"inv_tol_tol{t:g}"], 4)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--kmax", type=int, default=500)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--ms", type=int, nargs="+", default=[1, 4, 8])
    p.add_argument("--tols", type=float, nargs="+", default=[1e-4, 1e-8])
    p.add_argument("--step-timeout", type=float, default=420.0)
    p.add_argument("--worker", action="store_true", help="internal: time in-process")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    if a.worker:
        worker(a.arcs, a.kmax, a.ms, a.tols, a.reps, a.groups)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--kmax", str(a.kmax),
           "--reps", str(a.reps), "--groups", str(a.groups), "--worker", "--ms"] + \
          [str(m) for m in a.ms] + ["--tols"] + [repr(t) for t in a.tols]
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
