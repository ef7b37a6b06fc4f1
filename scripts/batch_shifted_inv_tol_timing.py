"""Dev tool: (A + sigma_i I)^-1 b_c for s right-hand sides and m shifts, every (column, shift)
stopped at a residual tolerance, timed at the 500k-arc headline size on
scripts/shifted_inv_tol_timing.py's instance and protocol (locality order pinned at 13 groups,
B and X resident on the device, alternated runs after one warm-up each, medians, minima and
maxima).

A0 = [[D, E^T], [E, 0]] with D = diag(2, 3, 4, 2, ...) on the arc rows (tests/fused_cases.py
with_d); the shifts start at sigma_0 = 1 and are spread over two decades (geometrically, up to
100); column c of B is (A0 + I) v_c with v_0 = 1 / sqrt(n) and v_c, c > 0, seeded normal
vectors. For each kmax in --kmaxs one process (under its own time limit) times, for each (s, m)
in --shapes and each tolerance:
  dev_<key>     solvers.lanczos_two_pass_batch_shifted_inv_tol as one graph per group
                (set_device_ftk(1): the graph at any kmax <= 1365);
  host_<key>    the same call on an operator under set_device_ftk(0): composed on the host;
  singles_<key> s calls of solvers.lanczos_two_pass_shifted_inv_tol on an operator in auto
                mode (its own routing): the parent tree's first way to the same bits;
  bmulti_<shape>  solvers.lanczos_two_pass_batch_multi with m ftk.inv_shift closures at
                k = kmax: the parent tree's second way (no stop).
Prints one JSON line per kmax: the M_c reached, whether the device path gives the host path's
bits and every column its single call's, medians / minima / maxima in ms, the ratios
(dev / host, either path over singles and over bmulti), and what the routing decision reads:
per shape the graph's median minus the host path's and the repetitions' noise (the larger
interquartile range of the two), and whether the graph is within that noise of the host path,
or faster, at every shape of this kmax (graph_no_slower_at_every_shape).

    python scripts/batch_shifted_inv_tol_timing.py [--arcs 500000] [--kmaxs 64 125 250 500]
        [--reps 7] [--shapes 2x1 4x1 4x4 4x8] [--tols 1e-4 1e-8]
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


def worker(arcs, kmax, shapes, tols, reps, groups):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import tpl_amd
    from tpl_amd import ftk, solvers
    from tpl_amd.utils.data_loader import load_kkt_system, write_qfc_3line

    import fused_cases as fc

    qfc = f"/tmp/batch_shifted_inv_tol_{arcs}.qfc"
    write_qfc_3line(qfc, arcs)
    kkt = load_kkt_system(os.path.join(ROOT, "tests", "golden", "kkt", f"netgen-{arcs}-3.dmx.xz"),
                          qfc)
    a0 = fc.with_d(kkt).tocsr()
    a0.sort_indices()
    n = a0.shape[0]

    def make_op(mode):
        op = tpl_amd.HipCsrOp(a0)
        if groups > 0:
            op.set_order_groups(groups)
        op.set_device_ftk(mode)
        return op

    dev, host, auto = make_op(1), make_op(0), make_op(2)
    a1 = (a0 + sp.identity(n, format="csr")).tocsr()
    smax = max(s for s, _ in shapes)
    rng = np.random.default_rng(17)
    vs = [np.full(n, 1.0 / np.sqrt(n))] + [v / np.linalg.norm(v)
                                           for v in rng.standard_normal((smax - 1, n))]
    Ball = torch.from_numpy(np.stack([a1 @ v for v in vs], axis=1)).cuda()  # n x smax
    cols = [Ball[:, c].contiguous() for c in range(smax)]

    def bits_equal(x, y):
        return bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))

    batch, single = solvers.lanczos_two_pass_batch_shifted_inv_tol, solvers.lanczos_two_pass_shifted_inv_tol
    variants, reached, same = {}, {}, {}
    for s, m in shapes:
        B = Ball[:, :s]
        sig = [float(v) for v in np.geomspace(1.0, 100.0, m)]
        for t in tols:
            key = f"s{s}_m{m}_tol{t:g}"
            x, info = batch(dev, B, kmax, sig, t, return_info=True)  # warm-up
            flags = dev.flags()
            xh, ih = batch(host, B, kmax, sig, t, return_info=True)
            xs = [single(auto, cols[c], kmax, sig, t) for c in range(s)]
            reached[key] = {"big_m": [int(v) for v in info["steps"].max(axis=0)],
                            "converged": bool(info["converged"].all()),
                            "one_graph": bool(flags & 32), "cached": bool(flags & 256),
                            "singles_one_graph": bool(auto.flags() & 32)}
            same[key] = {"device_is_host_path": bits_equal(x, xh)
                         and bool(np.array_equal(info["steps"], ih["steps"])),
                         "every_column_is_its_single_call": all(
                             bits_equal(x[:, :, c], xs[c]) for c in range(s))}
            variants[f"dev_{key}"] = lambda B=B, sig=sig, t=t: batch(dev, B, kmax, sig, t)
            variants[f"host_{key}"] = lambda B=B, sig=sig, t=t: batch(host, B, kmax, sig, t)
            variants[f"singles_{key}"] = lambda sig=sig, t=t, s=s: [
                single(auto, cols[c], kmax, sig, t) for c in range(s)]
        fs = [ftk.inv_shift(v) for v in sig]
        variants[f"bmulti_s{s}_m{m}"] = lambda B=B, fs=fs: solvers.lanczos_two_pass_batch_multi(
            host, B, kmax, fs)
        variants[f"bmulti_s{s}_m{m}"]()
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
           **{f"{name}_min_ms": round(min(times[name]), 4) for name in times},
           **{f"{name}_max_ms": round(max(times[name]), 4) for name in times}}
    def iqr(v):
        q = statistics.quantiles(v, n=4)
        return q[2] - q[0]

    verdicts = []
    for s, m in shapes:
        for t in tols:
            key = f"s{s}_m{m}_tol{t:g}"
            out[f"dev_over_host_{key}"] = round(med[f"dev_{key}"] / med[f"host_{key}"], 4)
            # the routing rule: the graph counts as no slower where its median is within the
            # repetitions' noise (the larger interquartile range of the two) of the host path's
            diff = med[f"dev_{key}"] - med[f"host_{key}"]
            noise = max(iqr(times[f"dev_{key}"]), iqr(times[f"host_{key}"]))
            out[f"dev_minus_host_ms_{key}"] = round(diff, 4)
            out[f"noise_ms_{key}"] = round(noise, 4)
            verdicts.append(diff <= noise)
            for path in ("dev", "host"):
                out[f"{path}_over_singles_{key}"] = round(
                    med[f"{path}_{key}"] / med[f"singles_{key}"], 4)
                out[f"{path}_over_bmulti_{key}"] = round(
                    med[f"{path}_{key}"] / med[f"bmulti_s{s}_m{m}"], 4)
    out["graph_no_slower_at_every_shape"] = all(verdicts)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arcs", type=int, default=500000)
    p.add_argument("--kmaxs", type=int, nargs="+", default=[64, 125, 250, 500])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--groups", type=int, default=13)
    p.add_argument("--shapes", nargs="+", default=["2x1", "4x1", "4x4", "4x8"])
    p.add_argument("--tols", type=float, nargs="+", default=[1e-4, 1e-8])
    p.add_argument("--step-timeout", type=float, default=240.0)
    p.add_argument("--worker", type=int, default=0, help="internal: time this kmax in-process")
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps must be at least 5")
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in a.shapes]
    if a.worker:
        worker(a.arcs, a.worker, shapes, a.tols, a.reps, a.groups)
        return 0
    for kmax in a.kmaxs:  # a fresh process per kmax, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--arcs", str(a.arcs), "--reps",
               str(a.reps), "--groups", str(a.groups), "--worker", str(kmax), "--shapes"] + \
              a.shapes + ["--tols"] + [repr(t) for t in a.tols]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"time limit of {a.step_timeout:.0f} s reached at kmax {kmax}; stopping",
                  flush=True)
            return 124
        if rc != 0:
            print(f"exit status {rc} at kmax {kmax}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
