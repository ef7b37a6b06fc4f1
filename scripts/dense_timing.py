"""Dev tool: the dense operator against the same matrix pushed through the CSR layout.

The reference's dense study matrix (src/bin/dense_tradeoff.rs: A = R + R^T, R ~ U[0, 1) from
StdRng(42), b = A 1 / sqrt(n)) at n = 4096 (128 MiB of matrix: inside the 256 MiB Infinity
Cache) and n = 10000 (763 MiB: outside it). Two kinds of leg, each a fresh process under its
own time limit, alternated --reps times on one box:
  dense  tpl_amd.HipDenseOp with this tree's library;
  csr    tpl_amd.HipCsrOp of the full matrix (every entry stored) with the library given by
         --csr-lib, imported through the Python mirror in --csr-pkg (the parent commit's
         build and package directory; default: this tree's, which runs the same CSR kernels) — its create runs under --create-limit seconds, and a size at which it runs
         past that, or fails, is recorded as such and compared no further.
Per leg and size: create time and device_bytes; the per-launch time of the three SpMV-shaped
kernels from graph replays divided by steps — pass one of k = 200 steps over k (k_dense_p1 +
k_p1_axpy, resp. k_p1_spmv + k_p1_axpy), pass two over k - 1 (k_dense_p2 resp. k_p2_spmv), and
the plain product as the mean of 50 tpl_op_apply calls on device vectors (kernel + one vector
copy each way + a synchronisation); each as n ld 8 bytes per second for the dense legs (ld:
the padded leading dimension) against the 8 TB/s specification and the ~6.3 TB/s a streaming
kernel achieves; and whole two-pass and one-pass solves (built-in inv, b and x on the device)
at k = 100 and k = 500, median of 5 after one warm-up.

    python scripts/dense_timing.py [--sizes 4096 10000] [--reps 3] [--csr-lib PATH --csr-pkg DIR]
                                   [--output profiles/dense_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a csr leg under another build imports that build's own Python mirror (--csr-pkg)
sys.path.insert(0, os.environ.get("TPL_DENSE_TIMING_PKG") or os.path.join(ROOT, "two-pass-lanczos_amd"))
P1_K = 200
SOLVE_KS = (100, 500)


def matrix_file(n):
    """R + R^T of the reference's study, made once per box and size."""
    import numpy as np
    path = os.path.join(tempfile.gettempdir(), f"tpl_dense_timing_{n}.npy")
    if not os.path.exists(path):
        from tpl_amd.utils.rng import std_rng_f64
        r = std_rng_f64(n * n, 42).reshape(n, n)
        np.save(path + ".tmp.npy", r + r.T)
        os.replace(path + ".tmp.npy", path)
    return path


def worker(kind, n):
    import numpy as np
    import torch
    import tpl_amd
    from tpl_amd import algorithms as alg, ftk, solvers

    a = np.load(matrix_file(n))
    b = torch.from_numpy(a @ np.full(n, 1.0 / np.sqrt(n))).cuda()
    out = {"kind": kind, "n": n, "lib": os.path.basename(tpl_amd.LIB_PATH)}
    t0 = time.perf_counter()
    if kind == "dense":
        op = tpl_amd.HipDenseOp(a)
        ld = 16 * (((n + 15) // 16) | 1)
        out["matrix_bytes"] = n * ld * 8
    else:
        rp = np.arange(0, n * n + 1, n, dtype=np.int64)
        ci = np.tile(np.arange(n, dtype=np.int32), n)
        op = tpl_amd.HipCsrOp((n, rp, ci, a.reshape(-1)))
        del rp, ci
    out["create_s"] = time.perf_counter() - t0
    out["device_bytes"] = op.device_bytes()
    print(json.dumps({"created": out}), flush=True)

    def timed(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return ts

    d = alg.lanczos_pass_one(op, b, P1_K)
    y = d.b_norm * ftk.INV(d.alphas, d.betas)
    out["p1_step_us"] = 1e6 * statistics.median(timed(lambda: alg.lanczos_pass_one(op, b, P1_K), 5)) / P1_K
    out["p2_step_us"] = 1e6 * statistics.median(
        timed(lambda: alg.lanczos_pass_two(op, b, d, y), 5)) / (d.steps_taken - 1)
    out["apply_us"] = 1e6 * statistics.mean(timed(lambda: op.apply(b), 50))
    out["device_bytes_after"] = op.device_bytes()
    for k in SOLVE_KS:
        out[f"two_pass_k{k}_ms"] = 1e3 * statistics.median(
            timed(lambda: solvers.lanczos_two_pass(op, b, k, ftk.INV), 5))
        out[f"one_pass_k{k}_ms"] = 1e3 * statistics.median(
            timed(lambda: solvers.lanczos(op, b, k, ftk.INV), 5))
    print(json.dumps({"result": out}), flush=True)


def run_leg(kind, n, lib, pkg, limit):
    env = dict(os.environ)
    if lib:
        env["TPL_LIB_PATH"] = os.path.abspath(lib)
    if pkg:
        env["TPL_DENSE_TIMING_PKG"] = os.path.abspath(pkg)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--n", str(n)]
    t0 = time.perf_counter()
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    created = result = None
    try:
        line = None
        # the create under its own limit: the first line the worker prints
        import select
        if select.select([p.stdout], [], [], limit)[0]:
            line = p.stdout.readline()
        if not line:
            p.kill()
            return {"kind": kind, "n": n, "refused": f"create not done within {limit} s"}
        created = json.loads(line).get("created")
        rest, _ = p.communicate(timeout=300)
        for ln in rest.splitlines():
            if ln.startswith('{"result"'):
                result = json.loads(ln)["result"]
    except (subprocess.TimeoutExpired, ValueError) as e:
        p.kill()
        return {"kind": kind, "n": n, "refused": repr(e), "created": created}
    if p.returncode != 0 or result is None:
        return {"kind": kind, "n": n, "refused": f"exit status {p.returncode}", "created": created}
    result["leg_s"] = time.perf_counter() - t0
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 10000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--csr-lib", default="")
    ap.add_argument("--csr-pkg", default="")
    ap.add_argument("--create-limit", type=float, default=60.0)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "dense_timing.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.n)
    lines = ["dense_timing: HipDenseOp (this tree) against HipCsrOp of the full matrix "
             f"({'the library ' + os.path.basename(a.csr_lib) if a.csr_lib else 'this tree'}),"
             f" alternated {a.reps} times on one box; times: p1 / p2 per step of a "
             f"{P1_K}-step pass, apply per call, solves median of 5"]
    for n in a.sizes:
        matrix_file(n)
        csr_ok = True
        for rep in range(a.reps):
            for kind in ("csr", "dense"):
                if kind == "csr" and not csr_ok:
                    continue
                # the matrix load and CSR arrays precede the create in the worker: allow for them
                r = run_leg(kind, n, a.csr_lib if kind == "csr" else "",
                            a.csr_pkg if kind == "csr" else "", a.create_limit + (60 if kind == "csr" else 30))
                if kind == "csr" and "refused" in r:
                    csr_ok = False
                if kind == "dense" and "matrix_bytes" in r:
                    for key in ("p1_step_us", "p2_step_us", "apply_us"):
                        r[key.replace("_us", "_TBps")] = round(r["matrix_bytes"] / r[key] / 1e6, 3)
                lines.append(json.dumps({"rep": rep, **r}))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
