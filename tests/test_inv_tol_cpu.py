"""CPU: the residual rule of the inverse solve that stops at a tolerance (include/tpl.h
tpl_ftk_inv_residuals, tpl_lanczos_two_pass_inv_tol) — what can be checked without a GPU: the
history against a restatement of its definition, the estimate against the true residual, the
argument errors that come before any device work, and the bindings' names.
"""
import math
import os
import re
import shutil
import subprocess
from ctypes import POINTER, byref, c_double, c_int32, c_size_t

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import tpl_amd
from tpl_amd import _lib, ftk, solvers

SYMBOLS = ("tpl_lanczos_two_pass_inv_tol", "tpl_ftk_inv_residuals")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def lanczos_tridiagonal(n, rng):
    """As tests/test_gpu_exp_times.py builds it, with beta_n kept: n alphas, n betas."""
    lam = np.linspace(-10.0, -0.1, 4 * n + 4)
    v = rng.random(lam.shape[0])
    v /= np.linalg.norm(v)
    vp = np.zeros_like(v)
    al, be, bprev = [], [], 0.0
    for _ in range(n):
        w = lam * v - bprev * vp
        a_ = v @ w
        w = w - a_ * v
        al.append(a_)
        bprev = np.linalg.norm(w)
        be.append(bprev)
        vp, v = v, w / bprev
    return np.array(al), np.array(be)


def kkt_like(n, rng):
    """Zero diagonal, positive off-diagonal (a pivot at every row), n betas."""
    return np.zeros(n), rng.uniform(0.5, 20.0, n)


def restated(alphas, betas):
    """The definition, in Python floats (IEEE double operations, one rounding each; a
    division by zero gives the IEEE inf / NaN)."""
    def div(a, b):
        if b != 0.0:
            return a / b
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)

    al, be = [float(v) for v in alphas], [float(v) for v in betas]
    L = min(len(al), len(be))
    if L == 0:
        return []
    d, du, b = al[0], be[0], 1.0
    res = [abs(be[0] * div(b, d))]
    for i in range(L - 1):
        dl, d1, du1 = be[i], al[i + 1], be[i + 1]
        if abs(d) >= abs(dl):
            fact = div(dl, d)
            nd = d1 - fact * du
            nb = 0.0 - fact * b
            ndu = du1
        else:
            fact = div(d, dl)
            nd = du - fact * d1
            ndu = -fact * du1
            nb = b - fact * 0.0
        d, du, b = nd, ndu, nb
        res.append(abs(du1 * div(b, d)))
    return res


def same_with_nan(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return (x.shape == y.shape and np.array_equal(nx, ny)
            and np.array_equal(bits(x[~nx]), bits(y[~ny])))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 500])
def test_history_is_the_restated_rule(n):
    rng = np.random.default_rng(7100 + n)
    for family, (al, be) in (("lanczos", lanczos_tridiagonal(n, rng)), ("kkt", kkt_like(n, rng))):
        for nb in (n, n - 1):  # a k-step pass one hands k - 1 betas
            res = ftk.inv_residuals(al, be[:nb])
            assert res.shape == (min(n, nb),), (family, nb)
            assert same_with_nan(res, restated(al, be[:nb])), (family, nb)
        if family == "lanczos":
            assert np.all(np.isfinite(res)) and (n < 3 or res[-1] < res[0])


def test_history_with_a_zero_first_alpha():
    """alphas[0] = 0: res[0] = |beta_0 (1 / 0)| = inf, and row 0 pivots."""
    rng = np.random.default_rng(7200)
    al, be = lanczos_tridiagonal(9, rng)
    al[0] = 0.0
    res = ftk.inv_residuals(al, be)
    assert np.isinf(res[0]) and not res[0] <= 1e300
    assert same_with_nan(res, restated(al, be))
    # a zero pivot later on (d_1 = 1 - 1 * 1): inf, never <= a finite tolerance
    res = ftk.inv_residuals(np.ones(2), np.ones(2))
    assert same_with_nan(res, restated(np.ones(2), np.ones(2)))
    assert res[0] == 1.0 and np.isinf(res[1]) and not res[1] <= 1e300


def test_capacity_and_null_are_reported():
    al, be = np.ones(4), np.ones(4)
    out, n = np.zeros(2), c_size_t(0)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    assert _lib.tpl_ftk_inv_residuals(pd(al), 4, pd(be), 4, pd(out), 2, byref(n)) != 0
    assert n.value == 4
    assert _lib.tpl_ftk_inv_residuals(pd(al), 4, pd(be), 3, None, 0, byref(n)) != 0 and n.value == 3
    assert _lib.tpl_ftk_inv_residuals(pd(al), 4, pd(be), 0, None, 0, byref(n)) == 0 and n.value == 0


def spd_lanczos(n, steps, seed):
    """numpy Lanczos on tridiag(-1, 2.5, -1): (A, b, V, alphas, betas), `steps` of each."""
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    b = np.random.default_rng(seed).standard_normal(n)
    V = np.zeros((n, steps + 1))
    V[:, 0] = b / np.linalg.norm(b)
    al, be = np.zeros(steps), np.zeros(steps)
    for j in range(steps):
        w = a @ V[:, j] - (be[j - 1] * V[:, j - 1] if j else 0.0)
        al[j] = V[:, j] @ w
        w = w - al[j] * V[:, j]
        be[j] = np.linalg.norm(w)
        V[:, j + 1] = w / be[j]
    return a, b, V, al, be


EST_BOUND = 5.6e-8   # 100 x the worst disagreement measured (below)


def test_estimate_follows_the_true_residual():
    """SPD tridiag(-1, 2.5, -1), n = 600, random b, 40 steps: for every m whose estimate is
    >= 1e-8 it agrees with numpy's true ||b - A x_m|| / ||b||, x_m = ||b|| V_m T_m^{-1} e_1.
    Measured here: worst relative disagreement 5.6e-10 (at m = 26, estimate 1.9e-8; 2.3e-11 at
    1e-6, 1e-15 at 1e-2 — it grows as the residual falls, being the rounding of x_m against a
    shrinking residual); the bound is 100 x the worst. The tolerances 1e-2 and 1e-6 are first met at m = 8 and 21."""
    a, b, V, al, be = spd_lanczos(600, 40, 11)
    est = ftk.inv_residuals(al, be)
    bn = np.linalg.norm(b)
    worst, checked = 0.0, 0
    for m in range(1, 41):
        if est[m - 1] < 1e-8:
            continue
        t = np.diag(al[:m]) + np.diag(be[:m - 1], 1) + np.diag(be[:m - 1], -1)
        xm = bn * (V[:, :m] @ np.linalg.solve(t, np.eye(m)[:, 0]))
        true = np.linalg.norm(b - a @ xm) / bn
        rel = abs(est[m - 1] - true) / true
        print(f"m={m:2d} est={est[m - 1]:.6e} true={true:.6e} rel={rel:.2e}")
        worst = max(worst, rel)
        checked += 1
    print(f"worst {worst:.3e} over {checked} steps")
    assert checked >= 20
    assert worst <= EST_BOUND, worst
    first = lambda tol: 1 + int(np.flatnonzero(est <= tol)[0])
    assert (first(1e-2), first(1e-6)) == (8, 21)


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in SYMBOLS:
        assert re.search(rf"\b(tpl_status|int)\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert tpl_amd.lanczos_two_pass_inv_tol is solvers.lanczos_two_pass_inv_tol
    assert "lanczos_two_pass_inv_tol" in tpl_amd.__all__


def test_argument_errors_in_the_documented_order():
    """On a host-only plan: NULL x_out, then a NaN or negative tol, are argument errors of
    their own; a valid tol (0, +inf) reaches the host-only refusal."""
    n = 12
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    plan = tpl_amd.HostPlan(a)
    b, x = np.ones(n), np.zeros(n)
    st, cv, rl = c_size_t(0), c_int32(0), c_size_t(0)
    res = np.zeros(5)

    def call(tol, xp=None, full=True):
        out = (byref(st), byref(cv), res.ctypes.data_as(POINTER(c_double)), byref(rl))
        return _lib.tpl_lanczos_two_pass_inv_tol(plan.handle, b.ctypes.data, n, 5, tol,
                                                 x.ctypes.data if xp is None else xp,
                                                 _lib.TPL_MEM_HOST,
                                                 *(out if full else (None, None, None, None)))

    for tol in (float("nan"), -1.0, -0.0 - 1e-300, float("-inf")):
        assert call(tol) == _lib.TPL_ERR_INVALID_ARGUMENT
        assert "tol" in _lib.last_error() and "host-only" not in _lib.last_error()
    assert call(float("nan"), xp=0) == _lib.TPL_ERR_INVALID_ARGUMENT
    assert "NULL" in _lib.last_error()
    for tol in (0.0, 1e-8, float("inf")):
        for full in (True, False):
            assert call(tol, full=full) == _lib.TPL_ERR_INVALID_ARGUMENT
            assert "host-only plan" in _lib.last_error()
    plan.close()


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_solver(tmp_path):
    tu = tmp_path / "inv_tol.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "std::vector<double> (*f1)(const tpl::HipCsrOp&, const std::vector<double>&, size_t, double,\n"
                  "               tpl::solvers::InvTolInfo*) = &tpl::solvers::lanczos_two_pass_inv_tol;\n"
                  "std::vector<double> (*f2)(const std::vector<double>&, const std::vector<double>&) =\n"
                  "    &tpl::ftk::inv_residuals;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def build_native(tmp_path):
    """tests/native/inv_tol_test.cpp against the built library. -> the program's path."""
    exe = str(tmp_path / "inv_tol_test")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "inv_tol_test.cpp"),
                    "-L", libdir, "-ltpl_amd", "-Wl,-rpath," + libdir], check=True)
    return exe


def test_cpp_api_history(tmp_path):
    p = subprocess.run([build_native(tmp_path), "--cpu"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "OK (0 failures)" in p.stdout, p.stdout + p.stderr


def test_rust_shim_names_the_solver():
    src = open(os.path.join(ROOT, "integration", "rust", "hip.rs")).read()
    assert "pub fn lanczos_two_pass_inv_tol<" in src
    for s in SYMBOLS:
        assert re.search(rf"\bfn {s}\(", src), s
