"""CPU: the batch shifted inverse solve that stops every (column, shift) at a tolerance
(include/tpl.h tpl_lanczos_two_pass_batch_shifted_inv_tol, tpl_lanczos_pass_two_batch_multi_cut,
tpl_batch_shifted_inv_tol_auto_k) — what can be checked without a GPU: the argument errors that
come before any device work, in their documented order, and the bindings' names and types.
"""
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_double, c_int32, c_size_t

import numpy as np
import scipy.sparse as sp

from conftest import ROOT

import tpl_amd
from tpl_amd import _lib, algorithms, solvers

SOLVERS = ("tpl_lanczos_two_pass_batch_shifted_inv_tol", "tpl_lanczos_pass_two_batch_multi_cut")
SYMBOLS = SOLVERS + ("tpl_batch_shifted_inv_tol_auto_k",)


def _plan(n=12):
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    return tpl_amd.HostPlan(a)


def test_argument_errors_in_the_documented_order():
    """On a host-only plan: NULL op / B / sigmas / x_out, then s, then m, then tol, then a
    non-finite shift, each an argument error of its own and ahead of everything later that is
    also wrong with the call; a valid call reaches the host-only refusal."""
    n, kmax = 12, 5
    plan = _plan(n)
    B, x = np.ones(n * 65), np.zeros(n * 64 * 8)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))

    def call(sig, s=2, m=None, tol=1e-6, op=True, bp=True, xp=True, sp_=True, full=True):
        sig = np.ascontiguousarray(sig, dtype=np.float64)
        m = sig.shape[0] if m is None else m
        st, rl = (c_size_t * 512)(), (c_size_t * 512)()
        cv, res = (c_int32 * 512)(), np.zeros(kmax * 512)
        out = (st, cv, pd(res), rl) if full else (None, None, None, None)
        rc = _lib.tpl_lanczos_two_pass_batch_shifted_inv_tol(
            plan.handle if op else None, B.ctypes.data if bp else None, n, s, kmax,
            pd(sig) if sp_ else None, m, tol, x.ctypes.data if xp else None, _lib.TPL_MEM_HOST,
            *out)
        return rc, _lib.last_error()

    nan, inf = float("nan"), float("inf")
    # 1. NULL, ahead of everything else that is wrong with the call
    for kw in ({"op": False}, {"bp": False}, {"sp_": False}, {"xp": False}):
        rc, msg = call([nan], s=0, m=0, tol=nan, **kw)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in msg, (kw, msg)
    # 2. s, ahead of m, tol and the shifts
    for s in (0, 65):
        rc, msg = call(np.full(65, nan), s=s, m=65, tol=nan)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_BATCH_MAX" in msg, (s, msg)
    # 3. m, ahead of tol and the shifts
    for m in (0, 65):
        rc, msg = call(np.full(65, nan), m=m, tol=nan)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_MULTI_MAX" in msg, (m, msg)
    # 4. tol, ahead of the shifts
    for tol in (nan, -1.0, -1e-300, -inf):
        rc, msg = call([1.0, nan], tol=tol)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "tol" in msg, (tol, msg)
    # 5. a non-finite shift, anywhere in the list
    for sig in ([nan], [0.0, inf], [1.0, 2.0, -inf], list(np.arange(63.0)) + [nan]):
        rc, msg = call(sig)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "sigma" in msg, (sig, msg)
        assert "host-only" not in msg
    # a valid call (tol = 0 and +inf included, every output optional) reaches the refusal
    for tol in (0.0, 1e-8, inf):
        for full in (True, False):
            for s, sig in ((1, [0.0]), (2, [0.0, 0.25, -2.0]), (4, [1.0]), (7, np.arange(64.0))):
                rc, msg = call(sig, s=s, tol=tol, full=full)
                assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "host-only plan" in msg, msg
    plan.close()


def test_pass_two_batch_multi_cut_checks_its_arguments():
    n, s, m, ld = 12, 3, 2, 4
    plan = _plan(n)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    B, x = np.ones(n * s), np.zeros(n * s * m)
    al, be, y, bn = np.ones(ld * s), np.ones(ld * s), np.ones(ld * s * m), np.ones(s)
    steps = (c_size_t * s)(4, 3, 2)

    def cut(cs=(4, 1, 3, 2, 2, 1), s_=s, m_=m, xp=True, csp=True):
        return _lib.tpl_lanczos_pass_two_batch_multi_cut(
            plan.handle, B.ctypes.data, n, s_, pd(al), pd(be), ld, steps, pd(bn), pd(y),
            (c_size_t * len(cs))(*cs) if csp else None, m_, x.ctypes.data if xp else None,
            _lib.TPL_MEM_HOST)

    assert cut(xp=False) == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in _lib.last_error()
    assert cut(csp=False) == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in _lib.last_error()
    for s_ in (0, 65):
        assert cut(s_=s_) == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_BATCH_MAX" in _lib.last_error()
    for m_ in (0, 65):
        assert cut(m_=m_) == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_MULTI_MAX" in _lib.last_error()
    # a count of 0 and of steps[c] + 1, in the first, a middle and the last (remainder) column
    for bad in ((0, 1, 3, 2, 2, 1), (5, 1, 3, 2, 2, 1), (4, 1, 3, 4, 2, 1), (4, 1, 3, 0, 2, 1),
                (4, 1, 3, 2, 2, 3), (4, 1, 3, 2, 0, 1)):
        assert cut(cs=bad) == _lib.TPL_ERR_INVALID_ARGUMENT, bad
        assert "col_steps" in _lib.last_error() and "host-only" not in _lib.last_error(), bad
    assert cut() == _lib.TPL_ERR_INVALID_ARGUMENT and "host-only plan" in _lib.last_error()
    plan.close()


def test_symbols_declared_exported_and_named_in_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in SYMBOLS:
        ret = "tpl_status" if s in SOLVERS else "size_t"
        assert re.search(rf"\b{ret}\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert 1 <= _lib.tpl_batch_shifted_inv_tol_auto_k() <= 1365
    assert (tpl_amd.lanczos_two_pass_batch_shifted_inv_tol
            is solvers.lanczos_two_pass_batch_shifted_inv_tol)
    assert "lanczos_two_pass_batch_shifted_inv_tol" in tpl_amd.__all__
    assert callable(algorithms.lanczos_pass_two_batch_multi_cut)


def test_new_kernels_are_in_the_library():
    """The hot path is native: the three kernels of tpl_k_batch_stol.hip are in the code object."""
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_bp1_axpy_stol", b"k_bp1_stol_fin", b"k_bp2_xacc_cut"):
        assert k in blob, k


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_solver(tmp_path):
    tu = tmp_path / "batch_shifted_inv_tol.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "tpl::Mat (*f1)(const tpl::HipCsrOp&, const tpl::Mat&, size_t,\n"
                  "               const std::vector<double>&, double, tpl::solvers::ShiftedInvTolInfo*) =\n"
                  "    &tpl::solvers::lanczos_two_pass_batch_shifted_inv_tol;\n"
                  "tpl_status (*f2)(tpl_op_t, const double*, int64_t, size_t, size_t, const double*,\n"
                  "                 size_t, double, double*, int, size_t*, int32_t*, double*, size_t*) =\n"
                  "    &tpl_lanczos_two_pass_batch_shifted_inv_tol;\n"
                  "tpl_status (*f3)(tpl_op_t, const double*, int64_t, size_t, const double*,\n"
                  "                 const double*, size_t, const size_t*, const double*, const double*,\n"
                  "                 const size_t*, size_t, double*, int) =\n"
                  "    &tpl_lanczos_pass_two_batch_multi_cut;\n"
                  "size_t (*f4)(void) = &tpl_batch_shifted_inv_tol_auto_k;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rust_shim_names_the_solver():
    src = open(os.path.join(ROOT, "integration", "rust", "hip.rs")).read()
    assert "pub fn lanczos_two_pass_batch_shifted_inv_tol<" in src
    assert "pub fn lanczos_pass_two_batch_multi_cut<" in src
    for s in SYMBOLS:
        assert re.search(rf"\bfn {s}\(", src), s
