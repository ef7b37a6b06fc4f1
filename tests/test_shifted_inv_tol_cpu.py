"""CPU: the shifted inverse solve that stops each shift at a tolerance (include/tpl.h
tpl_lanczos_two_pass_shifted_inv_tol, tpl_lanczos_pass_two_multi_cut,
tpl_op_ftk_inv_shifts_device) — what can be checked without a GPU: the argument errors that
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

SYMBOLS = ("tpl_lanczos_two_pass_shifted_inv_tol", "tpl_lanczos_pass_two_multi_cut",
           "tpl_op_ftk_inv_shifts_device")


def _plan(n=12):
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    return tpl_amd.HostPlan(a)


def test_argument_errors_in_the_documented_order():
    """On a host-only plan: NULL op / sigmas / x_out, then m, then tol, then a non-finite
    shift, each an argument error of its own; a valid call reaches the host-only refusal."""
    n, kmax = 12, 5
    plan = _plan(n)
    b, x = np.ones(n), np.zeros(n * 64)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))

    def call(sig, m=None, tol=1e-6, op=True, xp=True, sp_=True, full=True):
        sig = np.ascontiguousarray(sig, dtype=np.float64)
        m = sig.shape[0] if m is None else m
        st, rl = (c_size_t * 65)(), (c_size_t * 65)()
        cv, res = (c_int32 * 65)(), np.zeros(kmax * 65)
        out = (st, cv, pd(res), rl) if full else (None, None, None, None)
        rc = _lib.tpl_lanczos_two_pass_shifted_inv_tol(
            plan.handle if op else None, b.ctypes.data, n, kmax, pd(sig) if sp_ else None, m, tol,
            x.ctypes.data if xp else None, _lib.TPL_MEM_HOST, *out)
        return rc, _lib.last_error()

    nan, inf = float("nan"), float("inf")
    # 1. NULL, ahead of everything else that is wrong with the call
    for kw in ({"op": False}, {"sp_": False}, {"xp": False}):
        rc, msg = call([nan], m=0, tol=nan, **kw)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in msg, (kw, msg)
    # 2. m, ahead of tol and the shifts
    for m in (0, 65):
        rc, msg = call(np.full(65, nan), m=m, tol=nan)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_MULTI_MAX" in msg, (m, msg)
    # 3. tol, ahead of the shifts
    for tol in (nan, -1.0, -1e-300, -inf):
        rc, msg = call([1.0, nan], tol=tol)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "tol" in msg, (tol, msg)
    # 4. a non-finite shift, anywhere in the list
    for sig in ([nan], [0.0, inf], [1.0, 2.0, -inf], list(np.arange(63.0)) + [nan]):
        rc, msg = call(sig)
        assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "sigma" in msg, (sig, msg)
        assert "host-only" not in msg
    # a valid call (tol = 0 and +inf included, every output optional) reaches the refusal
    for tol in (0.0, 1e-8, inf):
        for full in (True, False):
            for sig in ([0.0], [0.0, 0.25, -2.0], np.arange(64.0)):
                rc, msg = call(sig, tol=tol, full=full)
                assert rc == _lib.TPL_ERR_INVALID_ARGUMENT and "host-only plan" in msg, msg
    plan.close()


def test_low_level_entry_points_check_their_arguments():
    n = 12
    plan = _plan(n)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    b, x = np.ones(n), np.zeros(n * 2)
    al, be, y = np.ones(4), np.ones(3), np.ones(8)
    cs = (c_size_t * 2)(4, 3)

    def cut(m=2, xp=True, csp=True):
        return _lib.tpl_lanczos_pass_two_multi_cut(
            plan.handle, b.ctypes.data, n, pd(al), 4, pd(be), 3, 4, 1.0, pd(y), 4,
            cs if csp else None, m, x.ctypes.data if xp else None, _lib.TPL_MEM_HOST)

    assert cut(xp=False) == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in _lib.last_error()
    assert cut(csp=False) == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in _lib.last_error()
    for m in (0, 65):
        assert cut(m=m) == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_MULTI_MAX" in _lib.last_error()
    assert cut() == _lib.TPL_ERR_INVALID_ARGUMENT and "host-only plan" in _lib.last_error()

    sig = np.array([0.0, 1.0])

    def shifts(nn=4, m=2, yp=True):
        return _lib.tpl_op_ftk_inv_shifts_device(plan.handle, pd(al), nn, pd(be), pd(sig), m,
                                                 pd(y) if yp else None)

    assert shifts(yp=False) == _lib.TPL_ERR_INVALID_ARGUMENT and "NULL" in _lib.last_error()
    for m in (0, 65):
        assert shifts(m=m) == _lib.TPL_ERR_INVALID_ARGUMENT and "TPL_MULTI_MAX" in _lib.last_error()
    assert shifts(nn=0) == _lib.TPL_ERR_INVALID_ARGUMENT
    assert shifts(nn=1366) == _lib.TPL_ERR_UNSUPPORTED
    assert shifts() == _lib.TPL_ERR_INVALID_ARGUMENT and "host-only plan" in _lib.last_error()
    plan.close()


def test_symbols_declared_exported_and_named_in_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in SYMBOLS:
        assert re.search(rf"\btpl_status\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert tpl_amd.lanczos_two_pass_shifted_inv_tol is solvers.lanczos_two_pass_shifted_inv_tol
    assert "lanczos_two_pass_shifted_inv_tol" in tpl_amd.__all__
    assert callable(algorithms.lanczos_pass_two_multi_cut)
    assert callable(tpl_amd.HipCsrOp.ftk_inv_shifts_device)


def test_new_kernels_are_in_the_library():
    """The hot path is native: the four kernels of tpl_k_p1_stol.hip are in the code object."""
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_p1_axpy_stol", b"k_p1_stol_fin", b"k_ftk_inv_shifts", b"k_p2_xacc_cut"):
        assert k in blob, k


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_solver(tmp_path):
    tu = tmp_path / "shifted_inv_tol.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "tpl::Mat (*f1)(const tpl::HipCsrOp&, const std::vector<double>&, size_t,\n"
                  "               const std::vector<double>&, double, tpl::solvers::ShiftedInvTolInfo*) =\n"
                  "    &tpl::solvers::lanczos_two_pass_shifted_inv_tol;\n"
                  "tpl_status (*f2)(tpl_op_t, const double*, int64_t, size_t, const double*, size_t,\n"
                  "                 double, double*, int, size_t*, int32_t*, double*, size_t*) =\n"
                  "    &tpl_lanczos_two_pass_shifted_inv_tol;\n"
                  "tpl_status (*f3)(tpl_op_t, const double*, int64_t, const double*, size_t,\n"
                  "                 const double*, size_t, size_t, double, const double*, size_t,\n"
                  "                 const size_t*, size_t, double*, int) = &tpl_lanczos_pass_two_multi_cut;\n"
                  "tpl_status (*f4)(tpl_op_t, const double*, size_t, const double*, const double*,\n"
                  "                 size_t, double*) = &tpl_op_ftk_inv_shifts_device;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rust_shim_names_the_solver():
    src = open(os.path.join(ROOT, "integration", "rust", "hip.rs")).read()
    assert "pub fn lanczos_two_pass_shifted_inv_tol<" in src
    assert "pub struct ShiftedInvTolInfo" in src
    for s in SYMBOLS:
        assert re.search(rf"\bfn {s}\(", src), s
