"""CPU: the multi-function solves' boundary (include/tpl.h tpl_lanczos_two_pass_multi,
tpl_lanczos_multi, tpl_lanczos_pass_two_multi) — what can be checked without a GPU: the
symbols, the refusal of a host-only plan, the two f(T_k) families over the built-ins
(ftk.exp_t, ftk.inv_shift), the Python-side validation and the C++ header.
"""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_double

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

from conftest import ROOT

import tpl_amd
from tpl_amd import _lib, algorithms, ftk, solvers

MULTI = ("tpl_lanczos_two_pass_multi", "tpl_lanczos_multi", "tpl_lanczos_pass_two_multi")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in MULTI:
        assert re.search(rf"\btpl_status\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert re.search(r"\bTPL_MULTI_MAX\s*=\s*64\b", hdr) and _lib.TPL_MULTI_MAX == 64


def test_host_plan_is_refused():
    """A host-only plan holds no device data: every multi entry point refuses it with
    TPL_ERR_INVALID_ARGUMENT (set_device), before anything else is touched."""
    n = 12
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    plan = tpl_amd.HostPlan(a)
    b = np.ones(n)
    x = np.zeros((2, n))
    fs = (ctypes.c_void_p * 2)(_lib.FTK_INV_PTR, _lib.FTK_SQ_PTR)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    for fn in (_lib.tpl_lanczos_two_pass_multi, _lib.tpl_lanczos_multi):
        assert fn(plan.handle, b.ctypes.data, n, 4, fs, None, 2, x.ctypes.data,
                  _lib.TPL_MEM_HOST) == _lib.TPL_ERR_INVALID_ARGUMENT
        assert "host-only plan" in _lib.last_error()
    al, be, y = np.full(3, 2.5), np.full(2, 1.0), np.ones((2, 3))
    assert _lib.tpl_lanczos_pass_two_multi(plan.handle, b.ctypes.data, n, pd(al), 3, pd(be), 2, 3,
                                           1.0, pd(y), 3, 2, x.ctypes.data,
                                           _lib.TPL_MEM_HOST) == _lib.TPL_ERR_INVALID_ARGUMENT
    assert "host-only plan" in _lib.last_error()
    plan.close()


def _random_t(rows=40, seed=11):
    rng = np.random.default_rng(seed)
    al = rng.uniform(1.0, 3.0, rows)
    be = rng.uniform(-0.5, 0.5, rows - 1)
    return al, be, np.diag(al) + np.diag(be, 1) + np.diag(be, -1)


@pytest.mark.parametrize("t", [0.5, 1e-3, -2.0])
def test_exp_t_matches_expm(t):
    al, be, T = _random_t()
    yr = scipy.linalg.expm(t * T)[:, 0]
    y = ftk.exp_t(t)(al, be)
    assert np.linalg.norm(y - yr) <= 1e-11 * np.linalg.norm(yr)


@pytest.mark.parametrize("sigma", [1.0, 2.0, 0.0])
def test_inv_shift_matches_dense_solve(sigma):
    al, be, T = _random_t()
    yr = np.linalg.solve(T + sigma * np.eye(len(al)), np.eye(len(al))[:, 0])
    y = ftk.inv_shift(sigma)(al, be)
    assert np.linalg.norm(y - yr) <= 1e-11 * np.linalg.norm(yr)


def test_empty_function_list_is_refused_in_python():
    """Validated before the operator is touched: no GPU needed to see it."""
    a = sp.identity(4, format="csr")
    op = tpl_amd.HostPlan(a)  # never reached as an operator
    for fn in (solvers.lanczos_two_pass_multi, solvers.lanczos_multi):
        with pytest.raises(ValueError):
            fn(op, np.ones(4), 3, [])
    d = algorithms.LanczosDecomposition(np.ones(3), np.ones(2), 3, 1.0)
    with pytest.raises(ValueError):
        algorithms.lanczos_pass_two_multi(op, np.ones(4), d, np.zeros((3, 0)))
    op.close()


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_multi_solvers(tmp_path):
    tu = tmp_path / "multi.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "auto* f1 = &tpl::solvers::lanczos_two_pass_multi;\n"
                  "auto* f2 = &tpl::solvers::lanczos_multi;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
