"""CPU: the batch-multi solves' boundary (include/tpl.h tpl_lanczos_two_pass_batch_multi,
tpl_lanczos_pass_two_batch_multi) — what can be checked without a GPU: the symbols, the
refusal of a host-only plan, the Python-side validation and the C++ header.
"""
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_double, c_size_t, c_void_p

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import tpl_amd
from tpl_amd import LanczosError, _lib, algorithms, ftk, solvers

SYMBOLS = ("tpl_lanczos_two_pass_batch_multi", "tpl_lanczos_pass_two_batch_multi")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in SYMBOLS:
        assert re.search(rf"\btpl_status\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert tpl_amd.lanczos_two_pass_batch_multi is solvers.lanczos_two_pass_batch_multi
    assert callable(algorithms.lanczos_pass_two_batch_multi)


def test_functions_per_launch_mirror():
    """_lib.BATCH_MULTI_FUNCS is the kernel's functions-per-launch (the GPU tests choose their
    function counts around it)."""
    src = open(os.path.join(ROOT, "two-pass-lanczos_amd", "csrc", "tpl_batch.h")).read()
    m = re.search(r"constexpr int kBatchMultiFuncs = (\d+);", src)
    assert m and int(m.group(1)) == _lib.BATCH_MULTI_FUNCS


def test_host_plan_is_refused():
    """A host-only plan holds no device data: both entry points refuse it with
    TPL_ERR_INVALID_ARGUMENT (set_device), before anything else is touched."""
    n = 12
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    plan = tpl_amd.HostPlan(a)
    B = np.ones((2, n))  # C-order (s, n) == column-major (n, s)
    x = np.zeros((2 * 2, n))
    al, be, y = np.full((2, 4), 2.5), np.full((2, 4), 1.0), np.ones((2 * 2, 4))
    st, bn = (c_size_t * 2)(3, 3), np.ones(2)
    fp = (c_void_p * 2)(_lib.FTK_SQ_PTR, _lib.FTK_SQ_PTR)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    H = _lib.TPL_MEM_HOST
    calls = [
        lambda: _lib.tpl_lanczos_two_pass_batch_multi(plan.handle, B.ctypes.data, n, 2, 4, fp, None,
                                                      2, x.ctypes.data, H),
        lambda: _lib.tpl_lanczos_pass_two_batch_multi(plan.handle, B.ctypes.data, n, 2, pd(al),
                                                      pd(be), 4, st, pd(bn), pd(y), 2,
                                                      x.ctypes.data, H),
    ]
    for call in calls:
        assert call() == _lib.TPL_ERR_INVALID_ARGUMENT
        assert "host-only plan" in _lib.last_error()
    plan.close()


def test_python_validates_before_any_device_call():
    """An empty B, an empty solver list and a B whose row count is not n are refused in
    Python: the operator here is a host-only plan, which no device call would accept."""
    a = sp.identity(4, format="csr")
    op = tpl_amd.HostPlan(a)
    d = algorithms.LanczosDecomposition(np.ones(3), np.ones(2), 3, 1.0)
    Y = np.ones((3, 2))
    with pytest.raises(ValueError):
        solvers.lanczos_two_pass_batch_multi(op, np.zeros((4, 0)), 3, [ftk.SQ])
    with pytest.raises(ValueError):
        solvers.lanczos_two_pass_batch_multi(op, np.ones((4, 2)), 3, [])
    with pytest.raises(ValueError):
        algorithms.lanczos_pass_two_batch_multi(op, np.zeros((4, 0)), [], [])
    text = "Dimension mismatch"
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch_multi(op, np.ones((5, 2)), 3, [ftk.SQ, ftk.SQ])
    assert text in str(e.value)
    with pytest.raises(LanczosError) as e:
        algorithms.lanczos_pass_two_batch_multi(op, np.ones((5, 2)), [d, d], [Y, Y])
    assert text in str(e.value)
    with pytest.raises(ValueError):  # one decomposition and one Y per column
        algorithms.lanczos_pass_two_batch_multi(op, np.ones((4, 2)), [d], [Y])
    with pytest.raises(ValueError):  # the same m for every column
        algorithms.lanczos_pass_two_batch_multi(op, np.ones((4, 2)), [d, d], [Y, Y[:, :1]])
    with pytest.raises(ValueError):  # at least one coefficient column
        algorithms.lanczos_pass_two_batch_multi(op, np.ones((4, 2)), [d, d], [Y[:, :0], Y[:, :0]])
    with pytest.raises(LanczosError) as e:  # the single call's y_k check, per column
        algorithms.lanczos_pass_two_batch_multi(op, np.ones((4, 2)), [d, d], [Y, Y[:2]])
    assert str(e.value) == "Parameter mismatch: `y_k` expects size 3, but got 2."
    op.close()


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_batch_multi_solver(tmp_path):
    tu = tmp_path / "batch_multi.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "auto* f1 = &tpl::solvers::lanczos_two_pass_batch_multi;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
