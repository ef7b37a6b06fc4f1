"""CPU: the batch exp-times solve's boundary (include/tpl.h
tpl_lanczos_two_pass_batch_exp_times, tpl_op_ftk_exp_times_batch_device) — what can be checked
without a GPU: the symbols, the refusal of a host-only plan, the Python-side validation and
the C++ header.
"""
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_double, c_int32, c_size_t

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import tpl_amd
from tpl_amd import LanczosError, _lib, solvers

SYMBOLS = ("tpl_lanczos_two_pass_batch_exp_times", "tpl_op_ftk_exp_times_batch_device")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True).stdout
    for s in SYMBOLS:
        assert re.search(rf"\btpl_status\s+{s}\s*\(", hdr), s
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s), s
        assert callable(getattr(_lib, s)), s
        assert re.search(rf"\bT {s}\b", nm), s
    assert tpl_amd.lanczos_two_pass_batch_exp_times is solvers.lanczos_two_pass_batch_exp_times
    assert "lanczos_two_pass_batch_exp_times" in tpl_amd.__all__
    assert callable(tpl_amd.HipCsrOp.ftk_exp_times_batch_device)


def test_table_size_mirrors_the_headers():
    """The hand-back table holds kBatchNbMax * TPL_MULTI_MAX entries: the widest group times the
    most times a call takes (the figures the device-bytes test of the GPU suite counts with)."""
    src = open(os.path.join(ROOT, "two-pass-lanczos_amd", "csrc", "tpl_batch.h")).read()
    w = re.search(r"constexpr int kBatchNbMax = (\d+);", src)
    hdr = open(os.path.join(ROOT, "include", "tpl.h")).read()
    mm = re.search(r"TPL_MULTI_MAX\s*=\s*(\d+)", hdr)
    assert w and mm and int(w.group(1)) == 4 and int(mm.group(1)) == _lib.TPL_MULTI_MAX == 64


def test_host_plan_is_refused():
    """A host-only plan holds no device data: both entry points refuse it with
    TPL_ERR_INVALID_ARGUMENT (set_device), before anything else is touched."""
    n = 12
    a = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    plan = tpl_amd.HostPlan(a)
    B = np.ones((2, n))  # C-order (s, n) == column-major (n, s)
    x = np.zeros((2 * 2, n))
    ts = np.array([0.5, 1.0])
    al, be, y = np.full((2, 4), -2.5), np.full((2, 4), 1.0), np.zeros((2 * 2, 4))
    st = (c_size_t * 2)(3, 3)
    on = np.zeros(4, dtype=np.int32)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    pi = on.ctypes.data_as(POINTER(c_int32))
    calls = [
        lambda: _lib.tpl_lanczos_two_pass_batch_exp_times(plan.handle, B.ctypes.data, n, 2, 4,
                                                          pd(ts), 2, x.ctypes.data,
                                                          _lib.TPL_MEM_HOST, pi),
        lambda: _lib.tpl_op_ftk_exp_times_batch_device(plan.handle, pd(al), pd(be), 4, st, 2,
                                                       pd(ts), 2, pd(y), pi),
    ]
    for call in calls:
        assert call() == _lib.TPL_ERR_INVALID_ARGUMENT
        assert "host-only plan" in _lib.last_error()
    plan.close()


def test_python_validates_before_any_device_call():
    """An empty B, an empty list of times and a B whose row count is not n are refused in
    Python: the operator here is a host-only plan, which no device call would accept."""
    op = tpl_amd.HostPlan(sp.identity(4, format="csr"))
    with pytest.raises(ValueError):
        solvers.lanczos_two_pass_batch_exp_times(op, np.zeros((4, 0)), 3, [1.0])
    with pytest.raises(ValueError):
        solvers.lanczos_two_pass_batch_exp_times(op, np.ones((4, 2)), 3, [])
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch_exp_times(op, np.ones((5, 2)), 3, [1.0, 2.0])
    assert "Dimension mismatch" in str(e.value)
    with pytest.raises(ValueError):  # one betas array per alphas array
        tpl_amd.HipCsrOp.ftk_exp_times_batch_device(op, [np.ones(3), np.ones(3)], [np.ones(2)],
                                                    [1.0])
    with pytest.raises(ValueError):  # steps_c - 1 betas
        tpl_amd.HipCsrOp.ftk_exp_times_batch_device(op, [np.ones(3), np.ones(3)],
                                                    [np.ones(2), np.ones(1)], [1.0])
    op.close()


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler found")


def test_cpp_header_names_the_batch_exp_times_solver(tmp_path):
    tu = tmp_path / "batch_exp_times.cpp"
    tu.write_text('#include "tpl.hpp"\n'
                  "tpl::Mat (*f1)(const tpl::HipCsrOp&, const tpl::Mat&, size_t,\n"
                  "               const std::vector<double>&, std::vector<int32_t>*) =\n"
                  "    &tpl::solvers::lanczos_two_pass_batch_exp_times;\n")
    r = subprocess.run([_clangxx(), "-std=c++17", "-fsyntax-only", "-Wall",
                        "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rust_shim_names_the_batch_exp_times_solver():
    src = open(os.path.join(ROOT, "integration", "rust", "hip.rs")).read()
    assert "pub fn lanczos_two_pass_batch_exp_times<" in src
    for s in SYMBOLS:
        assert re.search(rf"\bfn {s}\(", src), s
