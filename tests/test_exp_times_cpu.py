"""CPU: the host built-in tpl_ftk_exp_t (include/tpl.h) — exp(t T_k) e_1 with t behind `user`,
the C ABI's form of ``ftk.exp_t`` and the host fallback of tpl_lanczos_two_pass_exp_times.

Its contract is bits: tpl_ftk_exp on the arrays t * alphas, t * betas, every entry times t and
rounded once — what numpy's ``t * alphas`` gives, so it equals ``ftk.EXP(t * al, t * be)`` and
the ``ftk.exp_t(t)`` closure bit for bit. No compute on the GPU here.
"""
import ctypes
from ctypes import POINTER, byref, c_double, c_size_t

import numpy as np
import pytest

from tpl_amd import _lib, ftk


def call_exp_t(al, be, t):
    """tpl_ftk_exp_t through ctypes -> (return code, y, message); t None: a NULL `user`."""
    al = np.ascontiguousarray(al, dtype=np.float64)
    be = np.ascontiguousarray(be, dtype=np.float64)
    n = al.shape[0]
    y = np.zeros(n)
    ylen = c_size_t(0)
    err = ctypes.create_string_buffer(1024)
    tt = c_double(0.0 if t is None else t)
    user = None if t is None else ctypes.cast(byref(tt), ctypes.c_void_p)
    rc = _lib.tpl_ftk_exp_t(al.ctypes.data_as(POINTER(c_double)), n,
                            be.ctypes.data_as(POINTER(c_double)), be.shape[0],
                            y.ctypes.data_as(POINTER(c_double)), n, byref(ylen), err, 1024, user)
    return rc, y, err.value.decode(), int(ylen.value)


def tridiagonal(k):
    rng = np.random.default_rng(500 + k)
    return rng.uniform(-10.0, -0.1, k), rng.uniform(0.1, 3.0, k - 1)


@pytest.mark.parametrize("k", [1, 2, 7, 200])
@pytest.mark.parametrize("t", [0.0, 0.25, 1.0, -1.0])
def test_exp_t_is_exp_on_the_scaled_tridiagonal(k, t):
    al, be = tridiagonal(k)
    rc, y, msg, ylen = call_exp_t(al, be, t)
    assert rc == 0 and msg == "" and ylen == k
    assert np.array_equal(y.view(np.uint64), ftk.EXP(t * al, t * be).view(np.uint64))
    assert np.array_equal(y.view(np.uint64), ftk.exp_t(t)(al, be).view(np.uint64))
    if t == 0.0:  # exp(0) e_1
        assert np.array_equal(y, np.eye(k)[0])


def test_exp_t_leaves_its_inputs_alone():
    al, be = tridiagonal(7)
    al0, be0 = al.copy(), be.copy()
    assert call_exp_t(al, be, 0.5)[0] == 0
    assert np.array_equal(al, al0) and np.array_equal(be, be0)


def test_exp_t_null_user_is_an_error():
    al, be = tridiagonal(7)
    rc, _, msg, _ = call_exp_t(al, be, None)
    assert rc != 0 and msg != ""


def test_exp_t_reports_inconsistent_sizes_as_exp_does():
    al, be = tridiagonal(7)
    rc, _, msg, _ = call_exp_t(al, be[:3], 1.0)
    assert rc != 0 and msg == "inconsistent tridiagonal sizes"


def test_exp_t_is_a_usable_ftk_pointer():
    """The raw pointer the bindings hand to the multi-function solves."""
    assert _lib.FTK_EXP_T_PTR and _lib.FTK_EXP_T_PTR != _lib.FTK_EXP_PTR
    assert "tpl_ftk_exp_t" in _lib.EXPORTED
