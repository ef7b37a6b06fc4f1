"""High-level solvers — mirror of the reference's ``src/solvers.rs``.

``lanczos(operator, b, k, f_tk_solver)``           src/solvers.rs:46-107
``lanczos_two_pass(operator, b, k, f_tk_solver)``  src/solvers.rs:133-175

Same argument meaning and error behaviour as the reference (the ``stack``
workspace argument has no counterpart: the device workspace belongs to the
operator). ``operator`` is a ``HipCsrOp`` (upload once) or the caller's own scipy CSR / CSC
matrix (uploaded on first use and re-used while unchanged: ``operator.as_operator``).
``f_tk_solver`` is a callable ``(alphas, betas) -> y'`` or a built-in
from :mod:`tpl_amd.ftk` (``"inv"``, ``"exp"``, ``"sq"``). Returns x_k with the
shape of ``b`` flattened to (n,) — numpy for host ``b``, torch CUDA for device ``b``.

``lanczos_two_pass_multi(operator, b, k, f_tk_solvers)`` and ``lanczos_multi`` (no reference
counterpart) solve f_1(A) b ... f_m(A) b over one Krylov space: one pass one, every f_i on
the host, one pass two. They return shape (n, m) with strides (1, n) — column i is bitwise
the single solve with ``f_tk_solvers[i]`` evaluated on the host.

``lanczos_two_pass_batch(operator, B, k, f_tk_solver)`` (no reference counterpart) solves
f(A) b_1 ... f(A) b_s for the columns of ``B`` in one lock-step two-pass run. It returns shape
(n, s) with strides (1, n) — column c is bitwise the single solve of ``B[:, c]`` with
``f_tk_solver`` evaluated on the host.

``lanczos_two_pass_batch_multi(operator, B, k, f_tk_solvers)`` (no reference counterpart) has
both axes: f_i(A) b_c for m functions and the s columns of ``B`` in one run. It returns shape
(n, m, s) with strides (1, n, n m) — ``X[:, i, c]`` is bitwise the single solve of ``B[:, c]``
with ``f_tk_solvers[i]`` evaluated on the host.

``lanczos_two_pass_exp_times(operator, b, k, ts)`` (no reference counterpart) is the action of
the matrix exponential at a list of times: exp(t_i A) b for every t_i over one Krylov space,
every exp(t_i T_k) e_1 evaluated at once on the device between the two shared passes. It
returns shape (n, m) with strides (1, n).

``lanczos_two_pass_inv_tol(operator, b, kmax, tol)`` (no reference counterpart) is the inverse
solve that stops when the Lanczos residual estimate is <= ``tol``: bitwise
``lanczos_two_pass(operator, b, m*, "inv")`` for the first such step m* <= kmax.

``lanczos_two_pass_shifted_inv_tol(operator, b, kmax, sigmas, tol)`` (no reference counterpart)
is the same for (A + sigma_i I)^{-1} b at m shifts over the one Krylov space of A, every shift
stopped at its own step m*_i. It returns shape (n, m) with strides (1, n).

``lanczos_two_pass_batch_exp_times(operator, B, k, ts)`` (no reference counterpart) is the same
for the s columns of ``B`` in lock-step: exp(t_i A) b_c, every exp(t_i T_k) e_1 of a group of
columns evaluated by one device launch. It returns shape (n, m, s) with strides (1, n, n m).

``lanczos_two_pass_batch_shifted_inv_tol(operator, B, kmax, sigmas, tol)`` (no reference
counterpart) is ``lanczos_two_pass_shifted_inv_tol`` for the s columns of ``B`` in lock-step:
(A + sigma_i I)^{-1} b_c, every (column, shift) stopped at its own step. It returns shape
(n, m, s) with strides (1, n, n m).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, ftk
from ._vec import Cols, Vec
from .error import LanczosError, check
from .operator import as_operator


def _run(fn, operator, b, k, f_tk_solver):
    operator = as_operator(operator)
    bv = Vec(b)
    x = bv.empty(operator.nrows())
    fptr, keep = ftk.resolve(f_tk_solver)
    try:
        check(fn(operator.handle, bv.ptr, bv.n, k, fptr, None, Vec.ptr_of(x), bv.mem))
    except LanczosError as e:
        raise ftk.remap_error(e, keep) from None
    return x


def lanczos(operator, b, k: int, f_tk_solver):
    """f(A) b by standard one-pass Lanczos: V_k kept in HBM, x = ||b|| V_k f(T_k) e_1."""
    return _run(_lib.tpl_lanczos, operator, b, k, f_tk_solver)


def lanczos_two_pass(operator, b, k: int, f_tk_solver):
    """f(A) b by two-pass Lanczos: O(n) memory, the basis is regenerated in pass two."""
    return _run(_lib.tpl_lanczos_two_pass, operator, b, k, f_tk_solver)


def _run_multi(fn, operator, b, k, f_tk_solvers):
    fs = list(f_tk_solvers)
    if not fs:
        raise ValueError("f_tk_solvers must hold at least one solver")
    operator = as_operator(operator)
    bv = Vec(b)
    m = len(fs)
    x = bv.empty(m, operator.nrows())  # C-order (m, n) == column-major (n, m)
    resolved = [ftk.resolve(f) for f in fs]
    fptrs = (ctypes.c_void_p * m)(*[p for p, _ in resolved])
    try:
        check(fn(operator.handle, bv.ptr, bv.n, k, fptrs, None, m, Vec.ptr_of(x), bv.mem))
    except LanczosError as e:
        # the functions run in index order and the first failure ends the call: a solver
        # that recorded a column-count mismatch is the one that failed
        for _, keep in resolved:
            if keep is not None and keep.mismatch is not None:
                raise ftk.remap_error(e, keep) from None
        raise
    return x.T


def lanczos_multi(operator, b, k: int, f_tk_solvers):
    """f_i(A) b, i = 0 .. m-1, by ONE standard pass: column i = ``lanczos`` with f_i."""
    return _run_multi(_lib.tpl_lanczos_multi, operator, b, k, f_tk_solvers)


def lanczos_two_pass_multi(operator, b, k: int, f_tk_solvers):
    """f_i(A) b, i = 0 .. m-1, by ONE two-pass run: pass one once, every f_i(T_k) on the
    host, one pass two that regenerates the basis once for all m results."""
    return _run_multi(_lib.tpl_lanczos_two_pass_multi, operator, b, k, f_tk_solvers)


def lanczos_two_pass_exp_times(operator, b, k: int, ts, return_on_device: bool = False):
    """exp(t_i A) b for the m times ``ts`` by ONE two-pass run: pass one once, every
    exp(t_i T_k) e_1 at once on the device (one workgroup per time; a time the device hands
    back, and with ``set_device_ftk(0)`` every time, runs the native host ``exp_t``), one pass
    two for all m results. Column i is ``lanczos_two_pass`` with ``ftk.exp_t(ts[i])`` to the
    device exp's accuracy. With ``return_on_device`` also the (m,) bool array of the times
    whose y the device computed."""
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(ts, dtype=np.float64)).reshape(-1))
    m = int(t.shape[0])
    operator = as_operator(operator)
    bv = Vec(b)
    x = bv.empty(max(m, 1), operator.nrows())  # C-order (m, n) == column-major (n, m)
    on = np.zeros(max(m, 1), dtype=np.int32)
    check(_lib.tpl_lanczos_two_pass_exp_times(
        operator.handle, bv.ptr, bv.n, k, t.ctypes.data_as(_lib.PD), m, Vec.ptr_of(x), bv.mem,
        on.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return (x.T, on.astype(bool)) if return_on_device else x.T


def lanczos_two_pass_inv_tol(operator, b, kmax: int, tol: float, return_info: bool = False):
    """A^{-1} b by the two-pass solve with the built-in inv, stopped at the first step m* whose
    relative Lanczos residual (``ftk.inv_residuals``) is <= ``tol``, or at ``kmax``. Bitwise
    ``lanczos_two_pass(operator, b, m*, ftk.INV)``. On one GPU within the device-inv bounds
    (``set_device_ftk``) the whole call is one graph and the stop is taken on the device.
    With ``return_info`` also a dict: ``steps`` (m*), ``converged`` (bool) and ``residuals``
    (numpy: the history up to the last entry formed, at least the first
    min(m*, steps taken by pass one - 1))."""
    operator = as_operator(operator)
    bv = Vec(b)
    x = bv.empty(operator.nrows())
    kcap = max(int(kmax), 1)
    res = np.zeros(kcap, dtype=np.float64)
    steps, rlen, conv = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int32(0)
    check(_lib.tpl_lanczos_two_pass_inv_tol(
        operator.handle, bv.ptr, bv.n, kmax, float(tol), Vec.ptr_of(x), bv.mem,
        ctypes.byref(steps), ctypes.byref(conv), res.ctypes.data_as(_lib.PD), ctypes.byref(rlen)))
    if not return_info:
        return x
    return x, {"steps": int(steps.value), "converged": bool(conv.value),
               "residuals": res[: rlen.value].copy()}


def lanczos_two_pass_shifted_inv_tol(operator, b, kmax: int, sigmas, tol: float,
                                     return_info: bool = False):
    """(A + sigma_i I)^{-1} b for the m shifts ``sigmas`` by ONE two-pass run on A, each shift
    stopped at the first step m*_i whose relative Lanczos residual
    (``ftk.inv_residuals(alphas + sigma_i, betas)``) is <= ``tol``, or at the steps pass one
    took. Column i is bitwise ``algorithms.lanczos_pass_two`` on A's decomposition cut to m*_i
    steps with y_i = ||b|| INV(alphas[:m*_i] + sigma_i, betas[:m*_i - 1]); it depends neither on
    m nor on the other shifts. On one GPU within the device-inv bounds (``set_device_ftk``) the
    whole call is one graph: pass one's elimination workgroup runs one lane per shift and the
    stop is taken on the device when every shift has met the tolerance. Returns shape (n, m)
    with strides (1, n); with ``return_info`` also a dict: ``steps`` ((m,) int array of m*_i),
    ``converged`` ((m,) bool array) and ``residuals`` (a list of m numpy arrays: each history up
    to the last entry formed, at least the first min(m*_i, steps taken by pass one - 1))."""
    sg = np.ascontiguousarray(np.atleast_1d(np.asarray(sigmas, dtype=np.float64)).reshape(-1))
    m = int(sg.shape[0])
    operator = as_operator(operator)
    bv = Vec(b)
    x = bv.empty(max(m, 1), operator.nrows())  # C-order (m, n) == column-major (n, m)
    kcap = max(int(kmax), 1)
    res = np.zeros((max(m, 1), kcap), dtype=np.float64)  # column-major (kmax, m)
    steps = (ctypes.c_size_t * max(m, 1))()
    rlen = (ctypes.c_size_t * max(m, 1))()
    conv = (ctypes.c_int32 * max(m, 1))()
    check(_lib.tpl_lanczos_two_pass_shifted_inv_tol(
        operator.handle, bv.ptr, bv.n, kmax, sg.ctypes.data_as(_lib.PD), m, float(tol),
        Vec.ptr_of(x), bv.mem, steps, conv, res.ctypes.data_as(_lib.PD), rlen))
    if not return_info:
        return x.T
    return x.T, {"steps": np.array(steps[:m], dtype=np.int64),
                 "converged": np.array(conv[:m], dtype=bool),
                 "residuals": [res[i, : rlen[i]].copy() for i in range(m)]}


def lanczos_two_pass_batch(operator, B, k: int, f_tk_solver):
    """f(A) b_c for every column of ``B`` (n x s; a 1-D ``B`` is one column) by ONE lock-step
    two-pass run: pass one for all columns together, f(T_k) per column on the host in column
    order, one pass two. Each column keeps its own steps_taken."""
    bv = Cols(B)
    bv.check_rows(operator)
    operator = as_operator(operator)
    x = bv.empty(bv.s, bv.n)  # C-order (s, n) == column-major (n, s)
    fptr, keep = ftk.resolve(f_tk_solver)
    try:
        check(_lib.tpl_lanczos_two_pass_batch(operator.handle, bv.ptr, bv.n, bv.s, k, fptr, None,
                                              Vec.ptr_of(x), bv.mem))
    except LanczosError as e:
        raise ftk.remap_error(e, keep) from None
    return x.T


def lanczos_two_pass_batch_multi(operator, B, k: int, f_tk_solvers):
    """f_i(A) b_c for every solver i and every column c of ``B`` (n x s) by ONE run: per group
    of columns pass one in lock-step, every f_i(T_k) on the host (column by column, the
    solvers in index order), one pass two that regenerates the group's bases once for all
    its results. Returns shape (n, m, s): ``X[:, i, c]`` = f_i(A) ``B[:, c]``."""
    fs = list(f_tk_solvers)
    if not fs:
        raise ValueError("f_tk_solvers must hold at least one solver")
    bv = Cols(B)
    bv.check_rows(operator)
    operator = as_operator(operator)
    m = len(fs)
    x = bv.empty(bv.s, m, bv.n)  # C-order (s, m, n) == column-major n x (s m), column c m + i
    resolved = [ftk.resolve(f) for f in fs]
    fptrs = (ctypes.c_void_p * m)(*[p for p, _ in resolved])
    try:
        check(_lib.tpl_lanczos_two_pass_batch_multi(operator.handle, bv.ptr, bv.n, bv.s, k, fptrs,
                                                    None, m, Vec.ptr_of(x), bv.mem))
    except LanczosError as e:
        # as _run_multi: the first failure ends the call, so a solver that recorded a
        # column-count mismatch is the one that failed
        for _, keep in resolved:
            if keep is not None and keep.mismatch is not None:
                raise ftk.remap_error(e, keep) from None
        raise
    return x.permute(2, 1, 0) if hasattr(x, "permute") else x.transpose(2, 1, 0)


def lanczos_two_pass_batch_exp_times(operator, B, k: int, ts, return_on_device: bool = False):
    """exp(t_i A) b_c for the m times ``ts`` and every column c of ``B`` (n x s) by ONE run:
    per group of columns pass one in lock-step, every exp(t_i T_k) e_1 of every column at once
    on the device (one workgroup per time and column; what the device hands back, and with
    ``set_device_ftk(0)`` everything, runs the native host ``exp_t``), one pass two for the
    group's results. Returns shape (n, m, s): ``X[:, i, c]`` is bitwise
    ``lanczos_two_pass_exp_times(operator, B[:, c], k, ts)[:, i]``. With ``return_on_device``
    also the (m, s) bool array of the (time, column) pairs whose y the device computed."""
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(ts, dtype=np.float64)).reshape(-1))
    m = int(t.shape[0])
    if m == 0:
        raise ValueError("ts must hold at least one time")
    bv = Cols(B)
    bv.check_rows(operator)
    operator = as_operator(operator)
    x = bv.empty(bv.s, m, bv.n)  # C-order (s, m, n) == column-major n x (s m), column c m + i
    on = np.zeros(bv.s * m, dtype=np.int32)
    check(_lib.tpl_lanczos_two_pass_batch_exp_times(
        operator.handle, bv.ptr, bv.n, bv.s, k, t.ctypes.data_as(_lib.PD), m, Vec.ptr_of(x),
        bv.mem, on.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    X = x.permute(2, 1, 0) if hasattr(x, "permute") else x.transpose(2, 1, 0)
    return (X, on.reshape(bv.s, m).T.astype(bool)) if return_on_device else X


def lanczos_two_pass_batch_shifted_inv_tol(operator, B, kmax: int, sigmas, tol: float,
                                           return_info: bool = False):
    """(A + sigma_i I)^{-1} b_c for the m shifts ``sigmas`` and every column c of ``B`` (n x s)
    by ONE run: per group of columns pass one on A in lock-step, every (column, shift) stopped at
    the first step m*_{c,i} whose relative Lanczos residual is <= ``tol`` (or at the steps
    column c took), one pass two that cuts each of the group's results at its own step.
    ``X[:, i, c]`` is bitwise ``lanczos_two_pass_shifted_inv_tol(operator, B[:, c], kmax,
    sigmas, tol)[:, i]``, whatever s, m and the other columns hold. On one GPU within the
    device-inv bounds (``set_device_ftk``) a group is one graph: the elimination workgroup of
    pass one runs one lane per (column, shift), a column stops storing when all its shifts have
    met the tolerance, and the launches left when every column has stopped return at once.
    Returns shape (n, m, s) as ``lanczos_two_pass_batch_multi``; with ``return_info`` also a
    dict: ``steps`` ((m, s) int array of m*_{c,i}), ``converged`` ((m, s) bool array) and
    ``residuals`` (``residuals[c][i]``: the history of (c, i) up to the last entry formed)."""
    sg = np.ascontiguousarray(np.atleast_1d(np.asarray(sigmas, dtype=np.float64)).reshape(-1))
    m = int(sg.shape[0])
    if m == 0:
        raise ValueError("sigmas must hold at least one shift")
    bv = Cols(B)
    bv.check_rows(operator)
    operator = as_operator(operator)
    s = bv.s
    x = bv.empty(s, m, bv.n)  # C-order (s, m, n) == column-major n x (s m), column c m + i
    kcap = max(int(kmax), 1)
    res = np.zeros((max(s * m, 1), kcap), dtype=np.float64)  # column-major (kmax, s m)
    steps = (ctypes.c_size_t * max(s * m, 1))()
    rlen = (ctypes.c_size_t * max(s * m, 1))()
    conv = (ctypes.c_int32 * max(s * m, 1))()
    check(_lib.tpl_lanczos_two_pass_batch_shifted_inv_tol(
        operator.handle, bv.ptr, bv.n, s, kmax, sg.ctypes.data_as(_lib.PD), m, float(tol),
        Vec.ptr_of(x), bv.mem, steps, conv, res.ctypes.data_as(_lib.PD), rlen))
    X = x.permute(2, 1, 0) if hasattr(x, "permute") else x.transpose(2, 1, 0)
    if not return_info:
        return X
    return X, {"steps": np.array(steps[:s * m], dtype=np.int64).reshape(s, m).T,
               "converged": np.array(conv[:s * m], dtype=bool).reshape(s, m).T,
               "residuals": [[res[c * m + i, : rlen[c * m + i]].copy() for i in range(m)]
                             for c in range(s)]}
