"""Low-level Lanczos entry points — mirror of the reference's ``src/algorithms``.

=====================================  ================================================
this module                            reference
=====================================  ================================================
``TridiagonalSystemView``              src/algorithms/mod.rs:57-67
``LanczosDecomposition``               src/algorithms/mod.rs:94-108
``LanczosOutput``                      src/algorithms/mod.rs:115-122
``LanczosPassTwoOutput``               src/algorithms/mod.rs:130-135
``lanczos_standard``                   src/algorithms/lanczos.rs:55-156
``lanczos_pass_one``                   src/algorithms/lanczos_two_pass.rs:65-110
``lanczos_pass_two``                   src/algorithms/lanczos_two_pass.rs:128-140
``lanczos_pass_two_with_basis``        src/algorithms/lanczos_two_pass.rs:149-166
``lanczos_pass_two_multi``             (none: pass two for m coefficient vectors at once)
``lanczos_pass_two_multi_cut``         (none: the same, column i cut to its own step count)
``lanczos_pass_one_batch``             (none: pass one for s vectors b in lock-step)
``lanczos_pass_two_batch``             (none: pass two for s vectors b in lock-step)
``lanczos_pass_two_batch_multi``       (none: the same for m coefficient vectors per b)
``lanczos_pass_two_batch_multi_cut``   (none: the same, result (c, i) cut to its own steps)
=====================================  ================================================

Every call runs the recurrence on the GPU through libtpl_amd.so (C ABI,
include/tpl.h). ``b`` may be a numpy array (results come back as numpy) or a torch
CUDA tensor (results stay on the device as torch tensors).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, byref, c_double, c_size_t
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from . import _lib
from ._vec import Cols, Vec
from .error import LanczosError, check
from .operator import HipCsrOp, as_operator

BREAKDOWN_TOLERANCE = 1000.0 * np.finfo(np.float64).eps  # src/algorithms/mod.rs:140-143


@dataclass
class TridiagonalSystemView:
    alphas: np.ndarray
    betas: np.ndarray
    steps_taken: int


@dataclass
class LanczosDecomposition:
    alphas: np.ndarray
    betas: np.ndarray
    steps_taken: int
    b_norm: float


@dataclass
class LanczosOutput:
    v_k: object  # (n, steps) column-major; numpy or torch
    decomposition: LanczosDecomposition


@dataclass
class LanczosPassTwoOutput:
    x_k: object
    v_k: object


class DeviceBasisView:
    """The ``MatRef`` V_k handed to a step callback: a device pointer plus shape.

    ``numpy()`` copies it to the host (n x k, column-major like the reference)."""

    def __init__(self, ptr: int, n: int, k: int):
        self.ptr, self.shape = ptr, (n, k)

    def numpy(self) -> np.ndarray:
        n, k = self.shape
        out = np.empty((k, n), dtype=np.float64)
        if n * k:
            check(_lib.tpl_copy_to_host(out.ctypes.data, self.ptr, n * k * 8))
        return out.T


def _op(operator) -> HipCsrOp:
    """A HipCsrOp, or the caller's scipy matrix uploaded once (operator.as_operator)."""
    return as_operator(operator)


def _reorth_mode(r) -> int:
    if r in (False, None, 0):
        return 0
    if r in (True, 1, "cgs2"):
        return 1
    if r in (2, "selective"):
        return 2
    raise ValueError("reorthogonalize must be False, True / 'cgs2' or 'selective'")


def lanczos_standard(operator, b, k: int, callback: Optional[Callable] = None,
                     reorthogonalize=False) -> LanczosOutput:
    """One-pass Lanczos storing V_k (in HBM); src/algorithms/lanczos.rs:55-156.

    ``callback(k, v_k_view, t_k_view) -> bool`` mirrors ``LanczosCallback``
    (src/algorithms/mod.rs:82-86): return False to stop early.
    ``reorthogonalize=True`` (or ``"cgs2"``) adds CGS2 full re-orthogonalisation against
    V_k, ``"selective"`` the Kahan–Parlett variant (second pass only when needed) —
    extensions with no reference counterpart (not used by any reference path).
    """
    op = _op(operator)
    bv = Vec(b)
    alphas = np.zeros(max(k, 1))
    betas = np.zeros(max(k, 1))
    steps = c_size_t(0)
    bnorm = c_double(0.0)
    v_full = bv.empty(max(k, 1), op.nrows())  # C-order (k, n) == column-major (n, k)
    cb_c = None
    raised = []
    if callback is not None:
        def _cb(kk, vptr, n, pa, na, pb, nb, user):
            va = np.ctypeslib.as_array(pa, (na,)).copy() if na else np.zeros(0)
            vb = np.ctypeslib.as_array(pb, (nb,)).copy() if nb else np.zeros(0)
            try:
                return 1 if callback(int(kk), DeviceBasisView(vptr, int(n), int(kk)),
                                     TridiagonalSystemView(va, vb, int(kk))) else 0
            except BaseException as e:  # stop the device loop, re-raised below
                raised.append(e)
                return 0
        cb_c = _lib.STEP_CB(_cb)
    check(_lib.tpl_lanczos_standard(
        op.handle, bv.ptr, bv.n, k, alphas.ctypes.data_as(POINTER(c_double)),
        betas.ctypes.data_as(POINTER(c_double)), byref(steps), byref(bnorm), Vec.ptr_of(v_full),
        bv.mem, _reorth_mode(reorthogonalize), cb_c, None))
    if raised:
        raise raised[0]
    s = steps.value
    v_k = v_full[:s].T
    dec = LanczosDecomposition(alphas[:s].copy(), betas[:max(s - 1, 0)].copy(), s, bnorm.value)
    return LanczosOutput(v_k, dec)


def lanczos_pass_one(operator, b, k: int) -> LanczosDecomposition:
    """First pass: scalars only, O(n) memory; src/algorithms/lanczos_two_pass.rs:65-110."""
    op = _op(operator)
    bv = Vec(b)
    alphas = np.zeros(max(k, 1))
    betas = np.zeros(max(k, 1))
    steps = c_size_t(0)
    bnorm = c_double(0.0)
    check(_lib.tpl_lanczos_pass_one(op.handle, bv.ptr, bv.n, k,
                                    alphas.ctypes.data_as(POINTER(c_double)),
                                    betas.ctypes.data_as(POINTER(c_double)), byref(steps),
                                    byref(bnorm), bv.mem))
    s = steps.value
    return LanczosDecomposition(alphas[:s].copy(), betas[:max(s - 1, 0)].copy(), s, bnorm.value)


def _pass_two(operator, b, decomposition: LanczosDecomposition, y_k, store_basis: bool):
    op = _op(operator)
    bv = Vec(b)
    y = np.ascontiguousarray(np.asarray(y_k, dtype=np.float64).reshape(-1)) \
        if not hasattr(y_k, "is_cuda") else y_k.detach().double().cpu().numpy().reshape(-1)
    a = np.ascontiguousarray(decomposition.alphas, dtype=np.float64).reshape(-1)
    bb = np.ascontiguousarray(decomposition.betas, dtype=np.float64).reshape(-1)
    s = int(decomposition.steps_taken)
    x = bv.empty(op.nrows())
    v = bv.empty(max(s, 1), op.nrows()) if store_basis else None
    check(_lib.tpl_lanczos_pass_two(
        op.handle, bv.ptr, bv.n, a.ctypes.data_as(POINTER(c_double)), a.shape[0],
        bb.ctypes.data_as(POINTER(c_double)), bb.shape[0], s, float(decomposition.b_norm),
        y.ctypes.data_as(POINTER(c_double)), y.shape[0], Vec.ptr_of(x),
        Vec.ptr_of(v) if v is not None else None, bv.mem))
    return x, (v[:s].T if v is not None else None)


def lanczos_pass_two(operator, b, decomposition: LanczosDecomposition, y_k):
    """Second pass: regenerate v_j on the fly, x = sum_j y_j v_j;
    src/algorithms/lanczos_two_pass.rs:128-140. ``y_k`` = f(T_k) e_1 * ||b||."""
    return _pass_two(operator, b, decomposition, y_k, False)[0]


def lanczos_pass_two_with_basis(operator, b, decomposition: LanczosDecomposition,
                                y_k) -> LanczosPassTwoOutput:
    """Test variant returning the regenerated basis V'_k;
    src/algorithms/lanczos_two_pass.rs:149-166."""
    x, v = _pass_two(operator, b, decomposition, y_k, True)
    return LanczosPassTwoOutput(x, v)


def lanczos_pass_two_multi(operator, b, decomposition: LanczosDecomposition, Y):
    """Second pass for m coefficient vectors over one decomposition: ``Y`` is (steps, m),
    column i = f_i(T_k) e_1 * ||b||. The basis is regenerated once. Returns shape (n, m)
    with strides (1, n); column i is bitwise ``lanczos_pass_two`` with ``Y[:, i]``."""
    y = Y.detach().double().cpu().numpy() if hasattr(Y, "is_cuda") else np.asarray(Y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("Y must be a (steps, m) matrix")
    y_len, m = y.shape
    if m == 0:
        raise ValueError("Y must hold at least one column")
    op = _op(operator)
    bv = Vec(b)
    yt = np.ascontiguousarray(y.T)  # C-order (m, y_len) == column-major (y_len, m)
    a = np.ascontiguousarray(decomposition.alphas, dtype=np.float64).reshape(-1)
    bb = np.ascontiguousarray(decomposition.betas, dtype=np.float64).reshape(-1)
    x = bv.empty(m, op.nrows())
    check(_lib.tpl_lanczos_pass_two_multi(
        op.handle, bv.ptr, bv.n, a.ctypes.data_as(POINTER(c_double)), a.shape[0],
        bb.ctypes.data_as(POINTER(c_double)), bb.shape[0], int(decomposition.steps_taken),
        float(decomposition.b_norm), yt.ctypes.data_as(POINTER(c_double)), y_len, m,
        Vec.ptr_of(x), bv.mem))
    return x.T


def lanczos_pass_two_multi_cut(operator, b, decomposition: LanczosDecomposition, Y, col_steps):
    """``lanczos_pass_two_multi`` with a per-column cut: column i takes only the first
    ``col_steps[i]`` steps (1 <= col_steps[i] <= steps), so it is bitwise ``lanczos_pass_two``
    on the decomposition cut to ``col_steps[i]`` steps with ``Y[:col_steps[i], i]``; the rest
    of ``Y``'s column i is never used. Returns shape (n, m) with strides (1, n)."""
    y = Y.detach().double().cpu().numpy() if hasattr(Y, "is_cuda") else np.asarray(Y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("Y must be a (steps, m) matrix")
    ldy, m = y.shape
    cs = [int(c) for c in col_steps]
    if m == 0 or len(cs) != m:
        raise ValueError("Y must hold at least one column and col_steps one entry per column")
    if min(cs) < 0:
        raise ValueError("col_steps must not be negative")
    op = _op(operator)
    bv = Vec(b)
    yt = np.ascontiguousarray(y.T)  # C-order (m, ldy) == column-major (ldy, m)
    a = np.ascontiguousarray(decomposition.alphas, dtype=np.float64).reshape(-1)
    bb = np.ascontiguousarray(decomposition.betas, dtype=np.float64).reshape(-1)
    x = bv.empty(m, op.nrows())
    check(_lib.tpl_lanczos_pass_two_multi_cut(
        op.handle, bv.ptr, bv.n, a.ctypes.data_as(POINTER(c_double)), a.shape[0],
        bb.ctypes.data_as(POINTER(c_double)), bb.shape[0], int(decomposition.steps_taken),
        float(decomposition.b_norm), yt.ctypes.data_as(POINTER(c_double)), ldy,
        (ctypes.c_size_t * m)(*cs), m, Vec.ptr_of(x), bv.mem))
    return x.T


def lanczos_pass_one_batch(operator, B, k: int) -> list:
    """First pass for every column of ``B`` (n x s) in lock-step: a list of s
    ``LanczosDecomposition``; entry c is bitwise ``lanczos_pass_one`` of ``B[:, c]``."""
    bv = Cols(B)
    bv.check_rows(operator)
    op = _op(operator)
    kk = max(k, 1)
    alphas = np.zeros((bv.s, kk))  # C-order (s, k) == column-major (k, s)
    betas = np.zeros((bv.s, kk))
    steps = (c_size_t * bv.s)()
    bnorms = np.zeros(bv.s)
    check(_lib.tpl_lanczos_pass_one_batch(
        op.handle, bv.ptr, bv.n, bv.s, k, alphas.ctypes.data_as(POINTER(c_double)),
        betas.ctypes.data_as(POINTER(c_double)), steps, bnorms.ctypes.data_as(POINTER(c_double)),
        bv.mem))
    out = []
    for c in range(bv.s):
        st = int(steps[c])
        out.append(LanczosDecomposition(alphas[c, :st].copy(), betas[c, :max(st - 1, 0)].copy(),
                                        st, float(bnorms[c])))
    return out


def lanczos_pass_two_batch(operator, B, decompositions, ys):
    """Second pass for every column of ``B`` in lock-step: ``decompositions[c]`` and
    ``ys[c]`` (= f(T_k) e_1 * ||b_c||, ``steps_taken`` entries) belong to ``B[:, c]``.
    Returns shape (n, s) with strides (1, n); column c is bitwise ``lanczos_pass_two``."""
    bv = Cols(B)
    bv.check_rows(operator)
    decs, ys = list(decompositions), list(ys)
    if len(decs) != bv.s or len(ys) != bv.s:
        raise ValueError("one decomposition and one y per column of B")
    op = _op(operator)
    yl = [y.detach().double().cpu().numpy().reshape(-1) if hasattr(y, "is_cuda")
          else np.asarray(y, dtype=np.float64).reshape(-1) for y in ys]
    for d, y in zip(decs, yl):  # the single call's check, per column in ascending order
        if int(d.steps_taken) != y.shape[0]:
            raise LanczosError.parameter_mismatch("y_k", int(d.steps_taken), y.shape[0])
    ld = max([int(d.steps_taken) for d in decs] + [1])
    alphas = np.zeros((bv.s, ld))
    betas = np.zeros((bv.s, ld))
    yy = np.zeros((bv.s, ld))
    steps = (c_size_t * bv.s)()
    bnorms = np.zeros(bv.s)
    for c, (d, y) in enumerate(zip(decs, yl)):
        st = int(d.steps_taken)
        a = np.asarray(d.alphas, dtype=np.float64).reshape(-1)
        b = np.asarray(d.betas, dtype=np.float64).reshape(-1)
        if a.shape[0] < st or b.shape[0] + 1 < st:
            raise ValueError("decomposition arrays shorter than steps_taken")
        alphas[c, :st] = a[:st]
        betas[c, :max(st - 1, 0)] = b[:max(st - 1, 0)]
        yy[c, :st] = y
        steps[c] = st
        bnorms[c] = float(d.b_norm)
    x = bv.empty(bv.s, bv.n)
    check(_lib.tpl_lanczos_pass_two_batch(
        op.handle, bv.ptr, bv.n, bv.s, alphas.ctypes.data_as(POINTER(c_double)),
        betas.ctypes.data_as(POINTER(c_double)), ld, steps,
        bnorms.ctypes.data_as(POINTER(c_double)), yy.ctypes.data_as(POINTER(c_double)),
        Vec.ptr_of(x), bv.mem))
    return x.T


def lanczos_pass_two_batch_multi(operator, B, decompositions, Ys):
    """Second pass for m coefficient vectors per column of ``B`` in lock-step:
    ``decompositions[c]`` and ``Ys[c]`` (``steps_taken`` x m, column i = f_i(T_k) e_1 * ||b_c||)
    belong to ``B[:, c]``; every ``Ys[c]`` has the same m. Returns shape (n, m, s) with strides
    (1, n, n m); ``X[:, i, c]`` is bitwise ``lanczos_pass_two`` of ``B[:, c]`` with ``Ys[c][:, i]``."""
    bv = Cols(B)
    bv.check_rows(operator)
    decs, Ys = list(decompositions), list(Ys)
    if len(decs) != bv.s or len(Ys) != bv.s:
        raise ValueError("one decomposition and one Y per column of B")
    yl = [y.detach().double().cpu().numpy() if hasattr(y, "is_cuda")
          else np.asarray(y, dtype=np.float64) for y in Ys]
    if any(y.ndim != 2 for y in yl):
        raise ValueError("every Y must be a (steps, m) matrix")
    m = yl[0].shape[1]
    if m == 0 or any(y.shape[1] != m for y in yl):
        raise ValueError("every Y must hold the same number (at least one) of columns")
    for d, y in zip(decs, yl):  # the single call's check, per column in ascending order
        if int(d.steps_taken) != y.shape[0]:
            raise LanczosError.parameter_mismatch("y_k", int(d.steps_taken), y.shape[0])
    op = _op(operator)
    ld =max([int(d.steps_taken) for d in decs] + [1])
    alphas = np.zeros((bv.s, ld))
    betas = np.zeros((bv.s, ld))
    yy = np.zeros((bv.s, m, ld))  # column (c m + i) of the ld x (s m) table
    steps = (c_size_t * bv.s)()
    bnorms = np.zeros(bv.s)
    for c, (d, y) in enumerate(zip(decs, yl)):
        st = int(d.steps_taken)
        a = np.asarray(d.alphas, dtype=np.float64).reshape(-1)
        b = np.asarray(d.betas, dtype=np.float64).reshape(-1)
        if a.shape[0] < st or b.shape[0] + 1 < st:
            raise ValueError("decomposition arrays shorter than steps_taken")
        alphas[c, :st] = a[:st]
        betas[c, :max(st - 1, 0)] = b[:max(st - 1, 0)]
        yy[c, :, :st] = y.T
        steps[c] = st
        bnorms[c] = float(d.b_norm)
    x = bv.empty(bv.s, m, bv.n)
    check(_lib.tpl_lanczos_pass_two_batch_multi(
        op.handle, bv.ptr, bv.n, bv.s, alphas.ctypes.data_as(POINTER(c_double)),
        betas.ctypes.data_as(POINTER(c_double)), ld, steps,
        bnorms.ctypes.data_as(POINTER(c_double)), yy.ctypes.data_as(POINTER(c_double)), m,
        Vec.ptr_of(x), bv.mem))
    return x.permute(2, 1, 0) if hasattr(x, "permute") else x.transpose(2, 1, 0)


def lanczos_pass_two_batch_multi_cut(operator, B, decompositions, Ys, col_steps):
    """``lanczos_pass_two_batch_multi`` with a cut per (column, coefficient vector):
    ``col_steps[c][i]`` (1 <= it <= ``decompositions[c].steps_taken``) is the number of steps
    result (c, i) takes. ``X[:, i, c]`` is bitwise ``lanczos_pass_two`` of ``B[:, c]`` on
    ``decompositions[c]`` cut to that many steps with ``Ys[c][:col_steps[c][i], i]``; the
    entries of ``Ys[c][:, i]`` past the cut are never used. Returns shape (n, m, s)."""
    bv = Cols(B)
    bv.check_rows(operator)
    decs, Ys = list(decompositions), list(Ys)
    if len(decs) != bv.s or len(Ys) != bv.s:
        raise ValueError("one decomposition and one Y per column of B")
    yl = [y.detach().double().cpu().numpy() if hasattr(y, "is_cuda")
          else np.asarray(y, dtype=np.float64) for y in Ys]
    if any(y.ndim != 2 for y in yl):
        raise ValueError("every Y must be a (steps, m) matrix")
    m = yl[0].shape[1]
    if m == 0 or any(y.shape[1] != m for y in yl):
        raise ValueError("every Y must hold the same number (at least one) of columns")
    cs = np.asarray(col_steps, dtype=np.int64)
    if cs.shape != (bv.s, m):
        raise ValueError("col_steps must hold one count per (column, coefficient vector)")
    if np.any(cs < 0):
        raise ValueError("col_steps must not be negative")
    for d, y in zip(decs, yl):  # the single call's check, per column in ascending order
        if int(d.steps_taken) != y.shape[0]:
            raise LanczosError.parameter_mismatch("y_k", int(d.steps_taken), y.shape[0])
    op = _op(operator)
    ld = max([int(d.steps_taken) for d in decs] + [1])
    alphas = np.zeros((bv.s, ld))
    betas = np.zeros((bv.s, ld))
    yy = np.zeros((bv.s, m, ld))  # column (c m + i) of the ld x (s m) table
    steps = (c_size_t * bv.s)()
    counts = (c_size_t * (bv.s * m))(*[int(v) for v in cs.reshape(-1)])
    bnorms = np.zeros(bv.s)
    for c, (d, y) in enumerate(zip(decs, yl)):
        st = int(d.steps_taken)
        a = np.asarray(d.alphas, dtype=np.float64).reshape(-1)
        b = np.asarray(d.betas, dtype=np.float64).reshape(-1)
        if a.shape[0] < st or b.shape[0] + 1 < st:
            raise ValueError("decomposition arrays shorter than steps_taken")
        alphas[c, :st] = a[:st]
        betas[c, :max(st - 1, 0)] = b[:max(st - 1, 0)]
        yy[c, :, :st] = y.T
        steps[c] = st
        bnorms[c] = float(d.b_norm)
    x = bv.empty(bv.s, m, bv.n)
    check(_lib.tpl_lanczos_pass_two_batch_multi_cut(
        op.handle, bv.ptr, bv.n, bv.s, alphas.ctypes.data_as(POINTER(c_double)),
        betas.ctypes.data_as(POINTER(c_double)), ld, steps,
        bnorms.ctypes.data_as(POINTER(c_double)), yy.ctypes.data_as(POINTER(c_double)), counts, m,
        Vec.ptr_of(x), bv.mem))
    return x.permute(2, 1, 0) if hasattr(x, "permute") else x.transpose(2, 1, 0)
