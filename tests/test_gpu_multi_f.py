"""GPU: f_1(A) b ... f_m(A) b in one two-pass Lanczos run (include/tpl.h
tpl_lanczos_two_pass_multi, tpl_lanczos_multi, tpl_lanczos_pass_two_multi).

Pass one and the basis pass two regenerates are shared; k_p2_xacc applies each column's x
updates with the single solve's operations in its order (tpl_k_multi.hip), so the contract
is BITWISE, per column i, against two yardsticks that are never the multi path itself:
  (a) the canonical oracle's pass two on y_i = ||b|| f_i(T_k) e_1, and
  (b) the single solve solvers.lanczos_two_pass(op, b, k, f_i) with f(T_k) on the host.
NaN positions must agree (a singular T_k gives non-finite columns; a NaN's encoding may
differ between host and device), every other value is compared as a 64-bit pattern.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import harness_b

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import (HipCsrOp, LanczosError, LanczosErrorKind, TplError, _lib,  # noqa: E402
                     algorithms as alg, ftk, solvers)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same_bits_nan(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    nx, ny = np.isnan(x), np.isnan(y)
    return (x.shape == y.shape and np.array_equal(nx, ny)
            and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))


def _harmonic(al, be):
    return 1.0 / (1.0 + np.arange(len(al), dtype=np.float64))


# drawn in turn: column i of an m-column solve uses FUNCS[i % 6]
FUNCS = [ftk.INV, ftk.SQ, ftk.EXP, ftk.exp_t(0.5), ftk.inv_shift(1.0), _harmonic]


def funcs(m):
    return [FUNCS[i % len(FUNCS)] for i in range(m)]


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "is_cuda") else x


def oracle_columns(a, op, b, k, fs):
    """(steps, [x_i]) by the oracle in the operator's reduction order: comparison (a)."""
    o = oracle.Operator(a, op.schedule())
    al, be, st, bn, _ = o.pass_one(b, k)
    cols = []
    for f in fs:
        yp = np.asarray(f(al, be), dtype=np.float64).reshape(-1)
        cols.append(o.pass_two(b, al, be, st, bn, yp * bn)[0])
    return st, cols


def single_columns(op, b, k, fs):
    """[x_i] by the single solve with f(T_k) on the host: comparison (b)."""
    op.set_device_ftk(0)
    try:
        return [host(solvers.lanczos_two_pass(op, b, k, f)) for f in fs]
    finally:
        op.set_device_ftk(2)


def check_columns(X, refs, what):
    X = host(X)
    assert X.shape == (refs[0].shape[0], len(refs)), what
    assert X.strides == (8, 8 * X.shape[0]), what  # column-major, leading dimension n
    for i, r in enumerate(refs):
        assert same_bits_nan(X[:, i], r), (what, i)


def tridiag(n):
    return sp.diags([np.full(n - 1, -1.0), 2.5 + np.arange(n) / n, np.full(n - 1, -1.0)],
                    [-1, 0, 1], shape=(n, n)).tocsr()


# ---- 1. residues and column counts ---------------------------------------------------
@pytest.fixture(scope="module")
def tri513():
    a = tridiag(513)
    return a, HipCsrOp(a), np.random.default_rng(17).standard_normal(513)


@pytest.mark.parametrize("k", range(1, 9))
def test_every_flush_tail_and_column_count(k, tri513):
    """k = 1..8: every tail of the grouped flush, and steps = 1 (prologue only). m = 1..9:
    every k_p2_xacc<M> instance and the 8 + 1 split. The references are computed once per k
    for the nine function slots; an m-column solve is checked against the first m."""
    a, op, b = tri513
    fs = funcs(9)
    st, xo = oracle_columns(a, op, b, k, fs)
    assert st == k
    xs = single_columns(op, b, k, fs)
    for m in range(1, 10):
        X = solvers.lanczos_two_pass_multi(op, b, k, fs[:m])
        check_columns(X, xo[:m], ("oracle", k, m))
        check_columns(X, xs[:m], ("single", k, m))


# ---- 2. shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 257, 511, 512, 2049])
def test_shapes(n):
    """Odd n, a one-row last block, single and several element blocks; n = 1 and n = 2
    break down before k."""
    a = tridiag(n)
    op = HipCsrOp(a)
    b = np.random.default_rng(100 + n).standard_normal(n)
    k, fs = 8, funcs(3)
    st, xo = oracle_columns(a, op, b, k, fs)
    assert st == min(k, n) if n <= 2 else st == k
    X = solvers.lanczos_two_pass_multi(op, b, k, fs)
    check_columns(X, xo, ("oracle", n))
    check_columns(X, single_columns(op, b, k, fs), ("single", n))


# ---- 3. real layouts ----------------------------------------------------------------------
def test_kkt5k_reordered_host_and_device_b(kkt5k):
    """Locality order on (the default at this size), long rows, int8 values; a host b, then
    the same b on the device (X comes back as a torch tensor, strides (1, n)); then the
    caller's order."""
    import torch
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    b = std_rng_vector(n)
    k, fs = 50, [ftk.INV, ftk.SQ, ftk.exp_t(1e-3), ftk.inv_shift(2.0)]
    for reorder in (2, 0):
        op.set_reorder(reorder)
        assert (op.schedule()["perm"] is not None) == (reorder == 2)
        st, xo = oracle_columns(a, op, b, k, fs)
        assert st == k
        xs = single_columns(op, b, k, fs)
        X = solvers.lanczos_two_pass_multi(op, b, k, fs)
        check_columns(X, xo, ("oracle", reorder))
        check_columns(X, xs, ("single", reorder))
        if reorder == 2:
            Xd = solvers.lanczos_two_pass_multi(op, torch.from_numpy(b).cuda(), k, fs)
            assert Xd.is_cuda and tuple(Xd.shape) == (n, 4) and Xd.stride() == (1, n)
            check_columns(Xd, xo, "device b")


def skewed_matrix(n=12000, seed=7):
    """Short rows, long rows of 40..900 nnz and three 6000-nnz hubs (sliced), general
    (non +-1) values and a diagonal (the matrix family of tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        c = rng.integers(0, 4)
        rows += [i] * c
        cols += list(rng.integers(0, n, size=c))
    for h in range(50, 70):
        c = rng.choice(n, size=int(rng.integers(40, 900)), replace=False)
        rows += [h] * len(c)
        cols += list(c)
    for h in (100, 5000, 11000):
        c = rng.choice(n, size=6000, replace=False)
        rows += [h] * len(c)
        cols += list(c)
    vals = rng.standard_normal(len(rows))
    s = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    a = (s + s.T + sp.diags(rng.uniform(1, 2, n))).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def test_skewed_general_values():
    a = skewed_matrix()
    op = HipCsrOp(a)
    b = np.random.default_rng(3).standard_normal(a.shape[0])
    k, fs = 20, [ftk.INV, ftk.SQ]
    st, xo = oracle_columns(a, op, b, k, fs)
    assert st == k
    X = solvers.lanczos_two_pass_multi(op, b, k, fs)
    check_columns(X, xo, "oracle")
    check_columns(X, single_columns(op, b, k, fs), "single")


# ---- 4. breakdown -----------------------------------------------------------------------------
def test_breakdown_truncates_every_column():
    """Three distinct eigenvalues: the Krylov space is exhausted after 3 steps (beta_3 =
    1.1e-15 in exact data, under the 2.2e-13 tolerance), so steps_taken = 3 < k = 6."""
    a = sp.diags(np.tile([1.0, 2.0, 4.0], 200)).tocsr()
    op = HipCsrOp(a)
    b = np.ones(600)
    fs = funcs(6)
    st, xo = oracle_columns(a, op, b, 6, fs)
    assert st == 3
    X = solvers.lanczos_two_pass_multi(op, b, 6, fs)
    check_columns(X, xo, "oracle")
    check_columns(X, single_columns(op, b, 6, fs), "single")


# ---- 5. isolation of a bad column -----------------------------------------------------------
def test_non_finite_column_leaves_its_neighbours_alone(kkt5k):
    """Harness b on the KKT matrix gives alpha = 0, so an odd k makes T_k singular: the INV
    column is non-finite, and the SQ columns on either side must be untouched by it."""
    a = kkt5k.a
    op = HipCsrOp(a)
    b = harness_b(a)
    fs = [ftk.SQ, ftk.INV, ftk.SQ]
    xs = single_columns(op, b, 5, fs)
    assert not np.all(np.isfinite(xs[1]))
    assert np.all(np.isfinite(xs[0])) and np.all(np.isfinite(xs[2]))
    X = solvers.lanczos_two_pass_multi(op, b, 5, fs)
    check_columns(X, xs, "single")


# ---- 6. low level --------------------------------------------------------------------------
def test_pass_two_multi_low_level(kkt5k):
    a = kkt5k.a
    op = HipCsrOp(a)
    b = std_rng_vector(a.shape[0])
    o = oracle.Operator(a, op.schedule())
    al, be, st, bn, _ = o.pass_one(b, 7)
    assert st == 7
    d = alg.LanczosDecomposition(al, be, st, bn)
    Y = np.random.default_rng(5).standard_normal((st, 3))
    X = alg.lanczos_pass_two_multi(op, b, d, Y)
    check_columns(X, [o.pass_two(b, al, be, st, bn, Y[:, i])[0] for i in range(3)], "oracle")
    check_columns(X, [alg.lanczos_pass_two(op, b, d, Y[:, i]) for i in range(3)], "single")
    with pytest.raises(LanczosError) as e:
        alg.lanczos_pass_two_multi(op, b, d, Y[:-1])
    assert str(e.value) == "Parameter mismatch: `y_k` expects size 7, but got 6."


# ---- 7. one-pass sibling ----------------------------------------------------------------
def test_one_pass_sibling(kkt5k):
    a = kkt5k.a
    op = HipCsrOp(a)
    b = std_rng_vector(a.shape[0])
    fs = [ftk.INV, ftk.SQ, ftk.inv_shift(1.0)]
    op.set_device_ftk(0)
    xs = [solvers.lanczos(op, b, 30, f) for f in fs]
    op.set_device_ftk(2)
    X = solvers.lanczos_multi(op, b, 30, fs)
    check_columns(X, xs, "lanczos")
    assert not op.flags() & 32


# ---- 8. graph cache and state ---------------------------------------------------------------
def test_graph_cache_buffers_and_state(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    b1, b2 = std_rng_vector(n), np.random.default_rng(9).standard_normal(n)
    k, fs = 50, funcs(5)
    x_default = solvers.lanczos_two_pass(op, b1, k, ftk.INV)  # before any multi call
    ref1, ref2 = single_columns(op, b1, k, fs), single_columns(op, b2, k, fs)
    bytes0 = op.device_bytes()
    X2 = solvers.lanczos_two_pass_multi(op, b1, k, fs[:2])  # captures the (k, 2) graph
    check_columns(X2, ref1[:2], "capture")
    assert not op.flags() & 32
    assert op.device_bytes() - bytes0 >= 8 * n * 2
    check_columns(solvers.lanczos_two_pass_multi(op, b2, k, fs[:2]), ref2[:2], "replay")
    check_columns(solvers.lanczos_two_pass_multi(op, b1, k, fs), ref1, "grown to 5")
    check_columns(solvers.lanczos_two_pass_multi(op, b1, k, fs[:2]), ref1[:2], "back to 2")
    grown = op.device_bytes() - bytes0
    assert 8 * n * 5 <= grown < 8 * n * k  # five result vectors and the table, no basis
    assert same_bits_nan(solvers.lanczos_two_pass(op, b1, k, ftk.INV), x_default)
    solvers.lanczos(op, b1, k, ftk.SQ)  # allocates the basis: the cached graphs are dropped
    check_columns(solvers.lanczos_two_pass_multi(op, b1, k, fs[:2]), ref1[:2], "after lanczos")


# ---- 9. errors through the ABI -----------------------------------------------------------------
def test_errors(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    b = std_rng_vector(n)
    x = np.zeros((2, n))
    one = (ctypes.c_void_p * 1)(_lib.FTK_SQ_PTR)
    for fn in (_lib.tpl_lanczos_two_pass_multi, _lib.tpl_lanczos_multi):
        assert fn(op.handle, b.ctypes.data, n, 5, one, None, 0, x.ctypes.data,
                  _lib.TPL_MEM_HOST) == _lib.TPL_ERR_INVALID_ARGUMENT
        assert fn(op.handle, b.ctypes.data, n, 5, None, None, 1, x.ctypes.data,
                  _lib.TPL_MEM_HOST) == _lib.TPL_ERR_INVALID_ARGUMENT
        assert fn(op.handle, b.ctypes.data, n, 5, one, None, 1, None,
                  _lib.TPL_MEM_HOST) == _lib.TPL_ERR_INVALID_ARGUMENT
    for solve in (solvers.lanczos_two_pass_multi, solvers.lanczos_multi):
        with pytest.raises(TplError) as t:
            solve(op, b, 5, [ftk.SQ] * 65)
        assert t.value.status == _lib.TPL_ERR_INVALID_ARGUMENT
        assert solve(op, b, 5, [ftk.SQ] * 64).shape == (n, 64)

        def boom(al, be):
            raise RuntimeError("boom")

        def boom2(al, be):
            raise RuntimeError("second")
        with pytest.raises(LanczosError) as e:
            solve(op, b, 5, [ftk.SQ, boom, ftk.INV])
        assert str(e.value) == "The user-provided f(T_k) solver failed: boom"
        assert e.value.kind == LanczosErrorKind.SOLVER_ERROR
        with pytest.raises(LanczosError) as e:
            solve(op, b, 5, [ftk.SQ, lambda al, be: np.ones(len(al) + 1)])
        assert str(e.value) == "Parameter mismatch: `y_k_prime` expects size 5, but got 6."
        with pytest.raises(LanczosError) as e:
            solve(op, b, 5, [ftk.SQ, lambda al, be: np.ones((len(al), 2)), ftk.INV])
        assert e.value.kind == LanczosErrorKind.PARAMETER_MISMATCH
        assert e.value.payload["param_name"] == "y_k_prime" and e.value.payload["expected"] == 5
        with pytest.raises(LanczosError) as e:
            solve(op, np.zeros(n), 5, [ftk.SQ, ftk.INV])
        assert str(e.value) == "Invalid input parameter: Input vector `b` must not be a zero vector."
        with pytest.raises(LanczosError) as e:  # two failing functions: the first one's error
            solve(op, b, 5, [ftk.SQ, boom, boom2])
        assert str(e.value) == "The user-provided f(T_k) solver failed: boom"
        with pytest.raises(LanczosError) as e:
            solve(op, b, 5, [boom2, lambda al, be: np.ones(1)])
        assert str(e.value) == "The user-provided f(T_k) solver failed: second"
    # the operator is still usable after the failed calls
    check_columns(solvers.lanczos_two_pass_multi(op, b, 6, [ftk.SQ]),
                  single_columns(op, b, 6, [ftk.SQ]), "after errors")
