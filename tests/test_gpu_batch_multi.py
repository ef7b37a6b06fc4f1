"""GPU: f_i(A) b_c for m functions and s right-hand sides in one run (include/tpl.h
tpl_lanczos_two_pass_batch_multi, tpl_lanczos_pass_two_batch_multi).

A group's pass two runs the batch step kernels with every record's nflush = 0 and
k_bp2_xacc<NB, M> (tpl_k_batch_multi.hip) applies the grouped flush to M functions of the NB
columns, operation for operation the single solve's x update. So the contract is BITWISE per
(column, function) against yardsticks that are never the path under test:
  (a) oracle.Operator(a, op.schedule())'s pass_one / pass_two per column and function, and
  (b) the single solve with f(T_k) on the host (set_device_ftk(0)), or lanczos_pass_two.
Every comparison is on 64-bit patterns, NaN positions required to agree; no tolerances.
"""
from ctypes import POINTER, c_double, c_size_t, c_void_p

import numpy as np
import pytest

from conftest import harness_b
from layout_cases import EDGES, VARIANTS, case
from test_gpu_batch import (host, oracle_columns, oracle_decomps, same_bits_nan, single_columns,
                            single_decomps, stopping_columns, tridiag)

pytestmark = pytest.mark.gpu

from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import (HipCsrOp, LanczosError, LanczosErrorKind, TplError, _lib,  # noqa: E402
                     algorithms as alg, ftk, solvers)

M_CAP = _lib.BATCH_MULTI_FUNCS  # functions per k_bp2_xacc launch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def _harmonic(al, be):
    return 1.0 / (1.0 + np.arange(len(al), dtype=np.float64))


def _alternating(al, be):
    return (-0.5) ** np.arange(len(al), dtype=np.float64)


# ftk.SQ, a closure, and inv_shift values: M_CAP + 1 of them
POOL = [ftk.SQ, _harmonic, ftk.inv_shift(1.0), ftk.inv_shift(2.0), ftk.inv_shift(3.0)]
assert len(POOL) == M_CAP + 1


def single_table(op, B, k, fs):
    """refs[c][i]: the single host-f solve of B[:, c] with fs[i]: (b)."""
    per_f = [single_columns(op, B, k, f) for f in fs]
    return [[per_f[i][c] for i in range(len(fs))] for c in range(B.shape[1])]


def oracle_table(a, op, B, k, fs):
    o, od = oracle_decomps(a, op, B, k)
    per_f = [oracle_columns(o, od, B, f) for f in fs]
    return [[per_f[i][c] for i in range(len(fs))] for c in range(B.shape[1])]


def check_table(X, refs, what):
    """X: (n, m, s) with strides (8, 8 n, 8 n m); refs[c][i] the expected X[:, i, c]."""
    X = host(X)
    n, s, m = refs[0][0].shape[0], len(refs), len(refs[0])
    assert X.shape == (n, m, s), (what, X.shape)
    if n > 1:
        assert X.strides[0] == 8 and (m == 1 or X.strides[1] == 8 * n), (what, X.strides)
        assert s == 1 or X.strides[2] == 8 * n * m, (what, X.strides)
    for c in range(s):
        for i in range(m):
            assert same_bits_nan(X[:, i, c], refs[c][i]), (what, "column", c, "function", i)


def sub(refs, cols, funcs):
    return [[refs[c][i] for i in funcs] for c in cols]


# ---- 1. group and launch shapes -----------------------------------------------------------
@pytest.fixture(scope="module")
def tri513():
    a = tridiag(513)
    B = np.stack([np.random.default_rng(17 + c).standard_normal(513) for c in range(9)], axis=1)
    return a, HipCsrOp(a), B


@pytest.mark.parametrize("k", range(1, 9))
def test_group_and_launch_shapes(k, tri513):
    """k = 1..8: steps = 1 is the prologue only, the rest reach every tail of the grouped
    flush. s = 1..5 and 9: both NB instances, a remainder of three, more than two groups.
    m = 1, 2, 3, M_CAP, M_CAP + 1: every M instance and a second launch per flush. The
    references are computed once per k for the nine columns and the five functions."""
    a, op, B = tri513
    xs = single_table(op, B, k, POOL)
    xo = oracle_table(a, op, B, k, POOL)
    for s in (1, 2, 3, 4, 5, 9):
        for m in (1, 2, 3, M_CAP, M_CAP + 1):
            X = solvers.lanczos_two_pass_batch_multi(op, B[:, :s], k, POOL[:m])
            check_table(X, sub(xs, range(s), range(m)), ("single", k, s, m))
            check_table(X, sub(xo, range(s), range(m)), ("oracle", k, s, m))


# ---- 2. row counts ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 257, 512, 2049])
def test_row_counts(n):
    """Odd n, a one-row last block, several element blocks; n = 1 and n = 2 break down
    before k. s = 3: a group of two and a multi-function solve."""
    a = tridiag(n)
    op = HipCsrOp(a)
    B = np.random.default_rng(100 + n).standard_normal((n, 3))
    fs = [ftk.SQ, _harmonic]
    X = solvers.lanczos_two_pass_batch_multi(op, B, 8, fs)
    check_table(X, single_table(op, B, 8, fs), ("single", n))
    check_table(X, oracle_table(a, op, B, 8, fs), ("oracle", n))


# ---- 3. columns that stop at different steps ------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_columns_stop_at_different_steps(reverse):
    """Steps 3, 2, 8, 1, 5: every column of the group of four applies its own flush counts
    and stops storing at its own step (an uncaptured launch list); the fifth column runs the
    multi-function path. The yardstick is lanczos_pass_two per (c, i)."""
    a, B = stopping_columns()
    steps = [3, 2, 8, 1, 5]
    if reverse:
        B, steps = np.ascontiguousarray(B[:, ::-1]), steps[::-1]
    op = HipCsrOp(a)
    decs = single_decomps(op, B, 8)
    assert [d.steps_taken for d in decs] == steps
    fs = [_harmonic, _alternating, ftk.SQ]

    def pass_two_refs(Ys):
        return [[host(alg.lanczos_pass_two(op, B[:, c].copy(), decs[c], Ys[c][:, i]))
                 for i in range(3)] for c in range(5)]
    Yf = [np.stack([np.asarray(f(d.alphas, d.betas), dtype=np.float64) * d.b_norm for f in fs],
                   axis=1) for d in decs]
    X = solvers.lanczos_two_pass_batch_multi(op, B, 8, fs)
    check_table(X, pass_two_refs(Yf), ("high level", reverse))
    check_table(X, single_table(op, B, 8, fs), ("single", reverse))
    rng = np.random.default_rng(5)
    Yr = [rng.standard_normal((d.steps_taken, 3)) for d in decs]
    Xl = alg.lanczos_pass_two_batch_multi(op, B, decs, Yr)
    check_table(Xl, pass_two_refs(Yr), ("low level", reverse))
    # one function through the fused path (the high-level call takes the batch path there)
    Y1 = [y[:, :1] for y in Yr]
    check_table(alg.lanczos_pass_two_batch_multi(op, B, decs, Y1),
                sub(pass_two_refs(Yr), range(5), [0]), ("low level m = 1", reverse))


# ---- 4. independence ------------------------------------------------------------------------
def test_independence(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(40 + c).standard_normal(n) for c in range(4)], axis=1)
    k = 50
    fs = [ftk.SQ, ftk.inv_shift(1.0), _harmonic]
    X = host(solvers.lanczos_two_pass_batch_multi(op, B, k, fs))
    ref = [[X[:, i, c].copy() for i in range(3)] for c in range(4)]
    check_table(X, single_table(op, B, k, fs), "single")
    two = solvers.lanczos_two_pass_batch_multi
    check_table(two(op, B[:, [2, 0]], k, fs), sub(ref, [2, 0], range(3)), "b2 b0")
    check_table(two(op, B[:, [3, 1, 0]], k, fs), sub(ref, [3, 1, 0], range(3)), "b3 b1 b0")
    check_table(two(op, B, k, [fs[2], fs[0]]), sub(ref, range(4), [2, 0]), "f2 f0")
    check_table(two(op, B[:, [1]], k, fs), sub(ref, [1], range(3)), "b1")
    check_table(two(op, B, k, fs), ref, "twice")


# ---- 5. a bad column leaves its neighbours alone ---------------------------------------------
@pytest.mark.parametrize("s", [3, 4])
def test_bad_column_leaves_its_neighbours_alone(kkt5k, s):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([std_rng_vector(n), harness_b(a), np.random.default_rng(8).standard_normal(n),
                  np.random.default_rng(9).standard_normal(n)][:s], axis=1)
    fs = [ftk.INV, ftk.SQ, ftk.INV]
    refs = single_table(op, B, 5, fs)
    assert not np.all(np.isfinite(refs[1][0])) and not np.all(np.isfinite(refs[1][2]))
    for c in (0, 2):
        assert all(np.all(np.isfinite(r)) for r in refs[c])
    check_table(solvers.lanczos_two_pass_batch_multi(op, B, 5, fs), refs, "single")


# ---- 6. real layouts ------------------------------------------------------------------------
def test_kkt5k_reordered_host_and_device_B(kkt5k):
    import torch
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(60 + c).standard_normal(n) for c in range(4)], axis=1)
    fs = [ftk.INV, ftk.SQ]
    for reorder in (2, 0):
        op.set_reorder(reorder)
        assert (op.schedule()["perm"] is not None) == (reorder == 2)
        refs = single_table(op, B, 20, fs)
        X = solvers.lanczos_two_pass_batch_multi(op, B, 20, fs)
        assert isinstance(X, np.ndarray) and X.shape == (n, 2, 4)
        assert X.strides == (8, 8 * n, 16 * n)
        check_table(X, refs, ("host B", reorder))
        check_table(X, oracle_table(a, op, B, 20, fs), ("oracle", reorder))
        Xd = solvers.lanczos_two_pass_batch_multi(op, torch.from_numpy(B).cuda(), 20, fs)
        assert Xd.is_cuda and tuple(Xd.shape) == (n, 2, 4) and Xd.stride() == (1, n, 2 * n)
        check_table(Xd, refs, ("device B", reorder))


# ---- 7. layouts -------------------------------------------------------------------------------
I8_COL16 = "F056"  # int8 values, uint16 chunk and bin columns


@pytest.mark.parametrize("s", [3, 4])
@pytest.mark.parametrize("name", sorted(EDGES) + [I8_COL16])
def test_layouts(name, s):
    """The step kernels are the batch solve's own instances; what is new per layout is the
    element grid of k_bp2_minit / k_bp2_xacc over that layout's row blocks and the ring they
    read. s = 3: the NB = 2 instances and a multi-function solve, s = 4: the NB = 4 ones."""
    c = case(name)
    if name == I8_COL16:
        assert VARIANTS[name] & 8 and VARIANTS[name] & 16
    op = HipCsrOp(c.a)
    c.apply_setters(op)
    assert op.kernel_variant() == c.F
    B = np.random.default_rng(5).standard_normal((c.a.shape[0], s))
    fs = [ftk.SQ, _harmonic]
    X = solvers.lanczos_two_pass_batch_multi(op, B, 4, fs)
    check_table(X, single_table(op, B, 4, fs), (name, s, "single"))
    if name in EDGES:
        check_table(X, oracle_table(c.a, op, B, 4, fs), (name, s, "oracle"))


# ---- 8. state ---------------------------------------------------------------------------------
def test_buffers_graphs_and_rebuilds(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(90 + c).standard_normal(n) for c in range(4)], axis=1)
    k = 50
    fs = [ftk.SQ, ftk.inv_shift(1.0), _harmonic]
    refs = single_table(op, B, k, fs)
    two = solvers.lanczos_two_pass_batch_multi
    # the parents' buffers first (a group's batch vectors, a single column's multi vectors),
    # so that the growth below is the group's m result vectors' own
    solvers.lanczos_two_pass_batch(op, B, k, ftk.SQ)
    solvers.lanczos_two_pass_multi(op, B[:, 0].copy(), k, fs)
    bytes0 = op.device_bytes()
    check_table(two(op, B, k, fs), refs, "s = 4, m = 3")
    assert not op.flags() & 32
    grown = op.device_bytes() - bytes0
    assert grown >= 3 * 4 * 8 * n  # m group vectors of n x NB
    check_table(two(op, B[:, :2], k, fs[:2]), sub(refs, range(2), range(2)), "s = 2, m = 2")
    check_table(two(op, B[:, :3], k, fs[:2]), sub(refs, range(3), range(2)), "s = 3, m = 2")
    assert op.device_bytes() - bytes0 == grown
    check_table(two(op, B, k, fs), refs, "again")
    for method, kw in (("set_slices", {"slices": 2}), ("set_reorder", {"mode": 0}),
                       ("set_value_format", {"compress": False})):
        getattr(op, method)(**kw)
        check_table(two(op, B, k, fs), single_table(op, B, k, fs), method)
    assert not op.flags() & 32


# ---- 9. errors --------------------------------------------------------------------------------
def test_errors(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.random.default_rng(11).standard_normal((n, 3))
    Bc = np.ascontiguousarray(B.T)
    x = np.zeros((3 * 2, n))
    al, be, yy = np.full((3, 5), 2.0), np.ones((3, 5)), np.ones((3 * 2, 5))
    st, bn = (c_size_t * 3)(5, 5, 5), np.ones(3)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    H, BAD = _lib.TPL_MEM_HOST, _lib.TPL_ERR_INVALID_ARGUMENT
    fp = (c_void_p * 2)(_lib.FTK_SQ_PTR, _lib.FTK_SQ_PTR)
    two, p2 = _lib.tpl_lanczos_two_pass_batch_multi, _lib.tpl_lanczos_pass_two_batch_multi
    Bp, xp = Bc.ctypes.data, x.ctypes.data
    for s, m in ((0, 2), (65, 2), (3, 0), (3, 65)):
        assert two(op.handle, Bp, n, s, 5, fp, None, m, xp, H) == BAD, (s, m)
        assert p2(op.handle, Bp, n, s, pd(al), pd(be), 5, st, pd(bn), pd(yy), m, xp, H) == BAD, (s, m)
    assert two(op.handle, None, n, 3, 5, fp, None, 2, xp, H) == BAD
    assert two(op.handle, Bp, n, 3, 5, None, None, 2, xp, H) == BAD
    assert two(op.handle, Bp, n, 3, 5, fp, None, 2, None, H) == BAD
    assert p2(op.handle, None, n, 3, pd(al), pd(be), 5, st, pd(bn), pd(yy), 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), pd(be), 5, st, pd(bn), pd(yy), 2, None, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), pd(be), 5, None, pd(bn), pd(yy), 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), pd(be), 5, st, None, pd(yy), 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, None, pd(be), 5, st, pd(bn), pd(yy), 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), None, 5, st, pd(bn), pd(yy), 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), pd(be), 5, st, pd(bn), None, 2, xp, H) == BAD
    assert p2(op.handle, Bp, n, 3, pd(al), pd(be), 4, st, pd(bn), pd(yy), 2, xp, H) == BAD  # ld < steps
    with pytest.raises(TplError) as t:
        solvers.lanczos_two_pass_batch_multi(op, np.ones((n, 65)), 5, [ftk.SQ, ftk.SQ])
    assert t.value.status == BAD
    with pytest.raises(TplError) as t:
        solvers.lanczos_two_pass_batch_multi(op, B, 5, [ftk.SQ] * 65)
    assert t.value.status == BAD

    fs = [ftk.SQ, _harmonic]
    Bz = B.copy()
    Bz[:, 1] = 0.0
    zero_text = "Invalid input parameter: Input vector `b` must not be a zero vector."
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch_multi(op, Bz, 5, fs)
    assert str(e.value) == zero_text
    with pytest.raises(LanczosError) as e1:
        solvers.lanczos_two_pass(op, np.zeros(n), 5, ftk.SQ)
    assert str(e1.value) == zero_text

    calls = []

    def logged(i, fail_at=None):
        def f(al_, be_):
            calls.append((i, len(al_)))
            if len(calls) == fail_at:
                raise RuntimeError("boom")
            return np.ones(len(al_))
        return f
    # the (c = 1, i = 1) call is the fourth: (0, 0), (0, 1), (1, 0) ran before it
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch_multi(op, B, 5, [logged(0, 4), logged(1, 4)])
    assert str(e.value) == "The user-provided f(T_k) solver failed: boom"
    assert e.value.kind == LanczosErrorKind.SOLVER_ERROR
    assert calls == [(0, 5), (1, 5), (0, 5), (1, 5)]
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch_multi(op, B, 5,
                                             [ftk.SQ, lambda al_, be_: np.ones(len(al_) + 1)])
    assert str(e.value) == "Parameter mismatch: `y_k_prime` expects size 5, but got 6."
    # the low-level call: a y of the wrong length, with the single call's text
    decs = single_decomps(op, B, 5)
    Ys = [np.ones((5, 2)), np.ones((4, 2)), np.ones((5, 2))]
    with pytest.raises(LanczosError) as e:
        alg.lanczos_pass_two_batch_multi(op, B, decs, Ys)
    assert str(e.value) == "Parameter mismatch: `y_k` expects size 5, but got 4."
    with pytest.raises(LanczosError) as e1:
        alg.lanczos_pass_two(op, B[:, 1].copy(), decs[1], np.ones(4))
    assert str(e1.value) == str(e.value)
    # the operator is still usable after the failed calls
    check_table(solvers.lanczos_two_pass_batch_multi(op, B, 6, fs), single_table(op, B, 6, fs),
                "after errors")
    B4 = np.random.default_rng(13).standard_normal((n, 4))
    check_table(solvers.lanczos_two_pass_batch_multi(op, B4, 6, fs), single_table(op, B4, 6, fs),
                "after errors, a group of four")
