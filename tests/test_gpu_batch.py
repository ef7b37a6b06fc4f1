"""GPU: f(A) b_1 ... f(A) b_s in one lock-step two-pass Lanczos run (include/tpl.h
tpl_lanczos_two_pass_batch, tpl_lanczos_pass_one_batch, tpl_lanczos_pass_two_batch).

The batch kernels (tpl_k_batch_p1.hip, tpl_k_batch_p2.hip) run NB = 2 or 4 recurrences per
launch over interleaved vectors and perform, per column, the single-column kernels'
operations in their order, so the contract is BITWISE per column against two yardsticks that
are never the batch path itself:
  (a) oracle.Operator(a, op.schedule())'s pass_one / pass_two per column, and
  (b) the single solve with f(T_k) on the host (set_device_ftk(0)).
Every comparison is on 64-bit patterns, NaN positions required to agree; no tolerances.
"""
import ctypes
from ctypes import POINTER, c_double, c_size_t

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import harness_b
from layout_cases import EDGES, VARIANTS, WIDE, case
from test_gpu_multi_f import skewed_matrix

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


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "is_cuda") else x


def tridiag(n):
    return sp.diags([np.full(n - 1, -1.0), 2.5 + np.arange(n) / n, np.full(n - 1, -1.0)],
                    [-1, 0, 1], shape=(n, n)).tocsr()


def _harmonic(al, be):
    return 1.0 / (1.0 + np.arange(len(al), dtype=np.float64))


def oracle_decomps(a, op, B, k):
    """Per column (al, be, steps, ||b||) by the oracle in the operator's order: (a)."""
    o = oracle.Operator(a, op.schedule())
    return o, [o.pass_one(np.ascontiguousarray(B[:, c]), k)[:4] for c in range(B.shape[1])]


def oracle_columns(o, decs, B, f):
    out = []
    for c, (al, be, st, bn) in enumerate(decs):
        yp = np.asarray(f(al, be), dtype=np.float64).reshape(-1)
        out.append(o.pass_two(np.ascontiguousarray(B[:, c]), al, be, st, bn, yp * bn)[0])
    return out


def single_columns(op, B, k, f):
    """[x_c] by the single solve with f(T_k) on the host: (b)."""
    op.set_device_ftk(0)
    try:
        return [host(solvers.lanczos_two_pass(op, np.ascontiguousarray(B[:, c]), k, f))
                for c in range(B.shape[1])]
    finally:
        op.set_device_ftk(2)


def single_decomps(op, B, k):
    return [alg.lanczos_pass_one(op, np.ascontiguousarray(B[:, c]), k) for c in range(B.shape[1])]


def check_columns(X, refs, what):
    X = host(X)
    assert X.shape == (refs[0].shape[0], len(refs)), what
    assert X.strides == (8, 8 * X.shape[0]) or X.shape[0] == 1, what  # column-major, ld = n
    for c, r in enumerate(refs):
        assert same_bits_nan(X[:, c], r), (what, c)


def check_decomps(got, refs, what):
    """got: LanczosDecomposition list; refs: (al, be, st, bn) tuples or decompositions."""
    assert len(got) == len(refs), what
    for c, (d, r) in enumerate(zip(got, refs)):
        if not isinstance(r, tuple):
            r = (r.alphas, r.betas, r.steps_taken, r.b_norm)
        al, be, st, bn = r
        assert d.steps_taken == st, (what, c, d.steps_taken, st)
        assert same_bits_nan(d.alphas, np.asarray(al)[:st]), (what, c, "alphas")
        assert same_bits_nan(d.betas, np.asarray(be)[:max(st - 1, 0)]), (what, c, "betas")
        assert same_bits_nan(np.array([d.b_norm]), np.array([bn])), (what, c, "b_norm")


def check_all(a, op, B, k, f, what, with_oracle=True):
    """pass_one_batch and two_pass_batch of B against both yardsticks."""
    decs = alg.lanczos_pass_one_batch(op, B, k)
    check_decomps(decs, single_decomps(op, B, k), (what, "single p1"))
    X = solvers.lanczos_two_pass_batch(op, B, k, f)
    check_columns(X, single_columns(op, B, k, f), (what, "single"))
    if with_oracle:
        o, od = oracle_decomps(a, op, B, k)
        check_decomps(decs, od, (what, "oracle p1"))
        check_columns(X, oracle_columns(o, od, B, f), (what, "oracle"))
    return decs, X


# ---- 1. group shapes ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tri513():
    a = tridiag(513)
    B = np.stack([np.random.default_rng(17 + c).standard_normal(513) for c in range(9)], axis=1)
    return a, HipCsrOp(a), B


@pytest.mark.parametrize("k", range(1, 9))
def test_group_shapes(k, tri513):
    """k = 1..8: steps = 1 is the prologue only, the rest reach every tail of the grouped
    flush. s = 1..9: the NB = 2 and NB = 4 instances, every remainder, more than two groups.
    The references are computed once per k for the nine columns."""
    a, op, B = tri513
    o, od = oracle_decomps(a, op, B, k)
    assert [d[2] for d in od] == [k] * 9
    sd = single_decomps(op, B, k)
    refs = {}
    for name, f in (("sq", ftk.SQ), ("closure", _harmonic)):
        refs[name] = (f, oracle_columns(o, od, B, f), single_columns(op, B, k, f))
    for s in range(1, 10):
        decs = alg.lanczos_pass_one_batch(op, B[:, :s], k)
        check_decomps(decs, od[:s], ("oracle p1", k, s))
        check_decomps(decs, sd[:s], ("single p1", k, s))
        for name, (f, xo, xs) in refs.items():
            X = solvers.lanczos_two_pass_batch(op, B[:, :s], k, f)
            check_columns(X, xo[:s], ("oracle", name, k, s))
            check_columns(X, xs[:s], ("single", name, k, s))


# ---- 2. row counts --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 257, 511, 512, 2049])
def test_row_counts(n):
    """Odd n, a one-row last block, several element blocks; n = 1 and n = 2 break down
    before k."""
    a = tridiag(n)
    op = HipCsrOp(a)
    B = np.random.default_rng(100 + n).standard_normal((n, 3))
    decs, _ = check_all(a, op, B, 8, ftk.SQ, n)
    assert [d.steps_taken for d in decs] == [min(8, n) if n <= 2 else 8] * 3


# ---- 3. columns that stop at different steps ------------------------------------------------
def stopping_columns():
    n = 600
    a = sp.diags(np.arange(1.0, n + 1)).tocsr()
    rng = np.random.default_rng(21)
    B = np.zeros((n, 5))
    for c, support in enumerate([(5, 300, 599), (17, 411), None, (88,), (1, 2, 3, 4, 5)]):
        if support is None:
            B[:, c] = rng.standard_normal(n)
        else:
            for i in support:
                B[i, c] = rng.standard_normal()
    return a, B


@pytest.mark.parametrize("reverse", [False, True])
def test_columns_stop_at_different_steps(reverse):
    a, B = stopping_columns()
    op = HipCsrOp(a)
    o, od = oracle_decomps(a, op, B, 8)
    assert [d[2] for d in od] == [3, 2, 8, 1, 5]
    if reverse:
        B = np.ascontiguousarray(B[:, ::-1])
    decs, _ = check_all(a, op, B, 8, ftk.SQ, ("stop", reverse))
    assert [d.steps_taken for d in decs] == ([3, 2, 8, 1, 5][::-1] if reverse else [3, 2, 8, 1, 5])


# ---- 4. independence ------------------------------------------------------------------------
def test_independence(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(40 + c).standard_normal(n) for c in range(4)], axis=1)
    k = 50
    xs = single_columns(op, B, k, ftk.SQ)
    X4 = solvers.lanczos_two_pass_batch(op, B, k, ftk.SQ)
    check_columns(X4, xs, "b0 b1 b2 b3")
    check_columns(solvers.lanczos_two_pass_batch(op, B[:, [2, 0]], k, ftk.SQ), [xs[2], xs[0]],
                  "b2 b0")
    check_columns(solvers.lanczos_two_pass_batch(op, B[:, [3]], k, ftk.SQ), [xs[3]], "b3")
    op.set_device_ftk(0)
    x1 = solvers.lanczos_two_pass(op, B[:, 1].copy(), k, ftk.SQ)
    op.set_device_ftk(2)
    assert same_bits_nan(x1, xs[1])
    check_columns(solvers.lanczos_two_pass_batch(op, B, k, ftk.SQ), xs, "twice")


# ---- 5. a bad column leaves its neighbours alone ---------------------------------------------
def test_bad_column_leaves_its_neighbours_alone(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([std_rng_vector(n), harness_b(a), np.random.default_rng(8).standard_normal(n)],
                 axis=1)
    xs = single_columns(op, B, 5, ftk.INV)
    assert not np.all(np.isfinite(xs[1]))
    assert np.all(np.isfinite(xs[0])) and np.all(np.isfinite(xs[2]))
    check_columns(solvers.lanczos_two_pass_batch(op, B, 5, ftk.INV), xs, "single")


# ---- 6. real layouts ------------------------------------------------------------------------
def test_kkt5k_reordered_host_and_device_B(kkt5k):
    import torch
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(60 + c).standard_normal(n) for c in range(4)], axis=1)
    for reorder in (2, 0):
        op.set_reorder(reorder)
        assert (op.schedule()["perm"] is not None) == (reorder == 2)
        _, X = check_all(a, op, B, 20, ftk.INV, ("kkt", reorder))
        Xd = solvers.lanczos_two_pass_batch(op, torch.from_numpy(B).cuda(), 20, ftk.INV)
        assert Xd.is_cuda and tuple(Xd.shape) == (n, 4) and Xd.stride() == (1, n)
        check_columns(Xd, [host(X)[:, c] for c in range(4)], "device B")


def test_skewed_general_values():
    a = skewed_matrix()
    op = HipCsrOp(a)
    B = np.random.default_rng(3).standard_normal((a.shape[0], 4))
    check_all(a, op, B, 20, ftk.SQ, "skewed")


# ---- 7. every layout instance -----------------------------------------------------------------
@pytest.mark.parametrize("s", [3, 4])
@pytest.mark.parametrize("name", sorted(VARIANTS) + sorted(EDGES) + [sorted(WIDE)[0]])
def test_every_layout_instance(name, s):
    """Bins wider than one load batch, bins filled by piece count, the 8-slice hand-off and
    chunk widths above 4 meet the batch kernels here: s = 3 is a group of two and a single
    solve (the NB = 2 instances), s = 4 one group of four (the NB = 4 instances)."""
    c = case(name)
    op = HipCsrOp(c.a)
    c.apply_setters(op)
    assert op.kernel_variant() == c.F
    B = np.random.default_rng(5).standard_normal((c.a.shape[0], s))
    check_all(c.a, op, B, 4, ftk.SQ, (name, s), with_oracle=name in EDGES)


# ---- 8. low level -----------------------------------------------------------------------------
def test_pass_two_batch_low_level():
    a, B = stopping_columns()
    op = HipCsrOp(a)
    decs = single_decomps(op, B, 8)
    assert [d.steps_taken for d in decs] == [3, 2, 8, 1, 5]
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal(d.steps_taken) for d in decs]
    X = alg.lanczos_pass_two_batch(op, B, decs, ys)
    check_columns(X, [alg.lanczos_pass_two(op, B[:, c].copy(), decs[c], ys[c]) for c in range(5)],
                  "single")
    bad = list(ys)
    bad[2] = ys[2][:-1]
    with pytest.raises(LanczosError) as e:
        alg.lanczos_pass_two_batch(op, B, decs, bad)
    assert str(e.value) == "Parameter mismatch: `y_k` expects size 8, but got 7."
    with pytest.raises(LanczosError) as e1:
        alg.lanczos_pass_two(op, B[:, 2].copy(), decs[2], bad[2])
    assert str(e1.value) == str(e.value)


# ---- 9. state ---------------------------------------------------------------------------------
def test_buffers_graphs_and_rebuilds(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.stack([np.random.default_rng(90 + c).standard_normal(n) for c in range(4)], axis=1)
    k = 50
    xs = single_columns(op, B, k, ftk.SQ)
    bytes0 = op.device_bytes()
    check_columns(solvers.lanczos_two_pass_batch(op, B[:, :2], k, ftk.SQ), xs[:2], "s = 2")
    assert not op.flags() & 32
    grown2 = op.device_bytes() - bytes0
    assert 6 * 2 * 8 * n <= grown2 < 8 * n * k  # six interleaved vectors, no basis
    check_columns(solvers.lanczos_two_pass_batch(op, B, k, ftk.SQ), xs, "grown to 4")
    grown4 = op.device_bytes() - bytes0
    assert grown4 > grown2 and 6 * 4 * 8 * n <= grown4 < 8 * n * k
    check_columns(solvers.lanczos_two_pass_batch(op, B[:, :2], k, ftk.SQ), xs[:2], "back to 2")
    assert op.device_bytes() - bytes0 == grown4
    for method, kw in (("set_slices", {"slices": 2}), ("set_reorder", {"mode": 0}),
                       ("set_value_format", {"compress": False})):
        getattr(op, method)(**kw)
        check_columns(solvers.lanczos_two_pass_batch(op, B, k, ftk.SQ),
                      single_columns(op, B, k, ftk.SQ), method)
    assert not op.flags() & 32


# ---- 10. errors -------------------------------------------------------------------------------
def test_errors(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    op = HipCsrOp(a)
    B = np.random.default_rng(11).standard_normal((n, 3))
    Bc = np.ascontiguousarray(B.T)
    x = np.zeros((3, n))
    al, be = np.zeros((3, 5)), np.zeros((3, 5))
    st, bn = (c_size_t * 3)(), np.zeros(3)
    pd = lambda v: v.ctypes.data_as(POINTER(c_double))
    H, BAD = _lib.TPL_MEM_HOST, _lib.TPL_ERR_INVALID_ARGUMENT
    two = _lib.tpl_lanczos_two_pass_batch
    for s in (0, 65):
        assert two(op.handle, Bc.ctypes.data, n, s, 5, _lib.FTK_SQ_PTR, None, x.ctypes.data, H) == BAD
        assert _lib.tpl_lanczos_pass_one_batch(op.handle, Bc.ctypes.data, n, s, 5, pd(al), pd(be),
                                               st, pd(bn), H) == BAD
        assert _lib.tpl_lanczos_pass_two_batch(op.handle, Bc.ctypes.data, n, s, pd(al), pd(be), 5,
                                               st, pd(bn), pd(al), x.ctypes.data, H) == BAD
    assert two(op.handle, None, n, 3, 5, _lib.FTK_SQ_PTR, None, x.ctypes.data, H) == BAD
    assert two(op.handle, Bc.ctypes.data, n, 3, 5, None, None, x.ctypes.data, H) == BAD
    assert two(op.handle, Bc.ctypes.data, n, 3, 5, _lib.FTK_SQ_PTR, None, None, H) == BAD
    with pytest.raises(TplError) as t:
        solvers.lanczos_two_pass_batch(op, np.ones((n, 65)), 5, ftk.SQ)
    assert t.value.status == BAD
    B64 = np.random.default_rng(12).standard_normal((n, 64))
    X64 = solvers.lanczos_two_pass_batch(op, B64, 5, ftk.SQ)
    assert X64.shape == (n, 64)
    for c, r in zip((0, 63), single_columns(op, B64[:, [0, 63]], 5, ftk.SQ)):
        assert same_bits_nan(X64[:, c], r), ("s = 64", c)

    Bz = B.copy()
    Bz[:, 1] = 0.0
    zero_text = "Invalid input parameter: Input vector `b` must not be a zero vector."
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch(op, Bz, 5, ftk.SQ)
    assert str(e.value) == zero_text
    with pytest.raises(LanczosError) as e1:
        solvers.lanczos_two_pass(op, np.zeros(n), 5, ftk.SQ)
    assert str(e1.value) == zero_text
    with pytest.raises(LanczosError) as e:
        alg.lanczos_pass_one_batch(op, Bz, 5)
    assert str(e.value) == zero_text

    calls = []

    def second_fails(al_, be_):
        calls.append(len(al_))
        if len(calls) == 2:
            raise RuntimeError("boom")
        return np.ones(len(al_))
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch(op, B, 5, second_fails)
    assert str(e.value) == "The user-provided f(T_k) solver failed: boom"
    assert e.value.kind == LanczosErrorKind.SOLVER_ERROR
    assert calls == [5, 5]  # the first column's f ran exactly once, the third's never
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_batch(op, B, 5, lambda al_, be_: np.ones(len(al_) + 1))
    assert str(e.value) == "Parameter mismatch: `y_k_prime` expects size 5, but got 6."
    # the operator is still usable after the failed calls
    check_columns(solvers.lanczos_two_pass_batch(op, B, 6, ftk.SQ),
                  single_columns(op, B, 6, ftk.SQ), "after errors")
