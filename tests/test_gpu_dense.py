"""GPU: the dense symmetric operator (include/tpl.h tpl_op_create_dense; tpl_k_dense.hip).

Every row of a dense operator is a long row of the canonical order over all n columns, so the
oracle, unchanged, on the full CSR of the matrix (exact zeros stored) with the schedule the
operator reports is the checker, and the contract is BITWISE, as everywhere else: on the
reference's own R + R^T the coefficients of two summation orders differ by tenths within 20
steps, so a tolerance across orders would mean nothing. NaN positions must agree; every other
value is compared as a 64-bit pattern."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import dense_cases as dc
from dense_cases import same_bits_nan as same

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import (HipCsrOp, HipDenseOp, LanczosError, LanczosErrorKind, TplError, _lib,  # noqa: E402
                     algorithms as alg, ftk, solvers)

ONE_GRAPH, REORDERED, CACHED, FUSED, DENSE = 32, 64, 256, 512, 1024


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


class Case:
    """One matrix on the device (auto slices), its full CSR, a right-hand side, and the
    oracle in the operator's schedule; built once per (kind, n) and shared."""

    def __init__(self, kind, n):
        self.n = n
        self.a = {"ref": dc.reference_matrix, "normal": dc.normal_matrix,
                  "zeros": dc.zeros_matrix, "spd": dc.spd_matrix,
                  "scaled": lambda m: dc.normal_matrix(m) / np.sqrt(m)}[kind](n)
        self.csr = dc.full_csr(self.a)
        self.b = np.random.default_rng(100 + n).standard_normal(n)
        self.op = HipDenseOp(self.a)
        self.k = min(n, 24)

    def oracle(self):
        return oracle.Operator(self.csr, self.op.schedule())


_cases = {}


def case(kind, n):
    if (kind, n) not in _cases:
        _cases[(kind, n)] = Case(kind, n)
    return _cases[(kind, n)]


def _harmonic(al, be):
    return 1.0 / (1.0 + np.arange(len(al), dtype=np.float64))


# ---- 1. the operator and the plain product ------------------------------------------------
@pytest.mark.parametrize("n", dc.SHAPES)
def test_schedule_and_flags(n):
    c = case("ref", n)
    s = c.op.schedule()
    assert s["short_rows"].size == 0 and np.array_equal(s["long_rows"], np.arange(n))
    assert (s["G2"], s["E"], s["slices"], s["perm"]) == (*dc.elem_geometry(n), 1, None)
    assert c.op.flags() & DENSE and not c.op.flags() & (REORDERED | CACHED | FUSED)
    assert (c.op.nrows(), c.op.ncols(), c.op.nnz) == (n, n, n * n)
    assert int(_lib.tpl_op_nnz(c.op.handle)) == n * n


@pytest.mark.parametrize("n", dc.SHAPES)
@pytest.mark.parametrize("kind", ["ref", "normal", "zeros"])
def test_apply_is_bitwise_the_oracle(kind, n):
    c = case(kind, n)
    x = np.random.default_rng(n).standard_normal(n)
    assert same(c.op.apply(x), c.oracle().apply(x))
    assert same(c.op.apply(c.b), c.oracle().apply(c.b))


@pytest.mark.parametrize("n", dc.SHAPES)
def test_apply_from_device_memory_and_a_padded_host_buffer(n):
    import torch
    c = case("zeros", n)
    x = np.random.default_rng(n).standard_normal(n)
    want = c.oracle().apply(x)
    dev = HipDenseOp(torch.from_numpy(c.a).cuda())
    assert same(dev.apply(x), want)
    yd = dev.apply(torch.from_numpy(x).cuda())
    assert yd.is_cuda and same(host(yd), want)
    # a device view with a row stride above n, and a host buffer with lda > n whose padding
    # is NaN: padding never enters a sum
    wide = torch.full((n, n + 5), float("nan"), dtype=torch.float64).cuda()
    wide[:, :n] = torch.from_numpy(c.a).cuda()
    assert same(HipDenseOp(wide[:, :n]).apply(x), want)
    buf = np.full((n, n + 3), np.nan)
    buf[:, :n] = c.a
    assert same(HipDenseOp(buf[:, :n]).apply(x), want)
    # column-major storage of a symmetric matrix is the same operator
    assert same(HipDenseOp(np.asfortranarray(c.a)).apply(x), want)


@pytest.mark.parametrize("slices", dc.SLICES)
@pytest.mark.parametrize("n", dc.SLICED)
def test_slices_follow_set_slices(n, slices):
    """apply, pass one and a host-f solve after set_slices follow the new S (another sum), and
    back at the auto count the first bits return."""
    c = case("zeros", n)
    op = HipDenseOp(c.a)
    x1 = op.apply(c.b)
    op.set_slices(slices)
    s = op.schedule()
    assert s["slices"] == slices and s["short_rows"].size == 0
    o = oracle.Operator(c.csr, s)
    assert same(op.apply(c.b), o.apply(c.b))
    d = alg.lanczos_pass_one(op, c.b, c.k)
    al, be, st, bn, _ = o.pass_one(c.b, c.k)
    assert d.steps_taken == st and d.b_norm == bn
    assert same(d.alphas, al) and same(d.betas, be)
    assert same(solvers.lanczos_two_pass(op, c.b, c.k, ftk.SQ), o.lanczos_two_pass(c.b, c.k, ftk.SQ))
    op.set_slices(0)
    assert op.schedule()["slices"] == 1 and same(op.apply(c.b), x1)


# ---- 2. the passes -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.SHAPES)
@pytest.mark.parametrize("kind", ["ref", "normal"])
def test_pass_one_is_bitwise(kind, n):
    c = case(kind, n)
    d = alg.lanczos_pass_one(c.op, c.b, c.k)
    al, be, st, bn, _ = c.oracle().pass_one(c.b, c.k)
    assert (d.steps_taken, d.b_norm) == (st, bn)
    assert same(d.alphas, al) and same(d.betas, be)


@pytest.mark.parametrize("n", dc.SHAPES)
def test_basis_and_its_regeneration(n):
    c = case("ref", n)
    out = alg.lanczos_standard(c.op, c.b, c.k)
    al, be, st, bn, V = c.oracle().pass_one(c.b, c.k, store_basis=True)
    d = out.decomposition
    assert d.steps_taken == st and same(d.alphas, al) and same(d.betas, be)
    assert same(np.asarray(out.v_k), V)
    y = bn * ftk.SQ(al, be)
    p2 = alg.lanczos_pass_two_with_basis(c.op, c.b, d, y)
    assert same(np.asarray(p2.v_k), V)
    xo, Vo = c.oracle().pass_two(c.b, al, be, st, bn, y, store_basis=True)
    assert same(p2.x_k, xo) and same(np.asarray(p2.v_k), Vo)


@pytest.mark.parametrize("n", dc.SHAPES)
def test_host_f_solves_are_bitwise(n):
    c = case("normal", n)
    o = c.oracle()
    for f in (ftk.SQ, _harmonic):
        assert same(solvers.lanczos_two_pass(c.op, c.b, c.k, f), o.lanczos_two_pass(c.b, c.k, f))
        assert same(solvers.lanczos(c.op, c.b, c.k, f), o.lanczos(c.b, c.k, f))
    d = alg.lanczos_pass_one(c.op, c.b, c.k)
    y = d.b_norm * ftk.SQ(d.alphas, d.betas)
    xo = o.pass_two(c.b, d.alphas, d.betas, d.steps_taken, d.b_norm, y)[0]
    assert same(alg.lanczos_pass_two(c.op, c.b, d, y), xo)
    # a device b gives the same bits
    import torch
    xd = solvers.lanczos_two_pass(c.op, torch.from_numpy(c.b).cuda(), c.k, ftk.SQ)
    assert xd.is_cuda and same(host(xd), o.lanczos_two_pass(c.b, c.k, ftk.SQ))


@pytest.mark.parametrize("n", [2, 9, 65, 513, 1031, 2053])
def test_one_graph_builtins(n):
    c = case("spd", n)
    op = c.op
    x = solvers.lanczos_two_pass(op, c.b, c.k, ftk.INV)
    assert op.flags() & ONE_GRAPH and not op.flags() & (CACHED | FUSED)
    op.set_device_ftk(0)
    try:
        xh = solvers.lanczos_two_pass(op, c.b, c.k, ftk.INV)
        assert not op.flags() & ONE_GRAPH
    finally:
        op.set_device_ftk(2)
    assert same(x, xh)
    assert same(x, c.oracle().lanczos_two_pass(c.b, c.k, ftk.INV))
    # exp, on a spectrum of width about 6 (the standard-normal matrix over sqrt(n)): pass two
    # on the call's own decomposition with the y the device kernel returns
    c = case("scaled", n)
    op = c.op
    xe = solvers.lanczos_two_pass(op, c.b, c.k, ftk.EXP)
    assert op.flags() & ONE_GRAPH
    d = alg.lanczos_pass_one(op, c.b, c.k)
    y, on = op.ftk_device("exp", d.alphas, d.betas)
    assert on
    assert same(xe, alg.lanczos_pass_two(op, c.b, d, d.b_norm * y))
    c = case("spd", n)
    op = c.op
    # the one-pass solver with the device f
    assert same(solvers.lanczos(op, c.b, c.k, ftk.INV), c.oracle().lanczos(c.b, c.k, ftk.INV))


# ---- 3. the multi-function solves --------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 65, 513, 2053])
def test_multi_function_solves(n):
    c = case("spd", n)
    op, fs = c.op, [ftk.INV, ftk.inv_shift(1.0), ftk.SQ]
    X = solvers.lanczos_two_pass_multi(op, c.b, c.k, fs)
    X1 = solvers.lanczos_multi(op, c.b, c.k, fs)
    op.set_device_ftk(0)
    try:
        for i, f in enumerate(fs):
            assert same(X[:, i], solvers.lanczos_two_pass(op, c.b, c.k, f)), i
            assert same(X1[:, i], solvers.lanczos(op, c.b, c.k, f)), i
    finally:
        op.set_device_ftk(2)


@pytest.mark.parametrize("n", [7, 65, 513, 2053])
def test_exp_times(n):
    c = case("spd", n)
    ts = [0.25, -0.5, 1.0]
    X, on = solvers.lanczos_two_pass_exp_times(c.op, c.b, c.k, ts, return_on_device=True)
    d = alg.lanczos_pass_one(c.op, c.b, c.k)
    Y, on2 = c.op.ftk_exp_times_device(d.alphas, d.betas, ts)
    Y = np.array(Y)
    assert np.array_equal(on, on2)
    for i, t in enumerate(ts):
        if not on[i]:
            Y[:, i] = ftk.exp_t(t)(d.alphas, d.betas)
        assert same(X[:, i], alg.lanczos_pass_two(c.op, c.b, d, d.b_norm * Y[:, i])), i


@pytest.mark.parametrize("n", [65, 513, 2053])
def test_tolerance_solves(n):
    c = case("spd", n)
    op = c.op
    x, info = solvers.lanczos_two_pass_inv_tol(op, c.b, 40, 1e-10, return_info=True)
    assert info["converged"] and 1 <= info["steps"] < 40
    assert same(x, solvers.lanczos_two_pass(op, c.b, info["steps"], ftk.INV))
    assert same(x, c.oracle().lanczos_two_pass(c.b, info["steps"], ftk.INV))
    sig = [0.0, 0.5, 3.0]
    X, inf = solvers.lanczos_two_pass_shifted_inv_tol(op, c.b, 40, sig, 1e-10, return_info=True)
    assert all(inf["converged"])
    d = alg.lanczos_pass_one(op, c.b, 40)
    for i, s in enumerate(sig):
        m = int(inf["steps"][i])
        cut = alg.LanczosDecomposition(d.alphas[:m], d.betas[:m - 1], m, d.b_norm)
        y = d.b_norm * ftk.INV(d.alphas[:m] + s, d.betas[:m - 1])
        assert same(X[:, i], alg.lanczos_pass_two(op, c.b, cut, y)), i


# ---- 4. breakdown and errors --------------------------------------------------------------------
def test_breakdown_and_zero_b():
    n = 65
    op = HipDenseOp(2.0 * np.eye(n))
    b = np.random.default_rng(1).standard_normal(n)
    d = alg.lanczos_pass_one(op, b, 10)
    assert d.steps_taken == 1 and abs(d.alphas[0] - 2.0) < 1e-12
    assert same(solvers.lanczos_two_pass(op, b, 10, ftk.INV),
                oracle.Operator(dc.full_csr(2.0 * np.eye(n)), op.schedule())
                .lanczos_two_pass(b, 10, ftk.INV))
    for call in (lambda: alg.lanczos_pass_one(op, np.zeros(n), 5),
                 lambda: solvers.lanczos_two_pass(op, np.zeros(n), 5, ftk.INV),
                 lambda: solvers.lanczos(op, np.zeros(n), 5, ftk.SQ)):
        with pytest.raises(LanczosError) as e:
            call()
        assert e.value.kind == LanczosErrorKind.INPUT_ERROR
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass(op, np.zeros(n - 1), 5, ftk.INV)
    assert e.value.kind == LanczosErrorKind.DIMENSION_MISMATCH


def test_create_arguments():
    with pytest.raises(TplError):
        HipDenseOp(np.zeros((3, 4)))
    with pytest.raises(TplError):
        HipDenseOp(np.zeros((0, 0)))


# ---- 5. what a dense operator refuses -----------------------------------------------------------
def test_refused_calls_leave_the_operator_usable():
    c = case("spd", 129)
    op, b, n = c.op, c.b, c.n
    want = op.apply(b)
    B = np.asfortranarray(np.stack([b, 2 * b], axis=1))
    d = alg.lanczos_pass_one(op, b, 4)
    y = d.b_norm * ftk.SQ(d.alphas, d.betas)
    calls = {
        "two_pass_batch": lambda: solvers.lanczos_two_pass_batch(op, B, 4, ftk.SQ),
        "two_pass_batch_multi": lambda: solvers.lanczos_two_pass_batch_multi(op, B, 4, [ftk.SQ]),
        "two_pass_batch_exp_times": lambda: solvers.lanczos_two_pass_batch_exp_times(op, B, 4, [1.0]),
        "two_pass_batch_shifted_inv_tol":
            lambda: solvers.lanczos_two_pass_batch_shifted_inv_tol(op, B, 4, [0.0], 1e-3),
        "pass_one_batch": lambda: alg.lanczos_pass_one_batch(op, B, 4),
        "pass_two_batch": lambda: alg.lanczos_pass_two_batch(op, B, [d, d], [y, y]),
        "pass_two_batch_multi":
            lambda: alg.lanczos_pass_two_batch_multi(op, B, [d, d], [y[:, None], y[:, None]]),
        "pass_two_batch_multi_cut":
            lambda: alg.lanczos_pass_two_batch_multi_cut(op, B, [d, d], [y[:, None], y[:, None]],
                                                         [[d.steps_taken], [d.steps_taken]]),
        "ftk_exp_times_batch_device":
            lambda: op.ftk_exp_times_batch_device([d.alphas, d.alphas], [d.betas, d.betas], [1.0]),
        "set_schedule": lambda: op.set_schedule(8, 0),
        "set_reorder(1)": lambda: op.set_reorder(1),
        "tune_order": lambda: op.tune_order(),
        "set_order_groups": lambda: op.set_order_groups(12),
        "set_value_format": lambda: op.set_value_format(True),
        "set_long_cache(1)": lambda: op.set_long_cache(1, 1 << 20),
        "profile_kernel": lambda: op.profile_kernel(_lib.TPL_KERNEL_SPMV, 2),
    }
    for name, call in calls.items():
        with pytest.raises(TplError) as e:
            call()
        assert not isinstance(e.value, LanczosError), name
        assert e.value.status == _lib.TPL_ERR_UNSUPPORTED, (name, str(e.value))
        assert "dense" in str(e.value), (name, str(e.value))
        assert same(op.apply(b), want), name
    # the auto modes resolve to off and are accepted
    op.set_reorder(2), op.set_reorder(0), op.set_long_cache(2), op.set_long_cache(0)
    op.set_fused_pass_two(2), op.set_fused_pass_two(0)
    x = solvers.lanczos_two_pass(op, b, c.k, ftk.INV)
    assert not op.flags() & (REORDERED | CACHED | FUSED) and op.flags() & DENSE
    op.set_long_cache(2), op.set_fused_pass_two(2), op.set_reorder(2)
    assert same(x, solvers.lanczos_two_pass(op, b, c.k, ftk.INV))


# ---- 6. state ------------------------------------------------------------------------------------
def test_state_is_the_operators_own():
    """A CSR operator on the same context gives the same bits before and after dense solves;
    the same dense call twice gives the same bits, whatever ran between."""
    from state_cases import matrix
    a = matrix("band")  # n = 1501: short chunks and long rows
    bs = np.random.default_rng(5).standard_normal(a.shape[0])
    csr = HipCsrOp(a)
    before = (csr.apply(bs), solvers.lanczos_two_pass(csr, bs, 20, ftk.INV))
    c = case("spd", 520)
    x1 = solvers.lanczos_two_pass(c.op, c.b, c.k, ftk.INV)
    X1 = solvers.lanczos_two_pass_multi(c.op, c.b, c.k, [ftk.INV, ftk.SQ])
    d1 = alg.lanczos_standard(c.op, c.b, c.k)
    after = (csr.apply(bs), solvers.lanczos_two_pass(csr, bs, 20, ftk.INV))
    assert same(before[0], after[0]) and same(before[1], after[1])
    assert same(x1, solvers.lanczos_two_pass(c.op, c.b, c.k, ftk.INV))
    assert same(X1, solvers.lanczos_two_pass_multi(c.op, c.b, c.k, [ftk.INV, ftk.SQ]))
    assert same(np.asarray(d1.v_k), np.asarray(alg.lanczos_standard(c.op, c.b, c.k).v_k))
    assert same(x1, solvers.lanczos_two_pass(HipDenseOp(c.a), c.b, c.k, ftk.INV))


# ---- 7. memory -----------------------------------------------------------------------------------
def _ld(n):
    return 16 * (((n + 15) // 16) | 1)  # tpl_op.h dense_stride


@pytest.mark.parametrize("n", [9, 513, 2053])
def test_device_bytes(n):
    c = case("spd", n)
    op = HipDenseOp(c.a)
    assert op.device_bytes() >= n * _ld(n) * 8
    solvers.lanczos_two_pass(op, c.b, c.k, ftk.INV)
    solvers.lanczos_two_pass_multi(op, c.b, c.k, [ftk.INV, ftk.SQ])
    held = op.device_bytes()
    assert held < n * _ld(n) * 8 + (1 << 20) + 64 * 8 * (n + 64)  # the matrix, vectors and state
    solvers.lanczos_two_pass(op, c.b, c.k, ftk.INV)
    solvers.lanczos_two_pass_multi(op, c.b, c.k, [ftk.INV, ftk.SQ])
    op.apply(c.b)
    assert op.device_bytes() == held


def test_allocation_cap_refuses_the_matrix_and_leaves_nothing(monkeypatch):
    n = 513
    c = case("spd", n)
    monkeypatch.setenv("TPL_TEST_ALLOC_CAP", str(n * _ld(n) * 8 - 1))
    with pytest.raises(TplError) as e:
        HipDenseOp(c.a)
    assert e.value.status == _lib.TPL_ERR_OUT_OF_MEMORY
    monkeypatch.delenv("TPL_TEST_ALLOC_CAP")
    op = HipDenseOp(c.a)
    assert same(op.apply(c.b), c.op.apply(c.b))


# ---- 8. the reference's dense study ----------------------------------------------------------------
def test_harness_dense_tradeoff_rows(tmp_path):
    """src/bin/dense_tradeoff.rs through the harness: one fresh worker per variant, the
    reference's columns, rows grouped by variant with k ascending."""
    import csv
    from tpl_amd import harness
    out = str(tmp_path / "d.csv")
    harness.main(["dense-tradeoff", "--n", "129", "--k-start", "10", "--k-end", "30",
                  "--k-step", "10", "--output", out])
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == ["variant", "k", "time_s", "rss_kb"]
    assert [(r["variant"], int(r["k"])) for r in rows] == [
        ("standard", 10), ("standard", 20), ("standard", 30),
        ("two-pass", 10), ("two-pass", 20), ("two-pass", 30)]
    assert all(float(r["time_s"]) > 0 and int(r["rss_kb"]) > 0 for r in rows)
