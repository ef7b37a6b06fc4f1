"""GPU: every compiled instance of the SpMV-shaped kernels, and the edges of the layout they
read, bit for bit against the canonical oracle.

k_spmv<F>, k_p1_spmv<F> (and k_p1_spmv_wide<F>) and k_p2_spmv<F> are compiled once per
variant flag F (56 instances each) and must all compute the same bits: the oracle knows
nothing of F. tests/layout_cases.py holds one deterministic matrix per instance, a table of
layout edges (chunk widths, empty rows and chunks, piece lengths around the 8 / 16-lane
switch, bins filled by entries and by piece count, bins wider than a load batch, slice
counts) in two formats, and the matrices with more than 256 norm partials;
tests/test_layout_cases.py checks those tables without a GPU. Here each case asserts the
instance it ran (HipCsrOp.kernel_variant) and compares the product, pass one, the two-pass
solve (one graph and its replay from the cache, two graphs and theirs, a re-capture after
the basis allocation dropped the cache) and the one-pass solve with
oracle.Operator(a, op.schedule()). Every comparison is bitwise; where NaNs are expected,
NaN positions plus bitwise elsewhere. k_p1_spmv_gp<F> is not covered here (it needs ranks).
"""
import zlib

import numpy as np
import pytest

import layout_cases as lc

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

ONE_GRAPH = 32  # tpl_op_flags bit 5: the last two-pass solve ran as one device graph


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def same_bits_nan(x, y):
    """NaNs in the same places (their payloads are not part of the contract), every other
    element bit for bit."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    m = ~np.isnan(x)
    return np.array_equal(x[m].view(np.int64), y[m].view(np.int64))


def open_case(name):
    c = lc.case(name)
    op = HipCsrOp(c.a)
    c.apply_setters(op)
    F = op.kernel_variant()
    assert F == c.F, f"{name}: ran instance {F}, the table expects {c.F}"
    return c, op, oracle.Operator(c.a, op.schedule())


def check_pass_one(op, o, b, k, tag):
    d = alg.lanczos_pass_one(op, b, k)
    al, be, st, bn, _ = o.pass_one(b, k)
    assert d.steps_taken == st and d.b_norm == bn, tag
    assert same_bits(d.alphas, al), tag + ": alphas"
    assert same_bits(d.betas, be), tag + ": betas"
    return d


def check_all(name, second_k):
    c, op, o = open_case(name)
    tag = f"{name} F={c.F}"
    n = c.a.shape[0]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal(n)
    assert same_bits(op.apply(x), o.apply(x)), tag + ": k_spmv"
    b = rng.standard_normal(n)
    check_pass_one(op, o, b, 6, tag + ": pass one")
    ref7 = o.lanczos_two_pass(b, 7, ftk.INV)
    x7 = solvers.lanczos_two_pass(op, b, 7, ftk.INV)
    assert op.flags() & ONE_GRAPH, tag + ": the default path is one graph"
    assert same_bits(x7, ref7), tag + ": two-pass, one graph"
    # the same call again while its graph is cached: nothing since the capture drops the
    # cache (the state was sized by pass one above, no basis has been allocated yet), so
    # this launches the instantiated graph a second time
    assert same_bits(solvers.lanczos_two_pass(op, b, 7, ftk.INV), ref7), tag + ": graph replay"
    op.set_device_ftk(0)
    for what in ("host f", "host f, replay"):   # two graphs, captured then replayed
        xh = solvers.lanczos_two_pass(op, b, 7, ftk.INV)
        assert not op.flags() & ONE_GRAPH
        assert same_bits(xh, ref7), tag + ": two-pass, " + what
    op.set_device_ftk(2)
    if second_k:  # 7 = 3 + 3 + 1 and 8 = 3 + 3 + 2: both tails of pass two's grouped flush
        assert same_bits(solvers.lanczos_two_pass(op, b, 8, ftk.INV),
                         o.lanczos_two_pass(b, 8, ftk.INV)), tag + ": two-pass, k = 8"
    assert same_bits(solvers.lanczos(op, b, 5, ftk.INV), o.lanczos(b, 5, ftk.INV)), \
        tag + ": one-pass (Vcol)"
    # the one-pass solve allocated the basis, which drops the cached graphs: a re-capture
    assert same_bits(solvers.lanczos_two_pass(op, b, 7, ftk.INV), x7), tag + ": re-capture"
    op.close()


@pytest.mark.parametrize("name", list(lc.VARIANTS))
def test_variant_instance(name):
    check_all(name, second_k=True)


@pytest.mark.parametrize("name", list(lc.EDGES))
def test_layout_edge(name):
    check_all(name, second_k=False)


def test_all_empty_matrix():
    """n = 600 with no stored entry: two all-empty chunks (short_chunk_any with W = 0), no
    bins, A b = 0. The contract accepts it: y = +0.0, pass one breaks down after its first
    step with alpha_1 = 0, and inv(T_1) = 1 / 0 makes x infinite, as in the oracle."""
    c, op, o = open_case(lc.EMPTY_MATRIX)
    rng = np.random.default_rng(600)
    x = rng.standard_normal(600)
    y = op.apply(x)
    assert same_bits(y, o.apply(x)) and same_bits(y, np.zeros(600))
    b = rng.standard_normal(600)
    d = check_pass_one(op, o, b, 6, "all-empty")
    assert d.steps_taken == 1 and same_bits(d.alphas, np.zeros(1))
    for mode in (2, 0):
        op.set_device_ftk(mode)
        assert same_bits_nan(solvers.lanczos_two_pass(op, b, 7, ftk.INV),
                             o.lanczos_two_pass(b, 7, ftk.INV)), mode
    assert same_bits_nan(solvers.lanczos(op, b, 5, ftk.INV), o.lanczos(b, 5, ftk.INV))
    op.close()


@pytest.mark.parametrize("name", list(lc.WIDE))
def test_wide_norm_partials(name):
    """More than 256 norm partials: k_p1_spmv_wide<F> (its int8 instances of width 1 and 2
    carry launch bounds of their own); max_g2 = 256 on the same operator runs the
    one-partial k_p1_spmv<F> on the same layout."""
    c, op, _ = open_case(name)
    b = np.random.default_rng(zlib.crc32(name.encode())).standard_normal(c.a.shape[0])
    for max_g2 in (0, 256):
        if max_g2:
            op.set_schedule(max_g2=max_g2)
        sched = op.schedule()
        assert (sched["G2"] > 256) == (max_g2 == 0), sched["G2"]
        assert op.kernel_variant() == c.F
        d = check_pass_one(op, oracle.Operator(c.a, sched), b, 6, f"{name} max_g2={max_g2}")
        assert d.steps_taken == 6
    op.close()


@pytest.mark.parametrize("name", lc.SPECIAL)
def test_special_values_through_spmv(name):
    """Padding entries gather the vector's first element (internal column 0) or, in a
    window instance, the window's first element (the chunk's column base), and must stay
    out of the sum whatever it holds: layout_cases.poisoned_column picks the column that a
    padded row gathers and does not reference (the window path: F124 through chunk 0's
    base 0, F081 through the last chunk's). -0.0 and subnormals pass through exactly."""
    c, op, o = open_case(name)
    perm = op.schedule()["perm"]
    p = lc.plan(c.a, c.setters, perm)
    no_col0 = None
    for x0 in lc.SPECIAL_X0:
        x, p0 = lc.special_x(c.a, p, perm, x0)
        y = op.apply(x)
        assert same_bits_nan(y, o.apply(x)), f"{name} x0={x0}"
        # independently of the oracle: rows without a stored entry in that column do not
        # see it at all
        if no_col0 is None:
            no_col0 = np.ones(c.a.shape[0], dtype=bool)
            no_col0[np.repeat(np.arange(c.a.shape[0]), np.diff(c.a.indptr))[c.a.indices == p0]] = False
            assert 0 < no_col0.sum() < c.a.shape[0]
        x1 = x.copy()
        x1[p0] = 1.0
        y1 = op.apply(x1)
        assert same_bits(y[no_col0], y1[no_col0]), f"{name} x0={x0}: padding reached the sum"
        assert np.all(np.isfinite(y[no_col0]))
        assert not np.any(np.isfinite(y[~no_col0])), "rows that do reference the column"
    op.close()


def test_stored_zero_meets_infinity():
    """An explicitly stored 0.0 is an entry like any other (the input canonicalisation keeps
    it: tests/test_boundary.py): 0 * inf = NaN in its row, exactly where the oracle's is."""
    c = lc.case(lc.STORED_ZERO)
    a = lc.with_stored_zero(c.a)
    op = HipCsrOp(a)
    c.apply_setters(op)
    assert op.kernel_variant() == c.F
    sched = op.schedule()
    o = oracle.Operator(a, sched)
    assert sched["perm"] is None or sched["perm"][0] == 0
    for x0 in (np.inf, -np.inf):
        x, p0 = lc.special_x(a, lc.plan(a, c.setters, sched["perm"]), sched["perm"], x0)
        assert p0 == 0
        y, yo = op.apply(x), o.apply(x)
        assert same_bits_nan(y, yo), x0
        assert np.isnan(y[1]) and np.isnan(yo[1]), "row 1 stores 0.0 in column 0"
    op.close()
