"""GPU: the long-row cache in the multi-function and batch two-pass solves
(tpl_op_set_long_cache_solvers).

With its bit in the operator's solver mask, tpl_lanczos_two_pass_multi runs under the single
solve's cache (k_p2_cached at nflush = 0), and the batch solves keep a cache of the group's
own: the group's pass one (k_bp1_spmv) stores every long row's NB sums, its pass two reads
them back with k_bp2_cached instead of running the bins again. Pass two regenerates pass
one's basis bit for bit, so nothing may change: every result here is compared bitwise
(same_bits_nan, the NaN-aware idiom of test_gpu_batch.py: f = inv of the harness's b is not
finite at these k) against a fresh operator with the default mask, and where named against the single host-f solve of each column or
function. flags() bit 8 tells which path the last pass two took.

The 5k-arc KKT (n = 5,115; 114 long rows) and small synthetic matrices, k <= 20.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import banded_hub, harness_b

pytestmark = pytest.mark.gpu

from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, TplError, _lib, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

import layout_cases as lc  # noqa: E402

CACHED = 256
ONE, MULTI, BATCH, BATCH_MULTI, ALL = 1, 2, 4, 8, 15
K = 20


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same_bits_nan(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    nx, ny = np.isnan(x), np.isnan(y)
    return (x.shape == y.shape and np.array_equal(nx, ny)
            and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))


def fresh(a, mask=None, prep=None, mode=None, budget=0):
    """A new operator: `prep` (layout setters), the cache mode if given, the solver mask if
    given (None: the default mask, the setter never called)."""
    op = HipCsrOp(a)
    if prep:
        prep(op)
    if mode is not None:
        op.set_long_cache(mode, budget)
    if mask is not None:
        op.set_long_cache_solvers(mask)
    return op


def run(a, call, mask=None, **kw):
    """-> (result, flags after the call) of call(op) on a fresh operator."""
    op = fresh(a, mask, **kw)
    try:
        return np.asarray(call(op)), op.flags()
    finally:
        op.close()


def singles(a, B, k, fs, prep=None):
    """X[:, i, c] = the single host-f solve of column c with function i (a fresh operator,
    default mask)."""
    op = fresh(a, prep=prep)
    op.set_device_ftk(0)
    try:
        return np.stack([np.stack([solvers.lanczos_two_pass(op, np.ascontiguousarray(B[:, c]), k, f)
                                   for f in fs], axis=1) for c in range(B.shape[1])], axis=2)
    finally:
        op.close()


def n_long_of(a, prep=None):
    op = fresh(a, prep=prep)
    try:
        return len(op.schedule()["long_rows"])
    finally:
        op.close()


@pytest.fixture(scope="module")
def a5k(kkt5k):
    return kkt5k.a


@pytest.fixture(scope="module")
def B5k(a5k):
    """Five columns on the 5k-arc KKT; column 0 is the harness's b."""
    n = a5k.shape[0]
    cols = [harness_b(a5k), std_rng_vector(n) - 0.5]
    cols += [np.random.default_rng(70 + c).standard_normal(n) for c in range(3)]
    return np.stack(cols, axis=1)


FS9 = [ftk.INV, ftk.SQ] + [ftk.inv_shift(1.0 + i) for i in range(7)]
_REF = {}


def ref_singles(a, B, k, fs, key):
    """The singles of (key), computed once for the module and left unchanged."""
    if key not in _REF:
        _REF[key] = singles(a, B, k, fs)
        _REF[key].setflags(write=False)
    return _REF[key]


# ---- 1. multi --------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 9])
def test_multi_on_equals_off_and_singles(m, a5k, B5k):
    """m = 9: two k_p2_xacc launches per flush. Bit 8 with the solver's bit, not without."""
    b, fs = B5k[:, 0].copy(), FS9[:m]
    call = lambda op: solvers.lanczos_two_pass_multi(op, b, K, fs)
    x1, f1 = run(a5k, call, ONE)
    x2, f2 = run(a5k, call, ONE | MULTI)
    xb, fb = run(a5k, call, BATCH | BATCH_MULTI)   # other solvers' bits: not this one's
    assert f2 & CACHED and not f1 & CACHED and not fb & CACHED
    assert same_bits_nan(x2, x1) and same_bits_nan(xb, x1)
    assert same_bits_nan(x2, ref_singles(a5k, B5k[:, :1], K, FS9, "multi")[:, :m, 0])


@pytest.mark.parametrize("k", [1, 2])
def test_multi_short_runs(k, a5k, B5k):
    """k = 1: the prologue only, no step and no cached step; k = 2: one step."""
    b, fs = B5k[:, 0].copy(), FS9[:3]
    call = lambda op: solvers.lanczos_two_pass_multi(op, b, k, fs)
    x1, f1 = run(a5k, call)
    x2, f2 = run(a5k, call, MULTI)
    assert same_bits_nan(x2, x1)
    assert not f1 & CACHED and bool(f2 & CACHED) == (k == 2)


# ---- 2. batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [ftk.INV, ftk.SQ], ids=["inv", "sq"])
@pytest.mark.parametrize("s", [2, 3, 4, 5])
def test_batch_on_equals_off_and_singles(s, f, a5k, B5k):
    """NB = 2; 2 + the remainder column; NB = 4; 4 + the remainder column. The remainder
    follows the batch solver's bit (s = 3 and 5: bit 8 then tells of the single path)."""
    B = np.ascontiguousarray(B5k[:, :s])
    call = lambda op: solvers.lanczos_two_pass_batch(op, B, K, f)
    x1, f1 = run(a5k, call, ONE)
    x4, f4 = run(a5k, call, BATCH)
    xo, fo = run(a5k, call, ONE | MULTI | BATCH_MULTI)
    assert f4 & CACHED and not f1 & CACHED and not fo & CACHED
    assert same_bits_nan(x4, x1) and same_bits_nan(xo, x1)
    i = 0 if f is ftk.INV else 1
    assert same_bits_nan(x4, ref_singles(a5k, B5k, K, FS9[:2], "batch")[:, i, :s])


# ---- 3. batch-multi --------------------------------------------------------------------------
@pytest.mark.parametrize("s,m", [(4, 3), (2, 5), (3, 5), (4, 1)])
def test_batch_multi_on_equals_off_and_singles(s, m, a5k, B5k):
    """(2, 5): two k_bp2_xacc launches per flush (M = 4 + 1); (3, 5): a group of two and the
    multi-function solve of the last column; (4, 1) runs the batch solve under the
    batch-multi solver's bit."""
    B = np.ascontiguousarray(B5k[:, :s])
    fs = FS9[1:1 + m]
    call = lambda op: solvers.lanczos_two_pass_batch_multi(op, B, K, fs)
    x1, f1 = run(a5k, call, ONE)
    x8, f8 = run(a5k, call, BATCH_MULTI)
    xo, fo = run(a5k, call, ONE | MULTI | BATCH)
    assert f8 & CACHED and not f1 & CACHED and not fo & CACHED
    assert same_bits_nan(x8, x1) and same_bits_nan(xo, x1)
    assert x8.shape == (a5k.shape[0], m, s)
    assert same_bits_nan(x8, ref_singles(a5k, B5k[:, :4], K, FS9[1:6], "bm")[:, :m, :s])


# ---- 4. layouts ------------------------------------------------------------------------------
PREPS = {
    "slices8": lambda op: op.set_slices(8),
    "slices1": lambda op: op.set_slices(1),
    "caller_order": lambda op: op.set_reorder(0),
    "fp64_values": lambda op: op.set_value_format(0),
}


@pytest.mark.parametrize("name", sorted(PREPS))
def test_preparations_on_equals_off(name, a5k, B5k):
    prep = PREPS[name]
    b = B5k[:, 0].copy()
    calls = {
        "multi": (MULTI, lambda op: solvers.lanczos_two_pass_multi(op, b, K, FS9[:3])),
        "batch4": (BATCH, lambda op: solvers.lanczos_two_pass_batch(op, B5k[:, :4].copy(), K, ftk.SQ)),
        "batch2": (BATCH, lambda op: solvers.lanczos_two_pass_batch(op, B5k[:, :2].copy(), K, ftk.SQ)),
    }
    for what, (bit, call) in calls.items():
        x1, f1 = run(a5k, call, prep=prep)
        xc, fc = run(a5k, call, bit, prep=prep)
        assert fc & CACHED and not f1 & CACHED, what
        assert same_bits_nan(xc, x1), what


@pytest.mark.parametrize("s", [4, 3])
@pytest.mark.parametrize("name", list(lc.VARIANTS) + list(lc.EDGES))
def test_every_layout_case_on_equals_off(name, s):
    """Every chunk width and format instance of k_bp2_cached's chunk path, and the bins'
    shapes on the storing side (k = 4, as test_gpu_batch.py test_every_layout_instance)."""
    c = lc.case(name)
    B = np.random.default_rng(5).standard_normal((c.a.shape[0], s))

    def prep(op):
        c.apply_setters(op)
        assert op.kernel_variant() == c.F

    call = lambda op: solvers.lanczos_two_pass_batch(op, B, 4, ftk.SQ)
    x1, f1 = run(c.a, call, prep=prep)
    x4, f4 = run(c.a, call, BATCH, prep=prep)
    assert same_bits_nan(x4, x1)
    assert not f1 & CACHED
    assert bool(f4 & CACHED) == (n_long_of(c.a, prep) > 0)


def test_no_long_rows():
    n = 3001
    a = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    B = np.random.default_rng(9).standard_normal((n, 4))
    out = {}
    for mask in (ONE, ALL):
        op = fresh(a, mask)
        try:
            assert len(op.schedule()["long_rows"]) == 0
            xb = solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ)
            fb = op.flags()
            xm = solvers.lanczos_two_pass_multi(op, B[:, 0].copy(), K, FS9[:3])
            out[mask] = (np.asarray(xb), np.asarray(xm), op.device_bytes(), fb | op.flags())
        finally:
            op.close()
    assert same_bits_nan(out[ALL][0], out[ONE][0]) and same_bits_nan(out[ALL][1], out[ONE][1])
    assert out[ALL][2] == out[ONE][2]
    assert not out[ALL][3] & CACHED


# ---- 5. the last wave of the long-row workgroup ------------------------------------------------
@pytest.fixture(scope="module")
def hub66():
    a = banded_hub(n=6000, hub_every=91, hub_half=40)
    n = a.shape[0]
    B = np.stack([std_rng_vector(n) - 0.5] +
                 [np.random.default_rng(30 + c).standard_normal(n) for c in range(3)], axis=1)
    return a, B


@pytest.mark.parametrize("nb", [4, 2])
@pytest.mark.parametrize("reorder", [2, 0])
def test_last_wave_with_few_long_rows(reorder, nb, hub66):
    """66 long rows: one long-row workgroup whose second wave has two live lanes and whose
    other two have none. Reorder 0: the long rows are scattered and come from the index
    table behind the sums."""
    a, B = hub66

    def prep(op):
        op.set_reorder(reorder)
        assert len(op.schedule()["long_rows"]) == 66

    Bs = np.ascontiguousarray(B[:, :nb])
    call = lambda op: solvers.lanczos_two_pass_batch(op, Bs, K, ftk.INV)
    x1, f1 = run(a, call, prep=prep)
    x4, f4 = run(a, call, BATCH, prep=prep)
    assert f4 & CACHED and not f1 & CACHED
    assert same_bits_nan(x4, x1)
    if reorder == 2 and nb == 4:
        assert same_bits_nan(x4, singles(a, Bs, K, [ftk.INV])[:, 0, :])


# ---- 6. partial cache ------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1, 2, K - 2, K, 3 * K])
def test_partial_cache_batch(rows, a5k, B5k):
    """Mode 1 with a budget of `rows` steps of a group of four: steps 1 .. rows run
    k_bp2_cached, the rest k_bp2_spmv."""
    nl = n_long_of(a5k)
    B = np.ascontiguousarray(B5k[:, :4])
    call = lambda op: solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ)
    x1, _ = run(a5k, call)
    x4, f4 = run(a5k, call, BATCH, mode=1, budget=rows * 8 * nl * 4)
    assert same_bits_nan(x4, x1)
    assert bool(f4 & CACHED) == (rows >= 1)


@pytest.mark.parametrize("rows", [0, 1, 2, K - 2, K, 3 * K])
def test_partial_cache_multi(rows, a5k, B5k):
    nl = n_long_of(a5k)
    b = B5k[:, 0].copy()
    call = lambda op: solvers.lanczos_two_pass_multi(op, b, K, FS9[:3])
    x1, _ = run(a5k, call)
    x2, f2 = run(a5k, call, MULTI, mode=1, budget=rows * 8 * nl)
    assert same_bits_nan(x2, x1)
    assert bool(f2 & CACHED) == (rows >= 1)


# ---- 7. columns that stop at different steps, with long rows present ------------------------------
def stopping_with_long_rows():
    """The 66-long-row matrix beside diag(1 .. 600). Columns on 3, 2, 1 and 5 entries of the
    diagonal block stop after as many steps; the dense column on the hub block runs all k."""
    hub = banded_hub(n=6000, hub_every=91, hub_half=40)
    a = sp.block_diag([hub, sp.diags(np.arange(1.0, 601.0))]).tocsr()
    a.sort_indices()
    n, n0 = a.shape[0], hub.shape[0]
    rng = np.random.default_rng(21)
    B = np.zeros((n, 5))
    for c, support in enumerate([(5, 300, 599), (17, 411), None, (88,), (1, 2, 3, 4, 5)]):
        if support is None:
            B[:n0, c] = rng.standard_normal(n0)
        else:
            for i in support:
                B[n0 + i, c] = rng.standard_normal()
    return a, B


@pytest.mark.parametrize("reverse", [False, True])
def test_columns_stop_at_different_steps(reverse):
    """A stopped column stores nothing into the cache rows and reads whatever is there: it
    must neither change nor be changed. Batch-multi takes the uncaptured launch list here
    (uneven steps within the group of four)."""
    a, B = stopping_with_long_rows()
    steps = [3, 2, 8, 1, 5]
    if reverse:
        B, steps = np.ascontiguousarray(B[:, ::-1]), steps[::-1]
    op = fresh(a, ALL)
    try:
        assert len(op.schedule()["long_rows"]) == 66
        assert [d.steps_taken for d in alg.lanczos_pass_one_batch(op, B, 8)] == steps
        assert not op.flags() & CACHED
        # a first full-length batch leaves other words in the group's cache rows
        full = np.random.default_rng(4).standard_normal((a.shape[0], 4))
        solvers.lanczos_two_pass_batch(op, full, 8, ftk.SQ)
        xb_on = np.asarray(solvers.lanczos_two_pass_batch(op, B, 8, ftk.SQ))
        fb = op.flags()
        xm_on = np.asarray(solvers.lanczos_two_pass_batch_multi(op, B, 8, FS9[1:4]))
        fm = op.flags()
    finally:
        op.close()
    # the last pass two is the remainder column's: 5 or 3 steps, cached either way
    assert fb & CACHED and fm & CACHED
    xb_off, f0 = run(a, lambda o: solvers.lanczos_two_pass_batch(o, B, 8, ftk.SQ))
    xm_off, f1 = run(a, lambda o: solvers.lanczos_two_pass_batch_multi(o, B, 8, FS9[1:4]))
    assert not f0 & CACHED and not f1 & CACHED
    assert same_bits_nan(xb_on, xb_off) and same_bits_nan(xm_on, xm_off)
    xs = singles(a, B, 8, FS9[1:4])
    assert same_bits_nan(xm_on, xs) and same_bits_nan(xb_on, xs[:, 0, :])


# ---- 8. a non-finite column leaves its neighbours alone ------------------------------------------
def test_bad_column_leaves_its_neighbours_alone(a5k):
    n = a5k.shape[0]
    B = np.stack([std_rng_vector(n), harness_b(a5k), np.random.default_rng(8).standard_normal(n)],
                 axis=1)
    xs = singles(a5k, B, 5, [ftk.INV])[:, 0, :]
    assert not np.all(np.isfinite(xs[:, 1]))
    assert np.all(np.isfinite(xs[:, 0])) and np.all(np.isfinite(xs[:, 2]))
    x4, f4 = run(a5k, lambda op: solvers.lanczos_two_pass_batch(op, B, 5, ftk.INV), BATCH)
    assert f4 & CACHED
    assert same_bits_nan(x4, xs)


# ---- 9. no stale reuse -------------------------------------------------------------------------
def test_no_stale_reuse(a5k, B5k):
    """One operator with every solver's bit: each call's pass two may read only what its own
    pass one stored, and the stand-alone pass two nothing."""
    B, B2 = np.ascontiguousarray(B5k[:, :4]), np.ascontiguousarray(B5k[:, [4, 2, 0, 1]] * 0.5)
    b = B5k[:, 1].copy()
    fs = [ftk.INV, ftk.SQ]

    def call(op, what):
        if what == "batch_B":
            return solvers.lanczos_two_pass_batch(op, B, 20, ftk.SQ)
        if what == "batch_B2":
            return solvers.lanczos_two_pass_batch(op, B2, 12, ftk.SQ)
        if what == "pass_two_batch":
            ds = alg.lanczos_pass_one_batch(op, B2, 12)
            return alg.lanczos_pass_two_batch(op, B2, ds,
                                              [ftk.SQ(d.alphas, d.betas) * d.b_norm for d in ds])
        if what == "multi":
            return solvers.lanczos_two_pass_multi(op, b, 12, fs)
        if what == "single":
            return solvers.lanczos_two_pass(op, b, 16, ftk.INV)
        return solvers.lanczos_two_pass_batch_multi(op, B2, 12, fs)

    seq = ["batch_B", "batch_B2", "pass_two_batch", "multi", "single", "batch_multi", "batch_B"]
    want = {w: run(a5k, lambda op: call(op, w))[0] for w in set(seq)}
    op = fresh(a5k, ALL)
    try:
        for w in seq:
            assert same_bits_nan(np.asarray(call(op, w)), want[w]), w
            assert bool(op.flags() & CACHED) == (w != "pass_two_batch"), w
    finally:
        op.close()
    assert same_bits_nan(want["pass_two_batch"], want["batch_B2"])


# ---- 10. accounting and switching ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["kkt5k", "hub66_caller_order"])
def test_accounting(which, a5k, B5k, hub66):
    """The group's cache is rows_b x n_long x NB doubles, plus the row-index table when the
    long rows are not the operator's last rows, and gone after the bits are cleared."""
    if which == "kkt5k":
        a, B, prep = a5k, np.ascontiguousarray(B5k[:, :4]), None
    else:
        a, B, prep = hub66[0], hub66[1], (lambda op: op.set_reorder(0))
    n, nl = a.shape[0], n_long_of(a, prep)
    table = 0 if which == "kkt5k" else (4 * nl + 7) // 8 * 8
    op, op1 = fresh(a, ALL, prep), fresh(a, None, prep)
    try:
        assert op.device_bytes() == op1.device_bytes()   # nothing before the first batch solve
        x = solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ)
        x1 = solvers.lanczos_two_pass_batch(op1, B, K, ftk.SQ)
        rows_b = _lib.tpl_long_cache_rows(2, 0, n, nl, K)
        assert rows_b == K
        assert op.device_bytes() - op1.device_bytes() == rows_b * nl * 4 * 8 + table
        assert op.flags() & CACHED and same_bits_nan(x, x1)
        op.set_long_cache_solvers(ONE)
        assert np.array_equal(solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ), x1)
        assert op.device_bytes() == op1.device_bytes() and not op.flags() & CACHED
        with pytest.raises(TplError):
            op.set_long_cache_solvers(16)
        # the refused mask left the operator as it was
        assert np.array_equal(solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ), x1)
        assert op.device_bytes() == op1.device_bytes() and not op.flags() & CACHED
    finally:
        op.close()
        op1.close()


def test_mode_zero_caches_nothing(a5k, B5k):
    B, b = np.ascontiguousarray(B5k[:, :3]), B5k[:, 0].copy()
    op, op0 = fresh(a5k, ALL, mode=0), fresh(a5k, None, mode=0)
    try:
        for call in (lambda o: solvers.lanczos_two_pass_batch(o, B, K, ftk.SQ),
                     lambda o: solvers.lanczos_two_pass_multi(o, b, K, FS9[:3]),
                     lambda o: solvers.lanczos_two_pass_batch_multi(o, B, K, FS9[:3]),
                     lambda o: solvers.lanczos_two_pass(o, b, K, ftk.INV)):
            assert same_bits_nan(np.asarray(call(op)), np.asarray(call(op0)))
            assert not op.flags() & CACHED
            assert op.device_bytes() == op0.device_bytes()
    finally:
        op.close()
        op0.close()


# ---- 11. the default is unchanged -----------------------------------------------------------------
def test_default_mask_leaves_multi_and_batch_uncached(a5k, B5k):
    """Without the new setter the multi, batch and batch-multi solves never read the cache
    (this holds before the feature as well: it documents the default)."""
    B, b = np.ascontiguousarray(B5k[:, :3]), B5k[:, 0].copy()
    op = HipCsrOp(a5k)
    try:
        solvers.lanczos_two_pass_multi(op, b, K, FS9[:3])
        assert not op.flags() & CACHED
        solvers.lanczos_two_pass_batch(op, B, K, ftk.SQ)
        assert not op.flags() & CACHED
        solvers.lanczos_two_pass_batch_multi(op, B, K, FS9[:3])
        assert not op.flags() & CACHED
        solvers.lanczos_two_pass(op, b, K, ftk.INV)
        assert op.flags() & CACHED
    finally:
        op.close()
