"""GPU: the long-row cache of lanczos_two_pass (tpl_op_set_long_cache).

Pass one keeps every long row's sum (A v_j)_r, pass two's cached steps (k_p2_cached) read
them back instead of gathering the long rows again. Pass two regenerates pass one's basis
bit for bit, so the sums are the same words and nothing may change: every result here is
compared with `np.array_equal` against a fresh operator with the cache off (mode 0) — and
the plain solves against the device-order oracle, as test_gpu_parity.py does. flags() bit 8
tells which path the last solve's pass two took.

The 5k-arc KKT (n = 5,115; 114 long rows), k <= 50, except the one at-size case.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import harness_b, load_kkt

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_GRAPH, CACHED = 32, 256
K = 20


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


@pytest.fixture(scope="module")
def a5k(kkt5k):
    return kkt5k.a


@pytest.fixture(scope="module")
def b5k(a5k):
    return harness_b(a5k)


def fresh(a, mode, budget=0, prep=None):
    """A new operator with `prep` applied (layout setters), then the cache mode."""
    op = HipCsrOp(a)
    if prep:
        prep(op)
    op.set_long_cache(mode, budget)
    return op


def solve(a, b, k, f, mode, budget=0, prep=None):
    """-> (x, flags after the solve) of lanczos_two_pass on a fresh operator."""
    op = fresh(a, mode, budget, prep)
    try:
        return solvers.lanczos_two_pass(op, b, k, f), op.flags()
    finally:
        op.close()


def n_long_of(a):
    op = HipCsrOp(a)
    try:
        return len(op.schedule()["long_rows"])
    finally:
        op.close()


# ---- 1. cache on == cache off == oracle, on the three graph families -------------------
@pytest.mark.parametrize("path", ["one_graph", "host_f", "timed"])
def test_on_equals_off_and_oracle(path, a5k, b5k):
    """f = inv on the device (one graph), f on the host (two graphs around the call), live
    timing on (stamped pass one, the step launches a graph of their own)."""
    def prep(op):
        if path == "host_f":
            op.set_device_ftk(0)
        if path == "timed":
            op.enable_timing(True)

    k = 50
    x2, f2 = solve(a5k, b5k, k, ftk.INV, 2, prep=prep)
    x0, f0 = solve(a5k, b5k, k, ftk.INV, 0, prep=prep)
    assert f2 & CACHED and not f0 & CACHED
    assert bool(f2 & ONE_GRAPH) == bool(f0 & ONE_GRAPH) == (path != "host_f")
    assert np.array_equal(x2, x0)
    op = HipCsrOp(a5k)
    xo = oracle.Operator(a5k, op.schedule()).lanczos_two_pass(b5k, k, ftk.INV)
    op.close()
    assert np.array_equal(x2, xo)


def test_repeat_and_mode_switch_on_one_operator(a5k, b5k):
    """The graphs of both modes on one operator: on, on again (replayed), off, on."""
    x0, _ = solve(a5k, b5k, K, ftk.INV, 0)
    op = fresh(a5k, 2)
    try:
        for mode in (2, 2, 0, 2):
            op.set_long_cache(mode)
            assert np.array_equal(solvers.lanczos_two_pass(op, b5k, K, ftk.INV), x0)
            assert bool(op.flags() & CACHED) == (mode == 2)
        with pytest.raises(tpl_amd.TplError):
            op.set_long_cache(3)
    finally:
        op.close()


# ---- 2. the basis ------------------------------------------------------------------------
def test_basis_output_unchanged(a5k, b5k):
    """Pass two's basis output exists on the stand-alone pass two only, which never runs the
    cached kernel: after a cached solve on the same operator, V and x from it equal a
    mode-0 operator's, and the standard pass's V."""
    op2, op0 = fresh(a5k, 2), fresh(a5k, 0)
    try:
        solvers.lanczos_two_pass(op2, b5k, K, ftk.INV)
        assert op2.flags() & CACHED
        out = alg.lanczos_standard(op0, b5k, K)
        d = out.decomposition
        y = 0.1 * np.arange(1, d.steps_taken + 1)
        p2, p0 = (alg.lanczos_pass_two_with_basis(o, b5k, d, y) for o in (op2, op0))
        assert np.array_equal(np.asarray(p2.v_k), np.asarray(p0.v_k))
        assert np.array_equal(np.asarray(p2.v_k), np.asarray(out.v_k))
        assert np.array_equal(np.asarray(p2.x_k), np.asarray(p0.x_k))
    finally:
        op2.close()
        op0.close()


# ---- 3. hand-off shapes, 4. formats ------------------------------------------------------
PREPS = {
    "slices8": lambda op: op.set_slices(8),    # last arrivers beside single-piece rows
    "slices1": lambda op: op.set_slices(1),    # every row finished in place
    "caller_order": lambda op: op.set_reorder(0),      # the window variant
    "fp64_values": lambda op: op.set_value_format(0),
}


@pytest.mark.parametrize("name", sorted(PREPS))
@pytest.mark.parametrize("dev_f", [1, 0])
def test_layouts_on_equals_off(name, dev_f, a5k, b5k):
    def prep(op):
        PREPS[name](op)
        op.set_device_ftk(dev_f)

    x2, f2 = solve(a5k, b5k, K, ftk.INV, 2, prep=prep)
    x0, f0 = solve(a5k, b5k, K, ftk.INV, 0, prep=prep)
    assert f2 & CACHED and not f0 & CACHED
    assert np.array_equal(x2, x0)


def test_layout_variants_are_the_named_ones(a5k):
    """The preparations above reach the layouts they are named for."""
    op = HipCsrOp(a5k)
    try:
        op.set_slices(8)
        assert op.schedule()["slices"] == 8
        op.set_slices(0)
        op.set_reorder(0)
        assert op.kernel_variant() & 64 and not op.flags() & 64   # window, caller's order
        op.set_reorder(2)
        op.set_value_format(0)
        assert not op.kernel_variant() & (8 | 16 | 32)
    finally:
        op.close()


@pytest.mark.parametrize("reorder", [2, 0])
@pytest.mark.parametrize("dev_f", [1, 0])
def test_last_wave_with_few_long_rows(reorder, dev_f):
    """66 long rows: the second wave of the long-row workgroup has two live lanes, fewer
    than the eight whose record fields the epilogue reads with readlane (at 500k arcs,
    1,154 long rows leave two lanes as well). The long rows are scattered in the caller's
    order (reorder 0: their rows come from the cache's index table)."""
    from conftest import banded_hub
    a = banded_hub(n=6000, hub_every=91, hub_half=40)
    b = std_rng_vector(a.shape[0]) - 0.5

    def prep(op):
        op.set_reorder(reorder)
        op.set_device_ftk(dev_f)
        assert len(op.schedule()["long_rows"]) == 66

    x2, f2 = solve(a, b, K, ftk.INV, 2, prep=prep)
    x0, f0 = solve(a, b, K, ftk.INV, 0, prep=prep)
    assert f2 & CACHED and not f0 & CACHED
    assert np.array_equal(x2, x0)


# ---- every layout instance, both step kernels ---------------------------------------------
import layout_cases as lc  # noqa: E402


@pytest.mark.parametrize("name", list(lc.VARIANTS) + list(lc.EDGES))
def test_both_step_kernels_on_every_layout_case(name):
    """tests/test_gpu_variants.py runs every layout case with the default settings, which
    now means k_p2_cached<F> wherever the case has long rows. Here the same cases with the
    cache off and on: k_p2_spmv<F> stays pinned on all of its instances, and both kernels
    give the oracle's bits (k = 7 and 8: both tails of the grouped flush; one graph and f
    on the host)."""
    c = lc.case(name)
    b = np.random.default_rng(len(name)).standard_normal(c.a.shape[0])
    for mode in (0, 2):
        op = HipCsrOp(c.a)
        try:
            c.apply_setters(op)
            assert op.kernel_variant() == c.F
            op.set_long_cache(mode)
            o = oracle.Operator(c.a, op.schedule())
            has_long = len(op.schedule()["long_rows"]) > 0
            for dev_f in (1, 0):
                op.set_device_ftk(dev_f)
                for k in (7, 8):
                    x = solvers.lanczos_two_pass(op, b, k, ftk.INV)
                    assert np.array_equal(x, o.lanczos_two_pass(b, k, ftk.INV)), (mode, dev_f, k)
                    assert bool(op.flags() & CACHED) == (mode == 2 and has_long)
        finally:
            op.close()


# ---- 5. partial cache --------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1, 2, K - 2, K, 3 * K])
@pytest.mark.parametrize("dev_f", [1, 0])
def test_partial_cache(rows, dev_f, a5k, b5k):
    """A budget of `rows` steps: steps 1 .. rows run k_p2_cached, the rest k_p2_spmv."""
    nl = n_long_of(a5k)
    prep = lambda op: op.set_device_ftk(dev_f)
    x0, _ = solve(a5k, b5k, K, ftk.INV, 0, prep=prep)
    op = fresh(a5k, 1, 8 * nl * rows + 7, prep)   # + 7: the budget rounds down to whole rows
    try:
        base = op.device_bytes()
        x = solvers.lanczos_two_pass(op, b5k, K, ftk.INV)
        assert np.array_equal(x, x0)
        assert bool(op.flags() & CACHED) == (rows > 0)
        grown = op.device_bytes() - base
    finally:
        op.close()
    op = fresh(a5k, 0, 0, prep)
    try:
        base0 = op.device_bytes()
        solvers.lanczos_two_pass(op, b5k, K, ftk.INV)
        assert grown - (op.device_bytes() - base0) == 8 * nl * min(rows, K)
    finally:
        op.close()


# ---- 6. breakdown --------------------------------------------------------------------------
@pytest.mark.parametrize("dev_f", [1, 0])
def test_breakdown(dev_f, a5k, b5k):
    """Pass one stops before k: the KKT block beside diag(2, 3, 5), b on the diagonal block
    alone — e_1 (the existing breakdown test's right-hand side: one step) and e_1 + e_2 (two
    steps, one live cached step). Rows at and past the stop are never written by that pass;
    a first solve with a full b leaves other words in them, which the inactive launches of
    the one-graph solve read and must not store."""
    a = sp.block_diag([a5k, sp.diags([2.0, 3.0, 5.0])]).tocsr()
    a.sort_indices()
    n = a.shape[0]
    full = np.concatenate([b5k, np.ones(3)])
    for tail, steps in (([1.0, 0.0, 0.0], 1), ([1.0, 1.0, 0.0], 2)):
        b = np.concatenate([np.zeros(n - 3), tail])
        res = {}
        for mode in (2, 0):
            op = fresh(a, mode, prep=lambda op: op.set_device_ftk(dev_f))
            try:
                xf = solvers.lanczos_two_pass(op, full, K, ftk.INV)
                x = solvers.lanczos_two_pass(op, b, K, ftk.INV)
                flags = op.flags()
                res[mode] = (xf, x, alg.lanczos_pass_one(op, b, K).steps_taken)
            finally:
                op.close()
            # host f: pass two has steps - 1 launches; one graph: all k - 1 are launched
            assert bool(flags & ONE_GRAPH) == (dev_f == 1)
            assert bool(flags & CACHED) == (mode == 2 and (dev_f == 1 or steps >= 2))
        assert res[2][2] == res[0][2] == steps
        assert np.array_equal(res[2][0], res[0][0])
        assert np.array_equal(res[2][1], res[0][1])
        assert np.all(res[2][1][: n - 3] == 0.0) and np.any(res[2][1][n - 3:] != 0.0)


# ---- 7. no stale reuse -----------------------------------------------------------------------
def test_no_stale_reuse(a5k, b5k):
    """One operator: b1 at k = 20, b2 at k = 12, then the entry points that must never read
    the cache — each result equals a fresh operator's."""
    n = a5k.shape[0]
    b1, b2 = b5k, std_rng_vector(n) - 0.5
    B = np.stack([b2, b1, b2 + b1], axis=1)
    fs = [ftk.INV, ftk.SQ]

    def run(op, what):
        if what == "b1":
            return solvers.lanczos_two_pass(op, b1, 20, ftk.INV)
        if what == "b2":
            return solvers.lanczos_two_pass(op, b2, 12, ftk.INV)
        if what == "pass_two":
            d = alg.lanczos_pass_one(op, b2, 12)
            return alg.lanczos_pass_two(op, b2, d, ftk.INV(d.alphas, d.betas) * d.b_norm)
        if what == "multi":
            return solvers.lanczos_two_pass_multi(op, b2, 12, fs)
        return solvers.lanczos_two_pass_batch(op, B, 12, ftk.SQ)

    seq = ["b1", "b2", "pass_two", "multi", "batch", "b1"]
    want = {}
    for what in set(seq):
        op = fresh(a5k, 0)
        try:
            want[what] = np.asarray(run(op, what))
        finally:
            op.close()
    op = fresh(a5k, 2)
    try:
        for what in seq:
            got = np.asarray(run(op, what))
            assert np.array_equal(got, want[what]), what
            assert bool(op.flags() & CACHED) == (what in ("b1", "b2")), what
    finally:
        op.close()
    assert np.array_equal(want["pass_two"], want["b2"])


# ---- 8. no long rows ------------------------------------------------------------------------
def test_no_long_rows():
    n = 3001
    a = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    b = std_rng_vector(n) - 0.5
    out = {}
    for mode in (2, 0):
        op = fresh(a, mode)
        try:
            assert len(op.schedule()["long_rows"]) == 0
            x = solvers.lanczos_two_pass(op, b, K, ftk.INV)
            out[mode] = (x, op.device_bytes(), op.flags())
        finally:
            op.close()
    assert np.array_equal(out[2][0], out[0][0])
    assert out[2][1] == out[0][1]
    assert not out[2][2] & CACHED


# ---- 9. accounting ---------------------------------------------------------------------------
def test_accounting(a5k, b5k):
    """device_bytes grows by rows x n_long x 8 when the state is first sized (rows = the
    state's capacity at k = 20: the default budget holds more), and is the mode-0 figure
    again after set_long_cache(0) and a new solve."""
    from tpl_amd import _lib
    n, nl = a5k.shape[0], n_long_of(a5k)
    op0 = fresh(a5k, 0)
    op = fresh(a5k, 2)
    try:
        assert op.device_bytes() == op0.device_bytes()      # nothing before the first solve
        x0 = solvers.lanczos_two_pass(op0, b5k, K, ftk.INV)
        x = solvers.lanczos_two_pass(op, b5k, K, ftk.INV)
        rows = _lib.tpl_long_cache_rows(2, 0, n, nl, K)
        assert rows == K
        assert op.device_bytes() - op0.device_bytes() == rows * nl * 8
        op.set_long_cache(0, 0)
        assert np.array_equal(solvers.lanczos_two_pass(op, b5k, K, ftk.INV), x0)
        assert op.device_bytes() == op0.device_bytes() and not op.flags() & CACHED
        assert np.array_equal(x, x0)
    finally:
        op.close()
        op0.close()


# ---- 10. at size -------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_headline_digest_with_cache(kkt_tmp):
    """The operator the bench times (500k arcs, pinned locality order), k = 500, f = inv:
    the cache on (the default), the fixture's x digest."""
    sys.path.insert(0, ROOT)
    from bench import PINNED_ORDER_GROUPS
    a = load_kkt(500000, kkt_tmp).a
    op = HipCsrOp(a)
    try:
        op.set_order_groups(PINNED_ORDER_GROUPS[500000])
        x = solvers.lanczos_two_pass(op, harness_b(a), 500, ftk.INV)
        assert op.flags() & CACHED and op.flags() & ONE_GRAPH
    finally:
        op.close()
    with open(os.path.join(ROOT, "tests", "golden", "parity.json")) as f:
        exp = json.load(f)["workloads"]["headline"]
    digest = hashlib.sha256(x.tobytes()).hexdigest()[:16]
    assert digest == exp["x"] == "7bf2409fbbfac620"
