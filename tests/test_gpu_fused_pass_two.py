"""GPU: the fused pass two of lanczos_two_pass (tpl_op_set_fused_pass_two).

Where the long-row cache holds every step and the layout's rows decouple, pass two is two
launches (k_p2_hub, k_p2_rows) instead of steps - 1 step launches. Bits are the contract:
every result here is compared word for word (`np.array_equal` on the bits) against a fresh operator with the mode
off — and the plain solves against the device-order oracle. flags() bit 9 tells which path
the last pass two took (bit 8, the long-row cache, is set with it).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import banded_hub, harness_b

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

import fused_cases as fc  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402
from tpl_amd.operator import fused_pass_two_rows  # noqa: E402

ONE_GRAPH, CACHED, FUSED = 32, 256, 512
K = 20
PATHS = ["one_graph", "host_f", "timed"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


@pytest.fixture(scope="module")
def a5k(kkt5k):
    return kkt5k.a


@pytest.fixture(scope="module")
def b5k(a5k):
    """Not the harness b = A 1 / sqrt(n): on the KKT block it makes every alpha zero and an
    odd k's T_k singular."""
    return std_rng_vector(a5k.shape[0]) - 0.5


def same(x, y):
    """Word for word (np.array_equal on the bits: a NaN equals only itself)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def path_prep(path):
    def prep(op):
        if path == "host_f":
            op.set_device_ftk(0)
        if path == "timed":
            op.enable_timing(True)
    return prep


def fresh(a, mode, prep=None):
    op = HipCsrOp(a)
    if prep:
        prep(op)
    op.set_fused_pass_two(mode)
    return op


def solve(a, b, k, mode, prep=None, f=ftk.INV):
    """-> (x, flags after the solve) of lanczos_two_pass on a fresh operator."""
    op = fresh(a, mode, prep)
    try:
        return solvers.lanczos_two_pass(op, b, k, f), op.flags()
    finally:
        op.close()


def both(a, b, k, prep=None, fused=True):
    """Mode auto against mode off on fresh operators: equal bits, bit 9 as expected. -> x."""
    x2, f2 = solve(a, b, k, 2, prep)
    x0, f0 = solve(a, b, k, 0, prep)
    assert not f0 & FUSED
    assert bool(f2 & FUSED) == (fused and k >= 2), (k, f2)
    assert not f2 & FUSED or f2 & CACHED
    assert bool(f0 & CACHED) == bool(f2 & CACHED)
    assert same(x2, x0)
    return x2


# ---- 1. the 5k block: every tail of the grouped flush, the three graph families -----------
@pytest.fixture(scope="module")
def oracle5k(a5k, b5k):
    """The device-order oracle's x for every k below, computed once."""
    op = HipCsrOp(a5k)
    o = oracle.Operator(a5k, op.schedule())
    op.close()
    return {k: o.lanczos_two_pass(b5k, k, ftk.INV) for k in (1, 2, 3, 4, 5, 7, 8, 50)}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 50])
def test_fused_equals_steps_and_oracle(k, path, a5k, b5k, oracle5k):
    """n = 5,115, 114 long rows, the last chunk partial. k = 1: the empty pass (bit 9 clear,
    as bit 8 is); k = 2 .. 8: both tails of the grouped flush and the whole groups."""
    x = both(a5k, b5k, k, path_prep(path))
    assert same(x, oracle5k[k])


def test_timed_path_reports_the_regenerated_steps(a5k, b5k):
    op = fresh(a5k, 2, path_prep("timed"))
    try:
        solvers.lanczos_two_pass(op, b5k, K, ftk.INV)
        assert op.flags() & FUSED
        _, p2_us, launches = op.pass_timing()
        assert launches == K - 1 and p2_us > 0.0
    finally:
        op.close()


def test_50k_is_fused_under_the_defaults(kkt50k):
    a = kkt50k.a
    b = harness_b(a)
    op = HipCsrOp(a)
    try:
        x = solvers.lanczos_two_pass(op, b, K, ftk.INV)
        assert op.flags() & FUSED and op.flags() & CACHED
        xo = oracle.Operator(a, op.schedule()).lanczos_two_pass(b, K, ftk.INV)
    finally:
        op.close()
    assert same(x, xo)
    x0, f0 = solve(a, b, K, 0)
    assert not f0 & FUSED and same(x, x0)


# ---- 2. breakdown ------------------------------------------------------------------------
@pytest.mark.parametrize("dev_f", [1, 0])
def test_breakdown(dev_f, a5k, b5k):
    """Pass one stops after 1 and after 2 steps (the KKT block beside diag(2, 3, 5), b on the
    diagonal block alone; its rows are closed by their self column). On the one-graph path
    the step count is device-held. A full-b solve runs first on the same operator, so the
    cache rows hold its v_j."""
    a = sp.block_diag([a5k, sp.diags([2.0, 3.0, 5.0])]).tocsr()
    a.sort_indices()
    n = a.shape[0]
    full = np.concatenate([b5k, np.ones(3)])
    for tail, steps in (([1.0, 0.0, 0.0], 1), ([1.0, 1.0, 0.0], 2)):
        b = np.concatenate([np.zeros(n - 3), tail])
        res = {}
        for mode in (2, 0):
            op = fresh(a, mode, lambda op: op.set_device_ftk(dev_f))
            try:
                xf = solvers.lanczos_two_pass(op, full, K, ftk.INV)
                assert bool(op.flags() & FUSED) == (mode == 2)
                x = solvers.lanczos_two_pass(op, b, K, ftk.INV)
                flags = op.flags()
                res[mode] = (xf, x, alg.lanczos_pass_one(op, b, K).steps_taken)
            finally:
                op.close()
            assert bool(flags & ONE_GRAPH) == (dev_f == 1)
            # host f: the host knows steps (1: no pass two); one graph: the kernels find out
            assert bool(flags & FUSED) == (mode == 2 and (dev_f == 1 or steps >= 2))
        assert res[2][2] == res[0][2] == steps
        assert same(res[2][0], res[0][0])
        assert same(res[2][1], res[0][1])
        assert np.all(res[2][1][: n - 3] == 0.0) and np.any(res[2][1][n - 3:] != 0.0)


# ---- 3. open-set shapes ---------------------------------------------------------------------
def shape_case(name, kkt5k):
    """-> (matrix, layout setters, (eligible, n_open, n_hub) or None to skip that check)."""
    if name == "no_open_row":
        return fc.without_leaf(kkt5k), None, (True, 0, 0)
    if name == "open_rows_reference_open_rows":
        return fc.with_low_degree_nodes(kkt5k), None, None
    if name == "d_nonempty_w3":
        return fc.with_d(kkt5k), lambda op: op.set_schedule(4, 0), None
    if name == "kkt_66_long_rows":
        return fc.kkt_hubs(hubs=66, leaves=3), None, (True, 6, 9)
    if name == "hub_set_at_the_cap":
        return fc.kkt_hubs(hubs=30, leaves=113), None, (True, 226, 256)
    raise KeyError(name)


@pytest.mark.parametrize("path", ["one_graph", "host_f"])
@pytest.mark.parametrize("name", ["no_open_row", "open_rows_reference_open_rows", "d_nonempty_w3",
                                  "kkt_66_long_rows", "hub_set_at_the_cap"])
def test_open_set_shapes(name, path, kkt5k):
    a, setters, verdict = shape_case(name, kkt5k)
    if verdict is not None:
        assert fused_pass_two_rows(a) == verdict
    b = std_rng_vector(a.shape[0]) - 0.5

    def prep(op):
        if setters:
            setters(op)
        path_prep(path)(op)
        sched = op.schedule()
        if name == "kkt_66_long_rows":  # the long-row workgroup's last wave: two live lanes
            assert len(sched["long_rows"]) == 66
        if name == "d_nonempty_w3":
            assert op.kernel_variant() & 7 == 3
        if name == "open_rows_reference_open_rows":  # width-2 arcs beside nodes of width 2 - 4
            assert op.kernel_variant() & 7 == 0

    for k in (7, 8):
        x = both(a, b, k, prep)
        op = HipCsrOp(a)
        if setters:
            setters(op)
        xo = oracle.Operator(a, op.schedule()).lanczos_two_pass(b, k, ftk.INV)
        op.close()
        assert same(x, xo)


@pytest.mark.parametrize("dev_f", [1, 0])
def test_ineligible_layouts_fall_back(dev_f, a5k, b5k):
    """banded_hub (66 long rows, every short row open), the caller's row order (scattered
    long rows) and too many open rows: the step launches, equal bits, bit 9 clear."""
    prep = lambda op: op.set_device_ftk(dev_f)
    a = banded_hub(n=6000, hub_every=91, hub_half=40)
    assert not fused_pass_two_rows(a)[0]
    both(a, std_rng_vector(a.shape[0]) - 0.5, K, prep, fused=False)
    both(a5k, b5k, K, lambda op: (op.set_reorder(0), prep(op)), fused=False)
    a = fc.kkt_hubs(hubs=30, leaves=114)
    both(a, std_rng_vector(a.shape[0]) - 0.5, K, prep, fused=False)


# ---- 4. formats ----------------------------------------------------------------------------
@pytest.mark.parametrize("dev_f", [1, 0])
def test_fp64_values_and_int32_columns(dev_f, a5k, b5k):
    def prep(op):
        op.set_value_format(False)
        op.set_device_ftk(dev_f)
        assert not op.kernel_variant() & (8 | 16 | 32)

    both(a5k, b5k, K, prep)


# ---- 5. one operator across several solves ----------------------------------------------------
def test_one_operator_across_solves(a5k, b5k):
    """b1 at k = 20, b2 at k = 12, b1 again: the cache rows hold v_j after a fused solve and
    the next pass one must refill them. Then the mode off / auto / off / auto, then the
    multi-function and batch solves, which never run fused."""
    n = a5k.shape[0]
    b1, b2 = b5k, std_rng_vector(n) - 0.5
    ref = fresh(a5k, 0)
    op = fresh(a5k, 2)
    try:
        for b, k in ((b1, 20), (b2, 12), (b1, 20)):
            assert same(solvers.lanczos_two_pass(op, b, k, ftk.INV),
                                  solvers.lanczos_two_pass(ref, b, k, ftk.INV))
            assert op.flags() & FUSED and not ref.flags() & FUSED
        x1 = solvers.lanczos_two_pass(ref, b1, K, ftk.INV)
        for mode in (0, 2, 0, 2):
            op.set_fused_pass_two(mode)
            assert same(solvers.lanczos_two_pass(op, b1, K, ftk.INV), x1)
            assert bool(op.flags() & FUSED) == (mode == 2) and op.flags() & CACHED
        with pytest.raises(tpl_amd.TplError):
            op.set_fused_pass_two(1)
        fs = [ftk.INV, ftk.SQ]
        B = np.stack([b2, b1, b2 + b1], axis=1)
        for o in (op, ref):
            o.set_long_cache_solvers(1 | 2 | 4)
        xm, xm0 = (np.asarray(solvers.lanczos_two_pass_multi(o, b2, K, fs)) for o in (op, ref))
        assert not op.flags() & FUSED and op.flags() & CACHED
        assert same(xm, xm0)
        xb, xb0 = (np.asarray(solvers.lanczos_two_pass_batch(o, B, K, ftk.SQ)) for o in (op, ref))
        assert not op.flags() & FUSED
        assert same(xb, xb0)
        assert same(solvers.lanczos_two_pass(op, b1, K, ftk.INV), x1)
        assert op.flags() & FUSED
        assert op.device_bytes() == ref.device_bytes()
    finally:
        op.close()
        ref.close()


@pytest.mark.parametrize("dev_f", [1, 0])
def test_partial_budget_stays_on_the_step_launches(dev_f, a5k, b5k):
    """rows = k - 2: the cache does not hold every step, so the steps run as before."""
    op = HipCsrOp(a5k)
    nl = len(op.schedule()["long_rows"])
    op.close()

    def prep(op):
        op.set_device_ftk(dev_f)
        op.set_long_cache(1, 8 * nl * (K - 2))

    x2, f2 = solve(a5k, b5k, K, 2, prep)
    x0, _ = solve(a5k, b5k, K, 0, prep)
    assert f2 & CACHED and not f2 & FUSED
    assert same(x2, x0)


def test_device_bytes_equal_with_the_mode_off(a5k, b5k):
    op2, op0 = fresh(a5k, 2), fresh(a5k, 0)
    try:
        assert op2.device_bytes() == op0.device_bytes()
        for o in (op2, op0):
            solvers.lanczos_two_pass(o, b5k, K, ftk.INV)
        assert op2.flags() & FUSED and not op0.flags() & FUSED
        assert op2.device_bytes() == op0.device_bytes()
    finally:
        op2.close()
        op0.close()


# ---- 6. every layout case, fused off and auto -------------------------------------------------
import layout_cases as lc  # noqa: E402


@pytest.mark.parametrize("name", list(lc.VARIANTS) + list(lc.EDGES))
def test_every_layout_case_fused_off_and_auto(name):
    """With the mode off the cached step kernel k_p2_cached<F> stays pinned on every layout
    case that has long rows (under the defaults the eligible ones now run fused); with the
    mode auto every case gives the same oracle bits, fused exactly where the operator's own
    rows say so (k = 7 and 8: both tails of the grouped flush; one graph and f on the host)."""
    c = lc.case(name)
    b = np.random.default_rng(len(name)).standard_normal(c.a.shape[0])
    for mode in (0, 2):
        op = HipCsrOp(c.a)
        try:
            c.apply_setters(op)
            op.set_fused_pass_two(mode)
            sched = op.schedule()
            o = oracle.Operator(c.a, sched)
            has_long = len(sched["long_rows"]) > 0
            fused = set()
            for dev_f in (1, 0):
                op.set_device_ftk(dev_f)
                for k in (7, 8):
                    x = solvers.lanczos_two_pass(op, b, k, ftk.INV)
                    assert same(x, o.lanczos_two_pass(b, k, ftk.INV)), (mode, dev_f, k)
                    assert bool(op.flags() & CACHED) == has_long
                    fused.add(bool(op.flags() & FUSED))
            assert len(fused) == 1 and (mode == 2 or fused == {False})
        finally:
            op.close()
