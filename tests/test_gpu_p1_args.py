"""GPU: the argument plumbing of the pass-one kernels (k_p1_spmv*, k_p1_axpy<NP>).

Those kernels take compact argument structs filled by their launchers (tpl_device.h
P1SpmvArgs / P1AxpyArgs), and the one-graph inv's elimination workgroup is found by an
explicit block index, not through the grid size. The tests aim at a wrong field or a wrong
block: every comparison is BITWISE against the canonical oracle run in the device's layout
(oracle.Operator(a, op.schedule())), as tests/test_gpu_fuzz.py does.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import harness_b

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

ONE_GRAPH = 32  # tpl_op_flags bit 5: the last two-pass solve ran as one device graph
CHUNK_ROWS = 512


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def tridiag_spd(n, seed, hubs=0):
    """Symmetric, strictly diagonally dominant tridiagonal matrix with random values; `hubs`
    evenly spaced rows carry eight more entries (columns h +- 2..5), which makes them long
    rows (11 entries against a short-row threshold of 6) and leaves their neighbours short."""
    rng = np.random.default_rng(seed)
    i = np.arange(n - 1)
    rows, cols = [i], [i + 1]
    if hubs:
        h = (np.arange(hubs) * (n // hubs) + 8).astype(np.int64)
        assert n // hubs >= 11 and h[-1] + 5 < n
        for d in (2, 3, 4, 5):
            rows += [h, h - d]
            cols += [h + d, h]
    r, c = np.concatenate(rows), np.concatenate(cols)
    up = sp.coo_matrix((rng.uniform(-1.0, 1.0, r.size), (r, c)), shape=(n, n)).tocsr()
    a = up + up.T
    a = (a + sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, n))).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def check_pass_one(op, o, b, k):
    d = alg.lanczos_pass_one(op, b, k)
    al, be, st, bn, _ = o.pass_one(b, k)
    assert d.steps_taken == st and d.b_norm == bn
    assert same_bits(d.alphas, al), "alpha"
    assert same_bits(d.betas, be), "beta"
    return d


# ---------------------------------------------------------------- elimination block
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n,g2", [(300, 1), (3584, 7), (4096, 8), (4097, 9)])
def test_elimination_block_against_grid_padding(n, g2, k):
    """One-graph inv: the element grid holds 8 ceil(G2 / 8) blocks, so G2 = 1, 7 and 9 leave
    padding blocks in front of the elimination workgroup and G2 = 8 leaves none. k = 3 is
    the first step that eliminates a row."""
    a = tridiag_spd(n, seed=n)
    b = np.random.default_rng(n + k).standard_normal(n)
    op = HipCsrOp(a)
    sched = op.schedule()
    assert sched["G2"] == g2 and sched["E"] == 512
    o = oracle.Operator(a, sched)
    op.set_device_ftk(1)
    x = solvers.lanczos_two_pass(op, b, k, ftk.INV)
    assert op.flags() & ONE_GRAPH, "the one-graph path was not taken"
    assert same_bits(x, o.lanczos_two_pass(b, k, ftk.INV)), "x, one graph"
    assert same_bits(solvers.lanczos_two_pass(op, b, k, ftk.INV), x), "graph replay"
    op.set_device_ftk(0)
    xh = solvers.lanczos_two_pass(op, b, k, ftk.INV)
    assert not op.flags() & ONE_GRAPH
    assert same_bits(x, xh), "x, host f"
    check_pass_one(op, o, b, k)
    op.close()


# ---------------------------------------------------------------- every k_p1_axpy<NP>, wide
@pytest.fixture(scope="module")
def rhs_132k():
    return np.random.default_rng(11).standard_normal(132000)


@pytest.mark.parametrize("above", [512, 1024, 2048])
def test_axpy_instances_and_wide_spmv(above, rhs_132k):
    """NA_r = chunks + long rows just above 512, 1024 and 2048: k_p1_axpy<4>, <8> and <12>
    (<2> runs in every small case of this file). 132,000 rows make 258 row blocks of 512:
    more than 256 norm partials, reduced by k_p1_spmv_wide; with max_g2 = 256 the
    one-partial k_p1_spmv runs instead."""
    n = 132000
    # n_long = H, chunks = ceil((n - H) / 512): H + chunks = above + 1
    hubs = next(h for h in range(above) if h + -(-(n - h) // CHUNK_ROWS) == above + 1)
    a = tridiag_spd(n, seed=above, hubs=hubs)
    b = rhs_132k
    op = HipCsrOp(a)
    for max_g2 in (0, 256):
        if max_g2:
            op.set_schedule(max_g2=max_g2)
        sched = op.schedule()
        na = len(sched["long_rows"]) + -(-len(sched["short_rows"]) // CHUNK_ROWS)
        assert len(sched["long_rows"]) == hubs and na == above + 1
        assert (sched["G2"] > 256) == (max_g2 == 0), sched["G2"]
        d = check_pass_one(op, oracle.Operator(a, sched), b, 6)
        assert d.steps_taken == 6
    op.close()


# ---------------------------------------------------------------- edge steps and paths
def test_first_step_alone():
    """k = 1: only step j = 1 runs, where r_prev aliases r_cur and beta_0 does not exist."""
    a = tridiag_spd(1500, seed=3, hubs=20)
    b = np.random.default_rng(4).standard_normal(1500)
    op = HipCsrOp(a)
    o = oracle.Operator(a, op.schedule())
    check_pass_one(op, o, b, 1)
    for mode in (1, 0):
        op.set_device_ftk(mode)
        assert same_bits(solvers.lanczos_two_pass(op, b, 1, ftk.INV),
                         o.lanczos_two_pass(b, 1, ftk.INV)), mode
    assert same_bits(solvers.lanczos(op, b, 1, ftk.INV), o.lanczos(b, 1, ftk.INV))
    op.close()


def test_breakdown_on_an_eigenvector():
    """b an eigenvector: r_2 = 0 exactly, k_p1_spmv of step 2 sets the stop flag and every
    later launch of the graph, the elimination workgroup's included, does nothing."""
    n = 1500
    a = tridiag_spd(n, seed=5).tolil()
    a[700, 699] = a[699, 700] = a[700, 701] = a[701, 700] = 0.0  # row 700 stands alone
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    b = np.zeros(n)
    b[700] = 3.0
    op = HipCsrOp(a)
    o = oracle.Operator(a, op.schedule())
    d = check_pass_one(op, o, b, 5)
    assert d.steps_taken == 1
    for mode in (1, 0):
        op.set_device_ftk(mode)
        x = solvers.lanczos_two_pass(op, b, 5, ftk.INV)
        assert bool(op.flags() & ONE_GRAPH) == bool(mode)
        assert same_bits(x, o.lanczos_two_pass(b, 5, ftk.INV)), mode
    assert x[700] == 3.0 / a[700, 700] and np.count_nonzero(x) == 1
    op.close()


@pytest.mark.parametrize("n", [300, 4097])
def test_standard_variant(n):
    """solvers.lanczos: the same step kernels with Vcol non-null (V_k stored)."""
    a = tridiag_spd(n, seed=7 + n, hubs=n // 100)
    b = np.random.default_rng(n).standard_normal(n)
    op = HipCsrOp(a)
    o = oracle.Operator(a, op.schedule())
    assert same_bits(solvers.lanczos(op, b, 7, ftk.INV), o.lanczos(b, 7, ftk.INV))
    op.close()


# ---------------------------------------------------------------- stamp argument
def test_stamp_pointer_in_sampled_steps(kkt5k):
    """A timed one-graph solve with k = 40 passes a non-null stamp pointer to the launches
    of eight middle steps: the same x bit for bit, and every sampled launch wrote its stamp
    (start-to-start times are positive and of a launch's order of magnitude — a stamp left
    unwritten reads as zero and puts them far outside)."""
    a = kkt5k.a
    b = harness_b(a)
    op = HipCsrOp(a)
    op.set_device_ftk(1)
    x0 = solvers.lanczos_two_pass(op, b, 40, ftk.INV)
    assert op.flags() & ONE_GRAPH
    op.enable_timing(True)
    x1 = solvers.lanczos_two_pass(op, b, 40, ftk.INV)
    s_us, a_us, ns = op.step_samples()
    op.enable_timing(False)
    x2 = solvers.lanczos_two_pass(op, b, 40, ftk.INV)
    assert same_bits(x0, x1) and same_bits(x0, x2)
    assert same_bits(x0, oracle.Operator(a, op.schedule()).lanczos_two_pass(b, 40, ftk.INV))
    assert ns == 8 and 0.0 < s_us < 1e3 and 0.0 < a_us < 1e3, (s_us, a_us, ns)
    op.close()
