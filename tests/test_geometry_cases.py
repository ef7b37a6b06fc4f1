"""CPU: the geometry table (tests/geometry_cases.py) is what the layout rule gives, covers the
geometries it is meant to cover, changes the oracle's bits, and the composed oracle
(tests/composed_oracle.py) agrees with the oracle's own two-pass solve. No GPU.
"""
import numpy as np
import pytest

import composed_oracle as co
import geometry_cases as gc
import state_cases as sc
import tpl_amd
from tpl_amd import ftk

K, KB = sc.K_SMALL, sc.K_BIG


@pytest.mark.parametrize("case", gc.CASES, ids=gc.CASE_IDS)
def test_table_is_the_layout_rule(case):
    """conftest.canon_schedule on the locality-ordered matrix gives the table's G2, E, row split
    and empty trailing blocks; with no setter involved the runtime's own host plan agrees with
    it in every field."""
    a = gc.cached_matrix(case.mat)
    s = gc.host_schedule(case)
    assert (s["G2"], s["E"]) == (case.G2, case.E)
    assert (len(s["short_rows"]), len(s["long_rows"])) == (case.n_short, case.n_long)
    assert gc.empty_blocks(s, a.shape[0]) == case.empty
    assert case.E % 512 == 0 and case.G2 * case.E >= a.shape[0]
    if case.max_g2 is None:
        plan = tpl_amd.operator.HostPlan(a)
        try:
            assert gc.same_schedule(plan.schedule(), s)
        finally:
            plan.close()
    else:
        d = _default_of(case)
        assert (d["G2"], d["E"]) != (case.G2, case.E) and d["E"] == 512


def test_table_covers_the_geometries():
    """Chunks per block 2, 3 and at least 5; a chunk count that is no multiple of it; empty
    trailing blocks; more than eight row blocks (rb_first hands some XCDs two) with more than
    one chunk each; one row block. And the large band's default geometry, which no case runs,
    is the 512-row one."""
    cpes = {c.cpe for c in gc.CASES}
    assert {2, 3} <= cpes and max(cpes) >= 5
    assert any(c.cpe > 1 and c.n_chunks % c.cpe for c in gc.CASES)
    assert any(c.empty for c in gc.CASES) and all(c.empty < c.G2 for c in gc.CASES)
    assert any(c.G2 > 8 and c.cpe > 1 for c in gc.CASES)
    assert any(c.G2 == 1 for c in gc.CASES)
    assert {c.mat for c in gc.CASES} == set(gc.MATRICES)
    assert len(set(gc.CASE_IDS)) == len(gc.CASES)
    from conftest import elem_layout
    assert elem_layout(9473) == (19, 512)


def test_kkt_block_is_fused_eligible():
    """The KKT block runs the fused pass two at default settings: the row classes allow it
    (tpl_fused_pass_two_rows) and the default long-row cache holds K_BIG steps
    (tpl_long_cache_rows: two vectors' bytes). With 30 hubs no number of leaves past 113 is
    eligible, which is why the block is not the 30-hub one (geometry_cases' docstring)."""
    from fused_cases import kkt_hubs
    el, n_open, n_hub = tpl_amd.operator.fused_pass_two_rows(gc.cached_matrix("kkt3002"))
    assert (el, n_open, n_hub) == (True, 2 * gc.KKT_LEAVES, 3 * gc.KKT_LEAVES)
    n_long = next(c.n_long for c in gc.CASES if c.mat == "kkt3002")
    assert tpl_amd._lib.tpl_long_cache_rows(2, 0, 3002, n_long, sc.K_BIG) == sc.K_BIG
    assert tpl_amd._lib.tpl_long_cache_rows(2, 0, 3002, 320, sc.K_BIG) < sc.K_BIG
    assert tpl_amd.operator.fused_pass_two_rows(kkt_hubs(30, leaves=113, d=True))[0]
    assert not tpl_amd.operator.fused_pass_two_rows(kkt_hubs(30, leaves=114, d=True))[0]
    assert not tpl_amd.operator.fused_pass_two_rows(kkt_hubs(30, leaves=1366, d=True))[0]
    assert not tpl_amd.operator.fused_pass_two_rows(gc.cached_matrix("band3001"))[0]


def _default_of(case):
    from conftest import canon_schedule
    return canon_schedule(gc.cached_matrix(case.mat), reorder=True)


@pytest.mark.parametrize("case", [c for c in gc.CASES if c.max_g2 is not None],
                         ids=[c.id for c in gc.CASES if c.max_g2 is not None])
def test_geometry_changes_the_oracles_bits(case):
    """The oracle's pass one or its two-pass x at the case's geometry differs in at least one
    word from the default geometry's, at the K_BIG steps the GPU test runs: a device that
    ignored the setter, or that reduced in the 512-row order, cannot pass the bitwise GPU test.
    (Only the norms read G2 and E, and a square root often rounds two sums that differ in the
    last place to one value: band9473 at max_g2 = 9 coincides with the default geometry for
    column 0's first twelve steps, and parts at step 13.)"""
    import oracle
    I = gc.inputs(case)
    base = oracle.Operator(I.a, _default_of(case))
    w = lambda x: np.ascontiguousarray(x).view(np.uint64)
    al, be, st, bn, _ = I.oracle().pass_one(I.b, KB)
    al0, be0, st0, bn0, _ = base.pass_one(I.b, KB)
    x, x0 = I.oracle().lanczos_two_pass(I.b, KB, ftk.INV), base.lanczos_two_pass(I.b, KB, ftk.INV)
    assert np.all(np.isfinite(x)) and st == st0 == KB
    differ = int(np.sum(w(al) != w(al0))) + int(np.sum(w(be) != w(be0))) + int(bn != bn0)
    print("%s: %d of %d alphas/betas and %d of %d words of x differ from the default geometry"
          % (case.id, differ, 2 * KB, int(np.sum(w(x) != w(x0))), x.size))
    assert differ + int(np.sum(w(x) != w(x0))) >= 1


@pytest.mark.parametrize("case", gc.CASES, ids=gc.CASE_IDS)
def test_composed_oracle_is_the_single_solves(case):
    """Host only: what composed_oracle expects of the multi-function, batch and batch-multi
    solves is, column by column, oracle.Operator.lanczos_two_pass of that column with that
    function; of the cut passes and the tolerance solves, lanczos_two_pass at the cut."""
    I, o = gc.inputs(case), gc.inputs(case).oracle()
    m, s = 3, 3
    w = lambda x: np.ascontiguousarray(x).view(np.uint64)
    eq = lambda x, y: x.shape == y.shape and np.array_equal(w(x), w(y))
    fs = [ftk.inv_shift(sg) for sg in sc.sigmas(m)]
    single = {(c, i): o.lanczos_two_pass(I.B[:, c], K, fs[i]) for c in range(s) for i in range(m)}
    p = {"k": K, "m": m, "s": s}
    X, = co.expect("two_pass_multi", I, p)
    assert X.shape == (I.n, m) and all(eq(X[:, i], single[(0, i)]) for i in range(m))
    X, = co.expect("pass_two_multi", I, p)       # the same y, handed to the stand-alone pass
    assert all(eq(X[:, i], single[(0, i)]) for i in range(m))
    X, = co.expect("two_pass_batch_multi", I, p)
    assert X.shape == (I.n, m, s)
    assert all(eq(X[:, i, c], single[(c, i)]) for c in range(s) for i in range(m))
    X, = co.expect("pass_two_batch_multi", I, p)
    assert all(eq(X[:, i, c], single[(c, i)]) for c in range(s) for i in range(m))
    X, = co.expect("two_pass_batch_s3", I, p)
    assert all(eq(X[:, c], o.lanczos_two_pass(I.B[:, c], K, ftk.INV)) for c in range(s))
    X, = co.expect("two_pass_batch", I, p)
    assert all(eq(X[:, c], o.lanczos_two_pass(I.B[:, c], K, sc.sq_closure)) for c in range(s))
    # cut passes: column (c, i) is the cuts[i]-step solve (pass one's steps are a prefix)
    X, = co.expect("pass_two_batch_multi_cut", I, p)
    X1, = co.expect("pass_two_multi_cut", I, p)
    for c in range(s):
        for i, cut in enumerate(sc.cuts(I.dec(c, K).steps_taken, m, c)):
            d = I.dec(c, K)
            y = np.zeros(cut)
            y[:] = I.Y(c, K, m)[:cut, i]
            x = o.pass_two(I.B[:, c], d.alphas[:cut], d.betas[:cut - 1], cut, d.b_norm, y)[0]
            assert eq(X[:, i, c], x), (c, i, cut)
            if c == 0:
                assert eq(X1[:, i], x), (i, cut)
    # tolerance solves: x is the m*-step solve, and the mix of stops is not trivial
    x, steps, conv, _ = co.expect("two_pass_inv_tol_met", I, p)
    assert conv[0] and 1 <= steps[0] < K and eq(x, o.lanczos_two_pass(I.b, int(steps[0]), ftk.INV))
    x, steps, conv, _ = co.expect("two_pass_inv_tol_never", I, p)
    assert not conv[0] and steps[0] == K and eq(x, single_inv(o, I, K))
    X, steps, conv, pre = co.expect("two_pass_batch_shifted_inv_tol", I, p)
    assert X.shape == (I.n, m, s) and steps.shape == conv.shape == (m, s)
    for c in range(s):
        for i in range(m):
            assert eq(X[:, i, c], o.lanczos_two_pass(I.B[:, c], int(steps[i, c]), fs[i])), (c, i)
    assert len({int(v) for v in steps.ravel()}) >= 2 and conv.any()
    X1, steps1, conv1, _ = co.expect("two_pass_shifted_inv_tol", I, p)
    assert eq(X1, np.ascontiguousarray(X[:, :, 0])) and np.array_equal(steps1, steps[:, 0])


def single_inv(o, I, k):
    return o.lanczos_two_pass(I.b, k, ftk.INV)


def test_inputs_of_the_call_order_matrices_are_unchanged():
    """Inputs built from a matrix handed in are the Inputs built by name: the recipe is one
    piece of code (the call-order tests' fresh results rest on these right-hand sides)."""
    for mat in sc.MATRICES:
        I = sc.inputs(mat)
        J = sc.Inputs(mat + "-again", a=sc.matrix(mat))
        assert np.array_equal(I.B.view(np.uint64), J.B.view(np.uint64))
        assert (I.tol_met, I.tol_mix) == (J.tol_met, J.tol_mix)
        K2 = sc.Inputs(mat + "-shared", a=I.a, B=I.B)
        assert K2.B is I.B and K2.tol_mix == I.tol_mix


def test_large_matrix_eigenvectors_are_eigenvectors():
    """Past DENSE_EIG_MAX rows column 1's five eigenvectors come from shift-and-invert Lanczos:
    each is an eigenvector to rounding, and they are five different ones."""
    a = gc.cached_matrix("band9473")
    assert a.shape[0] > sc.DENSE_EIG_MAX >= 3002
    v = sc.Inputs.eigenvectors5(a)
    assert v.shape == (a.shape[0], 5)
    lam = np.einsum("ij,ij->j", v, a @ v)
    res = np.linalg.norm(a @ v - v * lam, axis=0)
    assert np.all(res <= 1e-9 * np.abs(lam)), res
    assert np.linalg.matrix_rank(v) == 5
