"""CPU: the fused pass two's row classes (tpl_fused_pass_two_rows, include/tpl.h
tpl_op_set_fused_pass_two; the host function the layout builder classifies with).

A short row is closed when every column is a long row or the row itself, open otherwise; the
hub set H is the open rows plus the long rows they reference. Eligible: some long row (at most
2048), no short row wider than 4, |H| <= 256, every column of an open row in H.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_kkt

import fused_cases as fc
from tpl_amd.operator import fused_pass_two_rows


@pytest.mark.parametrize("arcs", [5000, 50000, 500000])
def test_kkt_fixtures_have_one_leaf(arcs, kkt_tmp):
    """Each fixture has exactly one node of degree <= 4 (degree 1): that node and its arc are
    open, and they touch one further long row."""
    kkt = load_kkt(arcs, kkt_tmp)
    assert fused_pass_two_rows(kkt.a) == (True, 2, 3)
    deg = np.diff(kkt.a.indptr)[kkt.num_arcs:]
    assert np.count_nonzero(deg <= 4) == 1 and deg.min() == 1


def test_tridiagonal_is_all_open():
    n = 1000
    a = sp.diags([np.ones(n - 1), np.full(n, 4.0), np.ones(n - 1)], [-1, 0, 1]).tocsr()
    assert fused_pass_two_rows(a) == (False, n, n)


def test_too_many_open_rows():
    """300 degree-1 nodes: they and their arcs are open, 600 rows, over the cap of 256."""
    el, n_open, n_hub = fused_pass_two_rows(fc.kkt_hubs(hubs=30, leaves=300))
    assert (el, n_open) == (False, 600) and n_hub >= n_open


def test_hub_set_at_the_cap():
    """113 leaves on 30 hubs: 226 open rows + 30 long rows = 256 is allowed, one more leaf
    is not."""
    assert fused_pass_two_rows(fc.kkt_hubs(hubs=30, leaves=113)) == (True, 226, 256)
    assert fused_pass_two_rows(fc.kkt_hubs(hubs=30, leaves=114)) == (False, 228, 258)


def test_self_column_is_closed():
    """D non-empty: an arc row references itself and its two nodes."""
    a = fc.kkt_hubs(hubs=30, d=True)
    assert np.all(np.diff(a.indptr)[:240] == 3)
    assert fused_pass_two_rows(a) == (True, 0, 0)
    assert fused_pass_two_rows(fc.kkt_hubs(hubs=30, leaves=2, d=True)) == (True, 4, 6)


def test_no_long_row_and_wide_short_rows():
    assert fused_pass_two_rows(sp.identity(500, format="csr")) == (False, 0, 0)
    # threshold 16: the hubs (degree 16) are short rows themselves
    a = fc.kkt_hubs(hubs=30)
    assert fused_pass_two_rows(a, 4)[0] and not fused_pass_two_rows(a, 16)[0]


def test_open_shapes_from_the_5k_block(kkt5k):
    assert fused_pass_two_rows(fc.without_leaf(kkt5k)) == (True, 0, 0)
    # p, q and their three arcs; the leaf and its arc; the nodes of degree 2, 3, 4 and their
    # nine arcs: 5 + 2 + 12 open rows
    el, n_open, n_hub = fused_pass_two_rows(fc.with_low_degree_nodes(kkt5k))
    assert (el, n_open) == (True, 19) and n_open < n_hub <= n_open + 12
    # D on the arcs makes the auto threshold 6: the degree-5 and -6 nodes turn short and
    # wide; with the threshold at 4 the rows are the D = 0 block's
    a = fc.with_d(kkt5k)
    assert not fused_pass_two_rows(a)[0]
    assert fused_pass_two_rows(a, 4) == (True, 2, 3)
