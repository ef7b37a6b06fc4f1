"""GPU: the fused pass two with several steps per barrier (tpl_k_p2_fused.hip).

k_p2_rows<W, NL> stages S consecutive cache rows per barrier as one flat run, keeps
kRowsDepth such blocks in registers, reads the step records by scalar loads and lets a wave
whose rows have neither a self column nor padding (a clean wave) or no live row at all (an
idle wave) skip what it does not need; k_p2_hub steps a hub set of a few members by lane
broadcasts and sums only up to the widest open row. Every case solves with the mode auto and
with the mode off on fresh operators and compares the bits, then the device-order oracle's;
bits 8 and 9 of flags() say the cache and the fused kernels ran. S, B and the small-set bound
come from the source's constants (tests/fused_steps_cases.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

import fused_cases as fc  # noqa: E402
import fused_steps_cases as sc  # noqa: E402
import fused_tuned_cases as tc  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd.operator import fused_pass_two_rows  # noqa: E402

CACHED, FUSED = 256, 512
PATHS = ["one_graph", "host_f"]  # one graph: the step count is device-held (flags[2])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def solve(a, b, k, mode, path):
    op = HipCsrOp(a)
    try:
        if path == "host_f":
            op.set_device_ftk(0)
        op.set_fused_pass_two(mode)
        return solvers.lanczos_two_pass(op, b, k, ftk.INV), op.flags()
    finally:
        op.close()


_LAYOUT, _ORACLE, _MATS = {}, {}, {}


def layout(name, a):
    """(schedule, uniform chunk width or 0) of the matrix's operator, once per matrix."""
    if name not in _LAYOUT:
        op = HipCsrOp(a)
        _LAYOUT[name] = (op.schedule(), op.kernel_variant() & 7)
        op.close()
    return _LAYOUT[name]


def oracle_x(name, a, b, k):
    """The device-order oracle's x, once per (matrix, k)."""
    if (name, k) not in _ORACLE:
        _ORACLE[name, k] = oracle.Operator(a, layout(name, a)[0]).lanczos_two_pass(b, k, ftk.INV)
    return _ORACLE[name, k]


def check(name, a, b, k, path):
    x2, f2 = solve(a, b, k, 2, path)
    x0, f0 = solve(a, b, k, 0, path)
    assert f2 & FUSED and f2 & CACHED and not f0 & FUSED, (k, f2, f0)
    assert same(x2, x0)
    assert same(x2, oracle_x(name, a, b, k))


def with_b(name, make):
    if name not in _MATS:
        a = make()
        _MATS[name] = (a, std_rng_vector(a.shape[0]) - 0.5)
    return _MATS[name]


def hubs(h, leaves=0, d=False):
    return with_b("hubs%d_%d_%d" % (h, leaves, d), lambda: fc.kkt_hubs(h, leaves, d))


def n_long_of(name, a):
    return len(layout(name, a)[0]["long_rows"])


# ---- k_p2_rows: the blocks' edges ---------------------------------------------------------------
EDGE_HUBS = [30, 1154, 1300, 2048]  # NL = 1, 5 (the headline's class), 6, 8


def test_edge_matrices_cover_every_s():
    assert {sc.rows_block(h)[0] for h in EDGE_HUBS} == {sc.block_steps(nl) for nl in range(1, 9)}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("h,k", [(h, k) for h in EDGE_HUBS for k in sc.step_edge_ks(h)])
def test_rows_block_edges(h, k, path):
    """last = k - 1 at 1, S - 1, S, S + 1 (a part of a block, one block, one step more), B - 1,
    B, B + 1 (the same around what the registers hold) and 2 B + 1, for every S the instances
    take; the device-held count ends anywhere in a block."""
    a, b = hubs(h)
    name = "hubs%d" % h
    assert n_long_of(name, a) == h
    check(name, a, b, k, path)


# ---- k_p2_rows: the flat run's last load ----------------------------------------------------------
def boundary_hubs():
    """n_long with S n_long at, one past and just below a multiple of the 1,024 staging
    threads, for every S > 1: the block's last load full, with one (S = 3) to three live lanes,
    absent."""
    out = set()
    for nl in range(1, 9):
        s = sc.block_steps(nl)
        if s < 2:
            continue
        for m in range(1, s * nl * tc.TPB // 1024 + 1):
            for words in (1024 * m - s, 1024 * m, 1024 * m + s):
                h = -(-words // s)
                if (nl - 1) * tc.TPB < h <= nl * tc.TPB:
                    out.add(h)
    return sorted(out)


BOUNDARY = boundary_hubs()


def test_boundary_cases_hit_every_kind_of_last_load():
    full = [h for h in BOUNDARY if sc.staging_loads(h)[1] == 1024]
    one = [h for h in BOUNDARY if sc.staging_loads(h)[1] == 1]
    few = [h for h in BOUNDARY if 0 < sc.staging_loads(h)[1] <= 3]
    absent = [h for h in BOUNDARY if sc.staging_loads(h)[1] == 0]
    assert full and one and len(few) > len(one) and absent, (full, one, few, absent)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("h", BOUNDARY)
def test_flat_staging_boundary(h, path):
    a, b = hubs(h)
    name = "hubs%d" % h
    assert n_long_of(name, a) == h
    check(name, a, b, sc.rows_block(h)[1] + 2, path)


# ---- k_p2_rows: the wave classes ------------------------------------------------------------------
def kkt_d(hubs_, d_of):
    t, h = fc.hub_arcs(hubs_)
    a = fc.kkt_from_arcs(hubs_, t, h, d_of(len(t)))
    a.eliminate_zeros()
    a.sort_indices()
    return a


def one_d(m):
    d = np.zeros(m)
    d[m // 2] = 3.0
    return d


def half_d(m):
    return np.where(np.random.default_rng(7).random(m) < 0.5, 2.0 + np.arange(m) % 3, 0.0)


def classes(name, a):
    sched, uw = layout(name, a)
    return sc.wave_classes(a, sched, uw)


def wave_case(name, kkt5k=None):
    """-> (a, b, the precondition on the wave classes [workgroup][chunk][wave])."""
    full = lambda cl, c: (cl.reshape(-1, 4)[c] == sc.CLEAN).all()  # noqa: E731
    mixed_wg = lambda cl: any((w == sc.CLEAN).any() and (w == sc.GENERAL).any() for w in cl)  # noqa: E731
    if name == "no_d":  # every wave of a full chunk is clean
        a, b = hubs(150)
        return a, b, lambda cl: full(cl, 0) and full(cl, 1) and not (cl == sc.GENERAL).any()
    if name == "all_d":  # width 3, a self column on every row: all general
        a, b = hubs(150, d=True)
        return a, b, lambda cl: not (cl == sc.CLEAN).any() and (cl == sc.GENERAL).sum() >= 8
    if name == "one_d":  # one row with a self column: one general wave beside clean ones
        a, b = with_b(name, lambda: kkt_d(150, one_d))
        return a, b, lambda cl: (cl == sc.GENERAL).sum() >= 1 and mixed_wg(cl)
    if name == "half_d":
        a, b = with_b(name, lambda: kkt_d(150, half_d))
        return a, b, lambda cl: (cl == sc.GENERAL).sum() >= 4
    if name == "low_degree":  # open rows of widths 2 to 4 beside closed ones
        a, b = with_b(name, lambda: fc.with_low_degree_nodes(kkt5k))

        def pre(cl):
            is_open, width = open_rows(name, a)
            chunks = np.arange(len(is_open)) // sc.CHUNK_ROWS
            beside = any(is_open[chunks == c].any() and not is_open[chunks == c].all()
                         for c in np.unique(chunks))
            return {2, 3, 4} <= set(width[is_open]) and width[is_open].max() == 4 and beside and \
                (cl != sc.IDLE).sum() >= 16
        return a, b, pre
    if name == "three_missing":  # hubs30: one partial chunk, three of the workgroup's missing
        a, b = hubs(30)
        return a, b, lambda cl: cl.shape[0] == 1 and (cl[0, 1:] == sc.IDLE).all() and \
            (cl[0, 0] != sc.IDLE).all()
    if name == "partial_and_missing":  # hubs150: 1,200 rows: a partial third chunk, one missing
        a, b = hubs(150)
        return a, b, lambda cl: cl.shape[0] == 1 and (cl[0, 3] == sc.IDLE).all() and \
            (cl[0, 2] == sc.IDLE).any() and (cl[0, 2] != sc.IDLE).any()
    raise KeyError(name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["no_d", "all_d", "one_d", "half_d", "low_degree",
                                  "three_missing", "partial_and_missing"])
def test_wave_classes(name, path, kkt5k):
    a, b, pre = wave_case(name, kkt5k)
    cl = classes(name, a)
    assert pre(cl), cl
    check(name, a, b, sc.rows_block(n_long_of(name, a))[1] + 2, path)


# ---- k_p2_hub: the small hub set and the widest open row ------------------------------------------
def star(width, one_hub=False):
    """The hubs30 block plus one node of degree `width`, on that many hubs or by parallel arcs
    on one: the node's row is open (its arcs are short rows) and `width` entries wide, its
    arcs' rows are open and two wide. |H| = 2 width + 1, or width + 2 on one hub."""
    t, h = fc.hub_arcs(30)
    t = np.concatenate([t, np.full(width, 30)])
    h = np.concatenate([h, np.zeros(width, dtype=int) if one_hub else np.arange(width)])
    return fc.kkt_from_arcs(31, t, h)


def open_rows(name, a):
    """-> (which short rows, by internal position, are open: a short column other than the row
    itself; every short row's entry count)."""
    sched, _ = layout(name, a)
    perm, ns = sched["perm"], len(sched["short_rows"])
    ai = a.tocsr() if perm is None else a[perm][:, perm].tocsr()
    is_open = np.zeros(ns, dtype=bool)
    for p in range(ns):
        cols = ai.indices[ai.indptr[p]:ai.indptr[p + 1]]
        is_open[p] = np.any((cols < ns) & (cols != p))
    return is_open, np.diff(ai.indptr)[:ns]


def open_width(name, a):
    """The widest open row's entries."""
    is_open, width = open_rows(name, a)
    return int(width[is_open].max())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [tc.HUB_AHEAD + 1, tc.HUB_AHEAD + 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_hub_open_row_widths(width, k, path):
    """A node of degree 1 .. 4 among the open rows, through one whole block of kHubAhead and
    one step of the remainder. In a KKT-shaped matrix an open node row brings its arcs' rows
    (two entries) into the set, so the widest open row holds max(width, 2) entries; degree 1
    is the shape of the KKT instances' hub sets. Width 1: test_hub_pairs."""
    name = "star%d" % width
    a, b = with_b(name, lambda: star(width))
    el, n_open, n_hub = fused_pass_two_rows(a)
    assert (el, n_open, n_hub) == (True, width + 1, 2 * width + 1)
    assert open_width(name, a) == max(width, 2)
    check(name, a, b, k, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [tc.HUB_AHEAD + 1, tc.HUB_AHEAD + 2])
@pytest.mark.parametrize("size", [sc.HUB_LANES_MAX, sc.HUB_LANES_MAX + 1])
def test_hub_small_set_bound(size, k, path):
    """|H| at the lane-broadcast bound and one above it (the shuffle path): a node on one hub
    by size - 2 parallel arcs."""
    assert 3 <= size <= 6  # the family's reach: node rows of 1 .. 4 entries
    name = "multi%d" % size
    a, b = with_b(name, lambda: star(size - 2, one_hub=True))
    assert fused_pass_two_rows(a) == (True, size - 1, size)
    check(name, a, b, k, path)


def pairs(n, diag=False):
    """The hubs30 block beside n pairs of rows that reference only each other (and, with
    `diag`, themselves): open rows one entry wide (two with the diagonal), no long row among
    their columns, |H| = 2 n. Not KKT-shaped: built by hand, since an open arc row always has
    two entries."""
    import scipy.sparse as sp
    blk = np.array([[2.0, 1.5], [1.5, 3.0]]) if diag else np.array([[0.0, 1.5], [1.5, 0.0]])
    a = sp.block_diag([fc.kkt_hubs(30)] + [sp.csr_matrix(blk * (1 + i)) for i in range(n)],
                      format="csr")
    a.sort_indices()
    return a


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [tc.HUB_AHEAD + 1, tc.HUB_AHEAD + 2])
@pytest.mark.parametrize("n,diag", [(1, False), (2, False), (3, False), (1, True)])
def test_hub_pairs(n, diag, k, path):
    """The widest open row holds one entry: |H| = 2 (lane broadcasts), 4 and 6 (shuffle); with a
    diagonal |H| = 2 at width 2 — the chains of the smallest set."""
    name = "pairs%d_%d" % (n, diag)
    a, b = with_b(name, lambda: pairs(n, diag))
    assert fused_pass_two_rows(a) == (True, 2 * n, 2 * n)
    assert open_width(name, a) == (2 if diag else 1)
    check(name, a, b, k, path)
