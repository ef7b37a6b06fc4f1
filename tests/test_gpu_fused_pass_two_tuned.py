"""GPU: the edges of the tuned fused pass two (tpl_k_p2_fused.hip).

k_p2_hub takes whole blocks of kHubAhead steps without an exit and the remainder from its
registers; k_p2_rows keeps kRowsDepth steps of the cache row in registers, the same way, and
stages the row with 256 * kRowsGroup threads. Every case solves with the mode auto and with
the mode off on fresh operators and compares the bits (`np.array_equal` on the words), then
the device-order oracle's; bit 9 of flags() says the fused kernels ran. The step counts are
derived from the shipped constants (tests/fused_tuned_cases.py), so that every remainder of
the blocks, `last` equal to exactly one and two blocks, and the partial last staging load
are hit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

import fused_cases as fc  # noqa: E402
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


def solve(a, b, k, mode, path, n_long=None):
    op = HipCsrOp(a)
    try:
        if path == "host_f":
            op.set_device_ftk(0)
        op.set_fused_pass_two(mode)
        if n_long is not None:
            assert len(op.schedule()["long_rows"]) == n_long
        return solvers.lanczos_two_pass(op, b, k, ftk.INV), op.flags()
    finally:
        op.close()


_ORACLE = {}


def oracle_x(name, a, b, k):
    """The device-order oracle's x, once per (matrix, k)."""
    if (name, k) not in _ORACLE:
        op = HipCsrOp(a)
        sched = op.schedule()
        op.close()
        _ORACLE[name, k] = oracle.Operator(a, sched).lanczos_two_pass(b, k, ftk.INV)
    return _ORACLE[name, k]


def check(name, a, b, k, path, n_long=None):
    x2, f2 = solve(a, b, k, 2, path, n_long)
    x0, f0 = solve(a, b, k, 0, path)
    assert f2 & FUSED and f2 & CACHED and not f0 & FUSED, (k, f2, f0)
    assert same(x2, x0)
    assert same(x2, oracle_x(name, a, b, k))


_MATS = {}


def matrix(name, kkt5k=None):
    """-> (a, b, n_long or None). hubs<h>[_<l>]: fc.kkt_hubs(hubs=h, leaves=l); every hub node
    is a long row (16 arcs), every arc and leaf a short one."""
    if name not in _MATS:
        if name == "5k":
            a, nl = kkt5k.a, None
        else:
            h, _, l = name[4:].partition("_")
            a, nl = fc.kkt_hubs(hubs=int(h), leaves=int(l or 0)), int(h)
        _MATS[name] = (a, std_rng_vector(a.shape[0]) - 0.5, nl)
    return _MATS[name]


# ---- k_p2_hub: the blocks' edges --------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [l + 1 for l in tc.block_edge_lasts(tc.HUB_AHEAD)])
def test_hub_block_edges(k, path, kkt5k):
    """The 5k block (114 long rows, |H| = 3): last = k - 1 short of one block, one block
    exactly, one step more, and the same around two blocks. With k = 2 .. 5, 7, 8, 20, 50 of
    tests/test_gpu_fused_pass_two.py every remainder of the block is covered."""
    a, b, _ = matrix("5k", kkt5k)
    check("5k", a, b, k, path)


# ---- k_p2_rows: the staging's edges -----------------------------------------------------------
ROWS_KS = sorted({l + 1 for l in (1, tc.ROWS_DEPTH - 1, tc.ROWS_DEPTH, tc.ROWS_DEPTH + 1,
                                  2 * tc.ROWS_DEPTH + 1) if l >= 1})


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", ROWS_KS)
@pytest.mark.parametrize("name", ["hubs30", "hubs150", "5k", "hubs1300"])
def test_rows_staging_edges(name, k, path, kkt5k):
    """hubs30: 240 arcs, one partial chunk — three of the workgroup's four chunks missing;
    hubs150: 1,200 arcs, three chunks, the last partial, and one missing; the 5k block: ten
    chunks, so a last workgroup of two; hubs1300: two staging loads per thread, the second
    partial, 21 chunks. last = 1, D - 1, D, D + 1 and 2 D + 1 for the register depth D (one
    barrier per step ships: there is no group of steps to straddle)."""
    a, b, nl = matrix(name, kkt5k)
    check(name, a, b, k, path, nl)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hubs", [h for c in range(1, tc.ROWS_GROUP.bit_length() + 1)
                                  for h in (256 << (c - 1), (256 << (c - 1)) + 1)])
def test_staging_load_boundary(hubs, path):
    """n_long = 256 c and 256 c + 1 for the workgroup's 256 c threads: the last staging load
    full, and with one live lane."""
    a, b, nl = matrix("hubs%d" % hubs)
    check("hubs%d" % hubs, a, b, 9, path, nl)


# ---- the hub set beside the new loop ----------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [tc.HUB_AHEAD + 1, tc.HUB_AHEAD + 2])
@pytest.mark.parametrize("name", ["hubs66_3", "hubs10_27", "hubs11_27", "hubs30_113"])
def test_hub_set_workgroup(name, k, path):
    """|H| = 9 (6 open rows) and |H| = 64 (54 open rows): one wave steps H, its open rows
    reading v_j by shuffle; |H| = 65 and |H| = 256 (226 open rows, the cap): the hub workgroup
    exchanges through LDS with a barrier per step. Each through a whole block and one step
    of the tail; the long rows H owns are the lanes the long-row workgroups must not write."""
    a, b, nl = matrix(name)
    sizes = {"hubs66_3": (6, 9), "hubs10_27": (54, 64), "hubs11_27": (54, 65),
             "hubs30_113": (226, 256)}
    assert fused_pass_two_rows(a) == (True,) + sizes[name]
    check(name, a, b, k, path, nl)
