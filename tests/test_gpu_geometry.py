"""GPU: every solver family on row blocks wider than 512 rows, bit for bit the composed oracle.

The cases are tests/geometry_cases.py's: 2,301 to 9,473 rows under tpl_op_set_schedule(max_g2),
so that E = 1024, 1536, 2560 or 3072 — two, three, five and six chunks per row block, a chunk
count that is no multiple of it, empty trailing row blocks, ten row blocks over eight XCDs, one
row block — beside each matrix's default 512-row geometry. Everything else in the suite below
the 500k-arc fixtures runs at one chunk per block, one pair iteration per thread and no empty
block; the multi-function, batch, tolerance-stop, exp-times, cached and fused kernels had their
bits pinned there alone.

Per case the live operator must report the table's G2 and E and the schedule the restated layout
rule gives; tests/composed_oracle.py then composes the expectation of every covered call of the
state_cases catalogue from the oracle in that schedule's reduction order, and
tests/test_geometry_cases.py shows on the CPU that this order's bits differ from the default
geometry's. Every comparison is state_cases.same on the uint64 words of every array of the
result tuple; no tolerance appears. The path flags (bit 5 one graph, 8 long-row cache read,
9 fused) are asserted from include/tpl.h's rules (want_flags), so no case passes by taking
another path than the one its settings name.

Left out: the ftk_*device calls (composed_oracle.LEFT_OUT: they never read the geometry).

Measured figures of the checks that carry a bound: none — every comparison is word for word.
Wall time on one MI355X: 44.8 s for the 112 cases (16 geometries x 7 tests), the slowest 1.7 s
(the first, which makes the first matrix's right-hand sides), the median 0.3 s. Every case
passed on its first complete run: no kernel reads the row-block geometry wrongly at these
shapes.
"""
import re

import numpy as np
import pytest

import composed_oracle as co
import geometry_cases as gc
import state_cases as sc

pytestmark = pytest.mark.gpu

import tpl_amd  # noqa: E402

ONE_GRAPH, CACHED, FUSED = sc.ONE_GRAPH, sc.CACHED, sc.FUSED
K, M = sc.K_BIG, sc.M_DEFAULT
K_TAIL = 7            # 6 regenerated steps: the other tail of the fused pass two's groups of three
ALL_SOLVERS = 15      # every TPL_LONG_CACHE_* bit
CACHE_BIT = {"single": 1, "multi": 2, "batch": 4, "batch_multi": 8}
BUDGET_ROWS = 16      # the budget-limited cache: 16 of K's 24 steps (4 per column of a group of 4)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


# ---- settings ------------------------------------------------------------------------------------
# name -> (long-row cache mode, cached steps of a single solve or None for the default budget,
#          solver mask, fused pass two, device f(T_k))
PATHS = {
    "default": (2, None, 1, 2, 2),
    "cache_all_solvers": (2, None, ALL_SOLVERS, 2, 2),
    "cache_off": (0, None, ALL_SOLVERS, 2, 2),
    "cache_budget": (1, BUDGET_ROWS, ALL_SOLVERS, 2, 2),
    "fused_off": (2, None, ALL_SOLVERS, 0, 2),
    "host_ftk": (2, None, ALL_SOLVERS, 2, 0),
}


def open_case(case, path):
    """A new operator of the case's matrix under the case's max_g2 and the path's settings; the
    schedule it reports is the table's and the restated rule's, so the inputs' host
    decompositions (made in the restated schedule) are in the live operator's order."""
    mode, rows, mask, fused, dev = PATHS[path]
    op = tpl_amd.HipCsrOp(gc.cached_matrix(case.mat))
    try:
        if case.max_g2 is not None:
            op.set_schedule(max_g2=case.max_g2)
        s = op.schedule()
        assert (s["G2"], s["E"]) == (case.G2, case.E), (case.id, s["G2"], s["E"])
        assert gc.same_schedule(s, gc.host_schedule(case)), case.id
        if (mode, rows) != (2, None):
            op.set_long_cache(mode, 8 * case.n_long * rows if rows else 0)
        if mask != 1:
            op.set_long_cache_solvers(mask)
        if fused != 2:
            op.set_fused_pass_two(fused)
        if dev != 2:
            op.set_device_ftk(dev)
        s2 = op.schedule()
        assert (s2["G2"], s2["E"]) == (case.G2, case.E)   # no path setter rebuilt the grid
    except BaseException:
        op.close()
        raise
    return op


def last_group(s):
    """The columns of the last group of a batch call: fours while four remain, then twos, then
    a single remainder column."""
    c = 0
    while s - c > 4:
        c += 4
    left = s - c
    return list(range(c, s)) if left in (1, 2, 4) else [c + 2]


def want_flags(call, case, path, p, I, op, want):
    """The bits of call.defines after the call, by include/tpl.h: bit 8 where the cache is on,
    the operator has long rows, the entry point's bit is in the mask, the cache holds a step
    and the last pass two had at least two; bit 9 where moreover the call is the single
    two-pass solve (or its tolerance form) on the fused-eligible block with every step cached;
    bit 5 where f(T_k) ran on the device inside one graph. `want` is the call's expected result
    (for the steps a host-composed tolerance solve's pass two took)."""
    mode, rows, mask, fused, dev = PATHS[path]
    name, fam = call.name, call.family
    if call.defines != sc.FLAG_MASK:
        # the stand-alone passes never cache; tpl_lanczos defines bit 5 alone
        return ONE_GRAPH if name == "lanczos" and dev else 0
    k, m, host, tol = p["k"], p.get("m", 1), dev == 0, fam == "tol"
    if tol:
        fam = {"two_pass_shifted_inv_tol": "multi",
               "two_pass_batch_shifted_inv_tol": "batch_multi"}.get(name, "single")
    fixed_s = re.fullmatch(r"two_pass_batch_s(\d+)", name)
    s = int(fixed_s.group(1)) if fixed_s else p.get("s", 1)
    cols = last_group(s) if fam in ("batch", "batch_multi") else [0]
    # the steps of the last pass two: what pass one took; on the host-composed tolerance path
    # the largest stop of the last group
    p2_steps = max(int(I.dec(c, k).steps_taken) for c in cols)
    if tol and host:
        p2_steps = int(np.asarray(want[1]).reshape(m if fam != "single" else 1, -1)[:, cols].max())
    # a group's columns share a mode-1 budget (tpl_op_set_long_cache_solvers: n_long NB)
    share = 4 if mode == 1 and len(cols) > 1 else 1
    held = int(tpl_amd._lib.tpl_long_cache_rows(mode, 8 * case.n_long * (rows or 0), I.n,
                                                case.n_long * share, sc.K_BIG))
    cached = bool((mask & CACHE_BIT[fam]) and case.n_long and held > 0 and p2_steps >= 2)
    flags = CACHED if cached else 0
    if cached and fused and fam == "single" and case.mat == "kkt3002" and held >= k:
        flags |= FUSED
    if name == "two_pass_inv" or tol:
        flags |= 0 if host else ONE_GRAPH
    elif name == "two_pass_exp":
        flags |= ONE_GRAPH if co.exp_on_device(I, k, op, host) else 0
    return flags


def check(op, case, path, name, p, device=False):
    call, I = sc.calls()[name], gc.inputs(case)
    host = PATHS[path][4] == 0
    want = co.expect(name, I, p, op, host)
    got = sc.canonical(call.run(op, I, p, device))
    where = (case.id, path, name, p, "device b" if device else "host b")
    assert sc.same(got, sc.canonical(want)), "bits differ from the composed oracle: %s" % (where,)
    flags = op.flags() & call.defines
    assert flags == want_flags(call, case, path, p, I, op, want), (where, flags)


def sizes(call, k=K):
    """The parameter dicts of one call: k, m = 5, and every s of the ladder if it takes one."""
    base = {z: {"k": k, "m": M}[z] for z in call.takes if z != "s"}
    return [dict(base, s=s) for s in sc.S_LADDER] if "s" in call.takes else [base]


COVERED = co.covered()
SOLVERS = [n for n in COVERED if sc.calls()[n].defines == sc.FLAG_MASK]    # the two-pass families


# ---- 1. the whole catalogue at default settings ----------------------------------------------------
@pytest.mark.parametrize("case", gc.CASES, ids=gc.CASE_IDS)
def test_every_call_is_the_composed_oracle(case):
    """Every covered call at k = 24, m = 5 and s = 2, 3, 4, 7; the two-pass solvers also at k = 7.
    On the KKT block the single two-pass solves must have run fused, on the bands cached and
    unfused (want_flags), at both k."""
    assert len(COVERED) == len(sc.call_names()) - len(co.LEFT_OUT) >= 33 and len(SOLVERS) == 17
    op = open_case(case, "default")
    try:
        for name in COVERED:
            call = sc.calls()[name]
            for p in sizes(call):
                check(op, case, "default", name, p)
            if name in SOLVERS:
                for p in sizes(call, K_TAIL):
                    check(op, case, "default", name, p)
        fused_now = FUSED if case.mat == "kkt3002" else 0
        for k in (K, K_TAIL):
            check(op, case, "default", "two_pass_inv", {"k": k})
            assert op.flags() & (CACHED | FUSED) == CACHED | fused_now, (case.id, k, op.flags())
    finally:
        op.close()


# ---- 2. the two-pass families under the settings that change which kernel reads the geometry -------
@pytest.mark.parametrize("path", [n for n in PATHS if n != "default"])
@pytest.mark.parametrize("case", gc.CASES, ids=gc.CASE_IDS)
def test_two_pass_families_on_every_path(case, path):
    """Long-row cache for every solver, off, and budget-limited to 16 of the 24 steps (so pass
    two switches from the cached to the full step kernel on the way); fused pass two off; f(T_k)
    and the tolerance stops on the host. Each setting's flags are asserted with every call."""
    op = open_case(case, path)
    try:
        for name in SOLVERS:
            for p in sizes(sc.calls()[name]):
                check(op, case, path, name, p)
        for name in ("two_pass_inv", "two_pass_inv_tol_never", "two_pass_batch_s3",
                     "two_pass_batch_multi"):
            for p in sizes(sc.calls()[name], K_TAIL):
                check(op, case, path, name, p)
        # the setting did what it is named for
        check(op, case, path, "two_pass_multi", {"k": K, "m": M})
        want = 0 if path == "cache_off" else CACHED
        assert op.flags() & (CACHED | FUSED) == want, (case.id, path, op.flags())
        check(op, case, path, "two_pass_inv", {"k": K})
        kkt = case.mat == "kkt3002"
        want = {"cache_off": 0, "cache_budget": CACHED, "fused_off": CACHED}.get(
            path, CACHED | (FUSED if kkt else 0))
        assert op.flags() & (CACHED | FUSED) == want, (case.id, path, op.flags())
        assert bool(op.flags() & ONE_GRAPH) == (path != "host_ftk"), (case.id, path)
    finally:
        op.close()


# ---- 3. device-resident right-hand sides -------------------------------------------------------------
DEVICE_B = ("pass_two_batch_multi_cut", "pass_one_batch", "standard_reorth", "lanczos",
            "two_pass_inv", "two_pass_exp_times", "two_pass_inv_tol_met", "two_pass_batch_s4",
            "two_pass_batch", "two_pass_batch_multi", "two_pass_batch_exp_times",
            "two_pass_batch_shifted_inv_tol")


@pytest.mark.parametrize("case", gc.CASES, ids=gc.CASE_IDS)
def test_device_resident_b(case):
    """One call and more of every family with b / B a torch CUDA tensor: the interleave and
    de-interleave kernels read and write device memory the caller owns. s = 3: a group of two
    and a remainder column."""
    pytest.importorskip("torch")
    assert {sc.calls()[n].family for n in DEVICE_B} == \
        {"low", "standard", "single", "multi", "tol", "batch", "batch_multi"}
    op = open_case(case, "cache_all_solvers")
    try:
        for name in DEVICE_B:
            call = sc.calls()[name]
            p = {z: {"k": K, "m": M, "s": sc.S_DEFAULT}[z] for z in call.takes}
            check(op, case, "cache_all_solvers", name, p, device=True)
    finally:
        op.close()
