"""CPU: the long-row cache of the batch solves (tpl_op_set_long_cache_solvers, include/tpl.h):
the budget arithmetic of a group's cache through tpl_long_cache_rows, the solver mask's
argument check on a host-only plan, and the compiled kernels' resource counts
(scripts/entry_trips.py).

A group of NB columns caches rows_b steps of n_long x NB doubles. Mode 2: the budget is two
GROUP vectors' bytes, NB x tpl_long_cache_default_budget(n), so rows_b is the single solve's
row count, tpl_long_cache_rows(2, 0, n, n_long, kcap). Mode 1: budget_bytes over 8 n_long NB,
which is tpl_long_cache_rows(1, budget, n, n_long NB, kcap).
"""
import importlib.util
import os

import pytest
import scipy.sparse as sp

import tpl_amd
from tpl_amd import HostPlan, TplError, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rows = _lib.tpl_long_cache_rows
default_budget = _lib.tpl_long_cache_default_budget


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("n,nl,kcap", [(5115, 114, 20), (5115, 114, 1000), (501155, 1154, 500),
                                       (501155, 1154, 1000), (6000, 66, 16)])
def test_mode_two_gives_the_single_solves_rows(nb, n, nl, kcap):
    """B = NB x the default budget over 8 n_long NB bytes per step: NB cancels."""
    single = rows(2, 0, n, nl, kcap)
    assert min(kcap, nb * default_budget(n) // (8 * nl * nb)) == single
    assert rows(1, nb * default_budget(n), n, nl * nb, kcap) == single


@pytest.mark.parametrize("nb", [2, 4])
def test_mode_one_divides_by_nb_and_rounds_down(nb):
    n, nl, k = 5115, 114, 20
    for want in (0, 1, 2, k - 2, k):
        assert rows(1, 8 * nl * nb * want, n, nl * nb, k) == want
        assert rows(1, 8 * nl * nb * want + 8 * nl * nb - 1, n, nl * nb, k) == want
    assert rows(1, 8 * nl * nb * 3 * k, n, nl * nb, k) == k           # never past the capacity
    # the same budget holds 1 / NB of the steps it holds for a single solve
    assert rows(1, 8 * nl * 12, n, nl, k) == 12 and rows(1, 8 * nl * 12, n, nl * nb, k) == 12 // nb
    assert rows(0, 10 ** 9, n, nl * nb, k) == 0 and rows(1, 10 ** 9, n, 0, k) == 0


def test_headline_figures():
    """500k arcs, k = 500, NB = 4: all 500 steps, 18.5 MB, within four times the single
    solve's default budget."""
    n, nl, nb = 501155, 1154, 4
    assert rows(2, 0, n, nl, 500) == 500
    assert 500 * nl * nb * 8 == 18_464_000
    assert 500 * nl * nb * 8 <= nb * default_budget(n) == 4 * 8_018_944


def test_solver_mask_argument_check_on_a_plan():
    """The mask is checked before anything touches a device: a host-only plan takes every
    mask up to 15 and refuses anything above, as a live operator does."""
    assert (tpl_amd.LONG_CACHE_TWO_PASS, tpl_amd.LONG_CACHE_TWO_PASS_MULTI,
            tpl_amd.LONG_CACHE_TWO_PASS_BATCH, tpl_amd.LONG_CACHE_TWO_PASS_BATCH_MULTI) == (1, 2, 4, 8)
    plan = HostPlan(sp.identity(8, format="csr"))
    try:
        for mask in (0, 1, 6, 15):
            plan.set_long_cache_solvers(mask)
        for mask in (16, 17, 1 << 31):
            with pytest.raises(TplError) as e:
                plan.set_long_cache_solvers(mask)
            assert e.value.status == _lib.TPL_ERR_INVALID_ARGUMENT
        assert _lib.tpl_op_set_long_cache_solvers(None, 1) == _lib.TPL_ERR_INVALID_ARGUMENT
    finally:
        plan.close()


@pytest.fixture(scope="module")
def asm():
    spec = importlib.util.spec_from_file_location(
        "entry_trips", os.path.join(ROOT, "scripts", "entry_trips.py"))
    et = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(et)
    path = et.fresh_asm()
    if path is None:
        if not et.have_hipcc():
            pytest.skip("no up-to-date csrc/build/*.s and no hipcc to compile one")
        path = et.compile_asm()
    with open(path, errors="replace") as f:
        return et, f.read()


def scratch_bytes(text, sym):
    import re
    m = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), text, re.S)
    return int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(1)).group(1))


@pytest.mark.parametrize("kernel", ["k_bp2_cached<4, 3>", "k_bp2_cached<2, 3>",
                                    "k_bp1_spmv<4, 7>", "k_bp1_spmv<2, 7>"])
def test_no_vgpr_spill_and_no_scratch(kernel, asm):
    """The headline instances of the new kernel and of the pass-one kernel that now stores
    the sums: no register goes to memory."""
    et, text = asm
    r = et.report(text, kernel)
    print({k: v for k, v in r.items() if k not in ("symbol", "late_kernarg_loads")})
    assert r["vgpr_spill_count"] == 0
    assert scratch_bytes(text, r["symbol"]) == 0


@pytest.mark.parametrize("kernel", ["k_bp2_cached<4, 3>", "k_bp1_spmv<4, 7>"])
def test_no_sgpr_spill(kernel, asm):
    """The bound as set for the feature: no spill of any kind, SGPRs into VGPR lanes
    included. k_bp2_cached<4, 3>: 144 VGPRs, 102 SGPRs (the step records lane-wise in one
    VGPR pair, one column's fields read at a time, the per-column masks formed only where a
    column has stopped; 92 spilled with the records held as k_bp2_spmv<4, 7> holds them).
    k_bp1_spmv<4, 7>: 166 VGPRs, 96 SGPRs (the alive columns as one bit mask, beta_{j-2}
    loaded in the prologue; 56 spilled before)."""
    et, text = asm
    r = et.report(text, kernel)
    print({k: v for k, v in r.items() if k not in ("symbol", "late_kernarg_loads")})
    assert r["sgpr_spill_count"] == 0
