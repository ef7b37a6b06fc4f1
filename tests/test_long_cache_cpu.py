"""CPU: the long-row cache's budget rule (tpl_long_cache_rows, tpl_long_cache_default_budget:
the host functions the operator sizes its cache with, include/tpl.h tpl_op_set_long_cache)
and the compiled cached pass-two step kernel's entry (scripts/entry_trips.py).

rows = min(kcap, budget / (8 n_long)); the default budget is two vectors' bytes, a vector
being n rows padded to the stride of 64 doubles; mode 0 and n_long = 0 mean no cache.
"""
import importlib.util
import os

import pytest

from tpl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rows = _lib.tpl_long_cache_rows
default_budget = _lib.tpl_long_cache_default_budget


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5115, 501155, 5_000_000])
def test_default_budget_is_two_padded_vectors(n):
    padded = max(64, -(-n // 64) * 64)
    assert default_budget(n) == 2 * 8 * padded
    assert padded >= n and padded % 64 == 0 and padded - max(n, 1) < 64


def test_headline_figures():
    """500k arcs: n = 501,155 rows, 1,154 long. k = 500 fits (4.6 MB of the 8.0 MB); at
    k = 1,000 the first 868 steps are cached."""
    n, nl = 501155, 1154
    assert default_budget(n) == 2 * 8 * 501184 == 8018944
    assert rows(2, 0, n, nl, 500) == 500 and 500 * nl * 8 == 4616000
    assert rows(2, 0, n, nl, 1000) == 8018944 // (8 * nl) == 868
    # mode 2 ignores the budget argument, mode 1 takes it as given
    assert rows(2, 1, n, nl, 1000) == 868
    assert rows(1, 8018944, n, nl, 1000) == 868


def test_rows_arithmetic():
    n, nl, k = 5115, 115, 20
    for want in (0, 1, 2, k - 2, k):
        assert rows(1, 8 * nl * want, n, nl, k) == want           # exactly `want` rows
        assert rows(1, 8 * nl * want + 8 * nl - 1, n, nl, k) == want   # rounds down
    assert rows(1, 8 * nl * 1000, n, nl, k) == k                   # never past the capacity
    assert rows(1, 2 ** 63, n, nl, k) == k
    assert rows(2, 0, n, nl, 50) == 50 and rows(2, 0, n, nl, 1000) == 2 * 8 * 5120 // (8 * nl)


def test_no_cache_cases():
    assert rows(0, 10 ** 9, 5115, 115, 20) == 0      # off
    assert rows(2, 0, 3001, 0, 20) == 0              # no long rows
    assert rows(1, 10 ** 9, 3001, 0, 20) == 0
    assert rows(1, 0, 5115, 115, 20) == 0            # no budget
    assert rows(1, 8 * 115 - 1, 5115, 115, 20) == 0  # less than one row
    assert rows(2, 0, 5115, 115, 0) == 0             # no state yet


def test_cached_step_kernel_entry():
    """k_p2_cached<26> (the headline's format: width 2, int8 values, uint16 chunk columns):
    every kernel-argument load in the entry batch, no spills, within the SGPR bound the
    other headline kernels are held to (tests/test_entry_trips.py)."""
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
        r = et.report(f.read(), "k_p2_cached<26>")
    print({k: v for k, v in r.items() if k != "symbol"})
    assert not r["late_kernarg_loads"]
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["sgpr_count"] <= 80
