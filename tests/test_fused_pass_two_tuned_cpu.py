"""CPU: what the compiler made of the tuned fused pass two (k_p2_hub and every k_p2_rows<W, NL>
instance), read from the build's assembly and its resource-usage block as
tests/test_long_cache_cpu.py reads the cached step kernel's: no scratch, no spills, LDS
within what the launch asks for at the largest eligible n_long, and the headline instance's
grid resident in one round. Also: the constants the GPU tests derive their edges from
(tests/fused_tuned_cases.py) are the source's.
"""
import importlib.util
import os
import re

import pytest

import fused_tuned_cases as tc

ROOT = tc.ROOT
CUS = 256                # MI355X
LDS_PER_CU = 160 * 1024  # bytes
LDS_PER_WG = 64 * 1024   # the most one workgroup may ask for
N_LONG_MAX = 2048        # kFusedLongMax
WIDTHS, NLS = range(1, 5), range(1, N_LONG_MAX // tc.TPB + 1)
HEADLINE = (2, 5)        # width 2; 1,154 long rows
HEADLINE_CHUNKS, HEADLINE_N_LONG = 977, 1154


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


def usage(et, text, kernel):
    """The kernel's metadata counts plus the `; Kernel info:` block behind its code."""
    sym = et.find_symbol(text, kernel)
    r = et.metadata(text, sym)
    at = text.index("\n" + sym + ":")
    info = text[text.index("; Kernel info:", at):]
    info = info[:info.index("; Occupancy:") + 40]
    for key in ("ScratchSize", "LDSByteSize", "Occupancy", "NumVgprs"):
        r[key] = int(re.search(r"^; %s: (\d+)" % key, info, re.M).group(1))
    return r


def test_constants_are_the_sources():
    assert tc.source_constants() == (tc.HUB_AHEAD, tc.ROWS_GROUP, tc.ROWS_DEPTH)


def test_hub_resources(asm):
    et, text = asm
    r = usage(et, text, "k_p2_hub")
    print(r)
    assert r["ScratchSize"] == 0
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["LDSByteSize"] == 2 * tc.TPB * 8  # the hub workgroup's two exchange buffers
    assert r["Occupancy"] >= 1


@pytest.mark.parametrize("w", WIDTHS)
def test_rows_resources(w, asm):
    et, text = asm
    for nl in NLS:
        r = usage(et, text, "k_p2_rows<%d, %d>" % (w, nl))
        print(w, nl, r)
        assert r["ScratchSize"] == 0, (w, nl)
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (w, nl)
        # all of its LDS is the launch's: 2 n_long doubles, 32 KiB at the largest n_long
        assert r["LDSByteSize"] == 0, (w, nl)
        assert 2 * N_LONG_MAX * 8 <= LDS_PER_WG
        # a workgroup's waves fit a CU at all
        assert r["Occupancy"] * 4 >= tc.ROWS_GROUP * tc.TPB // 64, (w, nl)


def test_headline_grid_is_resident_in_one_round(asm):
    et, text = asm
    r = usage(et, text, "k_p2_rows<%d, %d>" % HEADLINE)
    waves = tc.ROWS_GROUP * tc.TPB // 64
    by_regs = r["Occupancy"] * 4 // waves
    by_lds = LDS_PER_CU // (2 * HEADLINE_N_LONG * 8)
    grid = -(-HEADLINE_CHUNKS // tc.ROWS_GROUP)
    print(r, by_regs, by_lds, grid)
    assert min(by_regs, by_lds) * CUS >= grid
