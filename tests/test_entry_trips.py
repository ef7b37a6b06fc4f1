"""CPU: the headline kernels fetch their arguments in one scalar round trip.

scripts/entry_trips.py reads the compiled gfx950 assembly (csrc/build/all_units.asm, every
unit's assembly joined, when the kernel sources are not newer, else `make asm` first,
about half a minute). For k_spmv<58>, k_p1_spmv<58>, k_p2_spmv<58> and every k_p1_axpy<NP>:

  * no kernel-argument load after the first `s_waitcnt lgkmcnt(0)`, outside the allow-list
    below — and no allow-listed one either on a path that has not issued a vector load yet;
  * no spills, at most 80 SGPRs (above that a workgroup per CU is lost).

Allow-list, by offset into the kernel-argument segment:
  * k_p1_axpy: `betas` and `lu` (one 16-byte load) and `kcap`, read by the elimination
    workgroup alone, off the critical path.
  * the SpMV-shaped kernels: the long rows' hand-off fields `P`, `Pcnt`, `ypart` and
    `long_defer`, read at the end of a bin behind its entries and gathers. Loading them at
    entry as well takes k_p1_spmv<58> to 82 SGPRs, over the limit this test holds.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location(
    "entry_trips", os.path.join(ROOT, "scripts", "entry_trips.py"))
et = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(et)

SGPR_MAX = 80

# struct offsets (tpl_device.h): CsrDev leads the arguments of k_spmv and k_p2_spmv
CSRDEV_HANDOFF = {0x58: "P", 0x60: "Pcnt", 0xB8: "ypart", 0xC0: "long_defer"}
P1SPMV_HANDOFF = {0xEC: "long_defer", 0xF0: "P", 0xF8: "Pcnt", 0x100: "ypart"}
P1AXPY_ELIM = {0x74: "kcap", 0x78: "betas, lu", 0x80: "lu"}

KERNELS = {
    "k_spmv<58>": CSRDEV_HANDOFF,
    "k_p1_spmv<58>": P1SPMV_HANDOFF,
    "k_p2_spmv<58>": CSRDEV_HANDOFF,
    "k_p1_axpy<2>": P1AXPY_ELIM,
    "k_p1_axpy<4>": P1AXPY_ELIM,
    "k_p1_axpy<8>": P1AXPY_ELIM,
    "k_p1_axpy<12>": P1AXPY_ELIM,
}


@pytest.fixture(scope="module")
def asm_text():
    path = et.fresh_asm()
    if path is None:
        if not et.have_hipcc():
            pytest.skip("no up-to-date csrc/build/*.s and no hipcc to compile one")
        path = et.compile_asm()
    with open(path, errors="replace") as f:
        return f.read()


def test_allow_list_matches_the_structs():
    """The offsets above are those of the named fields (LP64, natural alignment)."""
    import ctypes as C

    def offsets(fields):
        class S(C.Structure):
            _fields_ = [(n, t) for n, t in fields]
        return {n: getattr(S, n).offset for n, _ in fields}, C.sizeof(S)

    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    spmv, size = offsets(
        [(n, p) for n in ("Pb_r", "flags", "norms", "betas", "Pa", "xsrc", "r_cur", "r_prev", "W",
                          "Vcol", "stamp", "s_col", "s_val", "s_cbase", "srows")] + [("E", i64)] +
        [(n, i32) for n in ("j", "G2", "G2_r", "n_slice_blocks", "n_chunks", "n_short",
                            "s_identity", "n_slices", "bin_cap", "s_width")] +
        [(n, p) for n in ("b_col", "b_val", "b_cbase", "b_seg", "b_hdr", "c_base", "c_width")] +
        [(n, i32) for n in ("s_win", "s_win_max", "pb_ld", "long_defer")] +
        [(n, p) for n in ("P", "Pcnt", "ypart")])
    assert size == 264
    assert {spmv[n]: n for n in ("long_defer", "P", "Pcnt", "ypart")} == P1SPMV_HANDOFF
    axpy, size = offsets(
        [(n, p) for n in ("Pa_r", "W", "r_cur", "r_next", "flags", "norms", "alphas", "Pb",
                          "stamp")] + [(n, i64) for n in ("n", "E", "norm_n")] +
        [(n, i32) for n in ("NA_r", "G2", "j", "k", "elim_block", "kcap")] +
        [("betas", p), ("lu", p)])
    assert size == 136
    assert (axpy["kcap"], axpy["betas"], axpy["lu"]) == (0x74, 0x78, 0x80)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_one_argument_round_trip(asm_text, kernel):
    r = et.report(asm_text, kernel)
    allowed = KERNELS[kernel]
    print(kernel, {k: v for k, v in r.items() if k != "symbol"})
    bad = [l for l in r["late_kernarg_loads"]
           if l["offset"] not in allowed or l["before_vector_load"]]
    assert not bad, "kernel-argument loads behind the first s_waitcnt lgkmcnt(0): %s" % bad
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0
    assert r["sgpr_count"] <= SGPR_MAX, r["sgpr_count"]
    assert r["kernarg_segment_size"] is not None and r["vgpr_count"] is not None


def test_kernel_argument_segments_are_compact(asm_text):
    """The pass-one kernels take their own argument structs, not whole CsrDev + DevState
    (376 and 624 bytes before)."""
    assert et.report(asm_text, "k_p1_spmv<58>")["kernarg_segment_size"] == 264
    assert et.report(asm_text, "k_p1_axpy<12>")["kernarg_segment_size"] == 136
