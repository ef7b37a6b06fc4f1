"""CPU: the block structure of the fused pass two as the tests derive it
(tests/fused_steps_cases.py) against the source and the compiled kernels: S of every
k_p2_rows<W, NL> read back from the build's assembly (the second staging buffer lies at the
immediate offset S 256 NL 8), the LDS bound for every NL, the loop's record loads scalar, and
the wave classes of two small matrices computed by hand.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import fused_cases as fc
import fused_steps_cases as sc
import fused_tuned_cases as tc

NLS = range(1, 2048 // tc.TPB + 1)
WIDTHS = range(1, 5)


@pytest.fixture(scope="module")
def asm():
    spec = importlib.util.spec_from_file_location(
        "entry_trips", os.path.join(tc.ROOT, "scripts", "entry_trips.py"))
    et = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(et)
    path = et.fresh_asm()
    if path is None:
        if not et.have_hipcc():
            pytest.skip("no up-to-date csrc/build/*.s and no hipcc to compile one")
        path = et.compile_asm()
    with open(path, errors="replace") as f:
        return et, f.read()


def body(et, text, kernel):
    return "\n".join(et.body_lines(text, et.find_symbol(text, kernel)))


def test_constants():
    with open(tc.SOURCE) as f:
        src = f.read()
    assert "(64 * 1024) / (2 * kTPB * NL * (int)sizeof(double))" in src  # block_steps' rule
    assert 1 <= sc.STEPS_MAX <= 8
    assert 1 <= sc.HUB_LANES_MAX <= 64


@pytest.mark.parametrize("nl", NLS)
def test_blocks_fit_the_workgroups_lds(nl):
    s = sc.block_steps(nl)
    assert s >= 1
    assert 2 * s * tc.TPB * nl * 8 <= sc.LDS_PER_WG
    assert s == sc.STEPS_MAX or 2 * (s + 1) * tc.TPB * nl * 8 > sc.LDS_PER_WG
    for n_long in ((nl - 1) * tc.TPB + 1, nl * tc.TPB):
        assert sc.rows_block(n_long) == (s, s * tc.ROWS_DEPTH)


def test_the_instance_classes_take_more_than_one_s():
    assert len({sc.block_steps(nl) for nl in NLS}) >= 2
    assert sc.rows_block(1154) == (sc.block_steps(5), sc.block_steps(5) * tc.ROWS_DEPTH)


@pytest.mark.parametrize("w", WIDTHS)
def test_compiled_s_is_the_helpers(w, asm):
    """The staging writes of k_p2_rows<w, nl> go to offset 0 (even blocks) and to the second
    buffer, which the kernel places at S 256 nl doubles as an immediate."""
    et, text = asm
    for nl in NLS:
        b = body(et, text, "k_p2_rows<%d, %d>" % (w, nl))
        offs = {int(m.group(1) or 0)
                for m in re.finditer(r"ds_write_b64 v\d+, v\[\d+:\d+\](?: offset:(\d+))?", b)}
        assert offs == {0, sc.block_steps(nl) * tc.TPB * nl * 8}, (w, nl, offs)


def test_rows_loop_loads_its_records_scalar(asm):
    """The headline instance: the step records come by s_load (eight dwords: four fields), and
    no lane read is left in the kernel."""
    et, text = asm
    b = body(et, text, "k_p2_rows<2, 5>")
    assert len(re.findall(r"s_load_dwordx8 ", b)) >= sc.block_steps(5)
    assert "v_readlane_b32" not in b


def test_hub_keeps_its_lane_reads_to_the_small_set(asm):
    """k_p2_hub: the records' fields come as vector loads into every lane; the only lane reads
    left are the small hub set's member broadcasts."""
    et, text = asm
    b = body(et, text, "k_p2_hub")
    assert "global_load_dwordx4" in b
    lanes = {int(m.group(1)) for m in re.finditer(r"v_readlane_b32 s\d+, v\d+, (\d+)", b)}
    assert lanes and max(lanes) < sc.HUB_LANES_MAX


def natural_schedule(a, n_short):
    n = a.shape[0]
    return {"short_rows": np.arange(n_short), "long_rows": np.arange(n_short, n), "perm": None}


def test_wave_classes_by_hand():
    """kkt_hubs(30): 240 arc rows of two long-row columns, one partial chunk: waves 0 .. 3 of
    chunk 0 hold rows 0 .. 63 + 256 .. (none past 239), so waves 0 - 3 have live rows, all
    clean; the workgroup's other three chunks are missing. With D on every arc every wave
    with a row is general."""
    a = fc.kkt_hubs(30)
    cl = sc.wave_classes(a, natural_schedule(a, 240), 0)
    assert cl.shape == (1, tc.ROWS_GROUP, 4)
    assert (cl[0, 0] == sc.CLEAN).all() and (cl[0, 1:] == sc.IDLE).all()
    # uniform width 3 on the same rows: every entry list is padded
    assert (sc.wave_classes(a, natural_schedule(a, 240), 3)[0, 0] == sc.GENERAL).all()
    d = fc.kkt_hubs(30, d=True)
    assert (sc.wave_classes(d, natural_schedule(d, 240), 0)[0, 0] == sc.GENERAL).all()


def test_staging_loads():
    """n_long = 1024 m / S and one more, at the largest NL whose S > 1 divides 1,024 m."""
    threads = tc.TPB * tc.ROWS_GROUP
    for n_long in range(1, 2049):
        s, _ = sc.rows_block(n_long)
        nlb, inside = sc.staging_loads(n_long)
        assert nlb == -(-s * -(-n_long // tc.TPB) // tc.ROWS_GROUP)
        assert 0 <= inside <= threads
        assert (nlb - 1) * threads + inside == s * n_long or \
            (inside == 0 and s * n_long <= (nlb - 1) * threads)
