"""CPU: the case tables of tests/layout_cases.py say what they claim.

tests/test_gpu_variants.py runs every compiled instance of the SpMV-shaped kernels and the
edges of the layout through those tables; here, with no GPU, the tables are checked
against the runtime's own host plan (tpl_plan_create, wherever a case needs no setter) and
against build_layout restated (layout_cases.plan, every case): the expected variant flag,
one case per instance, and each structural claim counted in the matrix.
"""
import numpy as np
import pytest

import layout_cases as lc
from conftest import locality_perm

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HostPlan  # noqa: E402
from tpl_amd.operator import _as_csr_arrays  # noqa: E402


def variant_exists(F):  # tpl_kcommon.h variant_exists
    w, win, sc16 = F & 7, F & 64, F & 16
    return 0 <= F < 128 and w <= 4 and (not win or (w > 0 and sc16 != 0))


def planned(c):
    """layout_cases.plan of a case under the order the operator would hold."""
    sv = lc.setter_values(c.setters)
    perm = locality_perm(c.a, sv["short_row_max"]) if sv["reorder"] else None
    return lc.plan(c.a, c.setters, perm), perm


def nonempty_bins(p):
    return [b for per_slice in p["bins"] for b in per_slice if b]


def test_one_case_per_compiled_instance():
    want = {F for F in range(-8, 256) if variant_exists(F)}
    assert len(want) == 56
    got = list(lc.VARIANTS.values())
    assert len(got) == len(set(got)), "an instance listed twice"
    assert not set(got) & set(lc.UNREACHABLE)
    assert set(got) | set(lc.UNREACHABLE) == want
    assert lc.UNREACHABLE == {}, "every instance is reachable through build_layout"
    assert all(name == "F%03d" % F for name, F in lc.VARIANTS.items())
    assert all(variant_exists(F) for F in list(lc.WIDE.values()) + list(lc.EDGES.values()))


ALL = list(lc.VARIANTS) + list(lc.WIDE) + list(lc.EDGES) + [lc.EMPTY_MATRIX]


@pytest.mark.parametrize("name", ALL)
def test_expected_variant(name):
    """build_layout restated gives the expected F for every case; for a case without
    setters so does the runtime's host plan, which also confirms the restated order, short
    rows and slice count."""
    c = lc.case(name)
    assert (abs(c.a - c.a.T)).nnz == 0, "symmetric"
    assert c.a.shape[0] <= 150000 or name in lc.WIDE
    p, perm = planned(c)
    assert p["F"] == c.F
    if not c.setters:
        hp = HostPlan(c.a)
        assert hp.kernel_variant() == c.F
        s = hp.schedule()
        assert (s["perm"] is None) == (perm is None)
        assert perm is None or np.array_equal(s["perm"], perm)
        assert np.array_equal(s["short_rows"], p["short"]) and s["slices"] == p["slices"]
        hp.close()


@pytest.mark.parametrize("name", list(lc.VARIANTS) + list(lc.WIDE))
def test_variant_case_shape(name):
    """At least three chunks, a partial last chunk of more than one row, and — where the
    case has long rows — at least two bins that hold pieces."""
    c = lc.case(name)
    p, _ = planned(c)
    assert p["chunks"] >= 3 and p["n_short"] % lc.CHUNK not in (0, 1)
    if c.F & 7:
        assert p["widths"] == [c.F & 7] * p["chunks"]
    if p["long"].size or c.F & lc.BC16:
        assert len(nonempty_bins(p)) >= 2
        lens = {cnt for b in nonempty_bins(p) for _, cnt in b}
        assert min(lens) <= lc.BIG_PIECE < max(lens), "both piece-sum paths"
    if name in lc.WIDE:
        n = c.a.shape[0]
        assert 131073 <= n <= 196607 and -(-n // 512) > 256


def piece_lengths(p):
    return sorted(cnt for b in nonempty_bins(p) for _, cnt in b)


@pytest.mark.parametrize("fmt", ["i8", "f64"])
def test_edge_claims(fmt):
    """Every edge the table names is present, counted in the matrix."""
    def pl(base):
        return planned(lc.case("%s-%s" % (base, fmt)))[0]
    for W in (5, 8, 9, 16, 17, 32):
        p = pl("width%d" % W)
        assert p["widths"] == [W] * 3 and p["long"].size == 0
    p = pl("widths-1-2-3-4-7")
    assert p["widths"] == [7, 1, 7, 2, 7, 3, 7, 4, 7] and p["long"].size == 0
    p = pl("empty-chunk")
    assert p["widths"] == [3, 0, 3]
    assert np.all(np.diff(p["a"].indptr)[512:1024] == 0)
    p = pl("empty-rows")
    lens = np.diff(p["a"].indptr)
    assert p["long"].size == 0 and p["widths"] == [3, 3, 3]
    assert np.count_nonzero(lens == 0) >= 150 and np.count_nonzero(lens[:512] == 0) >= 50
    for ns in (1, 511, 512, 513):
        p = pl("nshort%d" % ns)
        assert p["n_short"] == ns and p["long"].size == lc.HUBS_A
    # pieces of every length around the 8 / 16-lane switch and the 128-entry blocks
    p = pl("pieces-S1")
    assert p["slices"] == 1 and set(piece_lengths(p)) >= set(lc.PIECE_LENGTHS) - {1}
    assert p["T"] == 2 and min(piece_lengths(p)) > 2, "a piece of one entry needs S > 1"
    p = pl("pieces-S4")
    assert p["slices"] == 4 and set(piece_lengths(p)) >= set(lc.PIECE_LENGTHS)
    p = pl("bin-counts")
    got = [(len(b), sum(cnt > lc.BIG_PIECE for _, cnt in b)) for b in nonempty_bins(p)]
    assert got == lc.BIN_COUNT_EXPECT
    assert [n - big for n, big in got][3:6] == [7, 8, 9] and [big for _, big in got][:3] == [3, 4, 5]
    p = pl("bins-by-count")
    assert p["long"].size >= 600 and set(piece_lengths(p)) == {3, 4, 5}
    assert [len(b) for b in nonempty_bins(p)] == [255, 255, 254]
    p = pl("wide-bins")
    assert piece_lengths(p) == [2049, 6000] and p["bin_cap"] == 6144 and p["slices"] == 1
    p = pl("forced-slices")
    assert int(np.diff(p["a"].indptr).max()) == 7937 > lc.BIN_MAX
    assert p["slices"] == 2, "forced up by the row, not set"
    assert all(m == "set_value_format" for m, _ in lc.case("forced-slices-" + fmt).setters)
    p = pl("slices-1-2-8")
    assert p["slices"] == 8
    assert [int(np.count_nonzero(q)) for q in p["pieces"]] == [1, 2, 8, 7]
    assert [int(q[0]) for q in p["pieces"]] == [0, 0, 5, 0], "rows whose slice 0 is empty"


def test_all_empty_matrix():
    c = lc.case(lc.EMPTY_MATRIX)
    assert c.a.shape == (600, 600) and c.a.nnz == 0
    p, perm = planned(c)
    assert perm is None and p["widths"] == [0, 0] and p["long"].size == 0


@pytest.mark.parametrize("name", lc.SPECIAL)
def test_special_value_cases(name):
    """The matrices that meet a non-finite value where padding gathers: internal column 0,
    or in a window instance the column base of a chunk that holds a padded row. That row
    must not reference the column. Plus three distinct referenced columns for the signed
    zero and the subnormals."""
    c = lc.case(name)
    p, perm = planned(c)
    assert p["window"] == bool(c.F & lc.WIN)
    p0, cols = lc.special_columns(c.a, p, perm)
    col = p0 if perm is None else int(np.nonzero(perm == p0)[0][0])   # internal index
    rows = lc.padded_rows_off_column(p, col)
    assert rows.size >= 1
    if p["window"]:   # the padding reads the window's first element: the chunk's base
        chunks = {int(np.searchsorted(p["short"], r)) // lc.CHUNK for r in rows}
        assert all(p["chunk_base"][ch] == col for ch in chunks)
    else:
        assert col == 0
    assert len(set(cols)) == 3 and p0 not in cols
    assert all(np.any(c.a.indices == j) for j in cols)


def test_special_case_selection():
    Fs = [lc.VARIANTS[n] for n in lc.SPECIAL]
    assert len(set(Fs)) == 6 and {F & 7 for F in Fs} == {0, 1, 3, 4}
    assert any(F & lc.WIN for F in Fs) and any(F & lc.V8 for F in Fs)
    assert any(lc.plan(lc.case(n).a, lc.case(n).setters)["slices"] == 4 and
               lc.case(n).F & lc.BC16 for n in lc.SPECIAL), "bins under S = 4"


def test_stored_zero_survives_canonicalisation():
    a = lc.with_stored_zero(lc.case(lc.STORED_ZERO).a)
    _, rp, ci, v = _as_csr_arrays(a)
    q = rp[1] + int(np.searchsorted(ci[rp[1]:rp[2]], 0))
    assert ci[q] == 0 and v[q] == 0.0 and not np.signbit(v[q])
    assert lc.plan(a, lc.case(lc.STORED_ZERO).setters,
                   locality_perm(a))["F"] == lc.VARIANTS[lc.STORED_ZERO]


@pytest.mark.parametrize("mode,nranks", [("single", 1), ("replicated", 2), ("rows", 2)])
def test_kernel_variant_on_host_plans_of_every_kind(kkt5k, mode, nranks):
    """tpl_op_kernel_variant reads the layout alone, so it is valid on a partitioned host
    plan too (a replicated plan has no device view to build); its format bits are the ones
    tpl_op_flags reports."""
    for rank in range(nranks):
        hp = HostPlan(kkt5k.a, mode=mode, nranks=nranks, rank=rank)
        F, fl = hp.kernel_variant(), hp.flags()
        assert variant_exists(F)
        assert (bool(F & lc.V8), bool(F & lc.SC16), bool(F & lc.BC16)) == \
            (bool(fl & 4), bool(fl & 8), bool(fl & 16))
        hp.close()
