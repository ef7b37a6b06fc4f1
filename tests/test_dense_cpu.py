"""Dense symmetric operator (include/tpl.h tpl_op_create_dense), the parts that need no GPU:
the schedule rule, the oracle in the dense schedule against extended precision, and the
boundary's declarations in every binding.

The oracle case passes without the feature: it documents that the canonical long-row order
the oracle already restates is the dense operator's order — the contract needs no new
oracle code."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import dense_cases as dc
import oracle

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sched(n, req=0):
    s, g2, e = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = _lib.tpl_dense_schedule(n, req, ctypes.byref(s), ctypes.byref(g2), ctypes.byref(e))
    return rc, s.value, g2.value, e.value


def test_dense_schedule_rule():
    for n in dc.SHAPES + [4096, 10000, 65536]:
        rc, s, g2, e = _sched(n)
        assert rc == _lib.TPL_OK and s == 1, n
        assert e % 512 == 0 and g2 * e >= n and g2 >= 1, (n, g2, e)
        assert (g2, e) == dc.elem_geometry(n), n
    assert _sched(65537)[1] == 2
    for req in (1, 2, 4, 8):
        assert _sched(513, req)[:2] == (_lib.TPL_OK, req)
    for bad in (3, 5, 16, -1):
        assert _sched(513, bad)[0] == _lib.TPL_ERR_INVALID_ARGUMENT, bad
    assert _sched(0)[0] == _lib.TPL_ERR_INVALID_ARGUMENT
    # outputs may be NULL
    assert _lib.tpl_dense_schedule(7, 0, None, None, None) == _lib.TPL_OK
    # the Python helper reports what HipDenseOp.schedule() would
    from tpl_amd.operator import dense_schedule
    d = dense_schedule(513, 8)
    assert (d["slices"], d["G2"], d["E"]) == (8, *dc.elem_geometry(513))
    assert d["short_rows"].size == 0 and np.array_equal(d["long_rows"], np.arange(513))


@pytest.mark.parametrize("n", [1, 7, 513, 2053, 10000])
def test_dense_schedule_geometry_is_the_csr_plan_s(n):
    """(G2, E) are what the host plan of a CSR matrix of the same n reports."""
    plan = tpl_amd.HostPlan(sp.identity(n, format="csr"))
    s = plan.schedule()
    assert _sched(n)[2:] == (s["G2"], s["E"])


_CASES = [(n, 1) for n in dc.SHAPES] + [(n, s) for n in dc.SLICED for s in dc.SLICES]


@pytest.mark.parametrize("n,slices", _CASES)
def test_oracle_in_the_dense_schedule_is_a_product(n, slices):
    """oracle.Operator on the full CSR with short_rows = [], long_rows = 0..n-1 against A x in
    extended precision: every row within 2 n 2^-53 (|A||x|)_i — n roundings of products and
    fewer than n of sums, each at most 2^-53 relative to a partial sum bounded by (|A||x|)_i."""
    for a in (dc.reference_matrix(n), dc.zeros_matrix(n)):
        x = np.random.default_rng(n + slices).standard_normal(n)
        y = oracle.Operator(dc.full_csr(a), dc.schedule(n, slices)).apply(x)
        exact = a.astype(np.longdouble) @ x.astype(np.longdouble)
        bound = 2.0 * n * 2.0 ** -53 * (np.abs(a) @ np.abs(x))
        assert np.all(np.abs(y.astype(np.longdouble) - exact) <= bound), (n, slices)


def test_header_declares_the_dense_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpl.h")).read(), flags=re.S)
    txt = re.sub(r"\s+", " ", txt)
    assert ("tpl_status tpl_op_create_dense(tpl_ctx_t ctx, int64_t n, const double* a, "
            "int64_t lda, int mem, tpl_op_t* out);") in txt
    assert ("tpl_status tpl_dense_schedule(int64_t n, int32_t slices_req, int32_t* slices, "
            "int32_t* G2, int64_t* E);") in txt


def test_python_mirror_exports_the_dense_operator():
    from tpl_amd import operator
    assert tpl_amd.HipDenseOp is operator.HipDenseOp and "HipDenseOp" in tpl_amd.__all__
    assert {"tpl_op_create_dense", "tpl_dense_schedule"} <= set(_lib.EXPORTED)
    # one surface, shared: the methods are the CSR operator's own functions, not copies
    for m in ("apply", "schedule", "flags", "device_bytes", "set_slices", "set_device_ftk",
              "ftk_device", "ftk_exp_times_device", "ftk_inv_shifts_device", "nrows", "ncols"):
        assert getattr(tpl_amd.HipDenseOp, m) is getattr(tpl_amd.HipCsrOp, m), m
    # as_operator still refuses a bare array
    with pytest.raises(TypeError):
        operator.as_operator(np.eye(3))


def test_null_arguments_are_invalid():
    a = np.eye(3)
    out = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    cases = [(None, 3, a.ctypes.data, 3, ctypes.byref(out)),
             (ctx, 3, None, 3, ctypes.byref(out)),
             (ctx, 3, a.ctypes.data, 3, None),
             (ctx, 0, a.ctypes.data, 3, ctypes.byref(out)),
             (ctx, -1, a.ctypes.data, 3, ctypes.byref(out)),
             (ctx, 3, a.ctypes.data, 2, ctypes.byref(out))]
    for c, n, p, lda, o in cases:
        assert _lib.tpl_op_create_dense(c, n, p, lda, _lib.TPL_MEM_HOST, o) == \
            _lib.TPL_ERR_INVALID_ARGUMENT, (n, lda)
        assert out.value is None
    assert _lib.tpl_op_create_dense(ctx, 2 ** 31, a.ctypes.data, 2 ** 31, _lib.TPL_MEM_HOST,
                                    ctypes.byref(out)) == _lib.TPL_ERR_UNSUPPORTED


def _norm(s):
    return re.sub(r"\s+", " ", s)


def test_rust_shim_has_the_dense_items():
    src = _norm(open(os.path.join(ROOT, "integration", "rust", "hip.rs")).read())
    assert ("fn tpl_op_create_dense(ctx: *mut TplCtx, n: i64, a: *const f64, lda: i64, "
            "mem: c_int, out: *mut *mut TplOp) -> c_int;") in src
    assert "pub struct HipDenseOp" in src
    assert re.search(r"pub fn from_mat\(a: MatRef<'_, f64>, device: i32\) -> "
                     r"Result<Self, LanczosError>", src)
    assert "impl LinOp<f64> for HipDenseOp" in src
    blk = src[src.index("impl LinOp<f64> for HipDenseOp"):]
    for m in ("apply_scratch", "nrows", "ncols", "apply", "conj_apply"):
        assert re.search(rf"\bfn {m}\(", blk[:blk.index("impl HipOperand for HipDenseOp")]), m
    assert "impl HipOperand for HipDenseOp" in src
    assert re.search(r"impl<'a> HipOperand for MatRef<'a, f64>", src)


def test_cpp_header_has_the_dense_operator():
    src = _norm(open(os.path.join(ROOT, "include", "tpl.hpp")).read())
    assert "class DenseOp : public HipCsrOp" in src
    assert "DenseOp(const Context& ctx, const Mat& a)" in src
    assert "tpl_op_create_dense(ctx.handle()" in src


def test_harness_dense_study_matches_the_published_schema():
    """The harness's dense-tradeoff columns and variants are those of the reference's published
    results/dense_tradeoff.csv (kept as data under tests/golden/reference_results), and its
    matrix is symmetric with b = A 1 / sqrt(n)."""
    import csv
    from tpl_amd import harness
    with open(os.path.join(ROOT, "tests", "golden", "reference_results", "dense_tradeoff.csv")) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == harness.DENSE_TRADEOFF_FIELDS
    assert sorted({r["variant"] for r in rows}) == sorted(harness.VARIANTS)
    assert [int(r["k"]) for r in rows if r["variant"] == "two-pass"] == list(range(100, 1001, 100))
    a, b = harness.dense_instance(9)
    assert np.array_equal(a, a.T) and np.all((a >= 0) & (a < 2))
    assert np.allclose(b, a.sum(axis=1) / 3.0, rtol=1e-15, atol=0)
    # R from StdRng(42): the first draw is the package's pinned b[0] (tpl_amd/utils/rng.py)
    assert abs(a[0, 0] / 2 - 0.52655741) < 1e-8
