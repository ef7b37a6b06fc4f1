"""GPU: the faults a solver entry point reports only once it has selected the device, and the
operator's state after one (tests/test_solver_arg_order_cpu.py pins the checks before that).

On the catalogue's smallest operator (tests/state_cases.py "kkt", n = 496), k = 5, m = 2 and
s = 7, so that a batch call walks a group of four, a group of two and the single-column remainder.
Per solve, through the C ABI:
  - a wrong b_len beside k = 0 (and a non-finite time, a short y, a zero ||b||): the dimension
    error with both sizes in its detail, not a NULL and not k;
  - k = 0 with a valid b (beside a non-finite time): the k error;
  - a zero b — for the batch calls a zero column in the group of four, in the group of two and as
    the remainder in turn; for the stand-alone passes two a zero ||b_c|| — gives the zero-vector
    status with the call's own message, and the same call with valid arguments on the same
    operator then returns the bits and flags of a fresh operator's (state_cases.fresh).
Every comparison is word for word; no check here carries a bound.
"""
import ctypes

import numpy as np
import pytest

import state_cases as sc
from test_solver_arg_order_cpu import Entry, bad_at, f64, u64

pytestmark = pytest.mark.gpu

import tpl_amd  # noqa: E402
from tpl_amd import _lib  # noqa: E402

MAT, K, M, S = "kkt", 5, 2, 7
ZERO_COLS = (1, 5, 6)            # in the group of four, in the group of two, the remainder
HOST = _lib.TPL_MEM_HOST
DIM = _lib.TPL_ERR_DIMENSION_MISMATCH
INPUT = _lib.TPL_ERR_INPUT
SOLVE_MSG = "Input vector `b` must not be a zero vector."
PASS_TWO_MSG = "The initial vector `b` must not be a zero vector."
NAN_TS = {"ts": np.array([0.25, float("nan")])}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def _table():
    """(catalogue call, Entry, what else is wrong beside a wrong b_len, zero-b faults, message)"""
    I = sc.inputs(MAT)
    n = I.n
    b, B = np.ascontiguousarray(I.b), np.asfortranarray(I.B[:, :S])
    X = np.zeros(n * S * M)
    al, be, bn = f64(K * S), f64(K * S), f64(S)
    steps = u64(*([K] * S))
    out = [("alphas", al.copy()), ("betas", be.copy()), ("steps", u64(*([0] * S))),
           ("b_norm", f64(S))]
    dec = [("alphas", al), ("n_alphas", K), ("betas", be), ("n_betas", K - 1), ("steps", K),
           ("b_norm", 1.0)]
    decs = [("alphas", al), ("betas", be), ("ld", K), ("steps", steps), ("b_norms", bn)]
    tol_out = [("steps_out", u64(*([0] * (S * M)))), ("converged", np.zeros(S * M, np.int32)),
               ("res_out", np.zeros(S * M * K)), ("res_len", u64(*([0] * (S * M))))]
    fs = (ctypes.c_void_p * M)(*([_lib.FTK_INV_PTR] * M))
    sig, ts, i32 = np.array(sc.sigmas(M)), np.array(sc.times(M)), np.zeros(S * M, np.int32)
    one = [("op", 0), ("b", b), ("b_len", n)]
    many = [("op", 0), ("b", B), ("b_len", n), ("s", S)]
    zero_b = [{"b": np.zeros(n)}]
    zero_col = [{"b": np.asfortranarray(bad_at(B.T, c, 0.0).T)} for c in ZERO_COLS]
    zero_norm = [{"b_norm": 0.0}]
    zero_norms = [{"b_norms": bad_at(bn, c, 0.0)} for c in ZERO_COLS]
    k0 = {"k": 0}
    tail = [("x", X), ("mem", HOST)]
    f_inv = [("f", _lib.FTK_INV_PTR), ("user", None)]
    rows = [
        ("pass_one", "tpl_lanczos_pass_one", one + [("k", K)] + out + [("mem", HOST)], k0, zero_b,
         SOLVE_MSG),
        ("standard", "tpl_lanczos_standard",
         one + [("k", K)] + out + [("v_out", None), ("mem", HOST), ("reorth", 0), ("cb", None),
                                   ("cb_user", None)], k0, zero_b, SOLVE_MSG),
        ("pass_two", "tpl_lanczos_pass_two",
         one + dec + [("y", f64(K)), ("y_len", K), ("x", X), ("v_out", None), ("mem", HOST)],
         {"y_len": K - 1, "b_norm": 0.0}, zero_norm, PASS_TWO_MSG),
        ("two_pass_inv", "tpl_lanczos_two_pass", one + [("k", K)] + f_inv + tail, k0, zero_b,
         SOLVE_MSG),
        ("two_pass_sq", "tpl_lanczos_two_pass", one + [("k", K), ("f", _lib.FTK_SQ_PTR),
                                                       ("user", None)] + tail, k0, zero_b,
         SOLVE_MSG),
        ("lanczos", "tpl_lanczos", one + [("k", K)] + f_inv + tail, k0, zero_b, SOLVE_MSG),
        ("two_pass_inv_tol_met", "tpl_lanczos_two_pass_inv_tol",
         one + [("k", K), ("tol", I.tol_met)] + tail + tol_out, k0, zero_b, SOLVE_MSG),
        ("two_pass_multi", "tpl_lanczos_two_pass_multi",
         one + [("k", K), ("fs", fs), ("users", None), ("m", M)] + tail, k0, zero_b, SOLVE_MSG),
        ("lanczos_multi", "tpl_lanczos_multi",
         one + [("k", K), ("fs", fs), ("users", None), ("m", M)] + tail, k0, zero_b, SOLVE_MSG),
        ("pass_two_multi", "tpl_lanczos_pass_two_multi",
         one + dec + [("y", f64(K * M)), ("y_len", K), ("m", M)] + tail,
         {"y_len": K + 1, "b_norm": 0.0}, zero_norm, PASS_TWO_MSG),
        ("two_pass_exp_times", "tpl_lanczos_two_pass_exp_times",
         one + [("k", K), ("ts", ts), ("m", M)] + tail + [("on_device", i32)],
         dict(k0, **NAN_TS), zero_b, SOLVE_MSG),
        ("two_pass_shifted_inv_tol", "tpl_lanczos_two_pass_shifted_inv_tol",
         one + [("k", K), ("sigmas", sig), ("m", M), ("tol", I.tol_mix)] + tail + tol_out, k0,
         zero_b, SOLVE_MSG),
        ("pass_two_multi_cut", "tpl_lanczos_pass_two_multi_cut",
         one + dec + [("y", f64(K * M)), ("ldy", K), ("col_steps", u64(K, 2)), ("m", M)] + tail,
         {"ldy": K - 1, "b_norm": 0.0}, zero_norm, PASS_TWO_MSG),
        ("two_pass_batch", "tpl_lanczos_two_pass_batch", many + [("k", K)] + f_inv + tail, k0,
         zero_col, SOLVE_MSG),
        ("pass_one_batch", "tpl_lanczos_pass_one_batch",
         many + [("k", K), ("alphas", al.copy()), ("betas", be.copy()),
                 ("steps", u64(*([0] * S))), ("b_norms", f64(S)), ("mem", HOST)], k0, zero_col,
         SOLVE_MSG),
        ("pass_two_batch", "tpl_lanczos_pass_two_batch", many + decs + [("y", f64(K * S))] + tail,
         {"b_norms": f64(S, 0.0)}, zero_norms, PASS_TWO_MSG),
        ("two_pass_batch_multi", "tpl_lanczos_two_pass_batch_multi",
         many + [("k", K), ("fs", fs), ("users", None), ("m", M)] + tail, k0, zero_col, SOLVE_MSG),
        ("pass_two_batch_multi", "tpl_lanczos_pass_two_batch_multi",
         many + decs + [("y", f64(K * S * M)), ("m", M)] + tail, {"b_norms": f64(S, 0.0)},
         zero_norms, PASS_TWO_MSG),
        ("two_pass_batch_exp_times", "tpl_lanczos_two_pass_batch_exp_times",
         many + [("k", K), ("ts", ts), ("m", M)] + tail + [("on_device", i32)], dict(k0, **NAN_TS),
         zero_col, SOLVE_MSG),
        ("two_pass_batch_shifted_inv_tol", "tpl_lanczos_two_pass_batch_shifted_inv_tol",
         many + [("k", K), ("sigmas", sig), ("m", M), ("tol", I.tol_mix)] + tail + tol_out, k0,
         zero_col, SOLVE_MSG),
        # its decomposition checks come before the device: the CPU file's subject; here the
        # dimension error behind them and the state after its zero ||b_c||
        ("pass_two_batch_multi_cut", "tpl_lanczos_pass_two_batch_multi_cut",
         many + decs + [("y", f64(K * S * M)), ("col_steps", u64(*([K, 2] * S))), ("m", M)] + tail,
         {}, zero_norms, PASS_TWO_MSG),
    ]
    return {name: (Entry(fn, args, []), also, zeros, msg) for name, fn, args, also, zeros, msg
            in rows}


_TABLE = None
NAMES = ["pass_one", "standard", "pass_two", "two_pass_inv", "two_pass_sq", "lanczos",
         "two_pass_inv_tol_met", "two_pass_multi", "lanczos_multi", "pass_two_multi",
         "two_pass_exp_times", "two_pass_shifted_inv_tol", "pass_two_multi_cut", "two_pass_batch",
         "pass_one_batch", "pass_two_batch", "two_pass_batch_multi", "pass_two_batch_multi",
         "two_pass_batch_exp_times", "two_pass_batch_shifted_inv_tol", "pass_two_batch_multi_cut"]


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = _table()
        assert list(_TABLE) == NAMES
    return _TABLE


def test_the_table_covers_every_solve_that_takes_b():
    import re
    hdr = open(sc.__file__.replace("tests/state_cases.py", "include/tpl.h")).read()
    want = set(re.findall(r"^tpl_status\s+(tpl_lanczos\w*)\s*\(", hdr, flags=re.M))
    assert {e.fn for e, _, _, _ in table().values()} == want


@pytest.mark.parametrize("name", NAMES)
def test_faults_behind_the_device_selection(name):
    e, also, zeros, msg = table()[name]
    n = sc.inputs(MAT).n
    p = sc.calls()[name].params(k=K, m=M, s=S)
    op = sc.new_op(MAT)
    try:
        # a wrong b_len, ahead of whatever else these checks would find
        rc, det = e.call(op, {"b_len": n + 1}, also)
        assert rc == DIM and det["status"] == DIM and "Dimension mismatch" in det["message"], det
        assert (det["operator_cols"], det["vector_rows"]) == (n, n + 1), det
        if "k" in dict(e.args):
            rc, det = e.call(op, also)
            assert rc == INPUT and "`k` must be at least 1" in det["message"], det
        for z in zeros:
            rc, det = e.call(op, z)
            assert rc == INPUT and det["status"] == INPUT and msg in det["message"], (z, det)
            got, want = sc.run_call(op, MAT, name, p), sc.fresh(MAT, sc.DEFAULT_SETTINGS, name, p)
            assert sc.same(got[0], want[0]), "bits differ from a fresh operator's after %s" % (z,)
            assert got[1] == want[1], "flags %d, fresh %d after %s" % (got[1], want[1], z)
    finally:
        op.close()
