"""CPU: which fault a solver entry point reports when a call has several (include/tpl.h; the
entry points of csrc/tpl_solvers*.cpp and csrc/tpl_ftk_device.cpp).

Every call here is made on a host-only plan (tpl_plan_create), so nothing touches a device: a
check that an entry point makes before it selects the device reports its own fault, and every
later check is hidden behind the plan's refusal ("host-only plan"). One table row per entry
point lists its early checks as stages, in the order the entry point makes them, each with the
faults that trip it. The test asserts, per row:
  - every fault alone: the stage's status and a substring of tpl_last_error_detail's message;
  - every pair of faults of two different stages: the earlier stage's status and message;
  - the faults the row lists as `late` (checked only once the device is selected: a wrong b_len,
    k = 0, a non-finite time ...): still the plan's refusal — that is the order;
  - with everything valid: the plan's refusal (or, for the two accessors that need no device,
    success).
tpl_lanczos_pass_two_batch_multi_cut checks its decompositions per column before the device;
its column order has a test of its own.
"""
import ctypes
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import tpl_amd
from tpl_amd import _lib

N, K, S, M, LD = 12, 5, 7, 2, 5          # s = 7: a group of four, a group of two, a remainder
NAN, INF = float("nan"), float("inf")
ARG, INPUT, UNSUP = (_lib.TPL_ERR_INVALID_ARGUMENT, _lib.TPL_ERR_INPUT, _lib.TPL_ERR_UNSUPPORTED)

NULL = (ARG, "NULL")
S_RANGE = (ARG, "s must be between 1 and TPL_BATCH_MAX")
M_RANGE = (ARG, "m must be between 1 and TPL_MULTI_MAX")
TOL = (ARG, "tol must be a number >= 0")
SIGMA = (ARG, "every shift sigma_i must be finite")
PLAN = (ARG, "host-only plan")
N_ZERO = (ARG, "n must be >= 1")
BOUND = (UNSUP, "k above the device f(T_k) bound")
OK = (_lib.TPL_OK, "")


@pytest.fixture(scope="module")
def plan():
    a = sp.diags([np.full(N - 1, -1.0), np.full(N, 2.5), np.full(N - 1, -1.0)], [-1, 0, 1]).tocsr()
    p = tpl_amd.HostPlan(a)
    yield p
    p.close()


def f64(n, v=1.0):
    return np.full(n, v, dtype=np.float64)


def u64(*v):
    return np.array(v, dtype=np.uint64)


def bad_at(arr, i, v):
    out = arr.copy()
    out[i] = v
    return out


def _conv(v, t):
    """A table value as the ctypes argument of type t (arrays stay alive in the table)."""
    if isinstance(v, np.ndarray):
        return v.ctypes.data if t is ctypes.c_void_p else ctypes.cast(v.ctypes.data, t)
    return v


class Entry:
    """fn: the C entry point; args: (name, valid value) in C order, "op" filled in per test;
    stages: [(expect, [fault, ...])] in the order the checks are made, a fault a dict of
    argument overrides; late: faults that only a check behind the device selection sees;
    valid: what an all-valid call on a plan reports."""

    def __init__(self, fn, args, stages, late=(), valid=PLAN):
        self.fn, self.args, self.stages, self.late, self.valid = fn, args, stages, late, valid

    def call(self, plan, *faults):
        a = dict(self.args)
        a["op"] = plan.handle
        for f in faults:
            a.update(f)
        fn = getattr(_lib, self.fn)
        rc = fn(*[_conv(a[name], t) for (name, _), t in zip(self.args, fn.argtypes)])
        return rc, _lib.last_error_detail()


def nulls(*names):
    return [{n: None} for n in names]


def count_faults(name, top):
    return [{name: 0}, {name: top + 1}]


FS = (ctypes.c_void_p * 64)(*([_lib.FTK_INV_PTR] * 64))
B1, BS = f64(N), f64(N * S)
X = np.zeros(N * S * M)
AL, BE, Y1 = f64(LD), f64(LD), f64(LD * M)            # one decomposition of LD steps
ALS, BES, YS = f64(LD * S), f64(LD * S), f64(LD * S * M)
STEPS_OUT, BN_OUT = u64(*([0] * S)), f64(S)
STEPS_S = u64(5, 4, 3, 5, 2, 1, 3)                    # steps[c] <= LD; column 5 takes one step
COLS_S = np.minimum(np.repeat(STEPS_S, M), u64(*([3, 1] * S)))
SIG, TS = f64(M, 0.5), f64(M, 0.25)
I32 = np.zeros(S * M, dtype=np.int32)
RES, RLEN = np.zeros(S * M * K), u64(*([0] * (S * M)))
TOL_FAULTS = [{"tol": NAN}, {"tol": -1.0}]
HOST = _lib.TPL_MEM_HOST


def ends(name, arr, v=NAN):
    """A non-finite entry at the first and at the last index."""
    return [{name: bad_at(arr, 0, v)}, {name: bad_at(arr, len(arr) - 1, INF)}]


SINGLE_LATE = [{"b": None}, {"b_len": N + 1}, {"k": 0}]
DEC_OUT = [("alphas", AL), ("betas", BE), ("steps", STEPS_OUT), ("b_norm", BN_OUT)]
DEC_IN = [("alphas", AL), ("n_alphas", LD), ("betas", BE), ("n_betas", LD - 1), ("steps", LD),
          ("b_norm", 1.0)]
DECS_IN = [("alphas", ALS), ("betas", BES), ("ld", LD), ("steps", STEPS_S), ("b_norms", f64(S))]
TOL_OUT = [("steps_out", RLEN.copy()), ("converged", I32), ("res_out", RES), ("res_len", RLEN)]

ENTRIES = [
    # ---- the single-column solves
    Entry("tpl_op_apply", [("op", 0), ("x", B1), ("y", X), ("mem", HOST)],
          [(NULL, nulls("op", "x", "y"))]),
    Entry("tpl_lanczos_pass_one",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K)] + DEC_OUT + [("mem", HOST)],
          [(NULL, nulls("op", "alphas", "betas", "steps", "b_norm"))], SINGLE_LATE),
    Entry("tpl_lanczos_standard",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K)] + DEC_OUT +
          [("v_out", None), ("mem", HOST), ("reorth", 0), ("cb", None), ("cb_user", None)],
          [(NULL, nulls("op", "alphas", "betas", "steps", "b_norm"))],
          SINGLE_LATE + [{"reorth": 7}]),
    Entry("tpl_lanczos_pass_two",
          [("op", 0), ("b", B1), ("b_len", N)] + DEC_IN +
          [("y", Y1), ("y_len", LD), ("x", X), ("v_out", None), ("mem", HOST)],
          [(NULL, nulls("op", "x"))],
          [{"b": None}, {"b_len": N - 1}, {"y_len": LD - 1}, {"b_norm": 0.0}, {"alphas": None}]),
    Entry("tpl_lanczos_two_pass",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("f", _lib.FTK_INV_PTR), ("user", None),
           ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "x"))], SINGLE_LATE + [{"f": None}]),
    Entry("tpl_lanczos",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("f", _lib.FTK_INV_PTR), ("user", None),
           ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "x"))], SINGLE_LATE + [{"f": None}]),
    Entry("tpl_lanczos_two_pass_inv_tol",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("tol", 1e-6), ("x", X), ("mem", HOST)] +
          TOL_OUT,
          [(NULL, nulls("op", "x")), (TOL, TOL_FAULTS)],
          SINGLE_LATE + [{"steps_out": None, "converged": None, "res_out": None, "res_len": None}]),
    # ---- m functions of one b
    Entry("tpl_lanczos_two_pass_multi",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("fs", FS), ("users", None), ("m", M),
           ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "fs", "x")), (M_RANGE, count_faults("m", 64))], SINGLE_LATE),
    Entry("tpl_lanczos_multi",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("fs", FS), ("users", None), ("m", M),
           ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "fs", "x")), (M_RANGE, count_faults("m", 64))], SINGLE_LATE),
    Entry("tpl_lanczos_pass_two_multi",
          [("op", 0), ("b", B1), ("b_len", N)] + DEC_IN +
          [("y", Y1), ("y_len", LD), ("m", M), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "x")), (M_RANGE, count_faults("m", 64))],
          [{"b": None}, {"b_len": N + 1}, {"y_len": LD + 1}, {"b_norm": 0.0}, {"y": None}]),
    Entry("tpl_lanczos_two_pass_exp_times",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("ts", TS), ("m", M), ("x", X),
           ("mem", HOST), ("on_device", I32)],
          [(NULL, nulls("op", "ts", "x")), (M_RANGE, count_faults("m", 64))],
          SINGLE_LATE + ends("ts", TS) + [{"on_device": None}]),
    Entry("tpl_lanczos_two_pass_shifted_inv_tol",
          [("op", 0), ("b", B1), ("b_len", N), ("k", K), ("sigmas", SIG), ("m", M), ("tol", 1e-6),
           ("x", X), ("mem", HOST)] + TOL_OUT,
          [(NULL, nulls("op", "sigmas", "x")), (M_RANGE, count_faults("m", 64)), (TOL, TOL_FAULTS),
           (SIGMA, ends("sigmas", SIG))], SINGLE_LATE),
    Entry("tpl_lanczos_pass_two_multi_cut",
          [("op", 0), ("b", B1), ("b_len", N)] + DEC_IN +
          [("y", Y1), ("ldy", LD), ("col_steps", u64(5, 2)), ("m", M), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "x", "col_steps", "y")), (M_RANGE, count_faults("m", 64))],
          [{"b": None}, {"b_len": N + 1}, {"steps": 0}, {"ldy": LD - 1}, {"col_steps": u64(0, 2)},
           {"col_steps": u64(5, 6)}, {"b_norm": 0.0}, {"alphas": None}]),
    # ---- s right-hand sides
    Entry("tpl_lanczos_two_pass_batch",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S), ("k", K), ("f", _lib.FTK_INV_PTR),
           ("user", None), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "b", "x", "f")), (S_RANGE, count_faults("s", 64))],
          [{"b_len": N + 1}, {"k": 0}]),
    Entry("tpl_lanczos_pass_one_batch",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S), ("k", K), ("alphas", ALS), ("betas", BES),
           ("steps", STEPS_OUT), ("b_norms", BN_OUT), ("mem", HOST)],
          [(NULL, nulls("op", "b", "alphas", "betas", "steps", "b_norms")),
           (S_RANGE, count_faults("s", 64))], [{"b_len": N + 1}, {"k": 0}]),
    Entry("tpl_lanczos_pass_two_batch",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S)] + DECS_IN +
          [("y", f64(LD * S)), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "b", "x", "steps", "b_norms")), (S_RANGE, count_faults("s", 64))],
          [{"b_len": N + 1}, {"b_norms": bad_at(f64(S), 0, 0.0)}, {"ld": 1}, {"alphas": None},
           {"y": None}, {"betas": None}]),
    Entry("tpl_lanczos_two_pass_batch_multi",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S), ("k", K), ("fs", FS), ("users", None),
           ("m", M), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "b", "fs", "x")), (S_RANGE, count_faults("s", 64)),
           (M_RANGE, count_faults("m", 64))], [{"b_len": N + 1}, {"k": 0}]),
    Entry("tpl_lanczos_pass_two_batch_multi",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S)] + DECS_IN +
          [("y", YS), ("m", M), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "b", "x", "steps", "b_norms")), (S_RANGE, count_faults("s", 64)),
           (M_RANGE, count_faults("m", 64))],
          [{"b_len": N + 1}, {"b_norms": bad_at(f64(S), S - 1, 0.0)}, {"ld": 1}, {"alphas": None},
           {"y": None}, {"betas": None}]),
    Entry("tpl_lanczos_two_pass_batch_exp_times",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S), ("k", K), ("ts", TS), ("m", M), ("x", X),
           ("mem", HOST), ("on_device", I32)],
          [(NULL, nulls("op", "b", "ts", "x")), (S_RANGE, count_faults("s", 64)),
           (M_RANGE, count_faults("m", 64))],
          [{"b_len": N + 1}, {"k": 0}, {"on_device": None}] + ends("ts", TS)),
    Entry("tpl_lanczos_two_pass_batch_shifted_inv_tol",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S), ("k", K), ("sigmas", SIG), ("m", M),
           ("tol", 1e-6), ("x", X), ("mem", HOST)] + TOL_OUT,
          [(NULL, nulls("op", "b", "sigmas", "x")), (S_RANGE, count_faults("s", 64)),
           (M_RANGE, count_faults("m", 64)), (TOL, TOL_FAULTS), (SIGMA, ends("sigmas", SIG))],
          [{"b_len": N + 1}, {"k": 0}]),
    Entry("tpl_lanczos_pass_two_batch_multi_cut",
          [("op", 0), ("b", BS), ("b_len", N), ("s", S)] + DECS_IN +
          [("y", YS), ("col_steps", COLS_S), ("m", M), ("x", X), ("mem", HOST)],
          [(NULL, nulls("op", "b", "x", "steps", "b_norms", "col_steps", "y", "alphas")),
           (S_RANGE, count_faults("s", 64)), (M_RANGE, count_faults("m", 64)),
           # the per-column checks as one stage here; their own order: test_cut_column_order
           ((ARG, "steps[c] must be >= 1 and ld >= steps[c]"),
            [{"steps": bad_at(STEPS_S, c, v)} for c in (0, 3, S - 1) for v in (0, LD + 1)])],
          [{"b_len": N + 1}]),
    # ---- the device f(T_k) probes and the accessors
    Entry("tpl_op_ftk_device",
          [("op", 0), ("which", 0), ("alphas", AL), ("n", LD), ("betas", BE), ("y", Y1),
           ("on_device", I32)],
          [(NULL, nulls("op", "alphas", "y", "on_device") + [{"betas": None, "n": 2}]),
           ((ARG, "which must be 0 (inv) or 1 (exp)"), [{"which": -1}, {"which": 2}]),
           (N_ZERO, [{"n": 0}]), (BOUND, [{"n": 1801}])],
          [{"n": 1, "betas": None}]),
    Entry("tpl_op_ftk_exp_times_device",
          [("op", 0), ("alphas", AL), ("n", LD), ("betas", BE), ("ts", TS), ("m", M), ("y", Y1),
           ("on_device", I32)],
          [(NULL, nulls("op", "alphas", "ts", "y", "on_device") + [{"betas": None, "n": 2}]),
           (M_RANGE, count_faults("m", 64)), (N_ZERO, [{"n": 0}]), (BOUND, [{"n": 1801}])],
          [{"n": 1, "betas": None}] + ends("ts", TS)),
    Entry("tpl_op_ftk_inv_shifts_device",
          [("op", 0), ("alphas", AL), ("n", LD), ("betas", BE), ("sigmas", SIG), ("m", M),
           ("y", Y1)],
          [(NULL, nulls("op", "alphas", "sigmas", "y") + [{"betas": None, "n": 2}]),
           (M_RANGE, count_faults("m", 64)),
           (N_ZERO, [{"n": 0}]), (BOUND, [{"n": 1366}])],
          [{"n": 1, "betas": None}] + ends("sigmas", SIG)),
    Entry("tpl_op_ftk_exp_times_batch_device",
          [("op", 0), ("alphas", ALS), ("betas", BES), ("ld", LD), ("steps", u64(5, 3, 1, 2)),
           ("nb", 4), ("ts", TS), ("m", M), ("y", np.zeros(LD * 4 * M)), ("on_device", I32)],
          [(NULL, nulls("op", "alphas", "steps", "ts", "y", "on_device")),
           ((ARG, "nb must be 2 or 4"), [{"nb": 0}, {"nb": 1}, {"nb": 3}, {"nb": 5}]),
           (M_RANGE, count_faults("m", 64)),
           ((ARG, "steps[c] must be between 1 and ld"),
            [{"steps": bad_at(u64(5, 3, 1, 2), c, v)} for c in (0, 2, 3) for v in (0, LD + 1)]),
           (BOUND, [{"steps": u64(1, 1, 1801, 1), "ld": 2000}])],
          [{"steps": u64(1, 1, 1, 1), "betas": None}] + ends("ts", TS)),
    Entry("tpl_op_set_device_ftk", [("op", 0), ("mode", 2)],
          [((ARG, "op is NULL"), nulls("op")),
           ((ARG, "device f(T_k) mode must be 0, 1 or 2"), [{"mode": -1}, {"mode": 3}])],
          valid=OK),
    Entry("tpl_op_reorth_second_passes", [("op", 0), ("count", np.zeros(1, dtype=np.int64))],
          [(NULL, nulls("op", "count"))], valid=OK),
]
IDS = [e.fn for e in ENTRIES]


def expect(e, got, want, what):
    rc, det = got
    status, text = want
    assert rc == status and det["status"] == status and text in det["message"], \
        (e.fn, what, rc, det["message"])
    if want != PLAN:
        assert "host-only" not in det["message"], (e.fn, what)


def test_the_table_covers_every_solver_entry_point():
    """The four units' exported entry points, from the library itself."""
    import re
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    have = set(re.findall(r"\bT (tpl_lanczos\w*|tpl_op_ftk_\w*device|tpl_op_apply|"
                          r"tpl_op_set_device_ftk|tpl_op_reorth_second_passes)\b", nm))
    assert have == set(IDS), have ^ set(IDS)
    # the one entry point without arguments
    assert 1 <= _lib.tpl_batch_shifted_inv_tol_auto_k() <= 1365


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_each_fault_alone(plan, e):
    for want, faults in e.stages:
        for f in faults:
            expect(e, e.call(plan, f), want, f)


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_the_earlier_check_wins(plan, e):
    """Every pair of faults of two stages, and every early fault beside every late one."""
    for (want, first), (_, second) in itertools.combinations(e.stages, 2):
        for f, g in itertools.product(first, second):
            if set(f) & set(g):
                continue            # the two faults need the same argument
            expect(e, e.call(plan, g, f), want, (f, g))
    for want, faults in e.stages:
        for f, g in itertools.product(faults, e.late):
            if not set(f) & set(g):
                expect(e, e.call(plan, g, f), want, (f, g))


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_late_faults_and_valid_calls_reach_the_plan_refusal(plan, e):
    expect(e, e.call(plan), e.valid, "valid")
    for g in e.late:
        expect(e, e.call(plan, g), PLAN, g)


def test_the_upper_ends_of_the_ranges_are_valid(plan):
    """s = TPL_BATCH_MAX, m = TPL_MULTI_MAX, tol = 0 and +inf pass the range checks."""
    by = {e.fn: e for e in ENTRIES}
    e = by["tpl_lanczos_two_pass_batch_shifted_inv_tol"]
    for tol in (0.0, INF):
        expect(e, e.call(plan, {"s": 64, "m": 64, "sigmas": f64(64, 0.5), "tol": tol}), PLAN, tol)
    e = by["tpl_lanczos_two_pass_shifted_inv_tol"]
    for tol in (0.0, INF):
        expect(e, e.call(plan, {"m": 64, "sigmas": f64(64, 0.5), "tol": tol}), PLAN, tol)
    expect(e, e.call(plan, {"m": 64, "sigmas": bad_at(f64(64, 0.5), 63, NAN)}), SIGMA, "last of 64")
    e = by["tpl_lanczos_two_pass_inv_tol"]
    for tol in (0.0, INF):
        expect(e, e.call(plan, {"tol": tol}), PLAN, tol)


def test_cut_column_order(plan):
    """tpl_lanczos_pass_two_batch_multi_cut, per column in ascending order and within a column
    steps, then col_steps, then the zero b, then betas: the first column at fault decides,
    whatever a later column's fault is, and within one column the earlier check."""
    e = next(x for x in ENTRIES if x.fn == "tpl_lanczos_pass_two_batch_multi_cut")
    STEPS = (ARG, "steps[c] must be >= 1 and ld >= steps[c]")
    CUT = (ARG, "every col_steps[c m + i] must be between 1 and steps[c]")
    ZERO_B = (INPUT, "The initial vector `b` must not be a zero vector.")
    BETAS = (ARG, "decomposition arrays shorter than steps_taken")
    cols = (0, 3, S - 1)             # in the group of four, in it again, the remainder column

    def fault(kind, c):
        if kind is STEPS:
            return {"steps": bad_at(STEPS_S, c, 0 if c else LD + 1)}
        if kind is CUT:              # above steps[c] in its first function, 0 in its last
            return {"col_steps": bad_at(COLS_S, c * M + (c % M), 0 if c % M else 9)}
        if kind is ZERO_B:
            return {"b_norms": bad_at(f64(S), c, 0.0)}
        return {"betas": None}       # every column of more than one step lacks its betas

    kinds = (STEPS, CUT, ZERO_B, BETAS)
    for k in kinds:
        for c in cols:
            expect(e, e.call(plan, fault(k, c)), k, (k, c))
    # betas == NULL is no fault for a column of one step (column 5): it is column 0's
    expect(e, e.call(plan, fault(BETAS, 0), fault(ZERO_B, 5)), BETAS, "betas before column 5")
    # within one column
    for (i, k1), (j, k2) in itertools.combinations(enumerate(kinds), 2):
        for c in cols:
            f, g = fault(k1, c), fault(k2, c)
            if k2 is BETAS and c > 0:
                continue             # a NULL betas is column 0's fault, ahead of column c's
            expect(e, e.call(plan, g, f), k1, (k1, k2, c))
    # across columns: the lower column's fault, of whichever kind
    for k1, k2 in itertools.permutations(kinds[:3], 2):
        for c1, c2 in itertools.combinations(cols, 2):
            f, g = fault(k1, c1), fault(k2, c2)
            if set(f) & set(g):
                continue
            expect(e, e.call(plan, g, f), k1, (k1, c1, k2, c2))
    # the range checks come before every column check, the plan's refusal after all of them
    for k in kinds:
        expect(e, e.call(plan, fault(k, 0), {"m": 65}), M_RANGE, k)
        expect(e, e.call(plan, fault(k, 0), {"s": 0}), S_RANGE, k)
        expect(e, e.call(plan, fault(k, S - 1), {"b_len": N + 1}), k, k)


def test_exp_times_batch_probe_column_order(plan):
    """tpl_op_ftk_exp_times_batch_device checks per column steps[c], then betas: a NULL betas
    is the fault of the first column of more than one step, ahead of a later column's count
    and behind an earlier one's; the bound on the largest count comes after every column."""
    e = next(x for x in ENTRIES if x.fn == "tpl_op_ftk_exp_times_batch_device")
    STEPS = (ARG, "steps[c] must be between 1 and ld")
    expect(e, e.call(plan, {"betas": None}), NULL, "betas")
    expect(e, e.call(plan, {"betas": None, "steps": u64(5, 3, 0, 2)}), NULL, "column 0 first")
    expect(e, e.call(plan, {"betas": None, "steps": u64(1, 0, 3, 2)}), STEPS, "column 1 first")
    expect(e, e.call(plan, {"betas": None, "steps": u64(6, 3, 1, 2)}), STEPS, "within column 0")
    expect(e, e.call(plan, {"betas": None, "m": 0}), M_RANGE, "m before the columns")
    expect(e, e.call(plan, {"steps": u64(1801, 1, 1, 0), "ld": 2000}), STEPS, "before the bound")
