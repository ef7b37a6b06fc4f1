"""GPU: whatever ran before on an operator, a call returns a fresh operator's bits and path flags.

An operator (two-pass-lanczos_amd/csrc/tpl_op.h) keeps about fifteen lazily sized buffer groups
and a cache of captured graphs that hold raw device pointers and baked-in scalars; the solver
entry points and the setters share all of it. The rules that keep this right — growing drops the
cached graphs, a buffer follows kcap, no graph holds a small table, the next solve's pass one
rewrites the cache rows — are prose in that header. Here they are one property, walked over the
cross product of the catalogue in tests/state_cases.py: every ordered pair of calls, resize
ladders in k, m and s, a setter between two calls, random walks, failed calls between good ones,
two operators on one stream, device-resident inputs.

Every comparison is np.array_equal on the uint64 words of every array of the result tuple, plus
equality of the flag bits (5: one graph, 8: long-row cache read, 9: fused pass two) that the call
itself defines (state_cases.Call.defines quotes the header). The reference is `fresh`: the same
call on a new operator under the same settings, itself compared bitwise with the device-order
oracle once per (matrix, settings) (state_cases.anchor).

Measured figures of the checks that carry a bound: none — every comparison is word for word.

Executed: 38 calls, so 2 x 38 x 38 = 2,888 ordered pairs (8,664 compared calls); 576 ladder steps
and the same 576 again with a compared call of another family after each (1,728 compared calls);
15 setter values x 7 calls x 2 matrices x 3 calls (max_g2 = 1 among them: the band's element grid
goes from three row blocks of 512 to one of 1536 and back); 16 walks x 40 steps x 2 matrices =
1,280 steps, 1,028 of them calls and 252 setters. No flag bit is masked beyond Call.defines.
`fresh` itself is anchored in the oracle for all 33 calls tests/composed_oracle.py composes.

Wall time on one MI355X: this file 15.2 s for its 118 cases (the slowest case 1.1 s, the first,
which fills `fresh`); tests/test_call_order_cpu.py 2.2 s on the host; the whole `-m gpu` run of
the commit before this file 190 s (1,554 cases), with it 208 s (1,671).

What it found in the runtime, each kept as a named regression test at the end of the file:
the multi-function, batch and basis-returning stand-alone passes two left bits 8 / 9 as an earlier
fused solve had set them; and, now and then, a first call with a cut table read zeros for its
cuts (test_first_cut_call_of_an_operator_reads_its_own_cuts states what is known of the cause).
"""
import numpy as np
import pytest

import state_cases as sc

pytestmark = pytest.mark.gpu

import tpl_amd  # noqa: E402
from tpl_amd import LanczosError, TplError, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

CALLS = sc.call_names()
D = sc.DEFAULT_SETTINGS
BAD = (LanczosError, TplError)   # which of the two a refusal raises is other tests' subject


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def check(op, mat, settings, name, params, where, device=False):
    """Run the call on `op` and compare it with fresh; `where` names the history."""
    got = sc.run_call(op, mat, name, params, device)
    want = sc.fresh(mat, settings, name, params)
    assert sc.same(got[0], want[0]), "bits differ from a fresh operator's: %s" % (where,)
    assert got[1] == want[1], "flags %d, fresh %d: %s" % (got[1], want[1], where)


def default_params(name):
    return sc.calls()[name].params()


# ---- 1. every ordered pair -------------------------------------------------------------------
@pytest.mark.parametrize("first", CALLS)
def test_every_ordered_pair(first):
    """A, then B equals fresh(B), then A again — a replay after B — equals fresh(A); for every
    B of the catalogue, on both matrices, at K_SMALL."""
    pa = default_params(first)
    for mat in sc.MATRICES:
        for second in CALLS:
            pb = default_params(second)
            op = sc.new_op(mat)
            try:
                check(op, mat, D, first, pa, (first, "alone", mat))
                check(op, mat, D, second, pb, (first, second, mat))
                check(op, mat, D, first, pa, (first, second, first, mat))
            finally:
                op.close()


# ---- 2. resize ladders -------------------------------------------------------------------------
def ladder(call):
    """The (k, m, s) steps of a call's ladders: k small, big, small, 1, big; m 1, 5, 64, 2;
    s 2, 4, 3, 7, 2 — each for the sizes the call takes."""
    steps = []
    if "k" in call.takes:
        steps += [call.params(k=k) for k in (sc.K_SMALL, sc.K_BIG, sc.K_SMALL, 1, sc.K_BIG)]
    if "m" in call.takes:
        steps += [call.params(m=m) for m in (1, 5, 64, 2)]
    if "s" in call.takes:
        steps += [call.params(s=s) for s in (2, 4, 3, 7, 2)]
    return steps or [call.params()] * 2


LADDER_STEPS = {name: len(ladder(sc.calls()[name])) for name in CALLS}


@pytest.mark.parametrize("name", CALLS)
def test_resize_ladders(name):
    """One operator per (call, matrix) walks the call's ladders, every step equal to fresh; a
    second operator walks them again with a call of another family between the steps (a single
    solve between batch steps, a batch solve between multi-function steps, a re-orthogonalised
    pass between tolerance steps, ...), itself compared at the step's k."""
    call = sc.calls()[name]
    other = sc.calls()[sc.INTERLEAVE[call.family]]
    for mat in sc.MATRICES:
        for interleave in (False, True):
            op = sc.new_op(mat)
            done = []
            try:
                for p in ladder(call):
                    done.append((name, p))
                    check(op, mat, D, name, p, (mat, done))
                    if interleave:
                        q = other.params(k=dict(p).get("k"))
                        done.append((other.name, q))
                        check(op, mat, D, other.name, q, (mat, done))
            finally:
                op.close()


# ---- 3. a setter between calls -----------------------------------------------------------------
SETTER_CASES = [(n, v) for n in sc.SETTING_NAMES for v in sc.SETTINGS[n][2]]


@pytest.mark.parametrize("setter,value", SETTER_CASES, ids=["%s=%s" % c for c in SETTER_CASES])
def test_setter_between_calls(setter, value):
    """The call, the setting changed, the call, the setting restored, the call: each against
    fresh under the settings in force at that moment (a layout rebuild changes the bits by
    design, so never across settings)."""
    changed = sc.with_setting(D, setter, value)
    for mat in sc.MATRICES:
        for name in sc.SETTER_CALLS:
            p = default_params(name)
            op = sc.new_op(mat)
            try:
                check(op, mat, D, name, p, (mat, name, "before", setter))
                sc.apply_setting(op, setter, value)
                check(op, mat, changed, name, p, (mat, name, "after", setter, value))
                sc.apply_setting(op, setter, sc.SETTINGS[setter][1])
                check(op, mat, D, name, p, (mat, name, "restored", setter))
            finally:
                op.close()


# ---- 4. random walks -----------------------------------------------------------------------------
def run_walk(mat, steps, label):
    op = sc.new_op(mat)
    settings = D
    try:
        for i, (kind, name, arg) in enumerate(steps):
            if kind == "set":
                sc.apply_setting(op, name, arg)
                settings = sc.with_setting(settings, name, arg)
            else:
                check(op, mat, settings, name, arg,
                      "%s on %s, steps so far:\n%s" % (label, mat, sc.describe(steps[:i + 1])))
    finally:
        op.close()


@pytest.mark.parametrize("seed", sc.WALK_SEEDS)
def test_random_walk(seed):
    """40 steps on one operator per matrix: random calls at random ladder sizes and, about one
    step in five, a random setter. Every call step is compared with fresh under the settings
    then in force. A failure prints the seed and the step list up to the failing step."""
    steps = sc.walk(seed)
    for mat in sc.MATRICES:
        run_walk(mat, steps, "walk seed %d" % seed)


# ---- 5. failed calls between good ones ---------------------------------------------------------
def _failures(I, op):
    """(label, exception, thunk): calls the runtime refuses on the host, or whose bad values the
    kernels carry as data."""
    n = I.n
    B_nan = I.B[:, :4].copy(order="F")
    B_nan[7, 2] = np.nan
    B_zero = I.B[:, :4].copy(order="F")
    B_zero[:, 1] = 0.0

    def raises(alphas, betas):
        raise RuntimeError("no f(T_k) today")

    return [
        ("zero b", BAD,
         lambda: solvers.lanczos_two_pass(op, np.zeros(n), sc.K_SMALL, "inv")),
        ("zero column", BAD,
         lambda: solvers.lanczos_two_pass_batch(op, B_zero, sc.K_SMALL, "inv")),
        ("NaN column", None,
         lambda: solvers.lanczos_two_pass_batch(op, B_nan, sc.K_SMALL, "inv")),
        ("m = 65", BAD,
         lambda: solvers.lanczos_two_pass_shifted_inv_tol(op, I.b, sc.K_SMALL,
                                                          np.arange(1.0, 66.0), 1e-3)),
        ("closure raises", BAD,
         lambda: solvers.lanczos_two_pass(op, I.b, sc.K_SMALL, raises)),
        ("closure of the wrong length", BAD,
         lambda: solvers.lanczos_two_pass_multi(op, I.b, sc.K_SMALL,
                                                ["inv", lambda a, b: np.ones(len(a) + 1)])),
        ("dimension mismatch", BAD,
         lambda: solvers.lanczos_two_pass(op, np.ones(n + 1), sc.K_SMALL, "inv")),
    ]


def test_errors_between_calls(monkeypatch):
    """After each failed call, and after a growth refused through TPL_TEST_ALLOC_CAP, the next
    good call of every family — single, multi, batch, batch-multi, tolerance, standard —
    equals fresh."""
    cap = "TPL_TEST_ALLOC_CAP"
    for mat in sc.MATRICES:
        I = sc.inputs(mat)
        op = sc.new_op(mat)
        try:
            family = [(name, default_params(name)) for name in sc.FAMILY_CALLS]
            for name, p in family:
                check(op, mat, D, name, p, (mat, "before any failure", name))
            for label, exc, thunk in _failures(I, op):
                if exc is None:
                    thunk()      # carried as data: the call succeeds
                else:
                    with pytest.raises(exc):
                        thunk()
                for name, p in family:
                    check(op, mat, D, name, p, (mat, "after", label, name))
            # a refused growth: the state, the batch buffers, the basis
            grow = [("two_pass_inv", "state"), ("two_pass_batch_s4", "batch buffers"),
                    ("standard_reorth", "basis")]
            for name, what in grow:
                big = sc.calls()[name].params(k=64)
                # every request is refused: the batch buffers and the basis are freed before
                # they grow, so a cap at the operator's present bytes could let the larger
                # buffer in where the freed ones were larger still
                monkeypatch.setenv(cap, "1")
                with pytest.raises(TplError) as e:
                    sc.run_call(op, mat, name, big)
                monkeypatch.delenv(cap)
                assert e.value.status == tpl_amd._lib.TPL_ERR_OUT_OF_MEMORY, (what, e.value)
                for other, p in family:
                    check(op, mat, D, other, p, (mat, "after a refused growth of the", what, other))
                check(op, mat, D, name, big, (mat, "the growth itself, allowed", what))
        finally:
            op.close()


# ---- 6. two operators, one context ---------------------------------------------------------------
def test_two_operators_one_context():
    """Operators of both matrices share the default context and its stream; their calls
    interleaved, each result equals its own fresh result."""
    ops = {mat: sc.new_op(mat) for mat in sc.MATRICES}
    try:
        assert len({op._ctx for op in ops.values()}) == 1
        order = CALLS + CALLS[::-1]
        for i, name in enumerate(order):
            other = order[(i + 7) % len(order)]
            check(ops["kkt"], "kkt", D, name, default_params(name), ("kkt", i, name))
            check(ops["band"], "band", D, other, default_params(other), ("band", i, other))
    finally:
        for op in ops.values():
            op.close()


# ---- 7. device-resident inputs ---------------------------------------------------------------------
DEVICE_CALLS = [n for n in CALLS if sc.calls()[n].device_b]


def test_device_inputs():
    """The pair test's diagonal (A, then A) with b / B as torch CUDA tensors: the bits of the
    host-input run."""
    pytest.importorskip("torch")
    assert len(DEVICE_CALLS) >= 30
    for mat in sc.MATRICES:
        for name in DEVICE_CALLS:
            p = default_params(name)
            op = sc.new_op(mat)
            try:
                check(op, mat, D, name, p, (mat, name, "device b"), device=True)
                check(op, mat, D, name, p, (mat, name, "device b, again"), device=True)
            finally:
                op.close()


# ---- 8. named regressions: the shortest sequences the generated tests reduced to -----------------
@pytest.mark.parametrize("second", ["pass_two_with_basis", "pass_two_multi", "pass_two_multi_cut",
                                    "pass_two_batch_multi", "pass_two_batch_multi_cut",
                                    "pass_two_batch"])
def test_unfused_pass_two_clears_the_fused_flag(second):
    """tpl.h: bit 8 tells of "the last pass two the operator ran", bit 9 that "that pass two ran
    fused". After a fused tpl_lanczos_two_pass, a stand-alone pass two of the multi-function,
    batch or basis-returning kind left bit 9 (the basis-returning one bit 8 too) as the solve
    had set it: only the single pass two and the solvers' scope cleared it. s = 2 keeps the
    batch pass two free of a remainder column, whose single pass two cleared the bits."""
    op = sc.new_op("kkt")
    try:
        _, flags = sc.run_call(op, "kkt", "two_pass_inv", default_params("two_pass_inv"))
        assert flags & (sc.CACHED | sc.FUSED) == sc.CACHED | sc.FUSED
        p = sc.calls()[second].params(s=2)
        check(op, "kkt", D, second, p, ("two_pass_inv", second))
        assert op.flags() & (sc.CACHED | sc.FUSED) == 0
    finally:
        op.close()


def test_first_cut_call_of_an_operator_reads_its_own_cuts():
    """An operator's first call with a cut table allocates and zeroes the table, then uploads
    the cuts on its stream. Seen: in a few runs of this file, one to three of the 76 pairs whose
    second call was pass_two_multi_cut differed from fresh, each time with the bits of a table of
    zeros (the uncut column held its first term only, the column cut at 1 was right). Supposed
    cause, not demonstrated: the zeroes went through the null stream, which is not ordered with
    the operator's non-blocking stream, and landed after the upload; the runtime now zeroes new
    allocations on the operator's stream, and no run since has shown the difference. This test
    cannot prove that: on the earlier runtime it passes in most runs. It pins the property all
    the same, against a reference that has no cut table: column i is tpl_lanczos_pass_two on the
    decomposition cut to cuts[i] steps, from one operator. Thirty-two new operators each make
    the single-b and the batch cut call their first call."""
    for mat in sc.MATRICES:
        I, k, m, s = sc.inputs(mat), sc.K_SMALL, sc.M_DEFAULT, 2
        ref = sc.new_op(mat)
        try:
            want = {}
            for c in range(s):
                d, Y = I.dec(c, k), I.Y(c, k, m)
                for i, cut in enumerate(sc.cuts(d.steps_taken, m, c)):
                    dc = alg.LanczosDecomposition(d.alphas[:cut], d.betas[:cut - 1], cut, d.b_norm)
                    x = alg.lanczos_pass_two(ref, I.B[:, c], dc, Y[:cut, i])
                    want[(c, i)] = sc.canonical((x,))
        finally:
            ref.close()
        decs = [I.dec(c, k) for c in range(s)]
        Ys = [I.Y(c, k, m) for c in range(s)]
        cs = [sc.cuts(d.steps_taken, m, c) for c, d in enumerate(decs)]
        for trial in range(32):
            op = sc.new_op(mat)
            try:
                x = alg.lanczos_pass_two_multi_cut(op, I.b, decs[0], Ys[0], cs[0])
                for i in range(m):
                    assert sc.same(sc.canonical((x[:, i],)), want[(0, i)]), (mat, trial, i)
            finally:
                op.close()
            op = sc.new_op(mat)
            try:
                X = alg.lanczos_pass_two_batch_multi_cut(op, I.B[:, :s], decs, Ys, cs)
                for c in range(s):
                    for i in range(m):
                        assert sc.same(sc.canonical((X[:, i, c],)), want[(c, i)]), (mat, trial, c, i)
            finally:
                op.close()


def test_tolerance_cases_mix_stops_on_the_device():
    """What tests/test_call_order_cpu.py asserts from the host histories, read back from the
    device at the default sizes: the shifted solves run (column 0, smallest shift) to kmax
    unconverged beside shifts that stop early, and in the batch solve column 1 stops under
    every shift beside column 0."""
    k = sc.K_DEFAULT
    for mat in sc.MATRICES:
        name = "two_pass_shifted_inv_tol"
        (_, steps, conv, _), flags = sc.fresh(mat, D, name, default_params(name))
        assert (int(steps[0]), int(conv[0])) == (k, 0) and conv[-1] == 1 and steps[-1] <= k // 4
        assert flags & sc.ONE_GRAPH
        name = "two_pass_batch_shifted_inv_tol"
        (_, steps, conv, _), flags = sc.fresh(mat, D, name, default_params(name))
        assert steps.shape == conv.shape == (sc.M_DEFAULT, sc.S_DEFAULT)
        assert (int(steps[0, 0]), int(conv[0, 0])) == (k, 0)
        assert conv[:, 1].all() and steps[:, 1].max() <= 6
        assert flags & sc.ONE_GRAPH
