"""GPU: exp(t_i A) b_c for m times and s right-hand sides in one run (include/tpl.h
tpl_lanczos_two_pass_batch_exp_times, tpl_op_ftk_exp_times_batch_device;
tpl_k_ftk_exp_times_batch.hip).

k_ftk_exp_times_batch runs k_ftk_exp's algorithm, one workgroup per (time, column) of a
lock-step group, on the tridiagonal (RN(t_i alpha_j), RN(t_i beta_j)) of that column. Its
contract is BITS: column (c, i) and its hand-back entry are what k_ftk_exp gives
(HipCsrOp.ftk_device("exp", ...)) on the host-scaled arrays t_i * alphas_c, t_i * betas_c, so the
single kernel's tolerance contract (tests/test_gpu_device_exp.py) carries over and no tolerance
is stated here, except test 4's, which is test_truncation_and_exactness's bound
(tests/test_gpu_exp_times.py) at that test's times on spaces of the same kind. The solver is
checked bitwise against the single-b call of every column, against the oracle's pass two with
the y that was used, and in host mode against the batch-multi solve with exp_t closures.

The shared times: t = 3000 makes the spectrum of t T_k too wide for the expansion on the
larger matrices here, so it is handed back there; the other six stay. The tests take the
hand-back pattern from the single kernel, not from this list, and assert only that at least
six of the seven columns of a Lanczos-family tridiagonal stay on the device.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import harness_b

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, LanczosError, TplError, _lib, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

TS = [0.0, 0.25, 0.5, 1.0, 2.0, -1.0, 3000.0]
ONE_GRAPH, CACHED = 32, 256
# the hand-back table (4 columns x 64 times, int32) and the times (64 doubles), which no call
# before the first batch exp-times call of the operator in test_device_bytes allocated
BATCH_EXP_TIMES_BYTES = 4 * 64 * 4 + 64 * 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def same_bits_nan(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    nx, ny = np.isnan(x), np.isnan(y)
    return (x.shape == y.shape and np.array_equal(nx, ny)
            and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))


# ---- 1. the kernel alone: bitwise the single kernel -----------------------------------------
@pytest.fixture(scope="module")
def op_small():
    return HipCsrOp(sp.diags(np.arange(1.0, 65.0)).tocsr())


def lanczos_tridiagonal(n, rng):
    """The Lanczos T_n of a diagonal spectrum in [-10, -0.1] and a random start (the shape the
    solver sees; as tests/test_gpu_device_exp.py builds it)."""
    lam = np.linspace(-10.0, -0.1, 4 * n + 4)
    v = rng.random(lam.shape[0])
    v /= np.linalg.norm(v)
    vp = np.zeros_like(v)
    al, be, bprev = [], [], 0.0
    for _ in range(n):
        w = lam * v - bprev * vp
        a_ = v @ w
        w = w - a_ * v
        al.append(a_)
        bprev = np.linalg.norm(w)
        be.append(bprev)
        vp, v = v, w / bprev
    return np.array(al), np.array(be[:n - 1])


def kkt_like(n, rng):
    """Zero diagonal, positive off-diagonal: the shape of T_k on the KKT runs."""
    return np.zeros(n), rng.uniform(0.5, 20.0, n - 1)


def group_of(n_max, nb, seed):
    """nb different tridiagonals (the two families alternating) with different step counts:
    column c is the leading steps_c rows of a tridiagonal of n_max rows. -> (family, al, be)."""
    rng = np.random.default_rng(seed)
    steps = [n_max, 1, max(1, n_max // 2), max(1, n_max - 1)][:nb]
    cols = []
    for c, st in enumerate(steps):
        family = "lanczos" if c % 2 == 0 else "kkt"
        al, be = (lanczos_tridiagonal if family == "lanczos" else kkt_like)(n_max, rng)
        cols.append((family, al[:st].copy(), be[:st - 1].copy()))
    return cols


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("n_max", [1, 2, 3, 257, 1800])
def test_kernel_is_bitwise_the_single_kernel(op_small, n_max, nb):
    """n_max: 257 is the first size past the one-wave recurrence, 1800 the LDS bound. Every
    column of the group has its own tridiagonal and its own step count, and ld = n_max + 3, so
    a column stride confused with a step count cannot pass. m = 1, 3, 64 with the times cycling
    through TS: every (c, i) against the single kernel on the host-scaled arrays (computed once
    per column), so a result depends neither on m nor on its neighbours, and a repeated time
    repeats its column."""
    cols = group_of(n_max, nb, 5000 + 10 * n_max + nb)
    ld = n_max + 3
    refs = []
    for family, al, be in cols:
        ref = [op_small.ftk_device("exp", t * al, t * be) for t in TS]
        for y, on in ref:
            assert on or np.all(y == 0.0)
        if family == "lanczos":  # a kernel that hands everything back cannot pass
            assert sum(on for _, on in ref) >= 6, [on for _, on in ref]
        refs.append(ref)
    for m in (1, 3, 64):
        ts = [TS[i % len(TS)] for i in range(m)]
        Y, on = op_small.ftk_exp_times_batch_device([c[1] for c in cols], [c[2] for c in cols],
                                                    ts, ld=ld)
        assert Y.shape == (ld, m, nb) and Y.strides == (8, 8 * ld, 8 * ld * m)
        assert on.shape == (m, nb)
        for c, (family, al, be) in enumerate(cols):
            st = al.shape[0]
            for i in range(m):
                yr, onr = refs[c][i % len(TS)]
                assert bool(on[i, c]) == onr, (family, m, c, i)
                assert same_bits(Y[:st, i, c], yr), (family, m, c, i)
                assert np.all(Y[st:, i, c] == 0.0) and not np.any(np.signbit(Y[st:, i, c]))
                if not onr:
                    assert np.all(Y[:, i, c] == 0.0), (family, m, c, i)
            for i in range(len(TS), m):  # the same time at two positions
                assert same_bits(Y[:, i, c], Y[:, i - len(TS), c]), (family, m, c, i)


def test_a_nan_column_is_handed_back_and_its_neighbours_keep_their_bits(op_small):
    cols = group_of(40, 4, 77)
    als, bes = [c[1] for c in cols], [c[2] for c in cols]
    ts = TS[1:5]
    Y0, on0 = op_small.ftk_exp_times_batch_device(als, bes, ts, ld=43)
    assert on0[:, 2].all()
    bad = als[2].copy()
    bad[7] = np.nan
    Y1, on1 = op_small.ftk_exp_times_batch_device([als[0], als[1], bad, als[3]], bes, ts, ld=43)
    assert not on1[:, 2].any() and np.all(Y1[:, :, 2] == 0.0)
    for c in (0, 1, 3):
        assert np.array_equal(on1[:, c], on0[:, c]) and same_bits(Y1[:, :, c], Y0[:, :, c]), c


# ---- 2. the hook's arguments ------------------------------------------------------------------
def test_kernel_entry_point_arguments(op_small):
    al, be = np.full(4, -1.0), np.full(3, 0.5)
    BAD, UNS = _lib.TPL_ERR_INVALID_ARGUMENT, _lib.TPL_ERR_UNSUPPORTED
    for nb in (1, 3, 5):
        with pytest.raises(TplError) as e:
            op_small.ftk_exp_times_batch_device([al] * nb, [be] * nb, [1.0])
        assert e.value.status == BAD, nb
    for ts in ([], [1.0] * 65):
        with pytest.raises(TplError) as e:
            op_small.ftk_exp_times_batch_device([al, al], [be, be], ts)
        assert e.value.status == BAD, len(ts)
    with pytest.raises(TplError) as e:  # a column without a step
        op_small.ftk_exp_times_batch_device([al, al[:0]], [be, be[:0]], [1.0])
    assert e.value.status == BAD
    with pytest.raises(TplError) as e:  # steps[1] = 4 above ld = 3
        op_small.ftk_exp_times_batch_device([al[:2], al], [be[:1], be], [1.0], ld=3)
    assert e.value.status == BAD
    with pytest.raises(TplError) as e:
        op_small.ftk_exp_times_batch_device([al, np.zeros(1801)], [be, np.ones(1800)], [1.0])
    assert e.value.status == UNS
    # the operator is still usable
    Y, on = op_small.ftk_exp_times_batch_device([al, al], [be, be], [1.0, 0.5])
    assert on.all() and same_bits(Y[:, :, 0], Y[:, :, 1])


# ---- 3. the solver: bitwise its parts ---------------------------------------------------------
S_MAX = 5


@pytest.fixture(scope="module")
def diag2000():
    a = sp.diags(np.linspace(-10.0, -0.1, 2000)).tocsr()
    B = np.stack([std_rng_vector(2000, 42 + c) for c in range(S_MAX)], axis=1)
    return a, HipCsrOp(a), B


@pytest.fixture(scope="module")
def kkt(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    B = np.stack([harness_b(a)] + [std_rng_vector(n, 42 + c) for c in range(1, S_MAX)], axis=1)
    return a, HipCsrOp(a), B


def single_refs(op, B, k, ts):
    """Per column the single-b call: [(X_c of shape (n, m), on_c)]."""
    return [tuple(host(v) for v in solvers.lanczos_two_pass_exp_times(
        op, B[:, c].copy(), k, ts, return_on_device=True)) for c in range(B.shape[1])]


def check_against_singles(X, on, refs, cols, what):
    """X: (n, m, s) with strides (8, 8 n, 8 n m); on: (m, s); refs[c] the single-b call of
    column c; cols: the reference column of every column of X."""
    X = host(X)
    n, m = refs[0][0].shape
    assert X.shape == (n, m, len(cols)) and on.shape == (m, len(cols)), what
    assert X.strides == (8, 8 * n, 8 * n * m), (what, X.strides)
    for j, c in enumerate(cols):
        assert np.array_equal(on[:, j], refs[c][1]), (what, j)
        assert same_bits_nan(X[:, :, j], refs[c][0]), (what, j)


def y_used(op, d, ts, on):
    """Y_c = ||b_c|| exp(t_i T_k) e_1 as the solver forms it: the single kernel's column where
    the device kept the time, the host exp_t where it handed it back."""
    al, be = np.asarray(d.alphas)[:d.steps_taken], np.asarray(d.betas)[:d.steps_taken - 1]
    Y = np.zeros((d.steps_taken, len(ts)))
    for i, t in enumerate(ts):
        if on[i]:
            y, kept = op.ftk_device("exp", t * al, t * be)
            assert kept
        else:
            y = ftk.exp_t(t)(al, be)
        Y[:, i] = y
    return Y * d.b_norm


@pytest.mark.parametrize("which", ["diag2000", "kkt"])
@pytest.mark.parametrize("k", [1, 2, 3, 50, 120])
def test_solver_is_bitwise_its_parts(request, which, k):
    """s = 2 .. 5: both group widths; s = 3 and s = 5 end in a remainder column. The single-b
    references are computed once per k for the five columns."""
    a, op, B = request.getfixturevalue(which)
    refs = single_refs(op, B, k, TS)
    if which == "diag2000":
        assert all(on.sum() >= 6 for _, on in refs), [on for _, on in refs]
    for s in (2, 3, 4, 5):
        X, on = solvers.lanczos_two_pass_batch_exp_times(op, B[:, :s], k, TS,
                                                         return_on_device=True)
        assert not op.flags() & ONE_GRAPH
        check_against_singles(X, on, refs, range(s), (which, k, s))
    if which != "kkt":
        return
    # the oracle's pass two in the operator's reduction order on lanczos_pass_one_batch's
    # decompositions, with the y that was used
    o = oracle.Operator(a, op.schedule())
    decs = alg.lanczos_pass_one_batch(op, B, k)
    X = host(X)
    for c, d in enumerate(decs):
        Yk = y_used(op, d, TS, on[:, c])
        for i in range(len(TS)):
            xo = o.pass_two(np.ascontiguousarray(B[:, c]), np.asarray(d.alphas),
                            np.asarray(d.betas), d.steps_taken, d.b_norm,
                            np.ascontiguousarray(Yk[:, i]))[0]
            assert same_bits_nan(X[:, i, c], xo), (c, i)


# ---- 4. columns that stop at different steps ------------------------------------------------
def stopping_columns():
    """A diagonal operator with 16 distinct eigenvalues (40 rows each) and columns that excite
    3, 5, 12, all 16 and 7 of them (constant within an eigenvalue's rows, so a column's Krylov
    space has exactly that dimension). With k = 12 the first two columns and the last break
    down at their own step, the third ends at k with an exact space, the fourth is truncated."""
    lam = np.repeat(np.linspace(-0.8, -0.05, 16), 40)
    groups = [[2, 8, 14], [0, 4, 7, 11, 15], [0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15],
              list(range(16)), [1, 3, 6, 8, 10, 12, 14]]
    rng = np.random.default_rng(21)
    B = np.zeros((lam.shape[0], len(groups)))
    for c, gs in enumerate(groups):
        for g in gs:
            B[40 * g:40 * g + 40, c] = rng.uniform(0.5, 1.5)
    return lam, B, [3, 5, 12, 12, 7], [True, True, True, False, True]


@pytest.mark.parametrize("reverse", [False, True])
def test_columns_stop_at_different_steps(reverse):
    lam, B, steps, exact = stopping_columns()
    if reverse:
        B, steps, exact = np.ascontiguousarray(B[:, ::-1]), steps[::-1], exact[::-1]
    op = HipCsrOp(sp.diags(lam).tocsr())
    k = 12
    assert [alg.lanczos_pass_one(op, B[:, c].copy(), k).steps_taken for c in range(5)] == steps
    assert [d.steps_taken for d in alg.lanczos_pass_one_batch(op, B, k)] == steps
    refs = single_refs(op, B, k, TS)
    X, on = solvers.lanczos_two_pass_batch_exp_times(op, B, k, TS, return_on_device=True)
    check_against_singles(X, on, refs, range(5), ("TS", reverse))
    # exactness where the Krylov space is exact: the bound and the times of
    # test_truncation_and_exactness (tests/test_gpu_exp_times.py)
    ts = [0.25, 1.0, -1.0]
    X, on = solvers.lanczos_two_pass_batch_exp_times(op, B, k, ts, return_on_device=True)
    check_against_singles(X, on, single_refs(op, B, k, ts), range(5), ("exact", reverse))
    assert on.all()
    for c in range(5):
        for i, t in enumerate(ts):
            xt = np.exp(t * lam) * B[:, c]
            err = np.linalg.norm(X[:, i, c] - xt)
            print(f"column {c} (steps {steps[c]}), t = {t}: relative error "
                  f"{err / np.linalg.norm(xt):.3e}")
            if exact[c]:
                assert err <= 1e-12 * np.linalg.norm(xt), (c, t, err)
    op.close()


# ---- 5. independence ------------------------------------------------------------------------
def test_independence(kkt):
    a, op, B = kkt
    n = a.shape[0]
    k = 50
    refs = single_refs(op, B, k, TS)
    two = lambda Bx: solvers.lanczos_two_pass_batch_exp_times(op, Bx, k, TS,
                                                              return_on_device=True)
    for cols in ([2, 0, 3, 1], [4, 2, 0], [1, 3], [0, 1, 2, 3, 4]):
        X, on = two(B[:, cols])
        check_against_singles(X, on, refs, cols, cols)
    # one column replaced by NaNs: where the call returns, the others keep their bits
    for s in (3, 4):
        Bn = B[:, :s].copy()
        Bn[:, 1] = np.nan
        try:
            xs = solvers.lanczos_two_pass_exp_times(op, Bn[:, 1].copy(), k, TS)
            single_error = None
        except LanczosError as e:
            single_error = e
        if single_error is not None:
            with pytest.raises(LanczosError) as e:
                two(Bn)
            assert e.value == single_error
            continue
        X, on = two(Bn)
        X = host(X)
        assert same_bits_nan(X[:, :, 1], host(xs))
        for c in (0, 2, 3)[:s - 1]:
            assert np.array_equal(on[:, c], refs[c][1]) and same_bits_nan(X[:, :, c], refs[c][0]), c
    # a zero column: the batch solve's error
    Bz = B[:, :4].copy()
    Bz[:, 2] = 0.0
    with pytest.raises(LanczosError) as e:
        two(Bz)
    with pytest.raises(LanczosError) as e1:
        solvers.lanczos_two_pass_batch(op, Bz, k, ftk.SQ)
    assert e.value == e1.value
    assert str(e.value) == "Invalid input parameter: Input vector `b` must not be a zero vector."
    X, on = two(B[:, :4])  # the operator is still usable
    check_against_singles(X, on, refs, range(4), "after the error")


# ---- 6. host mode and the bound ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["diag2000", "kkt"])
def test_host_mode_is_the_batch_multi_solve(request, which):
    a, op, B = request.getfixturevalue(which)
    fs = [ftk.exp_t(t) for t in TS]
    op.set_device_ftk(0)
    try:
        for k, s in ((1, 2), (3, 5), (50, 3), (50, 4)):
            X, on = solvers.lanczos_two_pass_batch_exp_times(op, B[:, :s], k, TS,
                                                             return_on_device=True)
            assert not on.any() and on.shape == (len(TS), s)
            Xm = solvers.lanczos_two_pass_batch_multi(op, B[:, :s], k, fs)
            assert same_bits_nan(host(X), host(Xm)), (k, s)
    finally:
        op.set_device_ftk(2)


def test_past_the_device_bound_every_time_runs_on_the_host(diag2000):
    """k = 1801 is one past the LDS bound of the kernel: s = 2, m = 2 keeps the host QL sweeps
    few."""
    a, op, B = diag2000
    ts = TS[1:3]
    X, on = solvers.lanczos_two_pass_batch_exp_times(op, B[:, :2], 1801, ts,
                                                     return_on_device=True)
    assert not on.any()
    Xm = solvers.lanczos_two_pass_batch_multi(op, B[:, :2], 1801, [ftk.exp_t(t) for t in ts])
    assert same_bits_nan(host(X), host(Xm))


# ---- 7. long-row cache ------------------------------------------------------------------------
def test_long_row_cache_follows_the_batch_multi_bit(kkt5k):
    a = kkt5k.a
    n = a.shape[0]
    B = np.stack([harness_b(a), std_rng_vector(n, 43), std_rng_vector(n, 44)], axis=1)
    op = HipCsrOp(a)
    assert len(op.schedule()["long_rows"]) > 0
    out = {}
    for mask in (1, 9):
        op.set_long_cache_solvers(mask)
        X, on = solvers.lanczos_two_pass_batch_exp_times(op, B, 50, TS, return_on_device=True)
        out[mask] = (np.array(X), on, op.flags())
    assert not out[1][2] & CACHED and out[9][2] & CACHED
    assert same_bits_nan(out[1][0], out[9][0]) and np.array_equal(out[1][1], out[9][1])
    op.close()


# ---- 8. a device B ----------------------------------------------------------------------------
def test_solver_takes_a_device_B(diag2000):
    import torch
    a, op, B = diag2000
    for s in (4, 3):
        X, on = solvers.lanczos_two_pass_batch_exp_times(op, B[:, :s], 50, TS,
                                                         return_on_device=True)
        Xd, ond = solvers.lanczos_two_pass_batch_exp_times(
            op, torch.from_numpy(B[:, :s]).cuda(), 50, TS, return_on_device=True)
        m = len(TS)
        assert Xd.is_cuda and tuple(Xd.shape) == (2000, m, s)
        assert Xd.stride() == (1, 2000, 2000 * m)
        assert np.array_equal(on, ond) and same_bits_nan(Xd.cpu().numpy(), X)


# ---- 9. device memory -------------------------------------------------------------------------
def test_device_bytes():
    """The hand-back table is allocated by the first batch exp-times call of an operator and by
    nothing else: an operator that only runs lanczos_two_pass_batch_multi reports the same
    figure before and after another operator's call, and the calling operator's figure grows
    by exactly the table and the times (which no call before allocated); a second call and a
    call of the kernel's hook add nothing."""
    a = sp.diags(np.linspace(-10.0, -0.1, 600)).tocsr()
    B = np.stack([std_rng_vector(600, 42 + c) for c in range(4)], axis=1)
    fs = [ftk.exp_t(t) for t in TS[:4]]
    other, caller = HipCsrOp(a), HipCsrOp(a)
    solvers.lanczos_two_pass_batch_multi(other, B, 20, fs)
    solvers.lanczos_two_pass_batch_multi(caller, B, 20, fs)
    before = other.device_bytes()
    assert caller.device_bytes() == before
    solvers.lanczos_two_pass_batch_exp_times(caller, B, 20, TS[:4])
    assert caller.device_bytes() == before + BATCH_EXP_TIMES_BYTES
    solvers.lanczos_two_pass_batch_exp_times(caller, B, 20, TS[:4])
    solvers.lanczos_two_pass_batch_exp_times(caller, B[:, :2], 20, TS[:3])
    caller.ftk_exp_times_batch_device([np.full(5, -1.0)] * 2, [np.full(4, 0.5)] * 2, TS[:4])
    assert caller.device_bytes() == before + BATCH_EXP_TIMES_BYTES
    solvers.lanczos_two_pass_batch_multi(other, B, 20, fs)
    assert other.device_bytes() == before
    other.close()
    caller.close()


# ---- 10. arguments ----------------------------------------------------------------------------
def test_arguments(diag2000):
    a, op, B = diag2000
    BAD = _lib.TPL_ERR_INVALID_ARGUMENT
    two = solvers.lanczos_two_pass_batch_exp_times
    with pytest.raises(ValueError):
        two(op, B[:, :2], 10, [])
    with pytest.raises(ValueError):
        two(op, B[:, :0], 10, [1.0])
    for ts in ([1.0] * 65, [1.0, np.nan], [np.inf], [0.5, -np.inf, 1.0]):
        with pytest.raises(TplError) as e:
            two(op, B[:, :3], 10, ts)
        assert e.value.status == BAD, ts
    with pytest.raises(TplError) as e:
        two(op, np.ones((2000, 65)), 10, [1.0])
    assert e.value.status == BAD
    with pytest.raises(LanczosError):
        two(op, B[:-1, :2], 10, [1.0])
    # the library's own checks of what Python refuses first: s = 0, no time, no times array
    Bc = np.ascontiguousarray(B[:, :2].T)
    x = np.zeros((2 * 2, 2000))
    t = np.array([0.5, 1.0])
    pd = t.ctypes.data_as(_lib.PD)
    H = _lib.TPL_MEM_HOST
    raw = _lib.tpl_lanczos_two_pass_batch_exp_times
    assert raw(op.handle, Bc.ctypes.data, 2000, 0, 10, pd, 2, x.ctypes.data, H, None) == BAD
    assert raw(op.handle, Bc.ctypes.data, 2000, 2, 10, pd, 0, x.ctypes.data, H, None) == BAD
    assert raw(op.handle, Bc.ctypes.data, 2000, 2, 10, None, 2, x.ctypes.data, H, None) == BAD
    assert raw(op.handle, Bc.ctypes.data, 1999, 2, 10, pd, 2, x.ctypes.data, H, None) != 0
    # on_device may be NULL
    assert raw(op.handle, Bc.ctypes.data, 2000, 2, 10, pd, 2, x.ctypes.data, H, None) == 0
    # the operator is still usable
    X = two(op, B[:, :3], 10, [1.0])
    assert np.all(np.isfinite(X)) and X.shape == (2000, 1, 3)
