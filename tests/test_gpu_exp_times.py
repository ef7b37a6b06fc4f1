"""GPU: exp(t_i A) b at m times over one Krylov space (include/tpl.h
tpl_lanczos_two_pass_exp_times, tpl_op_ftk_exp_times_device; tpl_k_ftk_exp_times.hip).

k_ftk_exp_times runs k_ftk_exp's algorithm, one workgroup per time, on the tridiagonal
(RN(t_i alpha_j), RN(t_i beta_j)). Its contract is BITS: column i and its hand-back entry are
what k_ftk_exp gives (HipCsrOp.ftk_device("exp", ...)) on the host-scaled arrays
t_i * alphas, t_i * betas — so the single kernel's tolerance contract
(tests/test_gpu_device_exp.py) carries over and no tolerance is stated here, except test 4's,
which is the one-graph exp test's bound on the same matrix. The solver is checked bitwise
against its parts: pass one's decomposition, the kernel's (Y, on) on it, the host exp_t for the
times handed back, and tpl_lanczos_pass_two_multi / the oracle's pass two on those y.

The shared times: t = 3000 makes the spectrum of t T_k too wide for the expansion on the
matrices here, so it is handed back; the other six stay (checked on the CPU with a numpy
Lanczos and oracle.ftk_ref.exp_chebyshev for k in {2, 3, 7, 60, 200}, the kept y within
1.1e-14 of LAPACK, relative). The tests take the hand-back pattern from the single kernel, not
from this list, and assert only that at least six of the seven columns stay on the device.
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
EXP_TIMES_BYTES = 64 * 8 + 64 * 4  # the times and the hand-back entries


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


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


@pytest.mark.parametrize("n", [1, 2, 3, 7, 200, 256, 257, 511, 1800])
def test_kernel_is_bitwise_the_single_kernel(op_small, n):
    """n: 256 / 257 straddle the one-wave and the LDS recurrence, 1800 is the LDS bound.
    m = 1, 3, 7, 64 with the times cycling through TS: every column against the single kernel
    on the host-scaled arrays (computed once per tridiagonal), so a column depends neither on
    m nor on its neighbours, and a repeated time repeats its column."""
    rng = np.random.default_rng(4000 + n)
    for family, (al, be) in (("lanczos", lanczos_tridiagonal(n, rng)), ("kkt", kkt_like(n, rng))):
        ref = [op_small.ftk_device("exp", t * al, t * be) for t in TS]
        for y, on in ref:
            assert on or np.all(y == 0.0)
        if family == "lanczos":  # a kernel that hands everything back cannot pass
            assert sum(on for _, on in ref) >= 6, [on for _, on in ref]
        for m in (1, 3, 7, 64):
            ts = [TS[i % len(TS)] for i in range(m)]
            Y, on = op_small.ftk_exp_times_device(al, be, ts)
            assert Y.shape == (n, m) and Y.strides == (8, 8 * n) and on.shape == (m,)
            for i in range(m):
                yr, onr = ref[i % len(TS)]
                assert bool(on[i]) == onr, (family, m, i)
                assert same_bits(Y[:, i], yr), (family, m, i)
                if not onr:
                    assert np.all(Y[:, i] == 0.0), (family, m, i)
            for i in range(len(TS), m):  # the same time at two positions
                assert same_bits(Y[:, i], Y[:, i - len(TS)]), (family, m, i)


def test_kernel_entry_point_arguments(op_small):
    al, be = np.full(4, -1.0), np.full(3, 0.5)
    for ts in ([], [1.0] * 65):
        with pytest.raises(TplError) as e:
            op_small.ftk_exp_times_device(al, be, ts)
        assert e.value.status == _lib.TPL_ERR_INVALID_ARGUMENT
    with pytest.raises(TplError) as e:
        op_small.ftk_exp_times_device(np.zeros(1801), np.ones(1800), [1.0])
    assert e.value.status == _lib.TPL_ERR_UNSUPPORTED
    # a non-finite T_k is handed back, as by the single kernel
    Y, on = op_small.ftk_exp_times_device(np.array([0.0, np.nan, 0.0]), np.ones(2), [1.0, 0.5])
    assert not on.any() and np.all(Y == 0.0)


# ---- 2. the solver: bitwise its parts ---------------------------------------------------------
@pytest.fixture(scope="module")
def diag2000():
    a = sp.diags(np.linspace(-10.0, -0.1, 2000)).tocsr()
    return a, HipCsrOp(a), std_rng_vector(2000)


@pytest.fixture(scope="module")
def kkt(kkt5k):
    a = kkt5k.a
    return a, HipCsrOp(a), harness_b(a)


def parts(op, b, k, ts):
    """(decomposition, Y_k = ||b|| exp(t_i T_k) e_1 as the solver forms it, on): pass one, the
    kernel alone on its decomposition, and the host exp_t for the times handed back."""
    d = alg.lanczos_pass_one(op, b, k)
    st = d.steps_taken
    al, be = np.asarray(d.alphas)[:st], np.asarray(d.betas)[:st - 1]
    Y, on = op.ftk_exp_times_device(al, be, ts)
    Y = np.array(Y)
    for i, t in enumerate(ts):
        if not on[i]:
            Y[:, i] = ftk.exp_t(t)(al, be)
    return d, Y * d.b_norm, on


@pytest.mark.parametrize("which", ["diag2000", "kkt"])
@pytest.mark.parametrize("k", [1, 2, 3, 50, 120])
def test_solver_is_bitwise_its_parts(request, which, k):
    a, op, b = request.getfixturevalue(which)
    d, Yk, on = parts(op, b, k, TS)
    assert d.steps_taken == k
    if which == "diag2000":
        assert on.sum() >= 6, on
    X, ond = solvers.lanczos_two_pass_exp_times(op, b, k, TS, return_on_device=True)
    assert not op.flags() & ONE_GRAPH
    assert X.shape == (a.shape[0], len(TS)) and X.strides == (8, 8 * a.shape[0])
    assert np.array_equal(ond, on)
    Xp = alg.lanczos_pass_two_multi(op, b, d, Yk)
    assert same_bits_nan(X, Xp)
    # the oracle's pass two in the operator's reduction order, with the same y
    o = oracle.Operator(a, op.schedule())
    for i in range(len(TS)):
        xo = o.pass_two(b, np.asarray(d.alphas), np.asarray(d.betas), d.steps_taken, d.b_norm,
                        np.ascontiguousarray(Yk[:, i]))[0]
        assert same_bits_nan(X[:, i], xo), i


def test_solver_takes_a_device_b(diag2000):
    import torch
    a, op, b = diag2000
    X = solvers.lanczos_two_pass_exp_times(op, b, 50, TS)
    Xd = solvers.lanczos_two_pass_exp_times(op, torch.from_numpy(b).cuda(), 50, TS)
    assert Xd.is_cuda and tuple(Xd.shape) == (2000, len(TS)) and Xd.stride() == (1, 2000)
    assert same_bits_nan(Xd.cpu().numpy(), X)


# ---- 3. host mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["diag2000", "kkt"])
def test_host_mode_is_the_multi_solve(request, which):
    a, op, b = request.getfixturevalue(which)
    op.set_device_ftk(0)
    try:
        for k in (1, 3, 50):
            X, on = solvers.lanczos_two_pass_exp_times(op, b, k, TS, return_on_device=True)
            assert not on.any()
            Xm = solvers.lanczos_two_pass_multi(op, b, k, [ftk.exp_t(t) for t in TS])
            assert same_bits_nan(X, Xm), k
    finally:
        op.set_device_ftk(2)


# ---- 4. truncation and exactness ------------------------------------------------------------
def test_truncation_and_exactness():
    lam = np.repeat([1.0, 2.0, 3.0], 100)
    op = HipCsrOp(sp.diags(lam).tocsr())
    b = np.ones(300)
    ts = [0.25, 1.0, -1.0]
    assert alg.lanczos_pass_one(op, b, 40).steps_taken == 3
    X, on = solvers.lanczos_two_pass_exp_times(op, b, 40, ts, return_on_device=True)
    assert on.all()
    for i, t in enumerate(ts):
        xt = np.exp(t * lam)
        err = np.linalg.norm(X[:, i] - xt)
        print(f"t = {t}: relative error {err / np.linalg.norm(xt):.3e}")
        assert err <= 1e-12 * np.linalg.norm(xt), (t, err)
    with pytest.raises(LanczosError) as e:
        solvers.lanczos_two_pass_exp_times(op, np.zeros(300), 40, ts)
    with pytest.raises(LanczosError) as e1:
        solvers.lanczos_two_pass(op, np.zeros(300), 40, ftk.EXP)
    assert e.value == e1.value
    op.close()


# ---- 5. long-row cache ----------------------------------------------------------------------
def test_long_row_cache_follows_the_multi_bit(kkt5k):
    a = kkt5k.a
    b = harness_b(a)
    op = HipCsrOp(a)
    assert len(op.schedule()["long_rows"]) > 0
    out = {}
    for mask in (1, 3):
        op.set_long_cache_solvers(mask)
        out[mask] = (np.array(solvers.lanczos_two_pass_exp_times(op, b, 50, TS)), op.flags())
    assert not out[1][1] & CACHED and out[3][1] & CACHED
    assert same_bits_nan(out[1][0], out[3][0])
    op.close()


# ---- 6. arguments and device memory -----------------------------------------------------------
def test_arguments(diag2000):
    a, op, b = diag2000
    for ts in ([], [1.0] * 65, [1.0, np.nan], [np.inf], [0.5, -np.inf, 1.0]):
        with pytest.raises(TplError) as e:
            solvers.lanczos_two_pass_exp_times(op, b, 10, ts)
        assert e.value.status == _lib.TPL_ERR_INVALID_ARGUMENT, ts
    with pytest.raises(LanczosError):
        solvers.lanczos_two_pass_exp_times(op, b[:-1], 10, [1.0])
    # the operator is still usable
    X = solvers.lanczos_two_pass_exp_times(op, b, 10, [1.0])
    assert np.all(np.isfinite(X)) and X.shape == (2000, 1)


def test_device_bytes():
    """The two small buffers are allocated by the first exp-times call of an operator and by
    nothing else: an operator that only runs lanczos_two_pass_multi reports the same figure
    before and after another operator's call, and the calling operator's figure grows by
    exactly the two buffers."""
    a = sp.diags(np.linspace(-10.0, -0.1, 600)).tocsr()
    b = std_rng_vector(600)
    fs = [ftk.exp_t(t) for t in TS[:4]]
    other, caller = HipCsrOp(a), HipCsrOp(a)
    solvers.lanczos_two_pass_multi(other, b, 20, fs)
    solvers.lanczos_two_pass_multi(caller, b, 20, fs)
    before = other.device_bytes()
    assert caller.device_bytes() == before
    solvers.lanczos_two_pass_exp_times(caller, b, 20, TS[:4])
    assert caller.device_bytes() == before + EXP_TIMES_BYTES
    solvers.lanczos_two_pass_exp_times(caller, b, 20, TS[:4])
    caller.ftk_exp_times_device(np.full(5, -1.0), np.full(4, 0.5), TS[:4])
    assert caller.device_bytes() == before + EXP_TIMES_BYTES
    solvers.lanczos_two_pass_multi(other, b, 20, fs)
    assert other.device_bytes() == before
    other.close()
    caller.close()
