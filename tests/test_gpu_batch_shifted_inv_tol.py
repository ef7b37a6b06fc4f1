"""GPU: (A + sigma_i I)^-1 b_c for s right-hand sides in lock-step groups and m shifts, every
(column, shift) stopped at a residual tolerance (include/tpl.h
tpl_lanczos_two_pass_batch_shifted_inv_tol; tpl_k_batch_stol.hip), and the low-level pass two
with a cut per (column, function) behind it (tpl_lanczos_pass_two_batch_multi_cut).

The contract is BITS. Result (c, i) is what tpl_lanczos_two_pass_shifted_inv_tol returns for
b_c — x, steps, converged and the guaranteed prefix of the history — which is also the single
fixed-k solve at k = m*_{c,i} with the shifted-inv closure. The host-composed path (the same
entry point under set_device_ftk(0)) is the oracle of the device path (one graph per group: a
lane per (column, shift) in pass one's elimination workgroup, k_ftk_inv_shifts per column, the
cut flush kernel). No tolerance is assumed to be met by a matrix: every tolerance comes from a
host history, so every m*_{c,i} is known in advance.

Measured figures of the checks that carry a bound: none — every comparison is word for word.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from oracle.rng import std_rng_vector  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, LanczosError, TplError, _lib, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402
from tpl_amd import (LONG_CACHE_TWO_PASS, LONG_CACHE_TWO_PASS_BATCH_MULTI,  # noqa: E402
                     LONG_CACHE_TWO_PASS_MULTI)

ONE_GRAPH, CACHED, FUSED = 32, 256, 512
SIG_A = (0.0, 0.25, 1.0, 4.0, 30.0, 1000.0)
SIG_B = (0.0, 0.5, 1.0, 5.0, 100.0)
batch = solvers.lanczos_two_pass_batch_shifted_inv_tol
single = solvers.lanczos_two_pass_shifted_inv_tol


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same(x, y):
    """Word for word (a NaN equals only itself)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def spd_banded(n=2003):
    """(a): SPD, five diagonals, spectrum within [0.5, 5.5], no long row; n is odd and no
    multiple of a chunk or of an element block."""
    e1, e7 = np.full(n - 1, -1.0), np.full(n - 7, -0.25)
    return sp.diags([e7, e1, np.full(n, 3.0), e1, e7], [-7, -1, 0, 1, 7]).tocsr()


def kkt_long_rows(hubs=30, leaves=113, span=8):
    """(b): the KKT block [[D, E^T], [E, 0]] of 30 hub nodes (hub i -> hub i + 1 .. i + 8: long
    rows) and 113 leaves hanging on them, D = diag(2, 3, 4, 2, ...) on the 353 arc rows:
    n = 496, indefinite, long rows."""
    t = np.repeat(np.arange(hubs), span)
    h = (t + np.tile(np.arange(1, span + 1), hubs)) % hubs
    t = np.concatenate([t, hubs + np.arange(leaves)])
    h = np.concatenate([h, np.arange(leaves) % hubs])
    m, ar = len(t), np.arange(len(t))
    e = sp.coo_matrix((np.concatenate([np.ones(m), -np.ones(m)]),
                       (np.concatenate([t, h]), np.concatenate([ar, ar]))),
                      shape=(hubs + leaves, m)).tocsr()
    a = sp.bmat([[sp.diags(2.0 + np.arange(m) % 3), e.T], [e, None]], format="csr")
    a.eliminate_zeros()
    a.sort_indices()
    assert a.shape == (496, 496)
    return a


def columns(a):
    """Seven right-hand sides that behave differently: 0 a random vector, 1 A applied to it
    twice, 2 a vector from a 5-dimensional invariant subspace (five eigenvectors spread over
    the spectrum), 3 another random vector, 4 A applied to it, 5 the constant vector, 6 a
    third random vector scaled by 1e-3."""
    n = a.shape[0]
    r0 = std_rng_vector(n) - 0.5
    rng = np.random.default_rng(3)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    _, v = np.linalg.eigh(a.toarray())
    idx = [n // 10, 3 * n // 10, n // 2, 7 * n // 10, 9 * n // 10]
    inv5 = v[:, idx] @ np.array([1.0, -0.7, 0.5, 1.3, -0.9])
    return np.asfortranarray(np.stack([r0, a @ (a @ r0), inv5, r1, a @ r1, np.ones(n),
                                       1e-3 * r2], axis=1))


class Case:
    """A matrix with a device-path operator (mode 2) and a host-path one (mode 0), seven
    columns, and per column the decomposition of a kmax-step pass one on the host-path
    operator. Every reference is computed once and kept."""

    def __init__(self, a, kmax, B=None, dev_mode=2):
        self.a, self.kmax = a, kmax
        self.B = columns(a) if B is None else B
        self.dev, self.host = HipCsrOp(a), HipCsrOp(a)
        self.dev.set_device_ftk(dev_mode)
        self.host.set_device_ftk(0)
        self._dec, self._hist, self._single, self._col = {}, {}, {}, {}

    def dec(self, c):
        if c not in self._dec:
            self._dec[c] = alg.lanczos_pass_one(self.host, self.B[:, c], self.kmax)
        return self._dec[c]

    def taken(self, c):
        return self.dec(c).steps_taken

    def hist(self, c, sigma):
        """The host history of (column c, shift sigma): taken - 1 entries."""
        if (c, sigma) not in self._hist:
            al = np.asarray(self.dec(c).alphas, dtype=np.float64)[:self.taken(c)] + float(sigma)
            self._hist[(c, sigma)] = ftk.inv_residuals(al, self.dec(c).betas)
            assert self._hist[(c, sigma)].shape == (self.taken(c) - 1,)
        return self._hist[(c, sigma)]

    def rule(self, c, sigma, tol, kmax=None):
        """(m*, converged) by the stop rule on the host history."""
        taken = min(self.taken(c), kmax or self.kmax)
        hit = np.flatnonzero(self.hist(c, sigma)[:taken - 1] <= tol)
        return (int(hit[0]) + 1, True) if hit.size else (taken, False)

    def big_m(self, c, sigmas, tol, kmax=None):
        return max(self.rule(c, sg, tol, kmax)[0] for sg in sigmas)

    def single(self, c, sigmas, tol, kmax):
        """tpl_lanczos_two_pass_shifted_inv_tol on b_c, host path."""
        key = (c, tuple(sigmas), float(tol), kmax)
        if key not in self._single:
            self._single[key] = single(self.host, self.B[:, c], kmax, sigmas, tol,
                                       return_info=True)
        return self._single[key]

    def column(self, c, sigma, m):
        """The single fixed-k solve of b_c at k = m with the shifted-inv closure, host path."""
        if (c, sigma, m) not in self._col:
            self._col[(c, sigma, m)] = solvers.lanczos_two_pass(self.host, self.B[:, c], m,
                                                                ftk.inv_shift(sigma))
        return self._col[(c, sigma, m)]

    def check(self, cols, sigmas, tol, kmax=None, dev=None, fixed=None, graph=True):
        """The device call on the columns `cols` against the rule, the host path, the single
        call per column and the fixed-k single solves (of the (position, shift index) pairs in
        `fixed`; default: all). -> (X, info) with info["flags"]."""
        kmax, dev = kmax or self.kmax, dev or self.dev
        B = self.B[:, list(cols)]
        X, info = batch(dev, B, kmax, sigmas, tol, return_info=True)
        flags = dev.flags()
        Xh, ih = batch(self.host, B, kmax, sigmas, tol, return_info=True)
        if len(cols) >= 2:
            assert bool(flags & ONE_GRAPH) == graph, (flags, graph)
            assert not self.host.flags() & ONE_GRAPH
        assert not flags & FUSED and not self.host.flags() & FUSED
        assert X.shape == Xh.shape == (self.a.shape[0], len(sigmas), len(cols))
        assert info["steps"].shape == info["converged"].shape == (len(sigmas), len(cols))
        for p, c in enumerate(cols):
            xs, i_s = self.single(c, sigmas, tol, kmax)
            taken = min(self.taken(c), kmax)
            for i, sg in enumerate(sigmas):
                at = (p, c, i, sg, tol, kmax)
                m, conv = self.rule(c, sg, tol, kmax)
                for who, inf in (("dev", info), ("host", ih)):
                    got = (int(inf["steps"][i, p]), bool(inf["converged"][i, p]))
                    assert got == (m, conv), (who, at, got, m, conv)
                assert (int(i_s["steps"][i]), bool(i_s["converged"][i])) == (m, conv), at
                assert same(X[:, i, p], Xh[:, i, p]), at
                assert same(X[:, i, p], xs[:, i]), at
                have = min(m, taken - 1)
                for inf in (info, ih):
                    r = inf["residuals"][p][i]
                    assert len(r) >= have, (at, len(r), have)
                    assert same(r[:have], self.hist(c, sg)[:have]), at
                if fixed is None or (p, i) in fixed:
                    assert same(X[:, i, p], self.column(c, sg, m)), at
        info["flags"] = flags
        return X, info

    def close(self):
        self.dev.close()
        self.host.close()


def distinct_stops(c, cols, sigmas, tol, want_big_m):
    """The fixture's demand on its inputs: the columns reach at least `want_big_m` distinct M_c
    and every column sees at least two distinct m*_{c,i}."""
    ms = {col: [c.rule(col, sg, tol)[0] for sg in sigmas] for col in cols}
    assert len({max(v) for v in ms.values()}) >= want_big_m, ms
    assert all(len(set(v)) >= 2 for v in ms.values()), ms


@pytest.fixture(scope="module")
def case_a():
    c = Case(spd_banded(), 64)
    assert [c.taken(k) for k in range(7)] == [64, 64, 5, 64, 64, 64, 64]
    # the tolerance of the main case: (column 0, shift 0)'s entry at step 23 (about 5e-7)
    c.tol = c.hist(0, 0.0)[22]
    distinct_stops(c, range(4), SIG_A, c.tol, 3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_b():
    c = Case(kkt_long_rows(), 24)
    assert all(c.taken(k) == 24 for k in (0, 1, 3))
    # (column 0, sigma = 5)'s entry at step 6: sigma = 100 meets it within 3 steps, sigma = 0.5
    # never does for the random columns, so one call mixes converged and non-converged results
    c.tol = c.hist(0, 5.0)[5]
    distinct_stops(c, range(4), SIG_B, c.tol, 3)
    assert c.rule(0, 0.5, c.tol) == (24, False) and c.rule(0, 100.0, c.tol)[1]
    yield c
    c.close()


# ---- 1. device is host is single ----------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("s", [2, 4])
def test_device_is_host_is_single(s, name, mode, case_a, case_b):
    c = case_a if name == "a" else case_b
    sig = SIG_A if name == "a" else SIG_B
    dev = c.dev
    if mode == 1:
        dev = HipCsrOp(c.a)
        dev.set_device_ftk(1)
    try:
        tols = [c.tol, c.hist(1, sig[1])[len(c.hist(1, sig[1])) // 2], c.hist(0, sig[-1])[1]]
        for tol in tols:
            x, info = c.check(range(s), sig, tol, dev=dev)
            if name == "a":
                assert not info["flags"] & CACHED
        if name == "b":
            x, info = c.check(range(s), sig, c.tol, dev=dev)
            conv = info["converged"].ravel().tolist()
            assert True in conv and False in conv, conv
    finally:
        if mode == 1:
            dev.close()


# ---- 2. grouping and position --------------------------------------------------------------
@pytest.mark.parametrize("s", [3, 5, 6, 7])
def test_grouping_and_position(s, case_a):
    """2 + 1, 4 + 1, 4 + 2 and 4 + 2 + 1: every column equals its single-b call (check), a
    permutation of the columns permutes the results, equal columns give equal results."""
    c = case_a
    cols = list(range(s))
    x, info = c.check(cols, SIG_A, c.tol, fixed=())
    perm = [(3 * p + 1) % s for p in range(s)] if s % 3 else list(reversed(cols))
    assert sorted(perm) == cols and perm != cols
    xp, ip = c.check(perm, SIG_A, c.tol, fixed=())
    for p, col in enumerate(perm):
        assert same(xp[:, :, p], x[:, :, col]), (p, col)
        assert np.array_equal(ip["steps"][:, p], info["steps"][:, col])
    dup = [cols[p // 2] for p in range(s)]  # 0 0 1 1 2 ...: equal columns inside and across groups
    xd, idup = c.check(dup, SIG_A, c.tol, fixed=())
    for p, col in enumerate(dup):
        assert same(xd[:, :, p], x[:, :, col]), (p, col)


# ---- 3. shift count --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 5, 8, 9, 64])
def test_number_of_shifts(m, case_a):
    """One and several flush launches of four functions, and the whole wavefront."""
    c = case_a
    sig = (1.0,) if m == 1 else tuple(float(v) for v in np.geomspace(0.01, 1000.0, m))
    fixed = None if m <= 9 else [(p, i) for p in range(2) for i in range(p, 64, 9)]
    x, info = c.check((0, 1), sig, c.tol, fixed=fixed)
    if m > 1:
        assert len(set(info["steps"].ravel().tolist())) >= 4


def test_too_many_shifts_or_columns(case_a):
    c = case_a
    with pytest.raises(TplError):
        batch(c.dev, c.B[:, :2], 8, np.arange(1.0, 66.0), 1e-3)
    with pytest.raises(TplError):
        batch(c.dev, np.asfortranarray(np.tile(c.B[:, :1], (1, 65))), 8, (1.0,), 1e-3)


# ---- 4. different stops inside one group -----------------------------------------------------
def test_one_column_stops_early_another_runs_to_kmax(case_a, case_b):
    # (b): every shift of column 1 (A applied twice) has stopped by step M_1 < 24 while column
    # 0 runs to kmax: pass one keeps running and column 1's bits are its single call's
    c = case_b
    m1, m0 = c.big_m(1, SIG_B, c.tol), c.big_m(0, SIG_B, c.tol)
    assert m1 + 3 < m0 == 24 and all(c.rule(1, sg, c.tol)[1] for sg in SIG_B)
    for cols in ((1, 0), (0, 1), (0, 1, 3, 0), (1, 1, 1, 0)):
        c.check(cols, SIG_B, c.tol)
    # (a): kmax one short of what (column 3, shift 0) needs, the constant column done before
    c = case_a
    fast, slow = c.big_m(5, SIG_A, c.tol), c.big_m(3, SIG_A, c.tol)
    assert fast + 1 < slow
    x, info = c.check((5, 3), SIG_A, c.tol, kmax=slow - 1)
    assert all(info["converged"][:, 0]) and not info["converged"][0, 1]


def test_shift_inside_the_spectrum(case_a):
    """sigma = -2 puts 0 inside the spectrum of A + sigma I: below the smallest entry of its
    histories that shift never stops, in any column, while the others do."""
    c = case_a
    cols = (0, 1, 3, 4)
    tol = np.nextafter(min(float(np.min(c.hist(k, -2.0))) for k in cols), 0.0)
    assert all(tol > c.hist(k, 1000.0)[-1] for k in cols)
    x, info = c.check(cols, (-2.0, 1.0, 1000.0), tol)
    assert not info["converged"][0].any() and (info["steps"][0] == 64).all()
    assert info["converged"][2].all()
    c.check((0, 1), (1.0, -2.0), float(np.sort(c.hist(0, -2.0))[31]))


def test_edge_tolerances(case_a):
    c, k = case_a, 32
    cols = (0, 1, 3, 4)
    x, info = c.check(cols, SIG_A, np.inf, k)
    assert (info["steps"] == 1).all() and info["converged"].all()
    x, info = c.check(cols, SIG_A, 0.0, k)
    assert (info["steps"] == k).all() and not info["converged"].any()
    h = c.hist(1, 1.0)
    assert h[10] < h[9]
    x, info = c.check(cols, SIG_A, h[10], k)  # an exact entry: (column 1, shift 1) stops at 11
    assert (int(info["steps"][2, 1]), bool(info["converged"][2, 1])) == (11, True)
    x, info = c.check(cols, SIG_A, np.nextafter(h[10], 0.0), k)  # one ulp below: not at 11
    assert int(info["steps"][2, 1]) > 11
    # (column 3, shift 0)'s entry at kmax - 1: the last the device can see, in the last launch
    last = c.hist(3, 0.0)[k - 2]
    x, info = c.check(cols, SIG_A, last, k)
    assert (int(info["steps"][0, 2]), bool(info["converged"][0, 2])) == (k - 1, True)
    x, info = c.check(cols, SIG_A, np.nextafter(last, 0.0), k)
    assert (int(info["steps"][0, 2]), bool(info["converged"][0, 2])) == (k, False)


# ---- 5. the shortest passes (the fin kernel's cases, per column) -----------------------------
@pytest.mark.parametrize("kmax", [1, 2, 3, 4])
def test_shortest_passes(kmax, case_a):
    c = case_a
    tols = [np.inf, 0.0] + [c.hist(k, sg)[m] for k, sg in ((0, 0.0), (1, 30.0)) for m in (0, 1, 2)]
    for tol in tols:
        c.check((0, 1, 2, 3), SIG_A, tol, kmax, fixed=[(p, i) for p in range(4) for i in (0, 4)])
    c.check((1, 2), SIG_A, tols[3], kmax)


# ---- 6. breakdown and bad columns ------------------------------------------------------------
def test_breakdown_beside_ordinary_columns(case_a):
    """Column 2 breaks down at step 5 of the 64 asked for and keeps steps_taken = 5 for the
    shifts that have not stopped; the others run on. Every entry of two of its histories."""
    c = case_a
    assert c.taken(2) == 5
    for tol in [0.0] + list(c.hist(2, 0.0)) + list(c.hist(2, 30.0)):
        x, info = c.check((0, 2, 1, 3), SIG_A, tol, fixed=[(1, i) for i in range(6)])
        assert (info["steps"][:, 1] <= 5).all()
    c.check((2, 0), SIG_A, c.tol)
    c.check((2, 2), SIG_A, c.hist(2, 0.0)[2])


def test_zero_and_nan_columns(case_a):
    c = case_a
    zero_text = "Invalid input parameter: Input vector `b` must not be a zero vector."
    for op in (c.dev, c.host):
        for s, zeros in ((4, (1, 3)), (2, (1,)), (3, (2,)), (5, (4,))):
            B = c.B[:, :s].copy(order="F")
            B[:, list(zeros)] = 0.0
            with pytest.raises(LanczosError) as e:
                batch(op, B, 16, SIG_A, c.tol)
            assert str(e.value) == zero_text
            with pytest.raises(LanczosError) as e1:
                single(op, B[:, zeros[0]], 16, SIG_A, c.tol)
            assert str(e1.value) == zero_text
    # a NaN in one column leaves the other columns' bits as they are
    for op in (c.dev, c.host):
        x = batch(op, c.B[:, :4], 20, SIG_A, c.tol)
        B = c.B[:, :4].copy(order="F")
        B[7, 2] = np.nan
        xn = batch(op, B, 20, SIG_A, c.tol)
        for p in (0, 1, 3):
            assert same(xn[:, :, p], x[:, :, p]), p
        assert np.isnan(xn[:, :, 2]).any()


# ---- 7. the long-row cache --------------------------------------------------------------------
@pytest.mark.parametrize("s", [4, 3])
def test_long_row_cache_on_and_off(s, case_b):
    """Bit 8 follows the mask's batch-multi bit, the remainder column included."""
    c = case_b
    out = {}
    for on in (True, False):
        dev = HipCsrOp(c.a)
        dev.set_long_cache_solvers(LONG_CACHE_TWO_PASS | LONG_CACHE_TWO_PASS_MULTI if not on
                                   else LONG_CACHE_TWO_PASS_BATCH_MULTI)
        try:
            x, info = c.check(range(s), SIG_B, c.tol, dev=dev)
            assert info["flags"] & ONE_GRAPH
            assert bool(info["flags"] & CACHED) == on, (on, info["flags"])
            out[on] = x
        finally:
            dev.close()
    assert same(out[True], out[False])


# ---- 8. one graph, any tolerance, shifts and B ------------------------------------------------
def test_replay_and_device_bytes(case_a):
    c, k, m = case_a, 40, 6
    dev = HipCsrOp(c.a)
    try:
        # the batch and batch-multi buffers of this (s, m, kmax), as any batch-multi call sizes them
        solvers.lanczos_two_pass_batch_multi(dev, c.B[:, :4], k, [ftk.inv_shift(s) for s in SIG_A])
        bytes0 = dev.device_bytes()
        c.check(range(4), SIG_A, c.tol, k, dev=dev)
        kcap = max(k, 16)
        added = 8 * (1 + m) + 4 * (8 * m * (3 + 5 * kcap) + 8 * m) + 1024
        assert dev.device_bytes() - bytes0 == added
        c.check((3, 1, 0, 2), (7.0, 0.5, 2.0, 0.0, 300.0, 0.125), c.hist(1, 4.0)[6], k, dev=dev,
                fixed=())
        c.check(range(4), SIG_A, c.tol, k, dev=dev, fixed=())
        assert dev.device_bytes() - bytes0 == added
    finally:
        dev.close()


# ---- 9. the cut alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("s", [2, 4, 5])
def test_pass_two_batch_multi_cut(s, name, case_a, case_b):
    c = case_a if name == "a" else case_b
    cols = [0, 2, 1, 3, 4][:s] if name == "a" else list(range(s))
    m = 6
    rng = np.random.default_rng(11)
    decs = [c.dec(k) for k in cols]
    Ys, Ycut, cs = [], [], []
    for p, d in enumerate(decs):
        st = d.steps_taken
        row = [st, max(st - 1, 1), max(st - 2, 1), max(st - 3 - p, 1), 1, min(2, st)]
        Y = rng.standard_normal((st, m))
        Yc = Y.copy()
        for i, n_i in enumerate(row):
            Yc[n_i:, i] = np.nan  # never used
        Ys.append(Y), Ycut.append(Yc), cs.append(row)
    B = c.B[:, cols]
    x = alg.lanczos_pass_two_batch_multi_cut(c.host, B, decs, Ycut, cs)
    assert x.shape == (c.a.shape[0], m, s)
    for p, (k, d) in enumerate(zip(cols, decs)):
        al, be = np.asarray(d.alphas), np.asarray(d.betas)
        for i, n_i in enumerate(cs[p]):
            cut = alg.LanczosDecomposition(al[:n_i], be[:n_i - 1], n_i, d.b_norm)
            ref = alg.lanczos_pass_two(c.host, c.B[:, k], cut, Ys[p][:n_i, i])
            assert same(x[:, i, p], ref), (p, k, i, n_i)
    # uncut, it is the batch-multi pass two
    full = [[d.steps_taken] * m for d in decs]
    xm = alg.lanczos_pass_two_batch_multi_cut(c.host, B, decs, Ys, full)
    assert same(xm, alg.lanczos_pass_two_batch_multi(c.host, B, decs, Ys))
    for p in (0, s - 1):
        for bad in (0, decs[p].steps_taken + 1):
            wrong = [list(r) for r in cs]
            wrong[p][m - 1] = bad
            with pytest.raises(TplError):
                alg.lanczos_pass_two_batch_multi_cut(c.host, B, decs, Ys, wrong)


# ---- 10. routing --------------------------------------------------------------------------------
def test_auto_mode_line(case_a):
    """Mode 2 takes the graph up to kBatchShiftedAutoK and composes longer passes on the host
    (one step past the line is past the device inv's own auto bound, 500, where the two
    coincide); mode 1 takes the graph there too. The bits do not depend on the route."""
    c = case_a
    line = int(_lib.tpl_batch_shifted_inv_tol_auto_k())
    assert 1 <= line <= 500
    sig = SIG_A[1:5]
    call = lambda op, k: batch(op, c.B[:, :2], k, sig, c.tol)
    dev = HipCsrOp(c.a)
    try:
        x_at = call(dev, line)
        assert dev.flags() & ONE_GRAPH
        assert same(x_at, call(c.host, line))
        x2 = call(dev, line + 1)
        assert not dev.flags() & ONE_GRAPH
        dev.set_device_ftk(1)
        x1 = call(dev, line + 1)
        assert dev.flags() & ONE_GRAPH
        assert same(x1, x2) and same(x1, call(c.host, line + 1))
    finally:
        dev.close()


def test_mode_1_at_kmax_1365():
    B = columns(spd_banded())[:, :2]
    c = Case(spd_banded(), 1365, B=np.asfortranarray(B), dev_mode=1)
    try:
        assert c.taken(0) == c.taken(1) == 1365
        sig = (0.0, 1.0, 30.0)
        x, info = c.check((0, 1), sig, c.hist(0, 0.0)[20])
        assert info["converged"].all()
        c.check((0, 1), sig, 0.0, fixed=())  # never met: 1365 rows per (column, shift)
        xg = batch(c.dev, c.B, 1366, sig, 0.5)  # past the bound: composed on the host
        assert not c.dev.flags() & ONE_GRAPH
        assert same(xg, batch(c.host, c.B, 1366, sig, 0.5))
    finally:
        c.close()
