"""GPU: (A + sigma_i I)^-1 b for m shifts over one Krylov space, each stopped at a residual
tolerance (include/tpl.h tpl_lanczos_two_pass_shifted_inv_tol; tpl_k_p1_stol.hip), and the two
low-level entry points behind it (tpl_lanczos_pass_two_multi_cut,
tpl_op_ftk_inv_shifts_device).

The contract is BITS. The definition is the host-composed path — the same entry point under
set_device_ftk(0): one pass one on A, per shift tpl_ftk_inv_residuals and tpl_ftk_inv on
alphas + sigma_i, one pass two cut per column. The device path (one graph: a lane per shift in
pass one's elimination workgroup, one workgroup per shift for y, the cut flush kernel) must
give its (x, steps, converged, history); each column is also the single fixed-k solve's at
k = m*_i with the shifted-inv closure. No tolerance is assumed to be met by a matrix: every
tolerance comes from the host histories themselves, so every m*_i is known.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from oracle.rng import std_rng_vector  # noqa: E402

import fused_cases as fc  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402
from tpl_amd import LONG_CACHE_TWO_PASS, LONG_CACHE_TWO_PASS_MULTI  # noqa: E402
from tpl_amd import TplError  # noqa: E402

ONE_GRAPH, CACHED, FUSED = 32, 256, 512
SIG_A = (0.0, 0.25, 1.0, 4.0, 30.0, 1000.0)
SIG_B = (0.0, 0.5, 1.0, 5.0, 100.0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


def same(x, y):
    """Word for word (a NaN equals only itself)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def same_with_nan(x, y):
    """Word for word, any NaN equal to any NaN."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and same(x[~nx], y[~ny])


def spd_banded(n=2003):
    """(a): SPD, five diagonals, spectrum within [0.5, 5.5], no long row; n is odd and no
    multiple of a chunk or of an element block."""
    e1, e7 = np.full(n - 1, -1.0), np.full(n - 7, -0.25)
    return sp.diags([e7, e1, np.full(n, 3.0), e1, e7], [-7, -1, 0, 1, 7]).tocsr()


def kkt_long_rows():
    """(b): 30 hub nodes (long rows) and 113 leaves, D = diag(2, 3, 4, ...) on the 353 arc rows:
    n = 496, long rows, eligible for the fused pass two (which this solve never takes)."""
    a = fc.kkt_hubs(hubs=30, leaves=113)
    return fc.with_d(SimpleNamespace(a=a, num_arcs=30 * 8 + 113))


def pivoted(alphas, betas):
    """Does tpl_ftk_inv's elimination take its pivoting branch (|d| < |beta_i|) at some row?"""
    d, du = float(alphas[0]), float(betas[0])
    for i in range(len(betas) - 1):
        dl, d1, du1 = float(betas[i]), float(alphas[i + 1]), float(betas[i + 1])
        if abs(d) >= abs(dl):
            d, du = d1 - (dl / d) * du, du1
        else:
            return True
    return False


class Case:
    """A matrix with a device-path operator and a host-path one (mode 0), and the
    decomposition of a kmax-step pass one on the host-path operator."""

    def __init__(self, a, kmax, dev_mode=2, b=None):
        self.a, self.kmax = a, kmax
        self.b = std_rng_vector(a.shape[0]) - 0.5 if b is None else b
        self.dev, self.host = HipCsrOp(a), HipCsrOp(a)
        self.dev.set_device_ftk(dev_mode)
        self.host.set_device_ftk(0)
        self.dec = alg.lanczos_pass_one(self.host, self.b, kmax)
        self.taken = self.dec.steps_taken
        self._hist, self._col = {}, {}

    def shifted(self, sigma):
        return np.asarray(self.dec.alphas, dtype=np.float64)[:self.taken] + float(sigma)

    def hist(self, sigma):
        """The host history of shift sigma: taken - 1 entries."""
        if sigma not in self._hist:
            self._hist[sigma] = ftk.inv_residuals(self.shifted(sigma), self.dec.betas)
            assert self._hist[sigma].shape == (self.taken - 1,)
        return self._hist[sigma]

    def rule(self, sigma, tol, kmax=None):
        """(m*, converged) by the stop rule on the host history."""
        taken = min(self.taken, kmax or self.kmax)
        hit = np.flatnonzero(self.hist(sigma)[:taken - 1] <= tol)
        return (int(hit[0]) + 1, True) if hit.size else (taken, False)

    def column(self, sigma, m):
        """The single fixed-k solve at k = m with the shifted-inv closure, host path."""
        if (sigma, m) not in self._col:
            self._col[(sigma, m)] = solvers.lanczos_two_pass(self.host, self.b, m,
                                                             ftk.inv_shift(sigma))
        return self._col[(sigma, m)]

    def check(self, sigmas, tol, kmax=None, dev=None, singles=None):
        """The device call against the rule, the host path and the single solves (of the
        columns in `singles`; default: all). -> (x, info) with info["flags"]."""
        kmax, dev = kmax or self.kmax, dev or self.dev
        x, info = solvers.lanczos_two_pass_shifted_inv_tol(dev, self.b, kmax, sigmas, tol,
                                                           return_info=True)
        flags = dev.flags()
        xh, ih = solvers.lanczos_two_pass_shifted_inv_tol(self.host, self.b, kmax, sigmas, tol,
                                                          return_info=True)
        assert flags & ONE_GRAPH and not self.host.flags() & ONE_GRAPH
        assert x.shape == xh.shape == (self.a.shape[0], len(sigmas))
        taken = min(self.taken, kmax)
        for i, sg in enumerate(sigmas):
            m, conv = self.rule(sg, tol, kmax)
            got = (int(info["steps"][i]), bool(info["converged"][i]))
            goth = (int(ih["steps"][i]), bool(ih["converged"][i]))
            assert got == (m, conv), (i, sg, tol, got, m, conv)
            assert goth == (m, conv), (i, sg, tol, goth, m, conv)
            assert same(x[:, i], xh[:, i]), (i, sg, tol)
            have = min(m, taken - 1)
            r, rh = info["residuals"][i], ih["residuals"][i]
            assert len(r) >= have and len(rh) >= have, (i, sg, len(r), len(rh), have)
            assert same(r[:have], self.hist(sg)[:have]), (i, sg, tol)
            assert same(rh[:have], self.hist(sg)[:have]), (i, sg, tol)
            if singles is None or i in singles:
                assert same(x[:, i], self.column(sg, m)), (i, sg, tol, m)
        info["flags"] = flags
        return x, info

    def close(self):
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def case_a():
    c = Case(spd_banded(), 64)
    assert c.taken == 64
    # the tolerance of the main case: shift 0's entry at step 23 (about 1e-6); every shift
    # meets it, at no fewer than four distinct steps (a numpy restatement gives six)
    c.tol = c.hist(0.0)[22]
    ms = [c.rule(sg, c.tol) for sg in SIG_A]
    assert all(conv for _, conv in ms), ms
    assert len({m for m, _ in ms}) >= 4, ms
    # m = 1, sigma = 0 against tpl_lanczos_two_pass_inv_tol needs no alpha to be -0
    al = np.asarray(c.dec.alphas)
    assert not np.any((al == 0.0) & np.signbit(al))
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_b():
    c = Case(kkt_long_rows(), 24)
    assert c.taken == 24
    # sigma = 100's entry at step 3: met by sigma = 100, not by sigma = 0.5 in 24 steps, so one
    # call mixes converged and non-converged columns and pass one runs to kmax
    c.tol = c.hist(100.0)[2]
    m100, conv100 = c.rule(100.0, c.tol)
    assert conv100 and m100 <= 3
    assert c.rule(0.5, c.tol) == (24, False)
    yield c
    c.close()


# ---- 1. device against host, column against single solve ----------------------------------
@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("name", ["a", "b"])
def test_device_is_the_host_path(name, mode, case_a, case_b):
    c = case_a if name == "a" else case_b
    sig = SIG_A if name == "a" else SIG_B
    dev = c.dev
    if mode == 1:
        dev = HipCsrOp(c.a)
        dev.set_device_ftk(1)
    try:
        tols = [c.tol, c.hist(sig[1])[len(c.hist(sig[1])) // 2], c.hist(sig[-1])[1]]
        for tol in tols:
            x, info = c.check(sig, tol, dev=dev)
            assert not info["flags"] & FUSED
            if name == "a":
                assert not info["flags"] & CACHED
        if name == "b":
            x, info = c.check(sig, c.tol, dev=dev)
            conv = list(info["converged"])
            assert True in conv and False in conv, conv
    finally:
        if mode == 1:
            dev.close()


# ---- 2. m = 1, sigma = 0 is the single solve that stops at a tolerance --------------------
def test_one_zero_shift_is_inv_tol(case_a):
    c = case_a
    for tol in (c.tol, c.hist(0.0)[40], 0.0):
        x, info = c.check((0.0,), tol, kmax=48)
        x1, i1 = solvers.lanczos_two_pass_inv_tol(c.dev, c.b, 48, tol, return_info=True)
        assert same(x[:, 0], x1)
        assert (int(info["steps"][0]), bool(info["converged"][0])) == (i1["steps"], i1["converged"])


# ---- 3. a column depends on its shift alone -----------------------------------------------
def test_column_independence(case_a):
    c = case_a
    x6, _ = c.check(SIG_A, c.tol)
    perm = (4, 2, 5, 0, 3, 1)
    xp, _ = c.check(tuple(SIG_A[p] for p in perm), c.tol)
    for i, sg in enumerate(SIG_A):
        x1, i1 = c.check((sg,), c.tol)
        assert same(x1[:, 0], x6[:, i]), sg
        assert same(x1[:, 0], xp[:, perm.index(i)]), sg
        xd, idup = c.check((sg, SIG_A[(i + 1) % 6], sg), c.tol, singles=())
        assert same(xd[:, 0], x1[:, 0]) and same(xd[:, 2], x1[:, 0]), sg
        assert idup["steps"][0] == idup["steps"][2] == i1["steps"][0]


# ---- 4. m: one and two flush launches, the whole wavefront, one too many ------------------
@pytest.mark.parametrize("m", [8, 9, 64])
def test_number_of_shifts(m, case_a):
    c = case_a
    sig = tuple(float(s) for s in np.geomspace(0.01, 1000.0, m))
    x, info = c.check(sig, c.tol, singles=None if m <= 9 else range(0, 64, 7))
    assert len(set(int(s) for s in info["steps"])) >= 4


def test_too_many_shifts(case_a):
    c = case_a
    with pytest.raises(TplError):
        solvers.lanczos_two_pass_shifted_inv_tol(c.dev, c.b, 8, np.arange(1.0, 66.0), 1e-3)


# ---- 5. edge tolerances -------------------------------------------------------------------
def test_edge_tolerances(case_a):
    c, k = case_a, 32
    h = c.hist(1.0)
    assert h[10] < h[9]
    x, info = c.check(SIG_A, h[10], k)            # an exact entry: shift 1 stops at 11
    assert (int(info["steps"][2]), bool(info["converged"][2])) == (11, True)
    x, info = c.check(SIG_A, np.nextafter(h[10], 0.0), k)  # one ulp below: not at 11
    assert int(info["steps"][2]) > 11
    x, info = c.check(SIG_A, np.inf, k)
    assert list(info["steps"]) == [1] * 6 and all(info["converged"])
    x, info = c.check(SIG_A, 0.0, k)
    assert list(info["steps"]) == [k] * 6 and not any(info["converged"])
    # shift 0's entry at kmax - 1: the last the device can see, written by the last launch
    x, info = c.check(SIG_A, c.hist(0.0)[k - 2], k)
    assert (int(info["steps"][0]), bool(info["converged"][0])) == (k - 1, True)
    x, info = c.check(SIG_A, np.nextafter(c.hist(0.0)[k - 2], 0.0), k)
    assert (int(info["steps"][0]), bool(info["converged"][0])) == (k, False)


# ---- 6. a shift inside the spectrum -------------------------------------------------------
def test_shift_inside_the_spectrum(case_a):
    """sigma = -2 puts 0 inside the spectrum of A + sigma I ([-1.5, 3.5]): lu_row pivots, and
    below the smallest entry of its history the shift never stops while the others do."""
    c = case_a
    assert pivoted(c.shifted(-2.0), np.asarray(c.dec.betas))
    h = c.hist(-2.0)
    tol = np.nextafter(float(np.min(h)), 0.0)
    assert tol > c.hist(1000.0)[-1]
    x, info = c.check((-2.0, 1.0, 1000.0), tol)
    assert not info["converged"][0] and info["steps"][0] == 64 and info["converged"][2]
    x, info = c.check((1.0, -2.0), float(np.sort(h)[len(h) // 2]))
    assert info["converged"][1]


# ---- 7. the shortest passes (the fin kernel's cases) --------------------------------------
@pytest.mark.parametrize("kmax", [1, 2, 3, 4])
def test_shortest_passes(kmax, case_a):
    c = case_a
    tols = [np.inf, 0.0] + [c.hist(sg)[m] for sg in (0.0, 30.0) for m in (0, 1, 2)]
    for tol in tols:
        c.check(SIG_A, tol, kmax)


# ---- 8. the long-row cache ----------------------------------------------------------------
def test_long_row_cache_on_and_off(case_b):
    c = case_b
    out = {}
    for on in (True, False):
        dev = HipCsrOp(c.a)
        dev.set_long_cache_solvers(LONG_CACHE_TWO_PASS | (LONG_CACHE_TWO_PASS_MULTI if on else 0))
        try:
            x, info = c.check(SIG_B, c.tol, dev=dev)
            assert info["flags"] & ONE_GRAPH and not info["flags"] & FUSED
            assert bool(info["flags"] & CACHED) == on, (on, info["flags"])
            out[on] = x
        finally:
            dev.close()
    assert same(out[True], out[False])


# ---- 9. one graph, any tolerance and any shifts -------------------------------------------
def test_replay_with_other_tolerance_and_shifts(case_a):
    c, k = case_a, 40
    dev = HipCsrOp(c.a)
    try:
        solvers.lanczos_two_pass_multi(dev, c.b, k, [ftk.inv_shift(s) for s in SIG_A])
        bytes0 = dev.device_bytes()
        c.check(SIG_A, c.tol, k, dev=dev)
        kcap = max(k, 16)
        assert dev.device_bytes() - bytes0 == 8 * (1 + 6 * (4 + 5 * kcap)) + 8 * 6 + 256
        c.check((7.0, 0.5, 2.0, 0.0, 300.0, 0.125), c.hist(4.0)[6], k, dev=dev)
        c.check(SIG_A, c.tol, k, dev=dev)
        assert dev.device_bytes() - bytes0 == 8 * (1 + 6 * (4 + 5 * kcap)) + 8 * 6 + 256
    finally:
        dev.close()


# ---- 10. breakdown ------------------------------------------------------------------------
def test_breakdown():
    """5 distinct eigenvalues: pass one stops after 5 steps of the 20 asked for. Every entry
    of two histories as the tolerance: some shifts stop, the others take the 5 steps."""
    a = sp.diags(np.repeat(np.arange(1.0, 6.0), 8)).tocsr()
    c = Case(a, 20, b=np.random.default_rng(5).standard_normal(a.shape[0]))
    try:
        assert c.taken == 5
        sig = (0.0, 1.0, 10.0)
        for tol in [0.0] + list(c.hist(0.0)) + list(c.hist(10.0)):
            c.check(sig, tol)
    finally:
        c.close()


# ---- 11. pass two with a per-column cut ---------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_pass_two_multi_cut(name, case_a, case_b):
    c = case_a if name == "a" else case_b
    steps = c.taken
    cs = [steps, steps - 1, steps - 2, steps - 3, 1, 2]
    Y = np.random.default_rng(11).standard_normal((steps, 6))
    Ycut = Y.copy()
    for i, s in enumerate(cs):
        Ycut[s:, i] = np.nan  # never used
    x = alg.lanczos_pass_two_multi_cut(c.host, c.b, c.dec, Ycut, cs)
    assert x.shape == (c.a.shape[0], 6)
    al, be = np.asarray(c.dec.alphas), np.asarray(c.dec.betas)
    for i, s in enumerate(cs):
        dec = alg.LanczosDecomposition(al[:s], be[:s - 1], s, c.dec.b_norm)
        assert same(x[:, i], alg.lanczos_pass_two(c.host, c.b, dec, Y[:s, i])), (i, s)
    # uncut, it is the multi-function pass two
    xm = alg.lanczos_pass_two_multi_cut(c.host, c.b, c.dec, Y, [steps] * 6)
    assert same(xm, alg.lanczos_pass_two_multi(c.host, c.b, c.dec, Y))
    for bad in ([steps + 1] + cs[1:], [0] + cs[1:]):
        with pytest.raises(TplError):
            alg.lanczos_pass_two_multi_cut(c.host, c.b, c.dec, Y, bad)


# ---- 12. k_ftk_inv_shifts alone -----------------------------------------------------------
def lanczos_tridiagonal(n, rng):
    """As tests/test_inv_tol_cpu.py builds it: n alphas, n betas."""
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
    return np.array(al), np.array(be)


def kkt_like(n, rng):
    """Zero diagonal, positive off-diagonal (a pivot at every row), n betas."""
    return np.zeros(n), rng.uniform(0.5, 20.0, n)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 500, 1365])
def test_ftk_inv_shifts_device(n, case_a):
    """sigma = 0 on the zero-diagonal family is singular for odd n (non-finite y) and leaves
    div_rn's range: the IEEE fallback. sigma = 5 puts 0 inside the lanczos family's spectrum."""
    rng = np.random.default_rng(7300 + n)
    sig = (0.0, 0.75, -0.5, 5.0, 11.0, 1e3, -1e-3, 2.0 ** -30, 64.0)
    for family, (al, be) in (("lanczos", lanczos_tridiagonal(n, rng)), ("kkt", kkt_like(n, rng))):
        be = be[:n - 1]
        Y = case_a.dev.ftk_inv_shifts_device(al, be, sig)
        assert Y.shape == (n, len(sig))
        for i, sg in enumerate(sig):
            assert same_with_nan(Y[:, i], ftk.INV(al + sg, be)), (family, n, sg)


# ---- 13. where auto mode draws its line, and mode 1 at k_ftk_inv's LDS bound ---------------
def test_auto_mode_routes_long_passes_to_the_host(case_a):
    """Mode 2 takes the one-graph path up to kmax = 64 and composes longer passes on the host
    (DESIGN 6.1); mode 1 takes the graph there too. The bits do not depend on the route."""
    c = case_a
    call = lambda op, k: solvers.lanczos_two_pass_shifted_inv_tol(op, c.b, k, SIG_A, c.tol)
    dev = HipCsrOp(c.a)
    try:
        call(dev, 64)
        assert dev.flags() & ONE_GRAPH
        x2 = call(dev, 65)
        assert not dev.flags() & ONE_GRAPH
        dev.set_device_ftk(1)
        x1 = call(dev, 65)
        assert dev.flags() & ONE_GRAPH
        assert same(x1, x2) and same(x1, call(c.host, 65))
    finally:
        dev.close()


def test_mode_1_at_kmax_1365():
    c = Case(spd_banded(), 1365, dev_mode=1)
    try:
        assert c.taken == 1365
        sig = (0.0, 1.0, 30.0)
        x, info = c.check(sig, c.hist(0.0)[20])
        assert all(info["converged"])
        c.check(sig, 0.0, singles=())  # never met: 1365 rows per shift in k_ftk_inv_shifts
        solvers.lanczos_two_pass_shifted_inv_tol(c.dev, c.b, 1366, sig, 0.5)  # past the bound
        assert not c.dev.flags() & ONE_GRAPH
    finally:
        c.close()
