"""GPU: the two-pass inverse solve that stops at a residual tolerance on the device
(include/tpl.h tpl_lanczos_two_pass_inv_tol; tpl_k_p1_tol.hip).

The contract is BITS. The rule is tpl_ftk_inv_residuals on pass one's decomposition (checked on
the CPU: tests/test_inv_tol_cpu.py); the device path — one graph whose elimination workgroup
forms the residuals and raises the stop — must give the (steps, converged, x, history) of the
host path, which is the same entry point under set_device_ftk(0) and is composed of
tpl_lanczos_pass_one, the rule, tpl_ftk_inv and tpl_lanczos_pass_two. x is also the fixed-k
solve's at k = steps. No tolerance is assumed to be met by a matrix: every tolerance is taken
from the host history itself, so the step it is first met at is known.
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

ONE_GRAPH, CACHED, FUSED = 32, 256, 512


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


def kkt_long_rows():
    """(b): 30 hub nodes (long rows) and 113 leaves, D = diag(2, 3, 4, ...) on the 353 arc rows:
    n = 496, eligible for the fused pass two."""
    a = fc.kkt_hubs(hubs=30, leaves=113)
    return fc.with_d(SimpleNamespace(a=a, num_arcs=30 * 8 + 113))


class Case:
    """A matrix with a device-path operator and a host-path one (mode 0), and the host
    history of a kmax-step pass one."""

    def __init__(self, a, kmax, dev_mode=2):
        self.a, self.kmax = a, kmax
        self.b = std_rng_vector(a.shape[0]) - 0.5
        self.dev, self.host = HipCsrOp(a), HipCsrOp(a)
        self.dev.set_device_ftk(dev_mode)
        self.host.set_device_ftk(0)
        dec = alg.lanczos_pass_one(self.host, self.b, kmax)
        self.taken = dec.steps_taken
        self.hist = ftk.inv_residuals(dec.alphas, dec.betas)
        assert self.hist.shape == (self.taken - 1,)

    def rule(self, tol, kmax=None):
        """(m*, converged) by the stop rule on the host history."""
        taken = min(self.taken, kmax or self.kmax)
        hit = np.flatnonzero(self.hist[:taken - 1] <= tol)
        return (int(hit[0]) + 1, True) if hit.size else (taken, False)

    def check(self, tol, kmax=None, dev=None):
        """The device call against the rule, the host path and the fixed-k solve. -> info."""
        kmax, dev = kmax or self.kmax, dev or self.dev
        x, info = solvers.lanczos_two_pass_inv_tol(dev, self.b, kmax, tol, return_info=True)
        flags = dev.flags()
        xh, ih = solvers.lanczos_two_pass_inv_tol(self.host, self.b, kmax, tol, return_info=True)
        assert flags & ONE_GRAPH and not self.host.flags() & ONE_GRAPH
        m, conv = self.rule(tol, kmax)
        assert (info["steps"], info["converged"]) == (m, conv), (tol, info, m, conv)
        assert (ih["steps"], ih["converged"]) == (m, conv), (tol, ih)
        assert same(x, xh), tol
        have = min(m, min(self.taken, kmax) - 1)
        assert len(info["residuals"]) >= have and len(ih["residuals"]) >= have
        assert same(info["residuals"][:have], self.hist[:have]), tol
        assert same(ih["residuals"][:have], self.hist[:have]), tol
        assert same(x, solvers.lanczos_two_pass(self.host, self.b, m, ftk.INV)), (tol, m)
        info["flags"] = flags
        return info

    def close(self):
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def case_a():
    c = Case(spd_banded(), 64)
    # what the edge tests below rely on: the history of (a) falls strictly while above 1e-12
    h = c.hist[c.hist > 1e-12]
    assert h.size >= 30 and np.all(np.diff(h) < 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_b():
    c = Case(kkt_long_rows(), 24)
    assert np.all(np.isfinite(c.hist))
    yield c
    c.close()


def tolerances(hist):
    """The value at a quarter, a half and the last index (hits for sure), and one strictly
    between two neighbouring entries."""
    n = len(hist)
    lo, hi = sorted((hist[n // 3], hist[n // 3 + 1]))
    return [hist[n // 4], hist[n // 2], hist[n - 1], lo + (hi - lo) / 2]


# ---- 1. device against host ---------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", ["a", "b"])
def test_device_is_the_host_path(name, which, case_a, case_b):
    """(a): no long row, the step launches of pass two. (b): long rows, cached and fused (bits
    8 and 9). The last index is a hit at m <= kmax - 1, the last the device can see."""
    c = case_a if name == "a" else case_b
    tol = tolerances(c.hist)[which]
    info = c.check(tol)
    if which < 3:
        assert info["converged"]
    if name == "b":
        assert info["flags"] & CACHED and info["flags"] & FUSED, info["flags"]
    else:
        assert not info["flags"] & (CACHED | FUSED)


# ---- 2. edge tolerances -------------------------------------------------------------------
def test_edge_tolerances(case_a):
    c, k = case_a, 16
    info = c.check(0.0, k)
    assert (info["steps"], info["converged"]) == (k, False)
    x = solvers.lanczos_two_pass_inv_tol(c.dev, c.b, k, 0.0)
    assert same(x, solvers.lanczos_two_pass(c.dev, c.b, k, ftk.INV))
    info = c.check(np.inf, k)
    assert (info["steps"], info["converged"]) == (1, True)
    info = c.check(c.hist[k - 2], k)  # first met at kmax - 1: written by the last launch
    assert (info["steps"], info["converged"]) == (k - 1, True)
    info = c.check(np.nextafter(c.hist[k - 2], 0.0), k)  # just missed: no hit
    assert (info["steps"], info["converged"]) == (k, False)


# ---- 3. hits at the first histories the elimination writes --------------------------------
@pytest.mark.parametrize("kmax", [1, 2, 3, 4, 64])
def test_first_hits(kmax, case_a):
    """m = 1 and 2 are both written by launch 3 (kmax = 3: the last), m = 3 by launch 4;
    kmax = 2 never runs the elimination workgroup and kmax = 1 has no history at all. A hit
    at m needs m <= kmax - 1; past that the same tolerance gives steps = kmax, not converged."""
    c = case_a
    for m in (1, 2, 3):
        info = c.check(c.hist[m - 1], kmax)
        want = (m, True) if m <= kmax - 1 else (kmax, False)
        assert (info["steps"], info["converged"]) == want, (kmax, m, info)


# ---- 4. one graph, any tolerance ----------------------------------------------------------
def test_cached_graph_carries_no_tolerance(case_a):
    c, k = case_a, 40
    t1, t2 = c.hist[30], c.hist[9]
    fresh = {}
    for t in (t1, t2):
        op = HipCsrOp(c.a)
        fresh[t] = solvers.lanczos_two_pass_inv_tol(op, c.b, k, t, return_info=True)
        op.close()
    op = HipCsrOp(c.a)
    for t in (t1, t2, t1, 0.0, t2):
        x, info = solvers.lanczos_two_pass_inv_tol(op, c.b, k, t, return_info=True)
        if t == 0.0:
            assert (info["steps"], info["converged"]) == (k, False)
            continue
        xf, inf = fresh[t]
        assert same(x, xf) and info["steps"] == inf["steps"] == c.rule(t, k)[0]
        assert info["converged"] and inf["converged"]
    op.close()


# ---- 5. breakdown -------------------------------------------------------------------------
def test_breakdown():
    """5 distinct eigenvalues: pass one stops after 5 steps of the 20 asked for. tol = 0: the
    fixed-k solve. Every entry of the history as the tolerance — the last one is met at
    m = 4, seen by launch 5 and acted on by launch 6, whose SpMV raised the breakdown."""
    a = sp.diags(np.repeat(np.arange(1.0, 6.0), 8)).tocsr()
    c = Case(a, 20)
    try:
        c.b = np.random.default_rng(5).standard_normal(a.shape[0])
        dec = alg.lanczos_pass_one(c.host, c.b, 20)
        c.taken, c.hist = dec.steps_taken, ftk.inv_residuals(dec.alphas, dec.betas)
        assert c.taken == 5 and c.hist.shape == (4,)
        info = c.check(0.0)
        assert (info["steps"], info["converged"]) == (5, False)
        x = solvers.lanczos_two_pass_inv_tol(c.dev, c.b, 20, 0.0)
        assert same(x, solvers.lanczos_two_pass(c.dev, c.b, 20, ftk.INV))
        for t in c.hist:
            assert c.check(t)["converged"]
    finally:
        c.close()


# ---- 6. the existing solve is unchanged ---------------------------------------------------
def test_fixed_k_solve_unchanged_and_bytes_counted(case_b):
    c, k = case_b, 24
    op = HipCsrOp(c.a)
    x0 = solvers.lanczos_two_pass(op, c.b, k, ftk.INV)
    f0, bytes0 = op.flags(), op.device_bytes()
    solvers.lanczos_two_pass_inv_tol(op, c.b, k, c.hist[k // 2])
    assert op.device_bytes() - bytes0 == 8 * (1 + max(k, 16))  # tol | res[kcap]
    x1 = solvers.lanczos_two_pass(op, c.b, k, ftk.INV)
    assert same(x0, x1) and op.flags() == f0
    op.close()


# ---- 7. mode 1 at k_ftk_inv's LDS bound ---------------------------------------------------
def test_mode_1_at_kmax_1365():
    c = Case(spd_banded(), 1365, dev_mode=1)
    try:
        assert c.taken == 1365
        info = c.check(c.hist[len(c.hist) // 2])
        assert info["converged"]
        solvers.lanczos_two_pass_inv_tol(c.dev, c.b, 1366, 0.5)  # past the bound: the host path
        assert not c.dev.flags() & ONE_GRAPH
    finally:
        c.close()


# ---- 8. the C++ host API ------------------------------------------------------------------
def test_cpp_api(tmp_path):
    """tests/native/inv_tol_test.cpp --gpu: tpl.hpp's mirror stops at 1e-6, returns the
    fixed-k solve's bits and a residual the true one confirms."""
    import subprocess

    from test_inv_tol_cpu import build_native
    p = subprocess.run([build_native(tmp_path), "--gpu"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "OK (0 failures)" in p.stdout, p.stdout + p.stderr
