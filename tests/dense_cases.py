"""Shapes, matrices and references of the dense-operator tests (test_dense_cpu.py,
test_gpu_dense.py). Not a test module.

Shapes are chosen for where a kernel that streams rows in column slices, on 8 or 16 lanes,
through an LDS tile, can go wrong — not for the workload."""
import numpy as np
import scipy.sparse as sp

from tpl_amd.utils.rng import std_rng_f64

SHAPES = [1, 2, 7, 8, 9, 64, 65, 129, 512, 513, 520, 1031, 2053]
# set_slices(2 | 4 | 8): n = 7 with S = 8 has empty slices, 512 / 8 is exactly 64 columns per
# slice (8 lanes), 520 / 8 is 65 (16 lanes), 513 mixes 64- and 65-column slices in one row
SLICED = [7, 512, 513, 520, 1031]
SLICES = [2, 4, 8]


def reference_matrix(n):
    """The reference's dense study (src/bin/dense_tradeoff.rs): A = R + R^T, R ~ U[0, 1) from
    StdRng(42), filled row by row here (no test depends on the fill order)."""
    r = std_rng_f64(n * n, 42).reshape(n, n)
    return r + r.T


def normal_matrix(n, seed=3):
    g = np.random.default_rng(seed).standard_normal((n, n))
    return g + g.T


def zeros_matrix(n, seed=4):
    """Mixed signs with exact +0.0 and -0.0 entries, placed symmetrically."""
    rng = np.random.default_rng(seed)
    a = normal_matrix(n, seed)
    u = np.triu(rng.random((n, n)))
    u = u + u.T
    a[u < 0.25] = 0.0
    a[(u >= 0.25) & (u < 0.4)] = -0.0
    return a


def spd_matrix(n):
    r = std_rng_f64(n * n, 42).reshape(n, n)
    a = r @ r.T / n + np.eye(n)
    return (a + a.T) / 2


def full_csr(a):
    """Every entry of a stored, exact zeros included: the CSR whose long-row order (with
    short_rows = []) is the dense operator's."""
    n = a.shape[0]
    return sp.csr_matrix((np.ascontiguousarray(a, dtype=np.float64).reshape(-1),
                          np.tile(np.arange(n, dtype=np.int32), n),
                          np.arange(0, n * n + 1, n, dtype=np.int64)), shape=(n, n))


def elem_geometry(n):
    """tpl_layout.cpp elem_geometry under the default schedule parameters."""
    er = 2048
    while er > 512 and -(-n // er) < 192:
        er //= 2
    g2 = max(1, min(1024, -(-n // er)))
    per = -(-n // g2)
    return g2, max(512, (per + 511) // 512 * 512)


def schedule(n, slices=1):
    """The schedule a dense operator of n rows reports (include/tpl.h tpl_op_create_dense)."""
    g2, e = elem_geometry(n)
    return {"short_rows": np.zeros(0, dtype=np.int32), "long_rows": np.arange(n, dtype=np.int32),
            "G2": g2, "E": e, "slices": slices, "perm": None}


def same_bits_nan(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    nx, ny = np.isnan(x), np.isnan(y)
    return (x.shape == y.shape and np.array_equal(nx, ny)
            and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))
