"""GPU parity AT SIZE for the BASELINE.json configs that the small-case suite
(test_gpu_parity.py) covers only in their instance family:

* configs[3] — 500k-arc KKT, one-pass k = 500 with CGS2 full re-orthogonalisation (V_k
  in HBM): properties at full size computed on the device (||I - V^T V||_F, the Lanczos
  relation), the CGS2 run bit for bit against the oracle's device-order restatement at
  k = 150, and the plain one-pass solver (src/solvers.rs:46-107) bit for bit at k = 500;
* configs[4] — the 5M-arc synthetic KKT (tpl_generate_kkt seed 42, bench.py's instance),
  two-pass k = 500 on one GPU: alphas/betas/x bit for bit against the canonical oracle,
  P0 determinism, P1 basis regeneration (compared on the device), the Lanczos relation,
  one-pass vs two-pass agreement; and both partitions over two ranks (host transport,
  the ranks share this box's GPU) against the single-GPU solve;
* the reference-order bridge at the headline size: the 500k
  instance's betas against the faithful (reference-order) oracle up to the chaotic
  onset (j <= 150), and f = exp at k = 500 within 1e-10 (measured 4.6e-14 on CPU).

Sizes and tolerances are stated per test; the oracle runs on the box's host cores
(OpenMP over independent rows/blocks — bitwise the same for any thread count).
"""
import numpy as np
import pytest

from conftest import harness_b, load_kkt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import oracle  # noqa: E402
from oracle import ftk_ref  # noqa: E402

tpl_amd = pytest.importorskip("tpl_amd")
from tpl_amd import HipCsrOp, ftk, solvers  # noqa: E402
from tpl_amd import algorithms as alg  # noqa: E402

ARCS_5M = 5_000_000


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if tpl_amd.device_count() < 1:
        pytest.skip("no GPU visible")


@pytest.fixture(scope="module")
def kkt500k(kkt_tmp):
    return load_kkt(500000, kkt_tmp)


@pytest.fixture(scope="module")
def op500k(kkt500k):
    op = HipCsrOp(kkt500k.a)
    yield op
    op.close()


@pytest.fixture(scope="module")
def kkt5m(kkt_tmp):
    return load_kkt(ARCS_5M, kkt_tmp)


@pytest.fixture(scope="module")
def op5m(kkt5m):
    op = HipCsrOp(kkt5m.a)
    assert not op.flags() & 64  # auto locality order: off above 2^20 rows
    yield op
    op.close()


def canon(op, a):
    return oracle.Operator(a, op.schedule())


def relation_residual(op, V, alphas, betas):
    """||A V_s - V_s T_s - beta_s v_{s+1} e_s^T||_F over the first s - 1 columns, on the
    device (V: torch (s, n) rows = basis vectors); the last column carries the next
    basis vector, which the run does not return."""
    s = len(alphas)
    tot = 0.0
    for j in range(s - 1):
        r = op.apply(V[j]) - float(alphas[j]) * V[j] - float(betas[j]) * V[j + 1]
        if j > 0:
            r -= float(betas[j - 1]) * V[j - 1]
        tot += float(torch.dot(r, r))
    return tot ** 0.5


def basis_rows(out):
    """torch (steps, n) view of a LanczosOutput's V_k (column-major n x steps)."""
    return out.v_k.T


# --------------------------------------------------------------------- configs[3]
@pytest.mark.timeout(600)
def test_config3_reorth_500k_k500_properties(op500k, kkt500k):
    """configs[3] workload itself: one-pass k = 500 + CGS2 on the 500k instance. V_k (2 GB)
    stays in HBM; orthonormality and the Lanczos relation are computed there."""
    a = kkt500k.a
    bd = torch.from_numpy(harness_b(a)).cuda()
    out = alg.lanczos_standard(op500k, bd, 500, reorthogonalize=True)
    d = out.decomposition
    assert d.steps_taken == 500
    V = basis_rows(out)
    G = V @ V.T
    loss = float(torch.linalg.norm(torch.eye(500, dtype=torch.float64, device="cuda") - G))
    assert loss < 1e-12, loss                     # measured 1.9e-14 in numpy
    rel = relation_residual(op500k, V, d.alphas, d.betas)
    assert rel < 1e-10, rel
    # re-orthogonalisation keeps the projection exact: alpha == 0 on the harness b
    # (disjoint supports) up to rounding of the corrections
    assert np.max(np.abs(d.alphas)) < 1e-12
    # determinism of the whole CGS2 run (P0)
    out2 = alg.lanczos_standard(op500k, bd, 500, reorthogonalize=True)
    assert np.array_equal(out2.decomposition.betas, d.betas)
    assert torch.equal(basis_rows(out2), V)


@pytest.mark.timeout(600)
def test_config3_reorth_500k_bitwise_k150(op500k, kkt500k):
    """CGS2 at 500k against the oracle's device-order restatement, bit for bit:
    alphas, betas, ||b|| and all 150 basis vectors."""
    a = kkt500k.a
    b = harness_b(a)
    k = 150
    out = alg.lanczos_standard(op500k, torch.from_numpy(b).cuda(), k, reorthogonalize=True)
    al, be, st, bn, Vo = canon(op500k, a).pass_one(b, k, reorth=True)
    d = out.decomposition
    assert d.steps_taken == st == k and d.b_norm == bn
    assert np.array_equal(d.alphas, al) and np.array_equal(d.betas, be)
    assert torch.equal(basis_rows(out), torch.from_numpy(np.ascontiguousarray(Vo.T)).cuda())


@pytest.mark.timeout(600)
def test_config3_selective_reorth_500k(op500k, kkt500k):
    """configs[3] with the selective (Kahan–Parlett) variant: k = 500 properties at size
    (orthonormality, Lanczos relation, determinism) and k = 150 bitwise vs the oracle."""
    a = kkt500k.a
    b = harness_b(a)
    bd = torch.from_numpy(b).cuda()
    out = alg.lanczos_standard(op500k, bd, 500, reorthogonalize="selective")
    d = out.decomposition
    assert d.steps_taken == 500
    V = basis_rows(out)
    loss = float(torch.linalg.norm(torch.eye(500, dtype=torch.float64, device="cuda") - V @ V.T))
    assert loss < 1e-12, loss
    assert relation_residual(op500k, V, d.alphas, d.betas) < 1e-10
    out2 = alg.lanczos_standard(op500k, bd, 500, reorthogonalize="selective")
    assert np.array_equal(out2.decomposition.betas, d.betas)
    k = 150
    out = alg.lanczos_standard(op500k, bd, k, reorthogonalize="selective")
    al, be, st, bn, Vo = canon(op500k, a).pass_one(b, k, reorth="selective")
    d = out.decomposition
    assert d.steps_taken == st == k and d.b_norm == bn
    assert np.array_equal(d.alphas, al) and np.array_equal(d.betas, be)
    assert torch.equal(basis_rows(out), torch.from_numpy(np.ascontiguousarray(Vo.T)).cuda())


@pytest.mark.timeout(600)
def test_config3_plain_one_pass_500k_k500_bitwise(op500k, kkt500k):
    """solvers::lanczos (standard pass + device GEMV x = ||b|| V_k y') at 500k, k = 500,
    f = inv: x bit for bit against the canonical oracle; V_k against pass two's
    regenerated basis (P1) on the device."""
    a = kkt500k.a
    b = harness_b(a)
    x = solvers.lanczos(op500k, b, 500, ftk.INV)
    assert np.array_equal(x, canon(op500k, a).lanczos(b, 500, ftk.INV))
    bd = torch.from_numpy(b).cuda()
    out = alg.lanczos_standard(op500k, bd, 500)
    d = out.decomposition
    p2 = alg.lanczos_pass_two_with_basis(op500k, bd, d, np.zeros(d.steps_taken))
    assert torch.equal(p2.v_k, out.v_k)


# ------------------------------------------------------------ reference-order bridge
@pytest.mark.timeout(600)
def test_500k_reference_order_bridge(op500k, kkt500k):
    """SURVEY §8(c) P3 at the headline size: before the chaotic onset (measured at
    step 155 on CPU) the GPU's betas agree with the reference-order oracle to 1e-10
    relative (measured 5.6e-12); every alpha is exactly 0 in both orders; and f = exp at
    k = 500 — insensitive to the onset — gives x within 1e-10 (measured 4.6e-14)."""
    a = kkt500k.a
    b = harness_b(a)
    of = oracle.Operator(a)  # faithful: row-sequential SpMV, sequential dot / norm
    d = alg.lanczos_pass_one(op500k, b, 500)
    alf, bef, sf, bnf, _ = of.pass_one(b, 500)
    assert d.steps_taken == sf == 500
    assert np.all(d.alphas == 0.0) and np.all(alf == 0.0)
    assert abs(d.b_norm - bnf) <= 1e-14 * bnf
    rel = np.abs(d.betas[:150] - bef[:150]) / np.abs(bef[:150])
    assert rel.max() < 1e-10, (rel.max(), int(np.argmax(rel)))
    x = solvers.lanczos_two_pass(op500k, b, 500, ftk.EXP)
    xf = of.lanczos_two_pass(b, 500, ftk_ref.exp)
    assert np.linalg.norm(x - xf) <= 1e-10 * np.linalg.norm(xf)


# --------------------------------------------------------------------- configs[4]
@pytest.mark.timeout(900)
def test_config4_5m_two_pass_k500_bitwise(op5m, kkt5m):
    """configs[4]'s instance (5M arcs, n = 5,003,651, nnz = 2e7) and k on ONE GPU:
    alphas, betas, ||b|| and x of lanczos_two_pass (f = inv) bit for bit against the
    canonical oracle; P0 run-to-run determinism."""
    a = kkt5m.a
    b = harness_b(a)
    o = canon(op5m, a)
    d = alg.lanczos_pass_one(op5m, b, 500)
    al, be, s, bn, _ = o.pass_one(b, 500)
    assert d.steps_taken == s == 500 and d.b_norm == bn
    assert np.array_equal(d.alphas, al) and np.array_equal(d.betas, be)
    x = solvers.lanczos_two_pass(op5m, b, 500, ftk.INV)
    xo, _ = o.pass_two(b, al, be, s, bn, ftk.INV(al, be) * bn)
    assert np.array_equal(x, xo)
    assert np.array_equal(x, solvers.lanczos_two_pass(op5m, b, 500, ftk.INV))


@pytest.mark.timeout(900)
def test_config4_5m_k500_basis_and_relation(op5m, kkt5m):
    """5M arcs, k = 500, on the device: pass two regenerates the standard pass's 20 GB
    basis bit for bit (P1, reference basis_drift_fro = 0.0); the Lanczos relation holds
    (||A V - V T||_F < 1e-9 over 499 columns, ||A|| ~ 52); one-pass and two-pass x agree
    (reference results/accuracy_*.csv relative_solution_deviation ~ 1e-16)."""
    a = kkt5m.a
    bd = torch.from_numpy(harness_b(a)).cuda()
    out = alg.lanczos_standard(op5m, bd, 500)
    d = out.decomposition
    V = basis_rows(out)
    y = ftk.EXP(d.alphas, d.betas) * d.b_norm
    p2 = alg.lanczos_pass_two_with_basis(op5m, bd, d, y)
    assert torch.equal(p2.v_k, out.v_k)
    rel = relation_residual(op5m, V, d.alphas, d.betas)
    assert rel < 1e-9, rel
    del p2, V, out
    torch.cuda.empty_cache()
    x1 = solvers.lanczos(op5m, bd, 500, ftk.EXP)
    x2 = solvers.lanczos_two_pass(op5m, bd, 500, ftk.EXP)
    dev = float(torch.linalg.norm(x1 - x2) / torch.linalg.norm(x2))
    assert dev < 1e-12, dev


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["replicated", "rows"])
def test_config4_5m_partitions_two_ranks(tmp_path, mode, op5m, kkt5m):
    """configs[4]'s partitioned operator at full size over two ranks (host transport; the
    ranks share this box's GPU — RCCL refuses two ranks on one device), k = 30: alphas,
    betas and x BIT FOR BIT against the partitioned order restated on the CPU
    (tests/partition_oracle.py), identical on both ranks, deterministic.

    Against the single-GPU order only the first ~15 betas agree: this instance's Krylov
    process amplifies summation-order differences fast (the canonical and the
    reference-order oracle differ by > 1e-6 from step 19 on, measured on CPU), so the
    single-GPU comparison is limited to the steps before that onset."""
    from partition_oracle import PartitionOracle
    from test_gpu_dist import _assemble, _run_ranks
    a = kkt5m.a
    b = harness_b(a)
    k = 30
    dec = alg.lanczos_pass_one(op5m, b, k)
    rs = _run_ranks(str(tmp_path), 2, "host", mode=mode, arcs=ARCS_5M, k=k)
    assert all(str(r["mode"]) == mode for r in rs)
    assert np.array_equal(rs[0]["al"], rs[1]["al"]) and np.array_equal(rs[0]["be"], rs[1]["be"])
    po = PartitionOracle(a, rs, mode)
    al, be, s, bn = po.pass_one(b, k)
    assert int(rs[0]["steps"]) == s == dec.steps_taken
    assert float(rs[0]["bn"]) == bn
    assert np.array_equal(rs[0]["al"], al) and np.array_equal(rs[0]["be"], be)
    xo = po.pass_two(b, al, be, s, bn, ftk.INV(al, be) * bn)
    xd = _assemble(rs, "x1", a.shape[0])
    assert np.array_equal(xd, xo)
    assert np.array_equal(xd, _assemble(rs, "x2", a.shape[0]))
    np.testing.assert_allclose(rs[0]["be"][:12], dec.betas[:12], rtol=1e-10)


@pytest.mark.timeout(600)
def test_replicated_wide_blocks_two_ranks(tmp_path):
    """The replicated partition's widened element-wise blocks (tpl_partition.cpp
    split_replicated: at most 256 norm partials per rank when that needs <= 4,096 rows per
    block — configs[4] at N = 8): a 1.5M-arc synthetic instance over two ranks holds
    ~750k rows per rank, 367 partials at the default 2,048 rows, so the rule widens the
    blocks to 3,072 rows (245 partials) and pass one's SpMV reduces the gathered partials
    itself (tpl_op_flags bit 7). k = 30: alphas, betas and x BIT FOR BIT against the
    partitioned order restated on the CPU, identical on both ranks."""
    from partition_oracle import PartitionOracle
    from test_gpu_dist import _assemble, _run_ranks
    arcs = 1500000
    a = load_kkt(arcs, str(tmp_path)).a
    b = harness_b(a)
    k = 30
    rs = _run_ranks(str(tmp_path), 2, "host", mode="replicated", arcs=arcs, k=k)
    for r in rs:
        assert int(r["flags"]) & 128, "gathered norm partials not used"
        assert int(r["s_E"]) == 3072 and int(r["s_G2"]) <= 256, (int(r["s_E"]), int(r["s_G2"]))
    assert np.array_equal(rs[0]["al"], rs[1]["al"]) and np.array_equal(rs[0]["be"], rs[1]["be"])
    po = PartitionOracle(a, rs, "replicated")
    al, be, s, bn = po.pass_one(b, k)
    assert int(rs[0]["steps"]) == s
    assert np.array_equal(rs[0]["al"], al) and np.array_equal(rs[0]["be"], be)
    xo = po.pass_two(b, al, be, s, bn, ftk.INV(al, be) * bn)
    xd = _assemble(rs, "x1", a.shape[0])
    assert np.array_equal(xd, xo)
