"""The catalogue of the call-order tests (tests/test_gpu_call_order.py, tests/test_call_order_cpu.py):
every solver entry point of include/tpl.h as a named call, every setter as a setting, the size
ladders, two tiny matrices, and `fresh` — the result of one call on a new operator, which is what
the rest of the GPU suite pins to the device-order oracle.

An operator keeps lazily sized buffers and a cache of captured graphs between calls
(two-pass-lanczos_amd/csrc/tpl_op.h). The rules that keep them right are prose there; the tests
built on this module state them as one property: whatever ran before, a call returns the bits and
the path flags a fresh operator returns.

Nothing here touches a GPU at import. `inputs`, `fresh` and `anchor` do when they are called.

Sizes. ensure_state and ensure_batch (tpl_operator.cpp) allocate max(k, 16) steps on their first
call and grow to max(k, kcap, 16) after it: the first capacity is 16, so K_SMALL = 12 fits the
first allocation whatever ran before and K_BIG = 24 outgrows it.
"""
import random
import re

import numpy as np

K_SMALL, K_BIG = 12, 24          # below / above the first capacity, max(k, 16) = 16
K_LADDER = (1, 2, 7, K_SMALL, K_BIG)
M_LADDER = (1, 2, 5, 64)
S_LADDER = (2, 3, 4, 7)
K_DEFAULT, M_DEFAULT, S_DEFAULT = K_SMALL, 5, 3   # s = 3: a group of two and a remainder column

ONE_GRAPH, CACHED, FUSED = 32, 256, 512           # tpl_op_flags bits 5, 8 and 9
FLAG_MASK = ONE_GRAPH | CACHED | FUSED

MATRICES = ("kkt", "band")
N_COLS = 7
DENSE_EIG_MAX = 4096             # Inputs.eigenvectors5: rows up to which it decomposes densely

# tpl.h entry points the catalogue leaves out on purpose (tests/test_call_order_cpu.py)
NOT_COVERED = {
    "tpl_op_tune_order": "timing-dependent: it keeps the group count that measured fastest",
}


# ------------------------------------------------------------------------------ matrices
def matrix(name):
    """kkt: the fused-eligible KKT block of fused_cases (30 hubs, 113 leaves, D != 0): n = 496,
    indefinite, 30 long rows. band: a diagonally dominant band of seven non-integer fp64
    entries per row with 15 long hub rows, n = 1501: short rows wider than 4 entries, so the
    long-row cache runs without the fused pass two."""
    if name == "kkt":
        from fused_cases import kkt_hubs
        a = kkt_hubs(30, leaves=113, d=True)
        assert a.shape == (496, 496)
        return a
    if name == "band":
        from conftest import banded_hub
        return banded_hub(n=1501, w=3, hub_every=97, hub_half=60, hub_step=7, seed=5)
    raise KeyError(name)


class Inputs:
    """The right-hand sides and host-made arguments of one matrix, made once and never changed.
    Column 0 is oracle.rng's vector (the single-b calls use it), 1 lies in a 5-dimensional
    invariant subspace (its residual falls to rounding level at step 5 under every shift; it
    does not break down within K_BIG steps), 2 is A applied twice to column 0, 3 and 4 another
    random vector and A applied to it, 5 the constant vector, 6 a third random vector scaled by
    1e-3. The decompositions the stand-alone passes take come from the oracle run in a default
    operator's reduction order (a host plan, no GPU).

    Two tolerances, both from column 0's host histories at K_BIG steps. tol_met, the smallest of
    its first five unshifted residuals, is met within five steps of any pass of seven or more
    (two_pass_inv_tol_met). tol_mix, half the smallest residual column 0 reaches in K_BIG steps
    under the smallest shift of `sigmas`, is never met by (column 0, that shift) at any k of
    the ladder, while the largest shift meets it within a few steps and column 1 meets it
    under every shift by step 6: the shifted solves run one shift to kmax beside shifts that
    stop early, and the batch ones a column that runs to kmax beside one that has stopped
    (tests/test_call_order_cpu.py asserts this mix on the host)."""

    def __init__(self, name, a=None, schedule=None, B=None):
        """a: the matrix (default: matrix(name)). schedule: the reduction order the host
        decompositions are made in (default: a default operator's, from a host plan).
        B: right_hand_sides(a) made earlier (tests/geometry_cases.py: one matrix under
        several schedules)."""
        self.name = name
        self.a = a = matrix(name) if a is None else a
        n = self.n = a.shape[0]
        self.B = self.right_hand_sides(a) if B is None else B
        assert self.B.shape == (n, N_COLS)
        self.b = np.ascontiguousarray(self.B[:, 0])
        self._dec, self._orc, self._schedule = {}, None, schedule
        self._dev = {}
        # 0.0 (two_pass_inv_tol_never) is never met: a residual is <= 0 only when it is 0
        from tpl_amd import ftk
        d = self.dec(0, K_BIG)
        self.tol_met = float(np.min(ftk.inv_residuals(d.alphas, d.betas)[:5]))
        self.tol_mix = 0.5 * float(np.min(self.history(0, K_BIG, SIGMA_MIN)))
        assert self.tol_met > 0.0 and self.tol_mix > 0.0

    @staticmethod
    def eigenvectors5(a):
        """Five eigenvectors of a spread over its spectrum. Up to DENSE_EIG_MAX rows those at
        the positions n/10, 3n/10, n/2, 7n/10 and 9n/10 of the dense decomposition; above it
        (a dense one takes half a minute at 10,000 rows) the eigenvector nearest each of those
        quantiles of the diagonal, by shift-and-invert Lanczos from the constant vector."""
        n = a.shape[0]
        if n <= DENSE_EIG_MAX:
            _, v = np.linalg.eigh(a.toarray())
            return v[:, [n // 10, 3 * n // 10, n // 2, 7 * n // 10, 9 * n // 10]]
        from scipy.sparse.linalg import eigsh
        diag = np.sort(a.diagonal())
        found = [eigsh(a.tocsc(), k=1, sigma=float(diag[i]), v0=np.ones(n))
                 for i in (n // 10, 3 * n // 10, n // 2, 7 * n // 10, 9 * n // 10)]
        lam = np.array([w[0] for w, _ in found])
        assert np.all(np.diff(lam) > 1e-8 * np.abs(lam).max()), lam   # five different ones
        return np.stack([v[:, 0] for _, v in found], axis=1)

    @staticmethod
    def right_hand_sides(a):
        from oracle.rng import std_rng_vector
        n = a.shape[0]
        r0 = std_rng_vector(n) - 0.5
        rng = np.random.default_rng(3)
        r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
        inv5 = Inputs.eigenvectors5(a) @ np.array([1.0, -0.7, 0.5, 1.3, -0.9])
        return np.asfortranarray(np.stack([r0, inv5, a @ (a @ r0), r1, a @ r1, np.ones(n),
                                           1e-3 * r2], axis=1))

    def oracle(self):
        if self._orc is None:
            import oracle
            if self._schedule is None:
                import tpl_amd
                plan = tpl_amd.operator.HostPlan(self.a)
                self._schedule = plan.schedule()
                plan.close()
            self._orc = oracle.Operator(self.a, self._schedule)
        return self._orc

    def oracle_schedule(self):
        self.oracle()
        return self._schedule

    def dec(self, c, k):
        """Column c's k-step decomposition (host, in the oracle's reduction order: a default
        operator's unless a schedule was handed in)."""
        if (c, k) not in self._dec:
            from tpl_amd import algorithms as alg
            al, be, st, bn, _ = self.oracle().pass_one(self.B[:, c], k)
            self._dec[(c, k)] = alg.LanczosDecomposition(al, be, st, bn)
        return self._dec[(c, k)]

    def history(self, c, k, sigma):
        """The host residual history of (column c, shift sigma) over a k-step pass."""
        from tpl_amd import ftk
        d = self.dec(c, k)
        return ftk.inv_residuals(np.asarray(d.alphas) + float(sigma), d.betas)

    def stop(self, c, k, sigma, tol):
        """(m*, converged) of (column c, shift sigma) by the stop rule on the host history."""
        d = self.dec(c, k)
        hit = np.flatnonzero(self.history(c, k, sigma)[:d.steps_taken - 1] <= tol)
        return (int(hit[0]) + 1, True) if hit.size else (int(d.steps_taken), False)

    def Y(self, c, k, m):
        """(steps, m): column i = ||b|| (T + sigma_i I)^-1 e_1 on dec(c, k)."""
        from tpl_amd import ftk
        d = self.dec(c, k)
        return np.stack([np.asarray(ftk.inv_shift(sg)(d.alphas, d.betas)) * d.b_norm
                         for sg in sigmas(m)], axis=1)

    def cols(self, s, device=False):
        return self.on(self.B[:, :s], device)

    def vec(self, device=False):
        return self.on(self.b, device)

    def on(self, x, device):
        """x itself, or its copy as a torch CUDA tensor (test_device_inputs)."""
        if not device:
            return x
        import torch
        return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = Inputs(name)
    return _INPUTS[name]


SIGMA_MIN, SIGMA_MAX = 0.01, 1000.0


def sigmas(m):
    """m shifts; from m = 2 on the first is SIGMA_MIN and the last SIGMA_MAX."""
    return (1.0,) if m == 1 else tuple(float(v) for v in np.geomspace(SIGMA_MIN, SIGMA_MAX, m))


def times(m):
    return (0.25,) if m == 1 else tuple(float(v) for v in np.linspace(0.01, 0.5, m))


def cuts(steps, m, c=0):
    """A cut per function: 1 <= cut <= steps, the first one uncut."""
    return [steps if i == 0 else 1 + (3 * i + c) % steps for i in range(m)]


def sq_closure(alphas, betas):
    """T_k^2 e_1 in Python: the host callback path (tpl_ftk_fn through ctypes)."""
    y = np.zeros(len(alphas))
    y[0] = alphas[0] * alphas[0] + (betas[0] * betas[0] if len(alphas) > 1 else 0.0)
    if len(alphas) > 1:
        y[1] = betas[0] * (alphas[0] + alphas[1])
    if len(alphas) > 2:
        y[2] = betas[0] * betas[1]
    return y


# ------------------------------------------------------------------------------ calls
class Call:
    """name; the C entry points it exercises; run(op, I, p, dev) -> result tuple, p a dict of
    k, m, s; which of those sizes it takes; its family; the flag bits its own result defines.

    defines: tpl.h says of bit 5 "the last tpl_lanczos_two_pass / tpl_lanczos evaluated f(T_k)
    on the device", of bit 8 "the last pass two the operator ran read long rows' sums from the
    long-row cache" and of bit 9 "that pass two ran fused". A call that is neither kind of
    solve leaves bit 5 as the solve before it set it, and a call that runs no pass two leaves
    bits 8 and 9: for such a call those bits are history by the header's own words and are
    masked, for that call only. Every two-pass solver documents all three bits after it."""

    def __init__(self, name, entry, run, takes, family, defines, device_b=True):
        self.name, self.entry, self.run = name, tuple(entry), run
        self.takes, self.family, self.defines = tuple(takes), family, defines
        self.device_b = device_b

    def ladder(self, size):
        return {"k": K_LADDER, "m": M_LADDER, "s": S_LADDER}[size] if size in self.takes else ()

    def params(self, k=None, m=None, s=None):
        """The hashable parameter tuple: the sizes the call takes, defaults filled in."""
        want = {"k": K_DEFAULT if k is None else k, "m": M_DEFAULT if m is None else m,
                "s": S_DEFAULT if s is None else s}
        return tuple((z, want[z]) for z in self.takes)


def _np(x):
    if type(x).__module__.startswith("torch"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x)


def canonical(result):
    """Every array of a result as its uint64 words (a NaN equals only itself), ints as ints."""
    out = []
    for r in result:
        if isinstance(r, (bool, int, np.integer)):
            out.append(int(r))
        else:
            a = _np(r)
            if a.dtype == np.float64:
                a = a.view(np.uint64)
            elif a.dtype == np.bool_:
                a = a.astype(np.uint64)
            else:
                a = a.astype(np.int64).view(np.uint64)
            out.append(a.copy())
    return tuple(out)


def same(x, y):
    if len(x) != len(y):
        return False
    for p, q in zip(x, y):
        if isinstance(p, int) != isinstance(q, int):
            return False
        if isinstance(p, int):
            if p != q:
                return False
        elif p.shape != q.shape or not np.array_equal(p, q):
            return False
    return True


def same_schedule(x, y):
    """Two schedule dicts (HipCsrOp.schedule(), conftest.canon_schedule) name one layout."""
    def eq(p, q):
        return (p is None) == (q is None) and (p is None or np.array_equal(p, q))
    return (int(x["G2"]), int(x["E"]), int(x["slices"])) == (int(y["G2"]), int(y["E"]),
                                                             int(y["slices"])) and \
        eq(x["short_rows"], y["short_rows"]) and eq(x["long_rows"], y["long_rows"]) and \
        eq(x["perm"], y["perm"])


def _dec_tuple(d):
    return (d.alphas, d.betas, int(d.steps_taken), np.array([d.b_norm]))


def _tol_tuple(x, info, s=None):
    """x, steps, converged and the guaranteed prefix of each history: the first m* entries
    when the tolerance was met, else the steps - 1 entries the pass formed."""
    steps = np.atleast_1d(np.asarray(info["steps"])).astype(np.int64)
    conv = np.atleast_1d(np.asarray(info["converged"])).astype(bool)
    res = info["residuals"]
    if isinstance(res, np.ndarray):
        res = [res]
    elif s is not None:          # residuals[c][i] against steps[i, c]
        m = len(res[0])
        res = [res[c][i] for i in range(m) for c in range(s)]
    pre = []
    for r, st, cv in zip(res, steps.ravel(), conv.ravel()):
        have = int(st) if cv else int(st) - 1
        assert len(r) >= have, (len(r), have)
        pre.append(np.asarray(r[:have], dtype=np.float64))
    return (x, steps, conv, np.concatenate(pre + [np.zeros(0)]))


def _build_calls():
    import tpl_amd  # noqa: F401  (host library only; no device is opened here)
    from tpl_amd import algorithms as alg
    from tpl_amd import ftk, solvers

    calls = []

    def add(name, entry, takes, family, defines, device_b=True):
        def deco(fn):
            calls.append(Call(name, entry, fn, takes, family, defines, device_b))
            return fn
        return deco

    NONE, P2, SOLVE1, ALL = 0, CACHED | FUSED, ONE_GRAPH, FLAG_MASK

    @add("apply", ["tpl_op_apply"], "", "low", NONE)
    def _(op, I, p, dev):
        return (op.apply(I.vec(dev)),)

    @add("pass_one", ["tpl_lanczos_pass_one"], "k", "low", NONE)
    def _(op, I, p, dev):
        return _dec_tuple(alg.lanczos_pass_one(op, I.vec(dev), p["k"]))

    @add("pass_two", ["tpl_lanczos_pass_two"], "k", "low", P2)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        return (alg.lanczos_pass_two(op, I.vec(dev), d, I.Y(0, p["k"], 1)[:, 0]),)

    @add("pass_two_with_basis", ["tpl_lanczos_pass_two"], "k", "low", P2)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        out = alg.lanczos_pass_two_with_basis(op, I.vec(dev), d, I.Y(0, p["k"], 1)[:, 0])
        return (out.x_k, out.v_k)

    @add("pass_two_multi", ["tpl_lanczos_pass_two_multi"], "km", "low", P2)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        return (alg.lanczos_pass_two_multi(op, I.vec(dev), d, I.Y(0, p["k"], p["m"])),)

    @add("pass_two_multi_cut", ["tpl_lanczos_pass_two_multi_cut"], "km", "low", P2)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        return (alg.lanczos_pass_two_multi_cut(op, I.vec(dev), d, I.Y(0, p["k"], p["m"]),
                                               cuts(d.steps_taken, p["m"])),)

    @add("pass_one_batch", ["tpl_lanczos_pass_one_batch"], "ks", "low", NONE)
    def _(op, I, p, dev):
        out = ()
        for d in alg.lanczos_pass_one_batch(op, I.cols(p["s"], dev), p["k"]):
            out += _dec_tuple(d)
        return out

    @add("pass_two_batch", ["tpl_lanczos_pass_two_batch"], "ks", "low", P2)
    def _(op, I, p, dev):
        decs = [I.dec(c, p["k"]) for c in range(p["s"])]
        ys = [I.Y(c, p["k"], 1)[:, 0] for c in range(p["s"])]
        return (alg.lanczos_pass_two_batch(op, I.cols(p["s"], dev), decs, ys),)

    @add("pass_two_batch_multi", ["tpl_lanczos_pass_two_batch_multi"], "kms", "low", P2)
    def _(op, I, p, dev):
        decs = [I.dec(c, p["k"]) for c in range(p["s"])]
        Ys = [I.Y(c, p["k"], p["m"]) for c in range(p["s"])]
        return (alg.lanczos_pass_two_batch_multi(op, I.cols(p["s"], dev), decs, Ys),)

    @add("pass_two_batch_multi_cut", ["tpl_lanczos_pass_two_batch_multi_cut"], "kms", "low", P2)
    def _(op, I, p, dev):
        decs = [I.dec(c, p["k"]) for c in range(p["s"])]
        Ys = [I.Y(c, p["k"], p["m"]) for c in range(p["s"])]
        cs = [cuts(d.steps_taken, p["m"], c) for c, d in enumerate(decs)]
        return (alg.lanczos_pass_two_batch_multi_cut(op, I.cols(p["s"], dev), decs, Ys, cs),)

    def standard(name, **kw):
        @add(name, ["tpl_lanczos_standard"], "k", "standard", NONE)
        def _(op, I, p, dev):
            out = alg.lanczos_standard(op, I.vec(dev), p["k"], **kw)
            return _dec_tuple(out.decomposition) + (out.v_k,)

    standard("standard")
    standard("standard_reorth", reorthogonalize=True)
    standard("standard_selective", reorthogonalize="selective")

    @add("standard_callback", ["tpl_lanczos_standard"], "k", "standard", NONE)
    def _(op, I, p, dev):
        stop, seen = max(1, p["k"] - 2), []

        def cb(kk, v, t):
            if kk == stop:   # the view at the step it stops at: the k columns it may read
                seen.append((v.numpy().copy(), t.alphas.copy(), t.betas.copy()))
            return kk < stop
        out = alg.lanczos_standard(op, I.vec(dev), p["k"], callback=cb)
        assert len(seen) == 1
        return _dec_tuple(out.decomposition) + (out.v_k,) + seen[0]

    @add("lanczos", ["tpl_lanczos"], "k", "single", SOLVE1)
    def _(op, I, p, dev):
        return (solvers.lanczos(op, I.vec(dev), p["k"], ftk.INV),)

    # bit 5's sentence names tpl_lanczos_two_pass and tpl_lanczos only
    @add("lanczos_multi", ["tpl_lanczos_multi"], "km", "multi", NONE)
    def _(op, I, p, dev):
        fs = [ftk.inv_shift(sg) for sg in sigmas(p["m"])]
        return (solvers.lanczos_multi(op, I.vec(dev), p["k"], fs),)

    def two_pass(name, f):
        @add(name, ["tpl_lanczos_two_pass"], "k", "single", ALL)
        def _(op, I, p, dev):
            return (solvers.lanczos_two_pass(op, I.vec(dev), p["k"], f),)

    two_pass("two_pass_inv", ftk.INV)
    two_pass("two_pass_exp", ftk.EXP)
    two_pass("two_pass_sq", ftk.SQ)
    two_pass("two_pass_closure", sq_closure)

    @add("two_pass_multi", ["tpl_lanczos_two_pass_multi"], "km", "multi", ALL)
    def _(op, I, p, dev):
        fs = [ftk.inv_shift(sg) for sg in sigmas(p["m"])]
        return (solvers.lanczos_two_pass_multi(op, I.vec(dev), p["k"], fs),)

    @add("two_pass_exp_times", ["tpl_lanczos_two_pass_exp_times"], "km", "multi", ALL)
    def _(op, I, p, dev):
        return solvers.lanczos_two_pass_exp_times(op, I.vec(dev), p["k"], times(p["m"]),
                                                  return_on_device=True)

    def inv_tol(name, met):
        @add(name, ["tpl_lanczos_two_pass_inv_tol"], "k", "tol", ALL)
        def _(op, I, p, dev):
            x, info = solvers.lanczos_two_pass_inv_tol(op, I.vec(dev), p["k"],
                                                       I.tol_met if met else 0.0, return_info=True)
            return _tol_tuple(x, info)

    inv_tol("two_pass_inv_tol_met", True)
    inv_tol("two_pass_inv_tol_never", False)

    @add("two_pass_shifted_inv_tol", ["tpl_lanczos_two_pass_shifted_inv_tol"], "km", "tol", ALL)
    def _(op, I, p, dev):
        x, info = solvers.lanczos_two_pass_shifted_inv_tol(op, I.vec(dev), p["k"], sigmas(p["m"]),
                                                           I.tol_mix, return_info=True)
        return _tol_tuple(x, info)

    def batch(s):
        @add("two_pass_batch_s%d" % s, ["tpl_lanczos_two_pass_batch"], "k", "batch", ALL)
        def _(op, I, p, dev):
            return (solvers.lanczos_two_pass_batch(op, I.cols(s, dev), p["k"], ftk.INV),)

    for s in S_LADDER:
        batch(s)

    @add("two_pass_batch", ["tpl_lanczos_two_pass_batch"], "ks", "batch", ALL)
    def _(op, I, p, dev):
        return (solvers.lanczos_two_pass_batch(op, I.cols(p["s"], dev), p["k"], sq_closure),)

    @add("two_pass_batch_multi", ["tpl_lanczos_two_pass_batch_multi"], "kms", "batch_multi", ALL)
    def _(op, I, p, dev):
        fs = [ftk.inv_shift(sg) for sg in sigmas(p["m"])]
        return (solvers.lanczos_two_pass_batch_multi(op, I.cols(p["s"], dev), p["k"], fs),)

    @add("two_pass_batch_exp_times", ["tpl_lanczos_two_pass_batch_exp_times"], "kms",
         "batch_multi", ALL)
    def _(op, I, p, dev):
        return solvers.lanczos_two_pass_batch_exp_times(op, I.cols(p["s"], dev), p["k"],
                                                        times(p["m"]), return_on_device=True)

    @add("two_pass_batch_shifted_inv_tol", ["tpl_lanczos_two_pass_batch_shifted_inv_tol"], "kms",
         "tol", ALL)
    def _(op, I, p, dev):
        x, info = solvers.lanczos_two_pass_batch_shifted_inv_tol(
            op, I.cols(p["s"], dev), p["k"], sigmas(p["m"]), I.tol_mix, return_info=True)
        return _tol_tuple(x, info, p["s"])

    def ftk_device(which):
        @add("ftk_device_" + which, ["tpl_op_ftk_device"], "k", "device", NONE, device_b=False)
        def _(op, I, p, dev):
            d = I.dec(0, p["k"])
            return op.ftk_device(which, 0.25 * d.alphas, 0.25 * d.betas)

    ftk_device("inv")
    ftk_device("exp")

    @add("ftk_exp_times_device", ["tpl_op_ftk_exp_times_device"], "km", "device", NONE,
         device_b=False)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        return op.ftk_exp_times_device(d.alphas, d.betas, times(p["m"]))

    @add("ftk_inv_shifts_device", ["tpl_op_ftk_inv_shifts_device"], "km", "device", NONE,
         device_b=False)
    def _(op, I, p, dev):
        d = I.dec(0, p["k"])
        return (op.ftk_inv_shifts_device(d.alphas, d.betas, sigmas(p["m"])),)

    @add("ftk_exp_times_batch_device", ["tpl_op_ftk_exp_times_batch_device"], "kms", "device",
         NONE, device_b=False)
    def _(op, I, p, dev):
        nb = 4 if p["s"] >= 4 else 2        # a group is two or four columns wide
        decs = [I.dec(c, p["k"]) for c in range(nb)]
        return op.ftk_exp_times_batch_device([d.alphas for d in decs], [d.betas for d in decs],
                                             times(p["m"]))

    return calls


_CALLS = None


def calls():
    """name -> Call, in catalogue order."""
    global _CALLS
    if _CALLS is None:
        _CALLS = {c.name: c for c in _build_calls()}
    return _CALLS


# A module-level view of the names, for pytest.mark.parametrize at collection time (no GPU).
def call_names():
    return list(calls())


# The call of another family run between the steps of a ladder (test_resize_ladders).
INTERLEAVE = {
    "single": "two_pass_batch_multi", "multi": "two_pass_batch_s4", "batch": "two_pass_inv",
    "batch_multi": "two_pass_inv", "tol": "standard_reorth", "standard": "two_pass_inv_tol_met",
    "low": "two_pass_shifted_inv_tol", "device": "two_pass_batch_shifted_inv_tol",
}
# One call per family for "the next good call of every family" (test_errors_between_calls).
FAMILY_CALLS = ("two_pass_inv", "two_pass_multi", "two_pass_batch_s4", "two_pass_batch_multi",
                "two_pass_inv_tol_met", "standard_reorth")
# test_setter_between_calls' subset
SETTER_CALLS = ("two_pass_inv", "two_pass_multi", "two_pass_batch_s4", "two_pass_batch_multi",
                "two_pass_inv_tol_met", "two_pass_batch_shifted_inv_tol", "standard_reorth")


# ------------------------------------------------------------------------------ settings
# name -> (C setter, default, the other values); a settings tuple holds one value per name in
# this order. The long-row cache's mode 1 takes 1,024 bytes: 4 rows of the KKT block's 30 long
# rows, 8 of the band's 15 (a quarter of that per column in a group of four).
SETTINGS = {
    "device_ftk": ("tpl_op_set_device_ftk", 2, (0, 1)),
    "long_cache": ("tpl_op_set_long_cache", (2, 0), ((0, 0), (1, 1024))),
    "long_cache_solvers": ("tpl_op_set_long_cache_solvers", 1, (15,)),
    "fused_pass_two": ("tpl_op_set_fused_pass_two", 2, (0,)),
    "value_format": ("tpl_op_set_value_format", 1, (0,)),
    "slices": ("tpl_op_set_slices", 0, (2, 4)),
    "short_row_max": ("tpl_op_set_schedule", -1, (24,)),   # 24: the KKT hub rows turn short
    "reorder": ("tpl_op_set_reorder", 2, (0, 1)),
    "order_groups": ("tpl_op_set_order_groups", 0, (4,)),
    "timing": ("tpl_op_enable_timing", 0, (1,)),
    # one row block: the band's element grid goes from G2 3, E 512 to G2 1, E 1536 and back (the
    # KKT block's 496 rows are one block of 512 either way)
    "max_g2": ("tpl_op_set_schedule", 1024, (1,)),
}
SETTING_NAMES = tuple(SETTINGS)
LAYOUT_SETTERS = ("value_format", "slices", "short_row_max", "reorder", "order_groups", "max_g2")
DEFAULT_SETTINGS = tuple(SETTINGS[n][1] for n in SETTING_NAMES)


def with_setting(settings, name, value):
    s = list(settings)
    s[SETTING_NAMES.index(name)] = value
    return tuple(s)


def apply_setting(op, name, value):
    if name == "device_ftk":
        op.set_device_ftk(value)
    elif name == "long_cache":
        op.set_long_cache(*value)
    elif name == "long_cache_solvers":
        op.set_long_cache_solvers(value)
    elif name == "fused_pass_two":
        op.set_fused_pass_two(value)
    elif name == "value_format":
        op.set_value_format(bool(value))
    elif name == "slices":
        op.set_slices(value)
    elif name == "short_row_max":
        op.set_schedule(short_row_max=value)
    elif name == "reorder":
        op.set_reorder(value)
    elif name == "order_groups":
        op.set_order_groups(value)
    elif name == "timing":
        op.enable_timing(bool(value))
    elif name == "max_g2":
        op.set_schedule(max_g2=value)
    else:
        raise KeyError(name)


def new_op(mat, settings=DEFAULT_SETTINGS):
    import tpl_amd
    op = tpl_amd.HipCsrOp(inputs(mat).a)
    for name, value in zip(SETTING_NAMES, settings):
        if value != SETTINGS[name][1]:
            apply_setting(op, name, value)
    return op


# ------------------------------------------------------------------------------ fresh
def run_call(op, mat, name, params, device=False):
    """-> (canonical result, the flag bits the call defines)."""
    c = calls()[name]
    res = canonical(c.run(op, inputs(mat), dict(params), device))
    return res, op.flags() & c.defines


_FRESH, _ANCHORED = {}, set()


def anchor(mat, settings):
    """Once per (matrix, settings): a fresh operator against the device-order oracle, bit for
    bit, wherever the oracle has a counterpart — apply, pass one, the two-pass and one-pass
    inverse solves, both re-orthogonalised passes — so that `fresh` is not anchored in the
    code under test alone. On default settings also the path flags the matrices were chosen
    for (the KKT block's two-pass solve runs fused, the band's reads the cache unfused) and,
    at the default sizes, every call tests/composed_oracle.py composes from the oracle — the
    whole catalogue but the ftk_*device calls."""
    if (mat, settings) in _ANCHORED:
        return
    import oracle
    from tpl_amd import algorithms as alg
    from tpl_amd import ftk, solvers
    I, k = inputs(mat), K_SMALL
    op = new_op(mat, settings)
    try:
        orc = oracle.Operator(I.a, op.schedule())
        w = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
        eq = lambda x, y: np.array_equal(w(x), w(y))
        assert eq(op.apply(I.b), orc.apply(I.b)), (mat, settings, "apply")
        al, be, st, bn, _ = orc.pass_one(I.b, k)
        d = alg.lanczos_pass_one(op, I.b, k)
        assert (d.steps_taken, d.b_norm) == (st, bn) and eq(d.alphas, al) and eq(d.betas, be), \
            (mat, settings, "pass_one")
        x = solvers.lanczos_two_pass(op, I.b, k, ftk.INV)
        flags = op.flags()
        assert eq(x, orc.lanczos_two_pass(I.b, k, ftk.INV)), (mat, settings, "two_pass")
        assert eq(solvers.lanczos(op, I.b, k, ftk.INV), orc.lanczos(I.b, k, ftk.INV)), \
            (mat, settings, "lanczos")
        for mode in (True, "selective"):
            al, be, st, bn, V = orc.pass_one(I.b, k, reorth=mode)
            out = alg.lanczos_standard(op, I.b, k, reorthogonalize=mode)
            dd = out.decomposition
            assert dd.steps_taken == st and eq(dd.alphas, al) and eq(dd.betas, be) and \
                eq(np.asarray(out.v_k), V), (mat, settings, "reorth", mode)
        if settings == DEFAULT_SETTINGS:
            want = CACHED | FUSED if mat == "kkt" else CACHED
            assert flags & (CACHED | FUSED) == want, (mat, flags)
            default_schedule = op.schedule()
    finally:
        op.close()
    if settings == DEFAULT_SETTINGS:
        # every call the oracle can compose (tests/composed_oracle.py), at the default sizes,
        # each on an operator of its own: `fresh` rests on the oracle for the whole catalogue
        import composed_oracle as co
        assert same_schedule(default_schedule, I.oracle_schedule()), mat
        for name in co.covered():
            p = calls()[name].params()
            op = new_op(mat, settings)
            try:
                want = co.canonical_expect(name, I, p, op)
                assert same(run_call(op, mat, name, p)[0], want), (mat, name, p)
            finally:
                op.close()
    _ANCHORED.add((mat, settings))


def fresh(mat, settings, name, params):
    """A new operator, the settings, that one call -> (result, flag bits); memoised."""
    key = (mat, settings, name, params)
    if key not in _FRESH:
        anchor(mat, settings)
        op = new_op(mat, settings)
        try:
            _FRESH[key] = run_call(op, mat, name, params)
        finally:
            op.close()
    return _FRESH[key]


# ------------------------------------------------------------------------------ walks
WALK_SEEDS = tuple(range(16))
WALK_STEPS = 40
BATCH_FAMILIES = ("batch", "batch_multi")


def _random_params(rng, c):
    return c.params(**{z: rng.choice(c.ladder(z)) for z in c.takes})


def _random_call(rng, names=None):
    c = calls()[rng.choice(names or call_names())]
    return ("call", c.name, _random_params(rng, c))


def _random_setter(rng, names=SETTING_NAMES):
    name = rng.choice(names)
    _, default, others = SETTINGS[name]
    return ("set", name, rng.choice((default,) + tuple(others)))


def walk(seed):
    """The step list of one walk: ("call", name, params) or ("set", name, value). About a fifth
    of the steps are setters. Every walk opens with a small call that a later step outgrows in
    k and in m, and holds a layout rebuild followed at once by a batch call; walk `seed` also
    holds the catalogue's calls seed, seed + 16, ... and setter seed mod 11, so the 16 walks
    cover every call and every setter."""
    rng = random.Random(7919 * seed + 13)
    names = call_names()
    steps = [_random_setter(rng) if rng.random() < 0.2 else _random_call(rng)
             for _ in range(WALK_STEPS)]
    grow = calls()["two_pass_shifted_inv_tol"]
    steps[0] = ("call", grow.name, grow.params(k=2, m=1))
    free = list(range(1, WALK_STEPS))
    rng.shuffle(free)
    at = sorted(free[:2])        # k grows at the first, m at the second (or the reverse)
    first = rng.random() < 0.5
    steps[at[0]] = ("call", grow.name, grow.params(k=K_BIG if first else 2, m=1 if first else 5))
    steps[at[1]] = ("call", grow.name, grow.params(k=K_BIG, m=M_LADDER[-1] if first else 5))
    free = [i for i in free[2:]]
    pair = next(i for i in free if i + 1 in free)
    free = [i for i in free if i not in (pair, pair + 1)]
    steps[pair] = _random_setter(rng, LAYOUT_SETTERS)
    batch_names = [n for n in names if calls()[n].family in BATCH_FAMILIES]
    steps[pair + 1] = _random_call(rng, batch_names)
    forced = [("call", n) for n in names[seed::len(WALK_SEEDS)]]
    forced.append(("set", SETTING_NAMES[seed % len(SETTING_NAMES)]))
    for (kind, name), i in zip(forced, free):
        steps[i] = _random_call(rng, [name]) if kind == "call" else _random_setter(rng, [name])
    return steps


def describe(steps):
    return "\n".join("%2d %s %s %s" % (i, kind, name, arg)
                     for i, (kind, name, arg) in enumerate(steps))


def header_entry_points(text):
    """Every tpl_lanczos* function, tpl_op_ftk_*device function and tpl_op_set_* setter that
    tpl.h declares, and tpl_op_enable_timing and tpl_op_tune_order."""
    found = re.findall(r"^tpl_status\s+(tpl_[a-z0-9_]+)\s*\(", text, flags=re.M)
    keep = lambda f: (f.startswith("tpl_lanczos") or re.fullmatch(r"tpl_op_ftk_\w*device", f)
                      or f.startswith("tpl_op_set_")
                      or f in ("tpl_op_enable_timing", "tpl_op_tune_order"))
    return sorted({f for f in found if keep(f)})
