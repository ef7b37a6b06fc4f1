"""What every call of the state_cases.calls() catalogue must return, composed from the
device-order oracle: oracle.Operator.apply, pass_one, pass_two (with store_basis) and lanczos,
the host f(T_k) functions of tpl_amd.ftk, and nothing else. include/tpl.h defines each entry
point in exactly these terms, in bits:

  multi, batch, batch-multi   result (c, i) is pass two of b_c on b_c's own decomposition with
                              y = ||b_c|| f_i(T_k) e_1 formed on the host;
  *_cut, the tolerance solves the same on the decomposition cut to m* steps; m*, `converged` and
                              the guaranteed prefix of each residual history by the stop rule
                              (state_cases.Inputs.stop) on ftk.inv_residuals of the oracle's
                              alphas and betas;
  standard*                   pass one with the basis, plain, CGS2 or selective; a callback
                              that stops at step j keeps the first j steps;
  the exp solves              the one contract that is not host arithmetic: y is what the device
                              kernel alone gives (HipCsrOp.ftk_device("exp", ...) on T_k,
                              ftk_exp_times_device for the times), the host ftk.EXP / ftk.exp_t
                              where the kernel hands a column back and everywhere under
                              set_device_ftk(0) — tests/test_gpu_exp_times.py's contract, taken
                              over as it stands. These expectations need the live operator.

`expect` returns the result tuple in the shape the catalogue's `run` produces, so
state_cases.canonical and state_cases.same compare the two word for word; no tolerance appears.

Left out: the five ftk_*device calls (family "device"). They evaluate f(T_k) on small host
arrays and never read the operator's row blocks, so no geometry can change them;
tests/test_gpu_device_ftk.py, test_gpu_device_exp.py and test_gpu_exp_times.py pin them.
"""
import re

import numpy as np

import state_cases as sc

LEFT_OUT = ("ftk_device_inv", "ftk_device_exp", "ftk_exp_times_device", "ftk_inv_shifts_device",
            "ftk_exp_times_batch_device")
NEEDS_OPERATOR = ("two_pass_exp", "two_pass_exp_times", "two_pass_batch_exp_times")


def covered():
    """The catalogue's calls that `expect` composes, in catalogue order."""
    return [n for n in sc.call_names() if n not in LEFT_OUT]


def _p2(I, c, d, y, cut=None, basis=False):
    """Pass two of column c on decomposition d cut to `cut` steps, y's first `cut` entries."""
    st = int(d.steps_taken) if cut is None else int(cut)
    al, be = np.asarray(d.alphas)[:st], np.asarray(d.betas)[:max(st - 1, 0)]
    x, V = I.oracle().pass_two(I.B[:, c], al, be, st, d.b_norm,
                               np.ascontiguousarray(np.asarray(y)[:st]), store_basis=basis)
    return (x, V) if basis else x


def _solve(I, c, k, f):
    """Column c's two-pass solve with f on the host: pass one, y = ||b|| f(T_k) e_1, pass two."""
    d = I.dec(c, k)
    return _p2(I, c, d, np.asarray(f(d.alphas, d.betas), dtype=np.float64).reshape(-1) * d.b_norm)


def _stack(cols):
    """Columns -> (n, m); lists of columns per right-hand side -> (n, m, s)."""
    if isinstance(cols[0], list):
        return np.stack([np.stack(col, axis=1) for col in cols], axis=2)
    return np.stack(cols, axis=1)


def _multi(I, c, k, m, cut_of=None):
    d, Y = I.dec(c, k), I.Y(c, k, m)
    cs = cut_of(d) if cut_of else [None] * m
    return [_p2(I, c, d, Y[:, i], cs[i]) for i in range(m)]


def _shifted(I, c, k, m, tol):
    """-> per shift (x, m*, converged, guaranteed prefix) of column c."""
    from tpl_amd import ftk
    d, out = I.dec(c, k), []
    for sg in sc.sigmas(m):
        ms, conv = I.stop(c, k, sg, tol)
        y = ftk.inv_shift(sg)(d.alphas[:ms], d.betas[:ms - 1]) * d.b_norm
        have = ms if conv else int(d.steps_taken) - 1
        out.append((_p2(I, c, d, y, ms), ms, conv, I.history(c, k, sg)[:have]))
    return out


def _exp_times(I, c, k, ts, op, host):
    """-> (columns x_i, on): y_i from the device kernel alone on column c's T_k, the host exp_t
    where it hands a time back and throughout in host mode."""
    from tpl_amd import ftk
    d = I.dec(c, k)
    st = int(d.steps_taken)
    al, be = np.asarray(d.alphas)[:st], np.asarray(d.betas)[:st - 1]
    if host:
        Y, on = np.zeros((st, len(ts))), np.zeros(len(ts), dtype=bool)
    else:
        Y, on = op.ftk_exp_times_device(al, be, ts)
        Y = np.array(Y)
    for i, t in enumerate(ts):
        if not on[i]:
            Y[:, i] = ftk.exp_t(t)(al, be)
    Y = Y * d.b_norm
    return [_p2(I, c, d, np.ascontiguousarray(Y[:, i])) for i in range(len(ts))], on


def exp_on_device(I, k, op, host):
    """Whether the single two-pass exp solve keeps f on the device (flag bit 5 afterwards)."""
    if host:
        return False
    d = I.dec(0, k)
    return bool(op.ftk_device("exp", d.alphas, d.betas)[1])


def expect(name, I, p, op=None, host_ftk=False):
    """The result tuple of catalogue call `name` at sizes p (a dict of k, m, s) on inputs I,
    whose oracle runs in the reduction order under test. op: the live operator, for the calls
    of NEEDS_OPERATOR only; host_ftk: the operator is in set_device_ftk(0)."""
    from tpl_amd import ftk
    o = I.oracle()
    k, m, s = p.get("k"), p.get("m"), p.get("s")
    dec_tuple = lambda d: (d.alphas, d.betas, int(d.steps_taken), np.array([d.b_norm]))

    if name == "apply":
        return (o.apply(I.b),)
    if name == "pass_one":
        return dec_tuple(I.dec(0, k))
    if name == "pass_two":
        return (_p2(I, 0, I.dec(0, k), I.Y(0, k, 1)[:, 0]),)
    if name == "pass_two_with_basis":
        return _p2(I, 0, I.dec(0, k), I.Y(0, k, 1)[:, 0], basis=True)
    if name == "pass_two_multi":
        return (_stack(_multi(I, 0, k, m)),)
    if name == "pass_two_multi_cut":
        return (_stack(_multi(I, 0, k, m, lambda d: sc.cuts(d.steps_taken, m))),)
    if name == "pass_one_batch":
        return sum((dec_tuple(I.dec(c, k)) for c in range(s)), ())
    if name == "pass_two_batch":
        return (_stack([_multi(I, c, k, 1)[0] for c in range(s)]),)
    if name == "pass_two_batch_multi":
        return (_stack([_multi(I, c, k, m) for c in range(s)]),)
    if name == "pass_two_batch_multi_cut":
        return (_stack([_multi(I, c, k, m, lambda d, c=c: sc.cuts(d.steps_taken, m, c))
                        for c in range(s)]),)

    if name in ("standard", "standard_reorth", "standard_selective", "standard_callback"):
        mode = {"standard_reorth": True, "standard_selective": "selective"}.get(name, False)
        al, be, st, bn, V = o.pass_one(I.b, k, store_basis=True, reorth=mode)
        if name != "standard_callback":
            return (al, be, st, np.array([bn]), V)
        j = min(st, max(1, k - 2))       # the callback stops at step max(1, k - 2)
        al, be, V = al[:j], be[:j - 1], np.ascontiguousarray(V[:, :j])
        return (al, be, j, np.array([bn]), V, V, al, be)

    if name == "lanczos":
        return (o.lanczos(I.b, k, ftk.INV),)
    if name == "lanczos_multi":
        return (_stack([o.lanczos(I.b, k, ftk.inv_shift(sg)) for sg in sc.sigmas(m)]),)
    if name in ("two_pass_inv", "two_pass_sq", "two_pass_closure"):
        f = {"two_pass_inv": ftk.INV, "two_pass_sq": ftk.SQ, "two_pass_closure": sc.sq_closure}
        return (_solve(I, 0, k, f[name]),)
    if name == "two_pass_exp":
        d = I.dec(0, k)
        y, on = (None, False) if host_ftk else op.ftk_device("exp", d.alphas, d.betas)
        return (_p2(I, 0, d, (y if on else ftk.EXP(d.alphas, d.betas)) * d.b_norm),)
    if name == "two_pass_multi":
        return (_stack([_solve(I, 0, k, ftk.inv_shift(sg)) for sg in sc.sigmas(m)]),)
    if name == "two_pass_exp_times":
        cols, on = _exp_times(I, 0, k, sc.times(m), op, host_ftk)
        return (_stack(cols), on)
    if name in ("two_pass_inv_tol_met", "two_pass_inv_tol_never"):
        d = I.dec(0, k)
        ms, conv = I.stop(0, k, 0.0, I.tol_met if name.endswith("met") else 0.0)
        have = ms if conv else int(d.steps_taken) - 1
        x = _p2(I, 0, d, ftk.INV(d.alphas[:ms], d.betas[:ms - 1]) * d.b_norm, ms)
        return (x, np.array([ms]), np.array([conv]),
                ftk.inv_residuals(d.alphas, d.betas)[:have])
    if name == "two_pass_shifted_inv_tol":
        r = _shifted(I, 0, k, m, I.tol_mix)
        return (_stack([x for x, _, _, _ in r]), np.array([ms for _, ms, _, _ in r]),
                np.array([cv for _, _, cv, _ in r]),
                np.concatenate([h for _, _, _, h in r] + [np.zeros(0)]))
    fixed_s = re.fullmatch(r"two_pass_batch_s(\d+)", name)
    if fixed_s:
        return (_stack([_solve(I, c, k, ftk.INV) for c in range(int(fixed_s.group(1)))]),)
    if name == "two_pass_batch":
        return (_stack([_solve(I, c, k, sc.sq_closure) for c in range(s)]),)
    if name == "two_pass_batch_multi":
        return (_stack([[_solve(I, c, k, ftk.inv_shift(sg)) for sg in sc.sigmas(m)]
                        for c in range(s)]),)
    if name == "two_pass_batch_exp_times":
        r = [_exp_times(I, c, k, sc.times(m), op, host_ftk) for c in range(s)]
        return (_stack([cols for cols, _ in r]), np.stack([on for _, on in r], axis=1))
    if name == "two_pass_batch_shifted_inv_tol":
        r = [_shifted(I, c, k, m, I.tol_mix) for c in range(s)]
        at = lambda j: np.array([[r[c][i][j] for c in range(s)] for i in range(m)])
        return (_stack([[x for x, _, _, _ in col] for col in r]), at(1), at(2),
                np.concatenate([r[c][i][3] for i in range(m) for c in range(s)] + [np.zeros(0)]))
    raise KeyError(name)


def canonical_expect(name, I, params, op=None, host_ftk=False):
    """`expect` for a catalogue parameter tuple, as state_cases.canonical words."""
    return sc.canonical(expect(name, I, dict(params), op, host_ftk))
