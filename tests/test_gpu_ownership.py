"""GPU tests of what an operator owns when an allocation is refused partway.

The solver state and the layout are built aside and swapped in, the basis frees before it
grows, and a handle's destructor is the only release path — so a refused allocation leaves
a working operator (or, in a create, no operator). The refusals come from the test hook
in the operator's one allocation path: with TPL_TEST_ALLOC_CAP=<bytes> set, a request that
would take the operator's accounted device bytes above the cap fails on the host exactly
as hipErrorOutOfMemory is reported (TPL_ERR_OUT_OF_MEMORY) and never reaches the runtime.
Each test checks the host-visible state before anything runs on the device again.

The 5k-arc KKT instance, k = 20, the built-in inv; references from fresh operators."""
import ctypes
import os
import sys
import types
from ctypes import POINTER, byref, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "two-pass-lanczos_amd"))

from conftest import harness_b, load_kkt  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = "TPL_TEST_ALLOC_CAP"
K, K_BIG = 20, 64


@pytest.fixture(scope="module")
def ref(kkt_tmp):
    """The instance and, from fresh operators: x0 (two-pass), xs (one-pass), the k = 64
    decomposition, and the device bytes of a fully created operator."""
    import tpl_amd
    assert CAP not in os.environ
    a = load_kkt(5000, kkt_tmp).a
    b = harness_b(a)
    op = tpl_amd.HipCsrOp(a)
    created = op.device_bytes()
    x0 = tpl_amd.lanczos_two_pass(op, b, K, "inv")
    op.close()
    op = tpl_amd.HipCsrOp(a)
    xs = tpl_amd.lanczos(op, b, K, "inv")
    op.close()
    op = tpl_amd.HipCsrOp(a)
    dec = tpl_amd.algorithms.lanczos_pass_one(op, b, K_BIG)
    op.close()
    return types.SimpleNamespace(a=a, b=b, x0=x0, xs=xs, created=created,
                                 alphas=dec.alphas.copy(), betas=dec.betas.copy())


def _host_state(op):
    return op.schedule(), op.flags(), op.device_bytes()


def _assert_host_state(op, before):
    sched, flags, nbytes = before
    after = op.schedule()
    assert after.keys() == sched.keys()
    for key, v in sched.items():
        assert np.array_equal(after[key], v) and (after[key] is None) == (v is None), key
    assert op.flags() == flags
    assert op.device_bytes() == nbytes


def _assert_oom(excinfo):
    from tpl_amd import _lib
    assert excinfo.value.status == _lib.TPL_ERR_OUT_OF_MEMORY
    assert str(excinfo.value).startswith("hipMalloc(p, bytes): ")


def test_failed_state_growth_keeps_state(ref, monkeypatch):
    """A pass that needs a larger solver state than the cap allows is refused with the old
    state, its capacity and the operator's host-visible state in place: the k = 20 solve
    repeats bit for bit, and the k = 64 pass then matches a fresh operator's."""
    import tpl_amd
    from tpl_amd.error import TplError
    op = tpl_amd.HipCsrOp(ref.a)
    try:
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, ref.b, K, "inv"), ref.x0)
        before = _host_state(op)
        monkeypatch.setenv(CAP, str(before[2]))
        with pytest.raises(TplError) as e:
            tpl_amd.algorithms.lanczos_pass_one(op, ref.b, K_BIG)
        _assert_oom(e)
        _assert_host_state(op, before)
        monkeypatch.delenv(CAP)
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, ref.b, K, "inv"), ref.x0)
        dec = tpl_amd.algorithms.lanczos_pass_one(op, ref.b, K_BIG)
        assert np.array_equal(dec.alphas, ref.alphas) and np.array_equal(dec.betas, ref.betas)
    finally:
        op.close()


def test_failed_basis_growth_keeps_operator(ref, monkeypatch):
    """The one-pass solve's n x k basis is refused: the accounted bytes are unchanged, the
    two-pass solve still gives x0, and the one-pass solve then matches a fresh operator's."""
    import tpl_amd
    from tpl_amd.error import TplError
    op = tpl_amd.HipCsrOp(ref.a)
    try:
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, ref.b, K, "inv"), ref.x0)
        nbytes = op.device_bytes()
        monkeypatch.setenv(CAP, str(nbytes))
        with pytest.raises(TplError) as e:
            tpl_amd.lanczos(op, ref.b, K, "inv")
        _assert_oom(e)
        assert op.device_bytes() == nbytes
        monkeypatch.delenv(CAP)
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, ref.b, K, "inv"), ref.x0)
        assert np.array_equal(tpl_amd.lanczos(op, ref.b, K, "inv"), ref.xs)
    finally:
        op.close()


def _csr_args(a):
    from tpl_amd.operator import _as_csr_arrays
    n, rp, ci, v = _as_csr_arrays(a)
    return n, (rp, ci, v), (rp.ctypes.data_as(POINTER(c_int64)),
                            ci.ctypes.data_as(POINTER(c_int32)),
                            v.ctypes.data_as(POINTER(c_double)))


def test_failed_create_yields_no_handle(ref, monkeypatch):
    """A create refused at its first, a middle or its last allocation reports out of memory
    and hands out no operator; a create after it works. (That the refused create's buffers
    were released is held by construction — the handle's destructor is the only release
    path — and cannot be observed through the ABI.)"""
    import tpl_amd
    from tpl_amd import _lib
    from tpl_amd.operator import context
    n, keep, (rp, ci, v) = _csr_args(ref.a)
    ctx = context(0)
    for cap in (1, ref.created // 2, ref.created - 8):
        monkeypatch.setenv(CAP, str(cap))
        h = c_void_p()
        st = _lib.tpl_op_create_csr(ctx, n, int(keep[0][-1]), rp, ci, v, byref(h))
        assert (st, h.value) == (_lib.TPL_ERR_OUT_OF_MEMORY, None), cap
        assert _lib.tpl_last_error().decode().startswith("hipMalloc(p, bytes): ")
    monkeypatch.delenv(CAP)
    op = tpl_amd.HipCsrOp(ref.a)
    try:
        assert op.device_bytes() == ref.created
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, ref.b, K, "inv"), ref.x0)
    finally:
        op.close()


def test_failed_replicated_create_yields_no_handle(ref, monkeypatch):
    """The same at the last allocation of a replicated operator (one rank over the host
    transport): the partition's extra buffers go through the same path."""
    import tpl_amd
    from tpl_amd import _lib
    from tpl_amd.dist import DistHipCsrOp

    def allgather(send, recv, nbytes, _user):
        ctypes.memmove(recv, send, nbytes)
        return 0

    cb = _lib.ALLGATHER_FN(allgather)
    d = c_void_p()
    assert _lib.tpl_dist_create_host(0, 0, 1, cb, None, byref(d)) == _lib.TPL_OK
    op = None
    try:
        dctx = types.SimpleNamespace(handle=d.value, device=0, rank=0, world=1)
        op = DistHipCsrOp(ref.a, dctx, mode="replicated")
        assert op.mode == "replicated"
        created = op.device_bytes()
        x0 = tpl_amd.lanczos_two_pass(op, op.local(ref.b), K, "inv")
        op.close()
        op = None
        n, keep, (rp, ci, v) = _csr_args(ref.a)
        monkeypatch.setenv(CAP, str(created - 8))
        h = c_void_p()
        st = _lib.tpl_dist_op_create_replicated(d.value, n, rp, ci, v, byref(h))
        assert (st, h.value) == (_lib.TPL_ERR_OUT_OF_MEMORY, None)
        monkeypatch.delenv(CAP)
        op = DistHipCsrOp(ref.a, dctx, mode="replicated")
        assert op.device_bytes() == created
        assert np.array_equal(tpl_amd.lanczos_two_pass(op, op.local(ref.b), K, "inv"), x0)
    finally:
        if op is not None:
            op.close()
        _lib.tpl_dist_destroy(d.value)
