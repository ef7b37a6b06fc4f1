"""CPU: a destroy call keeps the thread's recorded error (include/tpl.h tpl_last_error).

The Python mirror reads a failed call's error with two further calls (tpl_last_error,
tpl_last_error_detail). An operator that is only reachable through a reference cycle is
destroyed by the garbage collector whenever it next runs — possibly between the failed call
and those reads. tpl_op_destroy therefore leaves the record as it is; any other successful
call still resets it. A host-only plan stands in for the operator: no GPU needed.
"""
import gc
from ctypes import POINTER, byref, c_int32, c_int64

import numpy as np
import scipy.sparse as sp

import tpl_amd
from tpl_amd import _lib


def failing_call():
    """tpl_locality_order with a decreasing row_ptr -> its status."""
    rp = np.array([0, 2, 1], dtype=np.int64)
    ci = np.array([1, 0], dtype=np.int32)
    perm = np.zeros(2, dtype=np.int32)
    applied = c_int32()
    return _lib.tpl_locality_order(2, rp.ctypes.data_as(POINTER(c_int64)),
                                   ci.ctypes.data_as(POINTER(c_int32)), 0, 0,
                                   perm.ctypes.data_as(POINTER(c_int32)), byref(applied))


def assert_recorded(st):
    d = _lib.last_error_detail()
    assert d["status"] == st == _lib.TPL_ERR_INVALID_ARGUMENT
    assert d["message"] == _lib.last_error() == "row_ptr not monotone"


def test_destroy_keeps_the_recorded_error():
    plan = tpl_amd.HostPlan(sp.identity(8, format="csr"))
    st = failing_call()
    plan.close()
    assert_recorded(st)
    assert _lib.tpl_op_destroy(None) == _lib.TPL_OK  # NULL: nothing to do, nothing reset
    assert_recorded(st)


def test_collected_operator_keeps_the_recorded_error():
    """The operator of a reference cycle, never closed: the collector's finalizer runs after
    the failed call and before the error is read."""
    class Holder:
        pass

    h = Holder()
    h.plan = tpl_amd.HostPlan(sp.identity(8, format="csr"))
    h.me = h
    gc.collect()
    st = failing_call()
    del h
    assert gc.collect() > 0
    assert_recorded(st)


def test_success_elsewhere_still_resets():
    st = failing_call()
    assert_recorded(st)
    plan = tpl_amd.HostPlan(sp.identity(8, format="csr"))
    assert _lib.last_error_detail()["status"] == 0 and _lib.last_error() == ""
    plan.close()
