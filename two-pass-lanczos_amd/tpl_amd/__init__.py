"""tpl_amd — MI355X-native two-pass Lanczos engine for f(A) b.

Python mirror of the reference crate's public surface (lukefleed/two-pass-lanczos,
src/lib.rs:94-101) on top of the C ABI of libtpl_amd.so (include/tpl.h):

* ``lanczos``, ``lanczos_two_pass``          — src/solvers.rs (re-exported at the root)
* ``algorithms.*``                           — src/algorithms (low-level passes)
* ``error.LanczosError``                     — src/error.rs
* ``utils.data_loader.load_kkt_system``      — src/utils/data_loader.rs
* ``HipCsrOp``                               — the device-resident operator (faer LinOp)
"""
from . import _lib
from . import algorithms, error, ftk, solvers
from .error import DataLoaderError, LanczosError, LanczosErrorKind, TplError
from .operator import HipCsrOp, HipDenseOp, HostPlan, device_count, locality_order, refresh_uploaded
from .operator import (LONG_CACHE_TWO_PASS, LONG_CACHE_TWO_PASS_BATCH,
                       LONG_CACHE_TWO_PASS_BATCH_MULTI, LONG_CACHE_TWO_PASS_MULTI)
from .solvers import (lanczos, lanczos_multi, lanczos_two_pass, lanczos_two_pass_batch,
                      lanczos_two_pass_batch_exp_times, lanczos_two_pass_batch_multi,
                      lanczos_two_pass_batch_shifted_inv_tol,
                      lanczos_two_pass_exp_times, lanczos_two_pass_inv_tol,
                      lanczos_two_pass_multi, lanczos_two_pass_shifted_inv_tol)

__version__ = "0.1.0"
LIB_PATH = _lib.LIB_PATH

__all__ = [
    "lanczos", "lanczos_two_pass", "lanczos_multi", "lanczos_two_pass_multi", "lanczos_two_pass_batch", "lanczos_two_pass_batch_multi", "lanczos_two_pass_exp_times", "lanczos_two_pass_batch_exp_times", "lanczos_two_pass_inv_tol", "lanczos_two_pass_shifted_inv_tol", "lanczos_two_pass_batch_shifted_inv_tol", "algorithms", "solvers", "error", "ftk", "HipCsrOp", "HipDenseOp",
    "LanczosError", "LanczosErrorKind", "TplError", "DataLoaderError", "device_count",
    "locality_order", "HostPlan", "refresh_uploaded",
    "LONG_CACHE_TWO_PASS", "LONG_CACHE_TWO_PASS_MULTI", "LONG_CACHE_TWO_PASS_BATCH",
    "LONG_CACHE_TWO_PASS_BATCH_MULTI",
]
