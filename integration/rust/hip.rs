//! `src/hip.rs` for lukefleed/two-pass-lanczos: the Rust side of the drop-in boundary
//! (include/tpl.h). Added to the reference crate as `pub mod hip;` next to `solvers`;
//! `build.rs` gains the two lines of `integration/rust/build_rs_snippet.rs`.
//!
//! Every public item of the reference's Lanczos API has a counterpart here with the SAME
//! name, parameter names and parameter order, `stack: &mut MemStack` included, so a call
//! site compiles unchanged once its `use` line names `crate::hip` instead of
//! `crate::solvers` / `crate::algorithms::*`:
//!
//! | reference                                                           | here                                  |
//! |---------------------------------------------------------------------|---------------------------------------|
//! | `solvers::lanczos` (src/solvers.rs:46-57)                           | [`lanczos`] -> `tpl_lanczos`          |
//! | `solvers::lanczos_two_pass` (src/solvers.rs:133-144)                | [`lanczos_two_pass`] -> `tpl_lanczos_two_pass` |
//! | `lanczos::lanczos_standard` (src/algorithms/lanczos.rs:55-64)       | [`lanczos_standard`] -> `tpl_lanczos_standard` (+ `tpl_step_cb`) |
//! | `lanczos_two_pass::lanczos_pass_one` (lanczos_two_pass.rs:65-73)    | [`lanczos_pass_one`] -> `tpl_lanczos_pass_one` |
//! | `lanczos_two_pass::lanczos_pass_two` (lanczos_two_pass.rs:128-137)  | [`lanczos_pass_two`] -> `tpl_lanczos_pass_two` |
//! | `lanczos_two_pass::lanczos_pass_two_with_basis` (:149-158)          | [`lanczos_pass_two_with_basis`] -> `tpl_lanczos_pass_two` (`v_out`) |
//! | faer `LinOp<f64>` of `SparseColMatRef<usize, f64>` (mod.rs:177)     | `impl LinOp<f64> for HipCsrOp` -> `tpl_op_apply` |
//!
//! Two deliberate differences, both forced by the device:
//! * the scalar type is `f64` (the reference is generic over `T: ComplexField`, but every
//!   call site in `src/bin/*` and `tests/*` instantiates it with `f64`, and the engine is
//!   fp64 only); `T` and `T::Real` read `f64` below;
//! * `operator` is any [`HipOperand`] instead of any `LinOp<T>`: the engine's own
//!   [`HipCsrOp`] (upload once, the fast path), or the very `SparseColMatRef<usize, f64>` /
//!   `SparseColMat<usize, f64>` the call sites already pass (`&a.as_ref()` in
//!   src/bin/tradeoff.rs:268-284, src/bin/orthogonality.rs:180-197 and
//!   tests/correctness.rs:142), uploaded on first use and re-used while its operand key
//!   (include/tpl.h tpl_operand_key: the arrays' addresses and sizes plus a sampled
//!   checksum, O(4096) words per call) is unchanged; [`refresh_uploaded`] forces a new
//!   upload after an in-place change of values. [`HipCsrOp::from_csc`] once and `&op` per
//!   call is the zero-overhead form.
//!
//! `stack` is accepted and left untouched: the engine keeps its workspace in HBM
//! (faer's `apply_scratch` of [`HipCsrOp`] is empty for the same reason).
//!
//! Several GPUs (an extension: the reference is single-threaded, `Par::Seq`): one process
//! per GPU, each creates a [`HipDist`] (the RCCL communicator; rank 0's
//! [`HipDist::unique_id`] bytes reach the others by any channel the host program has —
//! MPI, a file, a socket) and then [`HipCsrOp::partitioned`] from the SAME whole matrix.
//! The functions below take the partitioned operator unchanged; `b` and the returned `x`
//! (and V_k) are then this rank's rows, [`HipCsrOp::local_rows`] — the same contract as
//! include/tpl.h's row-partitioned operators.
//!
//! Written against faer 0.22.6 (the reference's Cargo.toml). This image has no Rust
//! toolchain, so the file is UNCOMPILED here; tests/test_boundary.py type-checks every
//! `extern "C"` item, both callback types and the `#[repr(C)]` struct against
//! include/tpl.h, and every public signature against the reference's, and
//! tests/native/abi_driver.cpp / cpp_api_test.cpp make the same calls through the same
//! C ABI in the test suite.

use crate::algorithms::{
    LanczosCallback, LanczosDecomposition, LanczosOutput, LanczosPassTwoOutput,
    TridiagonalSystemView,
};
use crate::error::{LanczosError, LanczosErrorKind};
use faer::dyn_stack::{MemStack, StackReq};
use faer::matrix_free::LinOp;
use faer::sparse::{SparseColMat, SparseColMatRef};
use faer::{Mat, MatMut, MatRef, Par};
use std::cell::RefCell;
use std::ffi::{c_char, c_int, c_void, CStr};
use std::sync::{Arc, Mutex};

#[repr(C)]
pub struct TplCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct TplOp {
    _p: [u8; 0],
}
#[repr(C)]
pub struct TplDist {
    _p: [u8; 0],
}
/// TPL_DIST_ID_BYTES (include/tpl.h): the RCCL unique id rank 0 creates.
pub const TPL_DIST_ID_BYTES: usize = 128;
/// `tpl_ftk_fn` (include/tpl.h): the `f_tk_solver` closure behind a C callback.
type FtkFn = unsafe extern "C" fn(*const f64, usize, *const f64, usize, *mut f64, usize,
                                  *mut usize, *mut c_char, usize, *mut c_void) -> c_int;
/// `tpl_step_cb` (include/tpl.h): the `LanczosCallback` behind a C callback.
type StepCb = unsafe extern "C" fn(usize, *const f64, i64, *const f64, usize, *const f64,
                                   usize, *mut c_void) -> c_int;

const TPL_MEM_HOST: c_int = 0;

/// tpl_error_detail (include/tpl.h): the fields of the engine's LanczosErrorKind.
#[repr(C)]
struct TplErrorDetail {
    status: i32,
    message: *const c_char,
    inner: *const c_char,
    param_name: *const c_char,
    expected: u64,
    actual: u64,
    operator_cols: u64,
    vector_rows: u64,
    breakdown_step: u64,
}

extern "C" {
    fn tpl_last_error_detail(out: *mut TplErrorDetail) -> c_int;
    fn tpl_ctx_create(device: c_int, out: *mut *mut TplCtx) -> c_int;
    fn tpl_ctx_destroy(ctx: *mut TplCtx) -> c_int;
    fn tpl_op_create_csr(ctx: *mut TplCtx, n: i64, nnz: i64, row_ptr: *const i64,
                         col_idx: *const i32, vals: *const f64, out: *mut *mut TplOp) -> c_int;
    fn tpl_op_create_dense(ctx: *mut TplCtx, n: i64, a: *const f64, lda: i64, mem: c_int,
                           out: *mut *mut TplOp) -> c_int;
    fn tpl_op_destroy(op: *mut TplOp) -> c_int;
    fn tpl_op_apply(op: *mut TplOp, x: *const f64, y: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos(op: *mut TplOp, b: *const f64, b_len: i64, k: usize, f: FtkFn,
                   f_user: *mut c_void, x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass(op: *mut TplOp, b: *const f64, b_len: i64, k: usize, f: FtkFn,
                            f_user: *mut c_void, x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_standard(op: *mut TplOp, b: *const f64, b_len: i64, k: usize,
                            alphas: *mut f64, betas: *mut f64, steps: *mut usize,
                            b_norm: *mut f64, v_out: *mut f64, mem: c_int, reorth: c_int,
                            cb: Option<StepCb>, cb_user: *mut c_void) -> c_int;
    fn tpl_lanczos_pass_one(op: *mut TplOp, b: *const f64, b_len: i64, k: usize,
                            alphas: *mut f64, betas: *mut f64, steps: *mut usize,
                            b_norm: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_pass_two(op: *mut TplOp, b: *const f64, b_len: i64, alphas: *const f64,
                            n_alphas: usize, betas: *const f64, n_betas: usize, steps: usize,
                            b_norm: f64, y: *const f64, y_len: usize, x_out: *mut f64,
                            v_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass_multi(op: *mut TplOp, b: *const f64, b_len: i64, k: usize,
                                  fs: *const FtkFn, f_users: *mut *mut c_void, m: usize,
                                  x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass_exp_times(op: *mut TplOp, b: *const f64, b_len: i64, k: usize,
                                      ts: *const f64, m: usize, x_out: *mut f64, mem: c_int,
                                      on_device: *mut i32) -> c_int;
    fn tpl_lanczos_two_pass_inv_tol(op: *mut TplOp, b: *const f64, b_len: i64, kmax: usize,
                                    tol: f64, x_out: *mut f64, mem: c_int, steps: *mut usize,
                                    converged: *mut i32, res_out: *mut f64,
                                    res_len: *mut usize) -> c_int;
    fn tpl_ftk_inv_residuals(alphas: *const f64, n_alphas: usize, betas: *const f64,
                             n_betas: usize, res_out: *mut f64, res_cap: usize,
                             res_len: *mut usize) -> c_int;
    fn tpl_lanczos_two_pass_shifted_inv_tol(op: *mut TplOp, b: *const f64, b_len: i64,
                                            kmax: usize, sigmas: *const f64, m: usize, tol: f64,
                                            x_out: *mut f64, mem: c_int, steps: *mut usize,
                                            converged: *mut i32, res_out: *mut f64,
                                            res_len: *mut usize) -> c_int;
    fn tpl_lanczos_pass_two_multi_cut(op: *mut TplOp, b: *const f64, b_len: i64,
                                      alphas: *const f64, n_alphas: usize, betas: *const f64,
                                      n_betas: usize, steps: usize, b_norm: f64, y: *const f64,
                                      ldy: usize, col_steps: *const usize, m: usize,
                                      x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_op_ftk_inv_shifts_device(op: *mut TplOp, alphas: *const f64, n: usize,
                                    betas: *const f64, sigmas: *const f64, m: usize,
                                    y_out: *mut f64) -> c_int;
    fn tpl_op_ftk_exp_times_device(op: *mut TplOp, alphas: *const f64, n: usize,
                                   betas: *const f64, ts: *const f64, m: usize,
                                   y_out: *mut f64, on_device: *mut i32) -> c_int;
    fn tpl_ftk_exp_t(alphas: *const f64, n_alphas: usize, betas: *const f64, n_betas: usize,
                     y_out: *mut f64, y_cap: usize, y_len: *mut usize, err_msg: *mut c_char,
                     err_cap: usize, user: *mut c_void) -> c_int;
    fn tpl_lanczos_two_pass_batch_exp_times(op: *mut TplOp, B: *const f64, b_len: i64, s: usize,
                                            k: usize, ts: *const f64, m: usize, x_out: *mut f64,
                                            mem: c_int, on_device: *mut i32) -> c_int;
    fn tpl_op_ftk_exp_times_batch_device(op: *mut TplOp, alphas: *const f64, betas: *const f64,
                                         ld: usize, steps: *const usize, nb: usize,
                                         ts: *const f64, m: usize, y_out: *mut f64,
                                         on_device: *mut i32) -> c_int;
    fn tpl_lanczos_multi(op: *mut TplOp, b: *const f64, b_len: i64, k: usize,
                         fs: *const FtkFn, f_users: *mut *mut c_void, m: usize,
                         x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_pass_two_multi(op: *mut TplOp, b: *const f64, b_len: i64,
                                  alphas: *const f64, n_alphas: usize, betas: *const f64,
                                  n_betas: usize, steps: usize, b_norm: f64, y: *const f64,
                                  y_len: usize, m: usize, x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass_batch(op: *mut TplOp, B: *const f64, b_len: i64, s: usize, k: usize,
                                  f: FtkFn, f_user: *mut c_void, x_out: *mut f64,
                                  mem: c_int) -> c_int;
    fn tpl_lanczos_pass_one_batch(op: *mut TplOp, B: *const f64, b_len: i64, s: usize, k: usize,
                                  alphas: *mut f64, betas: *mut f64, steps: *mut usize,
                                  b_norms: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_pass_two_batch(op: *mut TplOp, B: *const f64, b_len: i64, s: usize,
                                  alphas: *const f64, betas: *const f64, ld: usize,
                                  steps: *const usize, b_norms: *const f64, y: *const f64,
                                  x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass_batch_multi(op: *mut TplOp, B: *const f64, b_len: i64, s: usize,
                                        k: usize, fs: *const FtkFn, f_users: *mut *mut c_void,
                                        m: usize, x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_pass_two_batch_multi(op: *mut TplOp, B: *const f64, b_len: i64, s: usize,
                                        alphas: *const f64, betas: *const f64, ld: usize,
                                        steps: *const usize, b_norms: *const f64, y: *const f64,
                                        m: usize, x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_lanczos_two_pass_batch_shifted_inv_tol(op: *mut TplOp, B: *const f64, b_len: i64,
                                                  s: usize, kmax: usize, sigmas: *const f64,
                                                  m: usize, tol: f64, x_out: *mut f64,
                                                  mem: c_int, steps: *mut usize,
                                                  converged: *mut i32, res_out: *mut f64,
                                                  res_len: *mut usize) -> c_int;
    fn tpl_lanczos_pass_two_batch_multi_cut(op: *mut TplOp, B: *const f64, b_len: i64, s: usize,
                                            alphas: *const f64, betas: *const f64, ld: usize,
                                            steps: *const usize, b_norms: *const f64,
                                            y: *const f64, col_steps: *const usize, m: usize,
                                            x_out: *mut f64, mem: c_int) -> c_int;
    fn tpl_batch_shifted_inv_tol_auto_k() -> usize;
    fn tpl_copy_to_host(dst: *mut c_void, src_device: *const c_void, bytes: usize) -> c_int;
    fn tpl_op_nrows(op: *mut TplOp) -> i64;
    fn tpl_op_local_rows(op: *mut TplOp, rows: *mut i64) -> c_int;
    fn tpl_dist_unique_id(id: *mut u8) -> c_int;
    fn tpl_dist_create(device: c_int, rank: c_int, nranks: c_int, id: *const u8,
                       out: *mut *mut TplDist) -> c_int;
    fn tpl_dist_destroy(d: *mut TplDist) -> c_int;
    fn tpl_dist_op_create_replicated(d: *mut TplDist, n: i64, row_ptr: *const i64,
                                     col_idx: *const i32, vals: *const f64,
                                     out: *mut *mut TplOp) -> c_int;
    fn tpl_dist_op_create_halo(d: *mut TplDist, n: i64, starts: *const i64,
                               row_ptr: *const i64, col_idx: *const i32, vals: *const f64,
                               out: *mut *mut TplOp) -> c_int;
    fn tpl_dist_op_create_auto(d: *mut TplDist, n: i64, row_ptr: *const i64,
                               col_idx: *const i32, vals: *const f64, out: *mut *mut TplOp,
                               mode: *mut c_int) -> c_int;
    fn tpl_operand_key(n: i64, ptr_arr: *const c_void, ptr_len: usize, ptr_elem: usize,
                       idx_arr: *const c_void, idx_len: usize, idx_elem: usize,
                       vals: *const f64, nnz: usize, samples: usize, key: *mut u64) -> c_int;
}

fn cstr(p: *const c_char) -> String {
    if p.is_null() {
        return String::new();
    }
    unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

/// tpl_status -> LanczosErrorKind, rebuilt from the variant's FIELDS (not by parsing the
/// message): the caller gets the reference's own variant, so `Display` and `PartialEq`
/// behave exactly as in src/error.rs:20-66.
fn check(st: c_int) -> Result<(), LanczosError> {
    if st == 0 {
        return Ok(());
    }
    let mut d = std::mem::MaybeUninit::<TplErrorDetail>::zeroed();
    let d = unsafe {
        tpl_last_error_detail(d.as_mut_ptr());
        d.assume_init()
    };
    let kind = match st {
        1 => LanczosErrorKind::Breakdown { k: d.breakdown_step as usize },
        2 => LanczosErrorKind::DimensionMismatch {
            operator_cols: d.operator_cols as usize,
            vector_rows: d.vector_rows as usize,
        },
        3 => LanczosErrorKind::InputError(cstr(d.inner)),
        4 => LanczosErrorKind::ParameterMismatch {
            param_name: cstr(d.param_name),
            expected: d.expected as usize,
            actual: d.actual as usize,
        },
        // the built-in exp's only failure is non-convergence (include/tpl.h tpl_ftk_exp)
        5 => LanczosErrorKind::EvdError(faer::linalg::evd::EvdError::NoConvergence),
        6 => LanczosErrorKind::SolverError(cstr(d.inner)),
        // Engine-only statuses (>= 100: argument, device, memory, loader) have no
        // LanczosErrorKind; they surface as SolverError with the engine's message.
        _ => LanczosErrorKind::SolverError(cstr(d.message)),
    };
    Err(LanczosError(kind))
}

/// Device-resident symmetric CSR operator (the faer `SparseColMatRef<usize, f64>` the
/// binaries build, src/utils/data_loader.rs:211-259; symmetric, so CSC == CSR).
pub struct HipCsrOp {
    ctx: *mut TplCtx,
    op: *mut TplOp,
    /// this operator's rows: all of A, or this rank's part of a partitioned A
    n: usize,
    /// One engine call at a time per operator (include/tpl.h: not re-entrant); this is
    /// what makes the operator `Sync`, as faer's `LinOp` requires. The operators of one
    /// communicator share ONE lock (their HipDist's): they share its stream and its RCCL
    /// communicator, so two of them must never capture graphs or issue collectives at once.
    lock: Arc<Mutex<()>>,
    /// partitioned: the communicator, kept alive until the operator is destroyed
    dist: Option<Arc<HipDist>>,
}

// SAFETY: the handles are only used under `lock`, and the engine's per-thread error
// text is read by `check` on the calling thread, inside the same critical section.
unsafe impl Send for HipCsrOp {}
unsafe impl Sync for HipCsrOp {}

impl core::fmt::Debug for HipCsrOp {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        f.debug_struct("HipCsrOp").field("n", &self.n).finish()
    }
}

/// The compact CSC arrays of `a` (faer allows non-compact storage: `col_nnz`), with the
/// engine's index types; A is symmetric, so these are also its CSR arrays.
fn compact_arrays(a: SparseColMatRef<'_, usize, f64>) -> (Vec<i64>, Vec<i32>, Vec<f64>) {
    let sym = a.symbolic();
    let mut rp = Vec::with_capacity(a.ncols() + 1);
    let mut ci = Vec::new();
    let mut v = Vec::new();
    rp.push(0i64);
    for j in 0..a.ncols() {
        ci.extend(sym.row_idx_of_col_raw(j).iter().map(|&r| r as i32));
        v.extend_from_slice(a.val_of_col(j));
        rp.push(ci.len() as i64);
    }
    (rp, ci, v)
}

impl HipCsrOp {
    /// Upload `a` once (the zero-overhead form: pass `&op` to the solvers below; no
    /// per-call host work beyond the call itself).
    pub fn from_csc(a: SparseColMatRef<'_, usize, f64>, device: i32)
                    -> Result<Self, LanczosError> {
        if a.nrows() != a.ncols() {
            return Err(LanczosError(LanczosErrorKind::DimensionMismatch {
                operator_cols: a.ncols(),
                vector_rows: a.nrows(),
            }));
        }
        let (rp, ci, v) = compact_arrays(a);
        Self::from_arrays(a.nrows(), &rp, &ci, &v, device)
    }

    fn from_arrays(n: usize, rp: &[i64], ci: &[i32], v: &[f64], device: i32)
                   -> Result<Self, LanczosError> {
        let mut ctx = std::ptr::null_mut();
        let mut op = std::ptr::null_mut();
        unsafe {
            check(tpl_ctx_create(device, &mut ctx))?;
            if let Err(e) = check(tpl_op_create_csr(ctx, n as i64, ci.len() as i64, rp.as_ptr(),
                                                    ci.as_ptr(), v.as_ptr(), &mut op)) {
                tpl_ctx_destroy(ctx);
                return Err(e);
            }
        }
        Ok(Self { ctx, op, n, lock: Arc::new(Mutex::new(())), dist: None })
    }

    /// This rank's part of the symmetric `a` over `dist`'s ranks (every rank passes the
    /// same whole matrix; collective: all ranks make the same calls in the same order).
    /// `Partition::Replicated` (the KKT form: tpl_dist_op_create_replicated, refused with
    /// a SolverError when a short row references another rank's short rows),
    /// `Partition::Halo` (any symmetric matrix: tpl_dist_op_create_halo over the
    /// byte-balanced row blocks), `Partition::Auto` (tpl_dist_op_create_auto: the rule the
    /// Python and C++ bindings share — replicated when it applies, else halo when the halo
    /// is at most half the widest block, else plain row blocks).
    pub fn partitioned(a: SparseColMatRef<'_, usize, f64>, dist: &Arc<HipDist>,
                       partition: Partition) -> Result<Self, LanczosError> {
        if a.nrows() != a.ncols() {
            return Err(LanczosError(LanczosErrorKind::DimensionMismatch {
                operator_cols: a.ncols(),
                vector_rows: a.nrows(),
            }));
        }
        let (rp, ci, v) = compact_arrays(a);
        let n = a.nrows() as i64;
        let mut op = std::ptr::null_mut();
        let _g = dist.lock.lock().unwrap();  // the communicator's stream and comm
        unsafe {
            match partition {
                Partition::Replicated => check(tpl_dist_op_create_replicated(
                    dist.d, n, rp.as_ptr(), ci.as_ptr(), v.as_ptr(), &mut op))?,
                Partition::Halo => check(tpl_dist_op_create_halo(
                    dist.d, n, std::ptr::null(), rp.as_ptr(), ci.as_ptr(), v.as_ptr(), &mut op))?,
                Partition::Auto => check(tpl_dist_op_create_auto(
                    dist.d, n, rp.as_ptr(), ci.as_ptr(), v.as_ptr(), &mut op,
                    std::ptr::null_mut()))?,
            }
            let nl = tpl_op_nrows(op) as usize;
            Ok(Self { ctx: std::ptr::null_mut(), op, n: nl, lock: dist.lock.clone(),
                      dist: Some(dist.clone()) })
        }
    }

    /// The global row of each entry of this operator's vectors (`b` and `x` of the
    /// functions below hold these rows, in this order).
    pub fn local_rows(&self) -> Result<Vec<i64>, LanczosError> {
        let mut rows = vec![0i64; self.n.max(1)];
        let _g = self.lock.lock().unwrap();
        unsafe { check(tpl_op_local_rows(self.op, rows.as_mut_ptr()))? };
        rows.truncate(self.n);
        Ok(rows)
    }

    pub fn nrows(&self) -> usize {
        self.n
    }

    /// y = A x for one host vector (the per-call compatibility path).
    pub fn apply_vec(&self, x: &[f64]) -> Result<Vec<f64>, LanczosError> {
        let mut y = vec![0.0; self.n];
        let _g = self.lock.lock().unwrap();
        unsafe { check(tpl_op_apply(self.op, x.as_ptr(), y.as_mut_ptr(), TPL_MEM_HOST))? };
        Ok(y)
    }
}

impl Drop for HipCsrOp {
    fn drop(&mut self) {
        unsafe {
            tpl_op_destroy(self.op);
            if !self.ctx.is_null() {
                tpl_ctx_destroy(self.ctx);
            }
        }
        // `dist` (the communicator) is released after the operator, when its field drops
    }
}

/// How [`HipCsrOp::partitioned`] splits the matrix over the ranks (include/tpl.h).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Partition {
    Replicated,
    Halo,
    Auto,
}

/// One rank's RCCL communicator over xGMI (tpl_dist_create).
pub struct HipDist {
    d: *mut TplDist,
    /// Held around every engine call that touches this communicator or its stream: every
    /// operator built on it takes THIS lock as its own (HipCsrOp::lock), so two operators
    /// sharing an `Arc<HipDist>` never capture graphs or issue collectives concurrently.
    lock: Arc<Mutex<()>>,
}

// SAFETY: the handle is only used under `lock` (operator creation here, every solver call
// through the operators, which share the lock).
unsafe impl Send for HipDist {}
unsafe impl Sync for HipDist {}

impl HipDist {
    /// Rank 0: the id every rank passes to [`HipDist::new`].
    pub fn unique_id() -> Result<[u8; TPL_DIST_ID_BYTES], LanczosError> {
        let mut id = [0u8; TPL_DIST_ID_BYTES];
        unsafe { check(tpl_dist_unique_id(id.as_mut_ptr()))? };
        Ok(id)
    }

    /// This process's rank of `nranks` on GPU `device` (collective over the ranks).
    pub fn new(device: i32, rank: i32, nranks: i32, id: &[u8; TPL_DIST_ID_BYTES])
               -> Result<std::sync::Arc<Self>, LanczosError> {
        let mut d = std::ptr::null_mut();
        unsafe { check(tpl_dist_create(device, rank, nranks, id.as_ptr(), &mut d))? };
        Ok(Arc::new(Self { d, lock: Arc::new(Mutex::new(())) }))
    }
}

impl Drop for HipDist {
    fn drop(&mut self) {
        unsafe {
            tpl_dist_destroy(self.d);
        }
    }
}

/// faer's `LinOp<f64>` over `tpl_op_apply`: a compatibility path, so the reference's own
/// generic code (e.g. `solvers::lanczos` itself) can run with the product on the GPU. The
/// solvers of this module never use it — they hand the whole recurrence to the engine.
/// (For a partitioned operator it is this rank's block of rows, a collective call.)
impl LinOp<f64> for HipCsrOp {
    fn apply_scratch(&self, _rhs_ncols: usize, _par: Par) -> StackReq {
        StackReq::EMPTY // the engine's workspace lives in HBM
    }
    fn nrows(&self) -> usize {
        self.n
    }
    fn ncols(&self) -> usize {
        self.n
    }
    fn apply(&self, mut out: MatMut<'_, f64>, rhs: MatRef<'_, f64>, _par: Par,
             _stack: &mut MemStack) {
        // faer's own products panic on a shape mismatch; so does this one
        assert!(rhs.nrows() == self.n && out.nrows() == self.n && out.ncols() == rhs.ncols());
        let mut x = vec![0.0; self.n];
        for j in 0..rhs.ncols() {
            for i in 0..self.n {
                x[i] = rhs[(i, j)];
            }
            let y = self.apply_vec(&x).unwrap_or_else(|e| panic!("tpl_op_apply: {e}"));
            for i in 0..self.n {
                out[(i, j)] = y[i];
            }
        }
    }
    fn conj_apply(&self, out: MatMut<'_, f64>, rhs: MatRef<'_, f64>, par: Par,
                  stack: &mut MemStack) {
        self.apply(out, rhs, par, stack) // real: conj(A) = A
    }
}

/// What the functions below accept as `operator`.
pub trait HipOperand {
    /// Runs `g` on the device operator holding this matrix.
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError>;
}

impl HipOperand for HipCsrOp {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        Ok(g(self))
    }
}

thread_local! {
    /// The last faer matrix uploaded on this thread: (operand key, operator).
    static UPLOADED: RefCell<Option<([u64; 2], HipCsrOp)>> = const { RefCell::new(None) };
}

/// Words of each array the operand key samples (include/tpl.h tpl_operand_key).
const KEY_SAMPLES: usize = 4096;

/// The identity of `a` as this thread last uploaded it (tpl_operand_key): its three
/// arrays' addresses and lengths, its dimension, and a checksum of 3 x (KEY_SAMPLES + 16)
/// words — O(KEY_SAMPLES) host work per solver call (≈10 µs), not the O(nnz) copy and
/// hash of the whole matrix (that cost sat inside the reference's own timing
/// window, src/bin/tradeoff.rs:267-286).
fn operand_key(a: SparseColMatRef<'_, usize, f64>) -> Result<[u64; 2], LanczosError> {
    let sym = a.symbolic();
    let (cp, ri, v) = (sym.col_ptr(), sym.row_idx(), a.val());
    let w = std::mem::size_of::<usize>();
    let mut key = [0u64; 2];
    unsafe {
        check(tpl_operand_key(a.nrows() as i64, cp.as_ptr() as *const c_void, cp.len(), w,
                              ri.as_ptr() as *const c_void, ri.len(), w, v.as_ptr(), v.len(),
                              KEY_SAMPLES, key.as_mut_ptr()))?
    };
    Ok(key)
}

/// Forget this thread's upload of a faer matrix: the next solver call uploads it again.
/// Needed only after changing a matrix's values IN PLACE (same arrays, same sizes) between
/// calls — the key sees new arrays, new sizes and any change in its sampled words, not a
/// change of every single word. `HipCsrOp::from_csc` (upload once, pass `&op`) has no
/// per-call host cost at all and is the form to use in new code.
pub fn refresh_uploaded() {
    UPLOADED.with(|cell| *cell.borrow_mut() = None);
}

/// The reference's call sites pass `&a.as_ref()`: upload on first use (device 0, or
/// `TPL_DEVICE`), reuse while the operand key is unchanged (per call: the key, no copy).
impl<'a> HipOperand for SparseColMatRef<'a, usize, f64> {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        if self.nrows() != self.ncols() {
            return Err(LanczosError(LanczosErrorKind::DimensionMismatch {
                operator_cols: self.ncols(),
                vector_rows: self.nrows(),
            }));
        }
        let key = operand_key(*self)?;
        UPLOADED.with(|cell| {
            let mut slot = cell.borrow_mut();
            if !matches!(&*slot, Some((k, _)) if *k == key) {
                *slot = None; // free the previous upload before the new one
                let device = std::env::var("TPL_DEVICE").ok()
                    .and_then(|s| s.parse().ok()).unwrap_or(0);
                *slot = Some((key, HipCsrOp::from_csc(*self, device)?));
            }
            Ok(g(&slot.as_ref().unwrap().1))
        })
    }
}

impl HipOperand for SparseColMat<usize, f64> {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        self.as_ref().with_hip_op(g)
    }
}

/// Device-resident dense symmetric operator (tpl_op_create_dense): faer's `LinOp<f64>` for the
/// dense `Mat<f64>` of tests/correctness.rs and src/bin/dense_tradeoff.rs. The engine handle
/// is the one every solver of this module takes, so the operator is its handle and nothing
/// else: every single-right-hand-side function below accepts `&HipDenseOp`; the `*_batch*`
/// ones return the engine's refusal (TPL_ERR_UNSUPPORTED, as a SolverError).
#[derive(Debug)]
pub struct HipDenseOp {
    handle: HipCsrOp,
}

impl HipDenseOp {
    /// Upload the symmetric `a` once. A is symmetric, so a column-major `Mat` (faer's own
    /// layout, row stride 1) is read in place as its row-major transpose with lda = the
    /// column stride; any other striding is copied first.
    pub fn from_mat(a: MatRef<'_, f64>, device: i32) -> Result<Self, LanczosError> {
        if a.nrows() != a.ncols() {
            return Err(LanczosError(LanczosErrorKind::DimensionMismatch {
                operator_cols: a.ncols(),
                vector_rows: a.nrows(),
            }));
        }
        let n = a.nrows();
        let (rs, cs) = (a.row_stride(), a.col_stride());
        let copy: Vec<f64>;
        let (ptr, lda) = if n > 0 && rs == 1 && cs >= n as isize {
            (a.as_ptr(), cs as i64)
        } else if n > 0 && cs == 1 && rs >= n as isize {
            (a.as_ptr(), rs as i64)
        } else {
            copy = (0..n * n).map(|e| a[(e / n, e % n)]).collect();
            (copy.as_ptr(), n as i64)
        };
        let mut ctx = std::ptr::null_mut();
        let mut op = std::ptr::null_mut();
        unsafe {
            check(tpl_ctx_create(device, &mut ctx))?;
            if let Err(e) = check(tpl_op_create_dense(ctx, n as i64, ptr, lda, TPL_MEM_HOST,
                                                      &mut op)) {
                tpl_ctx_destroy(ctx);
                return Err(e);
            }
        }
        Ok(Self { handle: HipCsrOp { ctx, op, n, lock: Arc::new(Mutex::new(())), dist: None } })
    }

    pub fn nrows(&self) -> usize {
        self.handle.n
    }

    /// y = A x for one host vector (the per-call compatibility path).
    pub fn apply_vec(&self, x: &[f64]) -> Result<Vec<f64>, LanczosError> {
        self.handle.apply_vec(x)
    }
}

/// faer's `LinOp<f64>` over `tpl_op_apply`, as for [`HipCsrOp`].
impl LinOp<f64> for HipDenseOp {
    fn apply_scratch(&self, rhs_ncols: usize, par: Par) -> StackReq {
        self.handle.apply_scratch(rhs_ncols, par)
    }
    fn nrows(&self) -> usize {
        self.handle.n
    }
    fn ncols(&self) -> usize {
        self.handle.n
    }
    fn apply(&self, out: MatMut<'_, f64>, rhs: MatRef<'_, f64>, par: Par, stack: &mut MemStack) {
        LinOp::apply(&self.handle, out, rhs, par, stack)
    }
    fn conj_apply(&self, out: MatMut<'_, f64>, rhs: MatRef<'_, f64>, par: Par,
                  stack: &mut MemStack) {
        LinOp::apply(&self.handle, out, rhs, par, stack) // real: conj(A) = A
    }
}

impl HipOperand for HipDenseOp {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        Ok(g(&self.handle))
    }
}

thread_local! {
    /// The last dense faer matrix uploaded on this thread: (operand key, operator).
    static UPLOADED_DENSE: RefCell<Option<([u64; 4], HipDenseOp)>> = const { RefCell::new(None) };
}

/// The identity of a dense `a` as this thread last uploaded it: its address, dimension and
/// strides, and an FNV-1a checksum of KEY_SAMPLES evenly spaced entries — O(KEY_SAMPLES) host
/// work per solver call, as for the sparse operand (`refresh_uploaded_dense` after changing
/// values in place).
fn dense_operand_key(a: MatRef<'_, f64>) -> [u64; 4] {
    let n = a.nrows();
    let mut h = 0xcbf29ce484222325u64;
    let total = n * n;
    let samples = KEY_SAMPLES.min(total);
    for s in 0..samples {
        let e = ((s as u128 * total as u128) / samples as u128) as usize;
        h = (h ^ a[(e / n, e % n)].to_bits()).wrapping_mul(0x100000001b3);
    }
    [a.as_ptr() as usize as u64, n as u64,
     (a.row_stride() as i64 as u64) ^ ((a.col_stride() as i64 as u64) << 32), h]
}

/// Forget this thread's upload of a dense faer matrix: the next solver call uploads it again.
pub fn refresh_uploaded_dense() {
    UPLOADED_DENSE.with(|cell| *cell.borrow_mut() = None);
}

/// The reference's dense call sites (src/bin/dense_tradeoff.rs, tests/correctness.rs) pass
/// `&a.as_ref()` of a `Mat<f64>`: upload on first use (device 0, or `TPL_DEVICE`), reuse while
/// the operand key is unchanged.
impl<'a> HipOperand for MatRef<'a, f64> {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        let key = dense_operand_key(*self);
        UPLOADED_DENSE.with(|cell| {
            let mut slot = cell.borrow_mut();
            if !matches!(&*slot, Some((k, _)) if *k == key) {
                *slot = None; // free the previous upload before the new one
                let device = std::env::var("TPL_DEVICE").ok()
                    .and_then(|s| s.parse().ok()).unwrap_or(0);
                *slot = Some((key, HipDenseOp::from_mat(*self, device)?));
            }
            Ok(g(&slot.as_ref().unwrap().1.handle))
        })
    }
}

impl HipOperand for Mat<f64> {
    fn with_hip_op<R, G: FnOnce(&HipCsrOp) -> R>(&self, g: G) -> Result<R, LanczosError> {
        self.as_ref().with_hip_op(g)
    }
}

/// The FnMut closure of `solvers::lanczos*` behind the C callback (called once).
unsafe extern "C" fn ftk_trampoline<F>(a: *const f64, na: usize, b: *const f64, nb: usize,
                                       y: *mut f64, cap: usize, len: *mut usize,
                                       err: *mut c_char, ecap: usize, user: *mut c_void) -> c_int
where
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let f = &mut *(user as *mut F);
    let sa = if na == 0 { &[][..] } else { std::slice::from_raw_parts(a, na) };
    let sb = if nb == 0 { &[][..] } else { std::slice::from_raw_parts(b, nb) };
    match f(sa, sb) {
        Ok(m) => {
            *len = m.nrows();
            if m.ncols() != 1 || m.nrows() > cap {
                // the engine reports ParameterMismatch (src/solvers.rs:78-85,158-165)
                *len = if m.nrows() != na { m.nrows() } else { na + 1 };
                return 0;
            }
            for i in 0..m.nrows() {
                *y.add(i) = m[(i, 0)];
            }
            0
        }
        Err(e) => {
            let s = e.to_string();
            let n = s.len().min(ecap.saturating_sub(1));
            std::ptr::copy_nonoverlapping(s.as_ptr() as *const c_char, err, n);
            *err.add(n) = 0;
            1
        }
    }
}

/// `LanczosCallback` behind `tpl_step_cb`. The engine hands V_k as a DEVICE pointer; the
/// host copy grows by the new columns only (O(nk) copied over the whole run, the same
/// memory the reference's stored basis takes), and the view the callback sees is the
/// reference's: n x k, column-major, plus T_k's scalars.
struct StepState<'c> {
    cb: &'c mut LanczosCallback<f64>,
    v: Vec<f64>,
    filled: usize,
    failed: Option<LanczosError>,
}

unsafe extern "C" fn step_trampoline(k: usize, v_dev: *const f64, n: i64, al: *const f64,
                                     na: usize, be: *const f64, nb: usize,
                                     user: *mut c_void) -> c_int {
    let st = &mut *(user as *mut StepState<'_>);
    let n = n as usize;
    if k > st.filled {
        let off = st.filled * n;
        let bytes = (k - st.filled) * n * std::mem::size_of::<f64>();
        if let Err(e) = check(tpl_copy_to_host(st.v.as_mut_ptr().add(off) as *mut c_void,
                                               v_dev.add(off) as *const c_void, bytes)) {
            st.failed = Some(e);
            return 0; // stop; the error is returned after the call
        }
        st.filled = k;
    }
    let view = TridiagonalSystemView {
        alphas: if na == 0 { &[][..] } else { std::slice::from_raw_parts(al, na) },
        betas: if nb == 0 { &[][..] } else { std::slice::from_raw_parts(be, nb) },
        steps_taken: k,
    };
    let v_k = MatRef::from_column_major_slice(&st.v[..k * n], n, k);
    (st.cb)(k, v_k, &view) as c_int
}

fn column(b: MatRef<'_, f64>) -> Vec<f64> {
    (0..b.nrows()).map(|i| b[(i, 0)]).collect()
}

fn column_major(v: &[f64], n: usize, cols: usize) -> Mat<f64> {
    Mat::from_fn(n, cols, |i, j| v[i + j * n])
}

/// Drop-in for `solvers::lanczos` (src/solvers.rs:46-107): V_k stays in HBM, x = ||b|| V_k y'.
pub fn lanczos<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    mut f_tk_solver: F,
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    let bv = column(b);
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos(op.op, bv.as_ptr(), bv.len() as i64, k, ftk_trampoline::<F>,
                              &mut f_tk_solver as *mut F as *mut c_void, x.as_mut_ptr(),
                              TPL_MEM_HOST))?;
        }
        Ok(Mat::from_fn(op.n, 1, |i, _| x[i]))
    })?
}

/// Drop-in for `solvers::lanczos_two_pass` (src/solvers.rs:133-175).
pub fn lanczos_two_pass<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    mut f_tk_solver: F,
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    let bv = column(b);
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_two_pass(op.op, bv.as_ptr(), bv.len() as i64, k,
                                       ftk_trampoline::<F>,
                                       &mut f_tk_solver as *mut F as *mut c_void,
                                       x.as_mut_ptr(), TPL_MEM_HOST))?;
        }
        Ok(Mat::from_fn(op.n, 1, |i, _| x[i]))
    })?
}

/// Drop-in for `algorithms::lanczos::lanczos_standard` (src/algorithms/lanczos.rs:55-156):
/// V_k is built in HBM and returned as the reference's `Mat`; the callback, when given,
/// sees exactly the reference's arguments and may stop the run early (a stop at step j
/// returns the j-step result, include/tpl.h `tpl_step_cb`).
pub fn lanczos_standard(
    operator: &impl HipOperand,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    callback: Option<&mut LanczosCallback<f64>>,
) -> Result<LanczosOutput<f64>, LanczosError> {
    let _ = stack;
    let bv = column(b);
    operator.with_hip_op(|op| {
        let n = op.n;
        let (mut al, mut be) = (vec![0.0; k.max(1)], vec![0.0; k.max(1)]);
        let (mut steps, mut bn) = (0usize, 0.0f64);
        let mut v = vec![0.0; n * k];
        let mut state = callback.map(|cb| StepState { cb, v: vec![0.0; n * k], filled: 0,
                                                      failed: None });
        let (cb, user): (Option<StepCb>, *mut c_void) = match state.as_mut() {
            Some(s) => (Some(step_trampoline as StepCb), s as *mut StepState<'_> as *mut c_void),
            None => (None, std::ptr::null_mut()),
        };
        let _g = op.lock.lock().unwrap();
        let st = unsafe {
            tpl_lanczos_standard(op.op, bv.as_ptr(), bv.len() as i64, k, al.as_mut_ptr(),
                                 be.as_mut_ptr(), &mut steps, &mut bn, v.as_mut_ptr(),
                                 TPL_MEM_HOST, 0, cb, user)
        };
        if let Some(e) = state.and_then(|s| s.failed) {
            return Err(e);
        }
        check(st)?;
        al.truncate(steps);
        be.truncate(steps.saturating_sub(1));
        Ok(LanczosOutput {
            v_k: column_major(&v, n, steps),
            decomposition: LanczosDecomposition { alphas: al, betas: be, steps_taken: steps,
                                                  b_norm: bn },
        })
    })?
}

/// Drop-in for `algorithms::lanczos_two_pass::lanczos_pass_one` (lanczos_two_pass.rs:65-110).
pub fn lanczos_pass_one(
    operator: &impl HipOperand,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
) -> Result<LanczosDecomposition<f64>, LanczosError> {
    let _ = stack;
    let bv = column(b);
    operator.with_hip_op(|op| {
        let (mut al, mut be) = (vec![0.0; k.max(1)], vec![0.0; k.max(1)]);
        let (mut steps, mut bn) = (0usize, 0.0f64);
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_pass_one(op.op, bv.as_ptr(), bv.len() as i64, k, al.as_mut_ptr(),
                                       be.as_mut_ptr(), &mut steps, &mut bn, TPL_MEM_HOST))?;
        }
        al.truncate(steps);
        be.truncate(steps.saturating_sub(1));
        Ok(LanczosDecomposition { alphas: al, betas: be, steps_taken: steps, b_norm: bn })
    })?
}

/// Both pass-two entry points: `v_out` = the regenerated basis (with_basis) or none.
fn pass_two(op: &HipCsrOp, b: MatRef<'_, f64>, d: &LanczosDecomposition<f64>,
            y_k: MatRef<'_, f64>, with_basis: bool)
            -> Result<(Mat<f64>, Option<Mat<f64>>), LanczosError> {
    let bv = column(b);
    let yv = column(y_k);
    let n = op.n;
    let mut x = vec![0.0; n];
    let mut v = if with_basis { vec![0.0; n * d.steps_taken] } else { Vec::new() };
    let v_ptr = if with_basis { v.as_mut_ptr() } else { std::ptr::null_mut() };
    let _g = op.lock.lock().unwrap();
    unsafe {
        check(tpl_lanczos_pass_two(op.op, bv.as_ptr(), bv.len() as i64, d.alphas.as_ptr(),
                                   d.alphas.len(), d.betas.as_ptr(), d.betas.len(),
                                   d.steps_taken, d.b_norm, yv.as_ptr(), yv.len(),
                                   x.as_mut_ptr(), v_ptr, TPL_MEM_HOST))?;
    }
    let basis = with_basis.then(|| column_major(&v, n, d.steps_taken));
    Ok((Mat::from_fn(n, 1, |i, _| x[i]), basis))
}

/// Drop-in for `algorithms::lanczos_two_pass::lanczos_pass_two` (:128-140); y_k already
/// scaled by ||b||.
pub fn lanczos_pass_two(
    operator: &impl HipOperand,
    b: MatRef<'_, f64>,
    decomposition: &LanczosDecomposition<f64>,
    y_k: MatRef<'_, f64>,
    stack: &mut MemStack,
) -> Result<Mat<f64>, LanczosError> {
    let _ = stack;
    operator.with_hip_op(|op| pass_two(op, b, decomposition, y_k, false).map(|(x, _)| x))?
}

/// Drop-in for `algorithms::lanczos_two_pass::lanczos_pass_two_with_basis` (:149-166):
/// x_k and the regenerated basis V'_k (bitwise the one pass one / `lanczos_standard`
/// generates on the device: DESIGN.md §5 P1).
pub fn lanczos_pass_two_with_basis(
    operator: &impl HipOperand,
    b: MatRef<'_, f64>,
    decomposition: &LanczosDecomposition<f64>,
    y_k: MatRef<'_, f64>,
    stack: &mut MemStack,
) -> Result<LanczosPassTwoOutput<f64>, LanczosError> {
    let _ = stack;
    operator.with_hip_op(|op| {
        pass_two(op, b, decomposition, y_k, true)
            .map(|(x_k, v_k)| LanczosPassTwoOutput { x_k, v_k: v_k.unwrap() })
    })?
}

/// The two multi-function solves: `call` is tpl_lanczos_two_pass_multi or tpl_lanczos_multi.
type MultiFn = unsafe extern "C" fn(*mut TplOp, *const f64, i64, usize, *const FtkFn,
                                    *mut *mut c_void, usize, *mut f64, c_int) -> c_int;

fn solve_multi<O, F>(operator: &O, b: MatRef<'_, f64>, k: usize, f_tk_solvers: &mut [F],
                     call: MultiFn) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let bv = column(b);
    let m = f_tk_solvers.len();
    let fns: Vec<FtkFn> = vec![ftk_trampoline::<F> as FtkFn; m];
    let mut users: Vec<*mut c_void> =
        f_tk_solvers.iter_mut().map(|f| f as *mut F as *mut c_void).collect();
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * m];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(call(op.op, bv.as_ptr(), bv.len() as i64, k, fns.as_ptr(), users.as_mut_ptr(),
                       m, x.as_mut_ptr(), TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, m))
    })?
}

/// f_1(A) b ... f_m(A) b by ONE two-pass run (no reference counterpart: its `f_tk_solver`
/// returns a `Mat` and rejects ncols != 1): pass one once, every closure once in index
/// order, one pass two. Column i is bitwise `lanczos_two_pass` with `f_tk_solvers[i]`.
pub fn lanczos_two_pass_multi<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    f_tk_solvers: &mut [F],
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    solve_multi(operator, b, k, f_tk_solvers, tpl_lanczos_two_pass_multi)
}

/// exp(t_i A) b for the times `ts` by ONE two-pass run (no reference counterpart): pass one
/// once, every exp(t_i T_k) e_1 at once on the device (a time the device hands back runs the
/// native host `tpl_ftk_exp_t`), one pass two. Returns the n x m result and, per time, whether
/// the device's y was used.
pub fn lanczos_two_pass_exp_times<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    ts: &[f64],
    stack: &mut MemStack,
) -> Result<(Mat<f64>, Vec<bool>), LanczosError> {
    let _ = stack;
    let bv = column(b);
    let m = ts.len();
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * m];
        let mut on = vec![0i32; m];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_two_pass_exp_times(op.op, bv.as_ptr(), bv.len() as i64, k,
                                                 ts.as_ptr(), m, x.as_mut_ptr(), TPL_MEM_HOST,
                                                 on.as_mut_ptr()))?;
        }
        Ok((column_major(&x, op.n, m), on.iter().map(|&v| v != 0).collect()))
    })?
}

/// What `lanczos_two_pass_inv_tol` reports beside x: the steps of the iterate it returns
/// (m*), whether the tolerance was met, and the residual history up to the last entry formed.
pub struct InvTolInfo {
    pub steps: usize,
    pub converged: bool,
    pub residuals: Vec<f64>,
}

/// A^{-1} b by the two-pass solve with the built-in inv, stopped at the first step m* <= kmax
/// whose relative Lanczos residual is <= `tol` (no reference counterpart): bitwise
/// `lanczos_two_pass` with k = m* and the native inv. On one GPU within the device-inv bounds
/// the call is one graph and the stop is taken on the device.
pub fn lanczos_two_pass_inv_tol<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    kmax: usize,
    tol: f64,
    stack: &mut MemStack,
) -> Result<(Mat<f64>, InvTolInfo), LanczosError> {
    let _ = stack;
    let bv = column(b);
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n];
        let mut res = vec![0.0; kmax.max(1)];
        let (mut steps, mut res_len, mut converged) = (0usize, 0usize, 0i32);
        let _g = op.lock.lock().unwrap();
        // SAFETY: b has n entries, x n, res kmax; the scalars outlive the call.
        unsafe {
            check(tpl_lanczos_two_pass_inv_tol(op.op, bv.as_ptr(), bv.len() as i64, kmax, tol,
                                               x.as_mut_ptr(), TPL_MEM_HOST, &mut steps,
                                               &mut converged, res.as_mut_ptr(), &mut res_len))?;
        }
        res.truncate(res_len);
        Ok((column_major(&x, op.n, 1),
            InvTolInfo { steps, converged: converged != 0, residuals: res }))
    })?
}

/// The residual history of the inverse solve (`tpl_ftk_inv_residuals`): entry m - 1 is the
/// relative Lanczos residual of the m-step iterate, m = 1 ..= min(alphas.len(), betas.len()).
pub fn inv_residuals(alphas: &[f64], betas: &[f64]) -> Vec<f64> {
    let mut res = vec![0.0; alphas.len().min(betas.len())];
    let mut len = 0usize;
    // SAFETY: the slices' own lengths; res holds min(n_alphas, n_betas) entries.
    let rc = unsafe {
        tpl_ftk_inv_residuals(alphas.as_ptr(), alphas.len(), betas.as_ptr(), betas.len(),
                              res.as_mut_ptr(), res.len(), &mut len)
    };
    assert_eq!(rc, 0, "tpl_ftk_inv_residuals");
    res.truncate(len);
    res
}

/// What `lanczos_two_pass_shifted_inv_tol` reports beside x, per shift: the steps of the
/// iterate in its column (m*_i), whether the tolerance was met, and the residual history up to
/// the last entry formed.
pub struct ShiftedInvTolInfo {
    pub steps: Vec<usize>,
    pub converged: Vec<bool>,
    pub residuals: Vec<Vec<f64>>,
}

/// (A + sigma_i I)^{-1} b for the shifts `sigmas` by ONE two-pass run on A (no reference
/// counterpart), each shift stopped at the first step m*_i whose relative Lanczos residual
/// (`inv_residuals` on alphas + sigma_i) is <= `tol`: column i of the n x m result is bitwise
/// `lanczos_pass_two` on A's decomposition cut to m*_i steps. On one GPU within the device-inv
/// bounds the call is one graph: one elimination lane per shift, the stop taken on the device.
pub fn lanczos_two_pass_shifted_inv_tol<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    kmax: usize,
    sigmas: &[f64],
    tol: f64,
    stack: &mut MemStack,
) -> Result<(Mat<f64>, ShiftedInvTolInfo), LanczosError> {
    let _ = stack;
    let bv = column(b);
    let m = sigmas.len();
    let ldr = kmax.max(1);
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * m];
        let mut res = vec![0.0; ldr * m.max(1)];
        let mut steps = vec![0usize; m.max(1)];
        let mut res_len = vec![0usize; m.max(1)];
        let mut converged = vec![0i32; m.max(1)];
        let _g = op.lock.lock().unwrap();
        // SAFETY: b has n entries, x n m, res kmax m; the per-shift arrays hold m entries.
        unsafe {
            check(tpl_lanczos_two_pass_shifted_inv_tol(op.op, bv.as_ptr(), bv.len() as i64, kmax,
                                                       sigmas.as_ptr(), m, tol, x.as_mut_ptr(),
                                                       TPL_MEM_HOST, steps.as_mut_ptr(),
                                                       converged.as_mut_ptr(), res.as_mut_ptr(),
                                                       res_len.as_mut_ptr()))?;
        }
        let residuals = (0..m).map(|i| res[i * ldr..i * ldr + res_len[i]].to_vec()).collect();
        steps.truncate(m);
        Ok((column_major(&x, op.n, m),
            ShiftedInvTolInfo { steps, converged: converged[..m].iter().map(|&v| v != 0).collect(),
                                residuals }))
    })?
}

/// `lanczos_pass_two` for m coefficient vectors with a per-column cut
/// (`tpl_lanczos_pass_two_multi_cut`): `y` is column-major with leading dimension `ldy`, column
/// i takes its first `col_steps[i]` steps only and is bitwise `lanczos_pass_two` at that count.
pub fn lanczos_pass_two_multi_cut<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    alphas: &[f64],
    betas: &[f64],
    steps: usize,
    b_norm: f64,
    y: &[f64],
    ldy: usize,
    col_steps: &[usize],
) -> Result<Mat<f64>, LanczosError> {
    let bv = column(b);
    let m = col_steps.len();
    assert!(y.len() >= ldy * m, "y holds fewer than ldy * m entries");
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * m];
        let _g = op.lock.lock().unwrap();
        // SAFETY: the slices' own lengths; y has ldy m entries, x n m.
        unsafe {
            check(tpl_lanczos_pass_two_multi_cut(op.op, bv.as_ptr(), bv.len() as i64,
                                                 alphas.as_ptr(), alphas.len(), betas.as_ptr(),
                                                 betas.len(), steps, b_norm, y.as_ptr(), ldy,
                                                 col_steps.as_ptr(), m, x.as_mut_ptr(),
                                                 TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, m))
    })?
}

/// `k_ftk_inv_shifts` alone (`tpl_op_ftk_inv_shifts_device`): (T_n + sigma_i I)^{-1} e_1 for
/// every shift, column-major n x m, unscaled; column i is bitwise the native inv on
/// (alphas + sigma_i, betas).
pub fn ftk_inv_shifts_device<O: HipOperand>(
    operator: &O,
    alphas: &[f64],
    betas: &[f64],
    sigmas: &[f64],
) -> Result<Vec<f64>, LanczosError> {
    let (n, m) = (alphas.len(), sigmas.len());
    operator.with_hip_op(|op| {
        let mut y = vec![0.0; n * m.max(1)];
        let _g = op.lock.lock().unwrap();
        // SAFETY: alphas has n entries, betas at least n - 1 (checked), y n m.
        assert!(betas.len() + 1 >= n, "betas holds fewer than n - 1 entries");
        unsafe {
            check(tpl_op_ftk_inv_shifts_device(op.op, alphas.as_ptr(), n, betas.as_ptr(),
                                               sigmas.as_ptr(), m, y.as_mut_ptr()))?;
        }
        Ok(y)
    })?
}

/// The one-pass sibling of `lanczos_two_pass_multi`: one standard pass, one reconstruction
/// per function.
pub fn lanczos_multi<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    f_tk_solvers: &mut [F],
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    solve_multi(operator, b, k, f_tk_solvers, tpl_lanczos_multi)
}

/// `lanczos_pass_two` for the m columns of `y_k` (steps x m) over one decomposition: the
/// basis is regenerated once; returns n x m.
pub fn lanczos_pass_two_multi(
    operator: &impl HipOperand,
    b: MatRef<'_, f64>,
    decomposition: &LanczosDecomposition<f64>,
    y_k: MatRef<'_, f64>,
    stack: &mut MemStack,
) -> Result<Mat<f64>, LanczosError> {
    let _ = stack;
    let bv = column(b);
    let (rows, m) = (y_k.nrows(), y_k.ncols());
    let yv: Vec<f64> = (0..rows * m).map(|t| y_k[(t % rows, t / rows)]).collect();
    let d = decomposition;
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * m];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_pass_two_multi(op.op, bv.as_ptr(), bv.len() as i64,
                                             d.alphas.as_ptr(), d.alphas.len(),
                                             d.betas.as_ptr(), d.betas.len(), d.steps_taken,
                                             d.b_norm, yv.as_ptr(), rows, m, x.as_mut_ptr(),
                                             TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, m))
    })?
}

/// f(A) b_1 ... f(A) b_s for the s columns of `b` (n x s) by ONE lock-step two-pass run (no
/// reference counterpart: its solver takes one `b`): pass one for all columns together, the
/// closure once per column in column order, one pass two. Column c is bitwise
/// `lanczos_two_pass` of `b`'s column c with the closure evaluated on the host.
pub fn lanczos_two_pass_batch<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    mut f_tk_solver: F,
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    let (n, s) = (b.nrows(), b.ncols());
    let bv: Vec<f64> = (0..n * s).map(|t| b[(t % n, t / n)]).collect();
    let user = &mut f_tk_solver as *mut F as *mut c_void;
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * s];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_two_pass_batch(op.op, bv.as_ptr(), n as i64, s, k,
                                             ftk_trampoline::<F> as FtkFn, user, x.as_mut_ptr(),
                                             TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, s))
    })?
}

/// f_i(A) b_c for the m closures and the s columns of `b` (n x s) by ONE run (no reference
/// counterpart): per group of columns pass one in lock-step, every closure once per column
/// (column by column, the closures in index order), one pass two. Column (c m + i) of the
/// n x (s m) result is bitwise `lanczos_two_pass` of `b`'s column c with `f_tk_solvers[i]`.
pub fn lanczos_two_pass_batch_multi<O, F>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    stack: &mut MemStack,
    f_tk_solvers: &mut [F],
) -> Result<Mat<f64>, LanczosError>
where
    O: HipOperand,
    F: FnMut(&[f64], &[f64]) -> Result<Mat<f64>, anyhow::Error>,
{
    let _ = stack;
    let (n, s) = (b.nrows(), b.ncols());
    let bv: Vec<f64> = (0..n * s).map(|t| b[(t % n, t / n)]).collect();
    let m = f_tk_solvers.len();
    let fns: Vec<FtkFn> = vec![ftk_trampoline::<F> as FtkFn; m];
    let mut users: Vec<*mut c_void> =
        f_tk_solvers.iter_mut().map(|f| f as *mut F as *mut c_void).collect();
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * s * m];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_two_pass_batch_multi(op.op, bv.as_ptr(), n as i64, s, k,
                                                   fns.as_ptr(), users.as_mut_ptr(), m,
                                                   x.as_mut_ptr(), TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, s * m))
    })?
}

/// (A + sigma_i I)^{-1} b_c for the shifts `sigmas` and the s columns of `b` (n x s) by ONE run
/// (no reference counterpart): per group of columns pass one on A in lock-step, every
/// (column, shift) stopped at the first step m*_{c,i} whose relative Lanczos residual is
/// <= `tol`, one pass two cut per result. Column (c m + i) of the n x (s m) result is bitwise
/// column i of `lanczos_two_pass_shifted_inv_tol` for `b`'s column c; the info's entries are
/// in the same order.
pub fn lanczos_two_pass_batch_shifted_inv_tol<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    kmax: usize,
    sigmas: &[f64],
    tol: f64,
    stack: &mut MemStack,
) -> Result<(Mat<f64>, ShiftedInvTolInfo), LanczosError> {
    let _ = stack;
    let (n, s) = (b.nrows(), b.ncols());
    let bv: Vec<f64> = (0..n * s).map(|t| b[(t % n, t / n)]).collect();
    let m = sigmas.len();
    let sm = s * m;
    let ldr = kmax.max(1);
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * sm];
        let mut res = vec![0.0; ldr * sm.max(1)];
        let mut steps = vec![0usize; sm.max(1)];
        let mut res_len = vec![0usize; sm.max(1)];
        let mut converged = vec![0i32; sm.max(1)];
        let _g = op.lock.lock().unwrap();
        // SAFETY: b has n s entries, x n s m, res kmax s m; the other arrays hold s m entries.
        unsafe {
            check(tpl_lanczos_two_pass_batch_shifted_inv_tol(
                op.op, bv.as_ptr(), n as i64, s, kmax, sigmas.as_ptr(), m, tol, x.as_mut_ptr(),
                TPL_MEM_HOST, steps.as_mut_ptr(), converged.as_mut_ptr(), res.as_mut_ptr(),
                res_len.as_mut_ptr()))?;
        }
        let residuals = (0..sm).map(|e| res[e * ldr..e * ldr + res_len[e]].to_vec()).collect();
        steps.truncate(sm);
        Ok((column_major(&x, op.n, sm),
            ShiftedInvTolInfo { steps, converged: converged[..sm].iter().map(|&v| v != 0).collect(),
                                residuals }))
    })?
}

/// The kmax up to which auto mode runs a group of `lanczos_two_pass_batch_shifted_inv_tol` as
/// one graph.
pub fn batch_shifted_inv_tol_auto_k() -> usize {
    // SAFETY: no arguments, no state.
    unsafe { tpl_batch_shifted_inv_tol_auto_k() }
}

/// `tpl_lanczos_pass_two_batch_multi` with a cut per (column, coefficient vector)
/// (`tpl_lanczos_pass_two_batch_multi_cut`): the decompositions as `lanczos_pass_one_batch`
/// wrote them (leading dimension `ld`), `y` column-major ld x (s m), `col_steps[c m + i]` the
/// steps result (c, i) takes (1 ..= steps[c]). Result (c, i) is bitwise `lanczos_pass_two` at
/// that count.
pub fn lanczos_pass_two_batch_multi_cut<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    alphas: &[f64],
    betas: &[f64],
    ld: usize,
    steps: &[usize],
    b_norms: &[f64],
    y: &[f64],
    col_steps: &[usize],
) -> Result<Mat<f64>, LanczosError> {
    let (n, s) = (b.nrows(), b.ncols());
    let bv: Vec<f64> = (0..n * s).map(|t| b[(t % n, t / n)]).collect();
    assert!(s > 0 && col_steps.len() % s == 0, "col_steps holds s m entries");
    let m = col_steps.len() / s;
    assert!(steps.len() == s && b_norms.len() == s, "one step count and one norm per column");
    assert!(alphas.len() >= ld * s && betas.len() >= ld * s && y.len() >= ld * s * m,
            "decomposition arrays hold fewer than ld entries per column");
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * s * m];
        let _g = op.lock.lock().unwrap();
        // SAFETY: the lengths asserted above; x has n s m entries.
        unsafe {
            check(tpl_lanczos_pass_two_batch_multi_cut(
                op.op, bv.as_ptr(), n as i64, s, alphas.as_ptr(), betas.as_ptr(), ld,
                steps.as_ptr(), b_norms.as_ptr(), y.as_ptr(), col_steps.as_ptr(), m,
                x.as_mut_ptr(), TPL_MEM_HOST))?;
        }
        Ok(column_major(&x, op.n, s * m))
    })?
}

/// exp(t_i A) b_c for the times `ts` and the s columns of `b` (n x s) by ONE run (no reference
/// counterpart): per group of columns pass one in lock-step, every exp(t_i T_k) e_1 of every
/// column at once on the device (what it hands back runs the native host `tpl_ftk_exp_t`), one
/// pass two. Returns the n x (s m) result, column (c m + i) = exp(ts[i] A) b_c — bitwise
/// `lanczos_two_pass_exp_times` of `b`'s column c — and, per column of it, whether the device's
/// y was used.
pub fn lanczos_two_pass_batch_exp_times<O: HipOperand>(
    operator: &O,
    b: MatRef<'_, f64>,
    k: usize,
    ts: &[f64],
    stack: &mut MemStack,
) -> Result<(Mat<f64>, Vec<bool>), LanczosError> {
    let _ = stack;
    let (n, s) = (b.nrows(), b.ncols());
    let bv: Vec<f64> = (0..n * s).map(|t| b[(t % n, t / n)]).collect();
    let m = ts.len();
    operator.with_hip_op(|op| {
        let mut x = vec![0.0; op.n * s * m];
        let mut on = vec![0i32; s * m];
        let _g = op.lock.lock().unwrap();
        unsafe {
            check(tpl_lanczos_two_pass_batch_exp_times(op.op, bv.as_ptr(), n as i64, s, k,
                                                       ts.as_ptr(), m, x.as_mut_ptr(),
                                                       TPL_MEM_HOST, on.as_mut_ptr()))?;
        }
        Ok((column_major(&x, op.n, s * m), on.iter().map(|&v| v != 0).collect()))
    })?
}
