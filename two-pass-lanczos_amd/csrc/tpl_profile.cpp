// tpl_profile.cpp — measurement entry points of the C ABI (include/tpl.h): the live
// timing of a solve's passes and sampled launches, the per-kernel profiler with its
// algorithmic byte counts, and the locality order's tuning by it.
#include "tpl_op.h"

using namespace tpl;

extern "C" {

double tpl_kernel_algo_bytes(tpl_op_t op, int kernel) {
  // B_spmv = 12 nnz + 4 (n+1) + 16 n (fp64 value + int32 column per
  // nonzero, int32 row_ptr, x read once, y written once). The fused kernels add the
  // epilogue vectors they must touch (DESIGN.md "Algorithmic bytes").
  if (!op) return 0.0;
  const double n = (double)op->part.n, nnz = (double)op->part.nnz;
  // a dense operator: the stored matrix, padding included, x read once, y written once
  const double spmv = op->dense ? 8.0 * n * (double)op->dense_ld + 16.0 * n
                                : 12.0 * nnz + 4.0 * (n + 1.0) + 16.0 * n;
  switch (kernel) {
    case TPL_KERNEL_SPMV: return spmv;
    case TPL_KERNEL_PASS1_SPMV: return spmv + 8.0 * n;   // + r_{j-1} read (w is the y write)
    case TPL_KERNEL_PASS1_AXPY: return 24.0 * n;         // w, r_j read; r_{j+1} written
    case TPL_KERNEL_PASS1_STEP: return spmv + 8.0 * n + 24.0 * n;
    // + v_{j-1} read; x read and written once per three steps (grouped x updates)
    case TPL_KERNEL_PASS2_SPMV: return spmv + 8.0 * n + 16.0 * n / 3.0;
    case TPL_KERNEL_EXCHANGE_P1:
    case TPL_KERNEL_EXCHANGE_P2: {
      if (!op->dist) return 0.0;
      const double R = (double)op->dist->nranks;
      if (op->part.hybrid) {  // per rank: n_long partials + its chunk alpha partials (y_ld1),
        // then the norm total; pass two: n_long partials + 1
        const double nl = (double)op->lay.lrows.size();
        return kernel == TPL_KERNEL_EXCHANGE_P1 ? 8.0 * R * (op->y_ld1 + 1.0)
                                                : 8.0 * R * (nl + 1.0);
      }
      const double vec = (double)(op->part.halo ? op->part.hH : op->ld);
      // pass one: the alpha and beta totals and one vector part per rank (halo: its halo
      // slot); pass two: the vector part only (the row-block pass two gathers v, no totals)
      return kernel == TPL_KERNEL_EXCHANGE_P1 ? 8.0 * R * (vec + 2.0) : 8.0 * R * vec;
    }
    default: return 0.0;
  }
}

tpl_status tpl_op_enable_timing(tpl_op_t op, int on) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    op->timing = on != 0;
    op->p2_launches = 0;
    op->p1_samples = 0;
  });
}

tpl_status tpl_op_step_samples(tpl_op_t op, double* p1_spmv_us, double* p1_axpy_us,
                               int32_t* samples) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    set_device(op);
    if (!op->timing || op->p1_samples <= 0 || !op->d_stamps)
      fail(TPL_ERR_INVALID_ARGUMENT,
           "no sampled solve (enable timing, then run a two-pass solve with a device f, k >= 11)");
    unsigned long long t[2 * kStampSteps + 1];
    HIPCHK(hipMemcpyAsync(t, op->d_stamps, sizeof(t), hipMemcpyDeviceToHost, op->stream));
    sync_checked(op);
    double s1 = 0.0, s2 = 0.0;  // 100 MHz ticks
    for (int i = 0; i < kStampSteps; ++i) {
      s1 += (double)(t[2 * i + 1] - t[2 * i]);
      s2 += (double)(t[2 * i + 2] - t[2 * i + 1]);
    }
    if (p1_spmv_us) *p1_spmv_us = 0.01 * s1 / kStampSteps;
    if (p1_axpy_us) *p1_axpy_us = 0.01 * s2 / kStampSteps;
    if (samples) *samples = kStampSteps;
  });
}

tpl_status tpl_op_pass_timing(tpl_op_t op, double* pass1_us, double* pass2_spmv_us,
                              int64_t* pass2_launches) {
  return guarded([&] {
    if (!op) fail(TPL_ERR_INVALID_ARGUMENT, "op is NULL");
    if (!op->timing || op->p2_launches <= 0)
      fail(TPL_ERR_INVALID_ARGUMENT, "no timed solve (enable timing, then run a two-pass solve)");
    set_device(op);
    HIPCHK(hipEventSynchronize(op->tev[3]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, op->tev[0], op->tev[1]));
    HIPCHK(hipEventElapsedTime(&b, op->tev[2], op->tev[3]));
    if (pass1_us) *pass1_us = 1000.0 * (double)a;
    if (pass2_spmv_us) *pass2_spmv_us = 1000.0 * (double)b;
    if (pass2_launches) *pass2_launches = op->p2_launches;
  });
}

tpl_status tpl_profile_kernel(tpl_op_t op, int kernel, int iters, double* avg_us,
                              double* algo_bytes) {
  return guarded([&] {
    if (!op || !avg_us || iters <= 0) fail(TPL_ERR_INVALID_ARGUMENT, "bad argument");
    refuse_dense(op, "the per-kernel profiler");
    set_device(op);
    if (op->st.kcap < 4) ensure_state(op, 4);
    const DevState& S = op->st.S;
    const CsrDev A = csr_dev(op);
    const CsrDev A1 = csr_dev(op, true);  // pass-one launches (hybrid: pass-one segment stride)
    const int big = (int)op->st.kcap; // j < k: the AXPY kernel does its vector work
    // Launch i of the timed sequence. The pass-two kernel re-runs step 2's record while
    // its three basis buffers rotate as in a real sweep (the gathered vector is the
    // previous launch's output); the pass-one kernels re-run step 2.
    auto launch_one = [&](int i) {
      switch (kernel) {
        case TPL_KERNEL_SPMV:
          HIPCHK(launch::spmv(A, op->V2[0], op->W, op->stream));
          break;
        case TPL_KERNEL_PASS1_SPMV:
          HIPCHK(launch::p1_spmv(A1, S, op->RG[2], op->R[2], op->b, op->W, nullptr, 2,
                                 op->stream));
          break;
        case TPL_KERNEL_PASS1_AXPY:
          HIPCHK(launch::p1_axpy(A1, S, op->W, op->R[2], op->R[0], 2, big, 0, op->stream));
          break;
        case TPL_KERNEL_PASS1_STEP:  // both pass-one launches, re-running step 2
          HIPCHK(launch::p1_spmv(A1, S, op->RG[2], op->R[2], op->b, op->W, nullptr, 2,
                                 op->stream));
          HIPCHK(launch::p1_axpy(A1, S, op->W, op->R[2], op->R[0], 2, big, 0, op->stream));
          break;
        case TPL_KERNEL_PASS2_SPMV:
          launch_p2_step(op, A, 2, i + 2, i % 3 == 2 ? 3 : 0, nullptr);
          break;
        case TPL_KERNEL_EXCHANGE_P1:
          enqueue_p1_exchange_a(op, A1);
          enqueue_p1_exchange_norm(op, A1, op->RG[0]);
          break;
        case TPL_KERNEL_EXCHANGE_P2:
          enqueue_p2_exchange(op, 2 + i);
          break;
        default: fail(TPL_ERR_INVALID_ARGUMENT, "unknown kernel id");
      }
    };
    auto launch_all = [&] {
      for (int i = 0; i < iters; ++i) launch_one(i);
    };
    const bool exchange = kernel == TPL_KERNEL_EXCHANGE_P1 || kernel == TPL_KERNEL_EXCHANGE_P2;
    if (exchange && !op->dist) fail(TPL_ERR_INVALID_ARGUMENT, "exchange ids need a partitioned operator");
    // Valid state for repeated launches: flags clear, partials/norms of a real step.
    HIPCHK(launch::p1_init(A1, S, op->b, op->stream));
    HIPCHK(launch::p1_spmv(A1, S, op->bG, op->b, nullptr, op->W, nullptr, 1, op->stream));
    HIPCHK(launch::p1_axpy(A1, S, op->W, op->b, op->R[2], 1, big, 0, op->stream));
    HIPCHK(hipMemcpyAsync(op->V2[1], op->b, op->part.n * sizeof(double), hipMemcpyDeviceToDevice,
                          op->stream));
    HIPCHK(hipMemcpyAsync(op->V2[2], op->R[2], op->part.n * sizeof(double), hipMemcpyDeviceToDevice,
                          op->stream));
    HIPCHK(launch::p2_coefs(S, (int)op->st.kcap, 0, op->stream));  // step 2's record
    sync_checked(op);
    // The launches are captured into one graph, as the solver runs them: back-to-back
    // hipLaunchKernel calls would time the host's submission rate for short kernels.
    // Exchanges run as the solver runs them: eagerly when the transport cannot be
    // captured (the host transport synchronises the stream; an RCCL that refused capture,
    // now or earlier, switched the operator to eager launches: capture_graph).
    GraphExec ge;
    if (!(exchange && (!op->dist->comm || op->eager || !use_graphs())))
      ge = capture_graph(op, launch_all);
    if (ge) {
      HIPCHK(hipGraphLaunch(ge.get(), op->stream));  // warm-up
    } else {
      launch_one(0);
      sync_checked(op);
    }
    HIPCHK(hipEventRecord(op->ev0, op->stream));
    if (ge)
      HIPCHK(hipGraphLaunch(ge.get(), op->stream));
    else
      launch_all();
    HIPCHK(hipEventRecord(op->ev1, op->stream));
    HIPCHK(hipEventSynchronize(op->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    *avg_us = 1000.0 * (double)ms / iters;
    if (algo_bytes) *algo_bytes = tpl_kernel_algo_bytes(op, kernel);
  });
}

// ------------------------------------------------------------ locality order
tpl_status tpl_op_tune_order(tpl_op_t op, const int32_t* groups, int32_t count, int32_t iters,
                             int32_t* chosen, double* best_us) {
  return guarded([&] {
    if (!op || count < 0 || (count > 0 && !groups) || iters <= 0)
      fail(TPL_ERR_INVALID_ARGUMENT, "bad argument");
    if (op->dist) fail(TPL_ERR_UNSUPPORTED, "the locality order is single-GPU only");
    refuse_dense(op, "the locality order");
    set_device(op);
    sync_checked(op);
    static const int32_t kDefault[] = {12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 24};
    const int32_t* list = count > 0 ? groups : kDefault;
    const int32_t cnt = count > 0 ? count : (int32_t)(sizeof(kDefault) / sizeof(kDefault[0]));
    for (int32_t i = 0; i < cnt; ++i)
      if (list[i] <= 0) fail(TPL_ERR_INVALID_ARGUMENT, "group counts must be positive");
    // a failed timing launch leaves the operator as it was (order mode, group count)
    const int saved_reorder = op->reorder;
    const SchedParams saved_sp = op->sp;
    try {
      SchedParams sp = op->sp;
      // any non-zero b: the timed SpMV launches need a step's valid partials and norms
      // (b is the solver's input staging buffer, re-written by every solve)
      const std::vector<double> unit(op->part.n, 1.0);
      double best = 0.0;
      int32_t best_g = op->sp.order_groups;
      for (int32_t i = 0; i < cnt; ++i) {
        sp.order_groups = list[i];
        rebuild_schedule(op, sp, 1);
        if (op->perm.empty()) break;  // no long rows: nothing to order
        if (op->part.n > 0)
          HIPCHK(hipMemcpy(op->b, unit.data(), op->part.n * sizeof(double), hipMemcpyHostToDevice));
        double t1 = 0.0, t2 = 0.0;
        for (const auto& kt : {std::make_pair(TPL_KERNEL_PASS1_SPMV, &t1),
                               std::make_pair(TPL_KERNEL_PASS2_SPMV, &t2)}) {
          const tpl_status st = tpl_profile_kernel(op, kt.first, iters, kt.second, nullptr);
          if (st != TPL_OK) fail(st, tpl_last_error());
        }
        if (i == 0 || t1 + t2 < best) {
          best = t1 + t2;
          best_g = list[i];
        }
      }
      sp.order_groups = best_g;
      rebuild_schedule(op, sp, 1);
      if (chosen) *chosen = best_g;
      if (best_us) *best_us = best;
    } catch (...) {
      hipGetLastError();
      rebuild_schedule(op, saved_sp, saved_reorder);
      throw;
    }
  });
}

} // extern "C"
