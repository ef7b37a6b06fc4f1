// spmv_lab2.hip — the library's k_spmv (included verbatim) vs a minimal SELL kernel,
// on the 500k KKT arc rows only. Build with -DTPL_CHUNK_ROWS=256.
#include "../two-pass-lanczos_amd/csrc/tpl_k_spmv.hip"
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

__global__ __launch_bounds__(256) void k_sell2(int n, const int* __restrict__ c, const double* __restrict__ v, const double* __restrict__ x, double* __restrict__ y) {
  int i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  int base = (i / 256) * 512 + (i % 256);
  int c0 = c[base], c1 = c[base + 256]; double a0 = v[base], a1 = v[base + 256];
  double s = 0.0; s = s + a0 * x[c0]; s = s + a1 * x[c1]; y[i] = s; }

int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); long long hdr[2]; fread(hdr, 8, 2, f);
  int n = (int)hdr[0], nnz = (int)hdr[1];
  std::vector<int> rp(n + 1), col(nnz); std::vector<double> val(nnz), x(n);
  fread(rp.data(), 4, n + 1, f); fread(col.data(), 4, nnz, f); fread(val.data(), 8, nnz, f); fclose(f);
  for (int i = 0; i < n; ++i) x[i] = 1.0 / (1 + i % 97);
  int m = 0; while (rp[m + 1] - rp[m] <= 32) ++m;  // arc rows
  const int CR = tpl::kChunkRows, nch = (m + CR - 1) / CR;
  std::vector<int> sc(nch * CR * 2, -1); std::vector<double> sv(nch * CR * 2, 0.0);
  for (int i = 0; i < m; ++i) for (int k = 0; k < 2; ++k) { int e = (i / CR) * CR * 2 + k * CR + i % CR; sc[e] = col[rp[i] + k]; sv[e] = val[rp[i] + k]; }
  int *d_sc; double *d_sv, *d_x, *d_y;
  CK(hipMalloc(&d_sc, 4 * sc.size())); CK(hipMalloc(&d_sv, 8 * sv.size())); CK(hipMalloc(&d_x, 8 * n)); CK(hipMalloc(&d_y, 8 * n));
  CK(hipMemcpy(d_sc, sc.data(), 4 * sc.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d_sv, sv.data(), 8 * sv.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_x, x.data(), 8 * n, hipMemcpyHostToDevice));
  tpl::CsrDev A{}; A.s_col = d_sc; A.s_val = d_sv; A.s_width = 2; A.s_identity = 1; A.n_short = m; A.n_chunks = nch;
  A.n_long = 0; A.n_groups = 0; A.n_slice_blocks = 0; A.G2 = 1; A.NA = nch; A.n = n; A.E = 1024;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto bench = [&](const char* name, auto launch) {
    for (int r = 0; r < 5; ++r) launch(); CK(hipDeviceSynchronize());
    const int iters = 300; CK(hipEventRecord(e0)); for (int r = 0; r < iters; ++r) launch();
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-40s %8.2f us\n", name, 1000.0 * ms / iters); };
  bench("lab sell2 (1 row/thread)", [&] { hipLaunchKernelGGL(k_sell2, dim3((m + 255) / 256), dim3(256), 0, 0, m, d_sc, d_sv, d_x, d_y); });
  bench("library k_spmv chunks only", [&] { hipLaunchKernelGGL(tpl::k_spmv, dim3(nch), dim3(256), 0, 0, A, d_x, d_y); });
  tpl::CsrDev B = A; B.n_slice_blocks = 2304; B.n_long = 0;
  bench("library k_spmv + 2304 empty slice blks", [&] { hipLaunchKernelGGL(tpl::k_spmv, dim3(nch + 2304), dim3(256), 0, 0, B, d_x, d_y); });
  return 0;
}
