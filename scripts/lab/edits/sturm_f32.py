# Lab edit: the device exp's Sturm bracket in single precision on T / max|Gershgorin end|
# (entries in [-1, 1], beta^2 <= 4), the bracket widened by 1e-5 * gmag for fp32's backward
# error (a count is exact for a matrix within a few ulps of the scaled T).
s = open('tpl_k_ftk_exp.hip').read()
a = '''  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, red[0][0]);'''
assert a in s
s = s.replace(a, a + '''
  const double bmax_all = red[0][0];''')
a = '''    const double w = (ghi - glo) / (double)(kExpShifts + 1);
    double sg[2], q[2];
    int c[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sg[u] = glo + w * (double)(u * kTPB + t + 1);  // shift s = u * 256 + t
      q[u] = al[0] - sg[u];
      if (fabs(q[u]) < pivmin) q[u] = -pivmin;
      c[u] = q[u] < 0.0;
    }
    for (int i = 1; i < n; ++i) {
      const double ai = al[i], bb = b2[i - 1];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        q[u] = (ai - sg[u]) - bb * rcp_nr(q[u]);
        if (fabs(q[u]) < pivmin) q[u] = -pivmin;
        c[u] += q[u] < 0.0;
      }
    }
    cnt[t] = c[0];'''
assert a in s
s = s.replace(a, '''    const double w = (ghi - glo) / (double)(kExpShifts + 1);
    const double smax = fmax(fmax(fabs(glo), fabs(ghi)), 1e-300);
    const double sinv = 1.0 / smax;
    float* a32 = reinterpret_cast<float*>(buf0);  // the Clenshaw buffers, re-zeroed below
    float* b32 = reinterpret_cast<float*>(buf1);
    for (int i = t; i < n; i += kTPB) {
      a32[i] = (float)(al[i] * sinv);
      b32[i] = (float)((b2[i] * sinv) * sinv);
    }
    __syncthreads();
    const float pivmin32 = 1.17549435e-38f * fmaxf(1.0f, (float)((bmax_all * sinv) * sinv));
    float sg[2], q[2];
    int c[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sg[u] = (float)((glo + w * (double)(u * kTPB + t + 1)) * sinv);  // shift s = u * 256 + t
      q[u] = a32[0] - sg[u];
      if (fabsf(q[u]) < pivmin32) q[u] = -pivmin32;
      c[u] = q[u] < 0.0f;
    }
    for (int i = 1; i < n; ++i) {
      const float ai = a32[i], bb = b32[i - 1];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        q[u] = (ai - sg[u]) - bb * __builtin_amdgcn_rcpf(q[u]);
        if (fabsf(q[u]) < pivmin32) q[u] = -pivmin32;
        c[u] += q[u] < 0.0f;
      }
    }
    __syncthreads();
    for (int i = t; i < n + 2; i += kTPB) buf0[i] = buf1[i] = 0.0;
    cnt[t] = c[0];''')
a = '''  const double a = (first[0] > 0 ? glo + wsh * (double)first[0] : glo) - 1e-9 * (1.0 + gmag);'''
assert a in s
s = s.replace(a, '''  const double a = (first[0] > 0 ? glo + wsh * (double)first[0] : glo) - 1e-9 * (1.0 + gmag) -
                   1e-5 * gmag;''')
a = '''                   1e-9 * (1.0 + gmag);'''
assert a in s
s = s.replace(a, '''                   1e-9 * (1.0 + gmag) + 1e-5 * gmag;''')
open('tpl_k_ftk_exp.hip', 'w').write(s)
