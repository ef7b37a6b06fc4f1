# Lab edit, TIMING ONLY (the open rows and H's long rows are not stepped: x is wrong there):
# k_p2_hub without the hub-set workgroup — what the long-row workgroups alone take.
s = open('tpl_k_p2_fused.hip').read()
a = '(A.n_long + kTPB - 1) / kTPB + (H.n_hub > 0 ? 1 : 0);'
assert a in s
open('tpl_k_p2_fused.hip', 'w').write(s.replace(a, '(A.n_long + kTPB - 1) / kTPB;'))
