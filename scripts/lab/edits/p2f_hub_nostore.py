# Lab edit, TIMING ONLY (x is wrong: k_p2_rows then reads the sums): k_p2_hub without its
# store of v_j into the cache row — what the chain costs when only loads count in vmcnt.
s = open('tpl_k_p2_fused.hip').read()
a = '    st_cache_row(a.ycache + (size_t)(j - 1) * nl, nl, soff, vc);'
assert a in s
open('tpl_k_p2_fused.hip', 'w').write(s.replace(a, '    (void)soff;'))
