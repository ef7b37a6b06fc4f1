# Lab edit: k_p2_hub with the cache and record loads N steps ahead of the chain (8 ships),
# N read from the variant's name: scripts/build_variant_src.sh p2f_hub<N> .../p2f_hub16.py
import os
import re

m = re.search(r'tplvar_p2f_hub(\d+)', os.getcwd())
assert m, os.getcwd()
s = open('tpl_k_p2_fused.hip').read()
a = 'constexpr int kHubAhead = 8;'
assert a in s
open('tpl_k_p2_fused.hip', 'w').write(s.replace(a, f'constexpr int kHubAhead = {m.group(1)};'))
