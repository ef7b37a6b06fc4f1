# Lab edit: k_p2_rows with another group size (chunks per workgroup) and prefetch depth, named
# by the variant: scripts/build_variant_src.sh p2f_c<C>d<D> scripts/lab/edits/p2f_rows.py
# builds kRowsGroup = C and kRowsDepth = D (the name is read from the working directory,
# /tmp/tplvar_<name>/...).
import os
import re

m = re.search(r'tplvar_p2f_c(\d)d(\d)', os.getcwd())
assert m, os.getcwd()
s = open('tpl_k_p2_fused.hip').read()
a = re.search(r'constexpr int kRowsGroup = \d+;', s)
b = re.search(r'constexpr int kRowsDepth = \d+;', s)
assert a and b
s = s.replace(a.group(0), f'constexpr int kRowsGroup = {m.group(1)};')
s = s.replace(b.group(0), f'constexpr int kRowsDepth = {m.group(2)};')
open('tpl_k_p2_fused.hip', 'w').write(s)
