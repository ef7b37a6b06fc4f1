"""The fused pass two's fixed tuning choices, as the tests see them (DESIGN.md §2;
two-pass-lanczos_amd/csrc/tpl_k_p2_fused.hip holds them as constexpr). The edge cases of
tests/test_gpu_fused_pass_two_tuned.py are derived from these, and
tests/test_fused_pass_two_tuned_cpu.py checks them against the source.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "two-pass-lanczos_amd", "csrc", "tpl_k_p2_fused.hip")

TPB = 256
HUB_AHEAD = 8      # kHubAhead: steps k_p2_hub's loads run ahead of the chain
ROWS_GROUP = 4     # kRowsGroup: chunks per k_p2_rows workgroup (256 threads each)
ROWS_DEPTH = 2     # kRowsDepth: steps of the cache row k_p2_rows keeps in registers


def source_constants():
    """-> (kHubAhead, kRowsGroup, kRowsDepth) as the source has them."""
    with open(SOURCE) as f:
        s = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, s).group(1))
                 for name in ("kHubAhead", "kRowsGroup", "kRowsDepth"))


def block_edge_lasts(depth):
    """The step counts `last` at the edges of a loop that takes whole blocks of `depth` steps
    and a tail: short of one block, exactly one, one more, and the same around two."""
    return sorted({max(1, depth - 3), depth, depth + 1, 2 * depth - 1, 2 * depth, 2 * depth + 1})
