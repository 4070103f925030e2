"""Source shape of the fixed-order reduction (csrc/block_reduce.h): the helpers are defined there, the kernel files that reduce through
them include it, and none of them writes a butterfly, a halving tree or a partials finalize out again.  No GPU (the kernels themselves:
tests/test_gpu_block_reduce.py, and tools/reduce_digest.py for bit equality between two builds)."""
import os
import re

from efficient_gnns_amd import build

HIP = ("feature_losses.hip", "losses.hip", "nce.hip", "pairwise.hip", "edge_softmax.hip", "gat.hip", "sign.hip", "similarity.hip",
       "scatter_softmax.hip", "saint.hip", "graph.hip", "rows_sum.hip")
HEADERS = ("common.h", "pair_tile.h")
HELPERS = ("group_sum", "group_max", "waves4_sum", "block_tree_fold", "block_tree_sum", "sum_partials_kernel", "colsum_partials_kernel",
           "colsum_partials", "capped_blocks")
GONE = ("block4_sum", "sub16_sum", "sub16_max", "sub_sum", "sub_max", "wave_sum_f64", "fl_sum_kernel", "fl_sumq_kernel",
        "nce_finalize_sum_kernel", "lsp_loss_final_kernel", "gat_partials_final_kernel", "colsum_wave_final_kernel",
        "split_counts_final_kernel")
# a tree over LDS: `for (int o = ...; o > 0; o >>= 1) { if ((int)threadIdx.x < o) ...`, whatever the counter is called
HALVING = re.compile(r"for\s*\(\s*int\s+(\w+)\s*=[^;]*;[^;]*;\s*\1\s*>>=\s*1\s*\)\s*\{?\s*if\s*\(\s*(?:\(int\)\s*)?threadIdx\.x\s*<\s*\1\s*\)")
# The butterflies that stay written out, by file -> number of __shfl_xor calls:
#   losses.hip  the 16-lane argmax of split_accuracy_kernel: a compare-and-take over (value, column), not a sum or a max
#   nce.hip     the 32-lane row merge of nce_fwd_kernel: its offsets ASCEND (1 ... 16), for the plain sum and for the (max, sum) merge;
#               group_sum descends, and another order of the additions would change the bits of the loss
KEPT = {"losses.hip": 2, "nce.hip": 3}


def _read(name):
    return open(os.path.join(build.CSRC, name)).read()


def _defines(name, text):
    return re.search(r"^[^/\n]*[\w>&*]\s+" + name + r"\s*\([^;{]*\)\s*\{", text, flags=re.M)


def test_block_reduce_h_defines_every_helper_once():
    text = _read("block_reduce.h")
    assert text.count("namespace egnn_reduce {") == 1
    for name in HELPERS:
        assert _defines(name, text), f"block_reduce.h does not define {name}"
    assert text.count("__shfl_xor") == 2                       # group_sum and group_max
    assert len(HALVING.findall(text)) == 1                     # block_tree_fold
    assert "atomic" not in text.replace("floating-point atomic", "")
    assert re.search(r"enum Assoc \{ PAIRWISE, SERIAL \}", text)


def test_the_kernel_files_reduce_through_block_reduce_h_only():
    for f in HIP:
        assert '#include "block_reduce.h"' in _read(f), f"{f} does not include block_reduce.h"
    assert '#include "block_reduce.h"' in _read("common.h") and '#include "block_reduce.h"' in _read("pair_tile.h")
    for f in HIP + HEADERS:
        text = _read(f)
        assert not HALVING.search(text), f"{f} writes an LDS halving tree out"
        assert text.count("__shfl_xor") == KEPT.get(f, 0), f"{f} writes a butterfly out"
        for name in GONE:
            assert not re.search(r"\b" + name + r"\b", text), f"{f} still has {name}"
        for name in HELPERS:
            assert not _defines(name, text), f"{f} defines {name} again"


def test_the_kept_butterflies_are_the_two_named_exceptions():
    losses, nce = _read("losses.hip"), _read("nce.hip")
    argmax = re.search(r"for \(int o = 8; o > 0; o >>= 1\) \{[^\n]*argmax[^\n]*\n(.*?)\n    \}", losses, flags=re.S)
    assert argmax and argmax.group(1).count("__shfl_xor") == 2 and "take" in argmax.group(1)
    assert len(re.findall(r"for \(int o = 1; o < 32; o <<= 1\)", nce)) == 2 and "o >>= 1" not in nce


def test_the_historical_names_are_aliases():
    common = _read("common.h")
    for alias, target in (("egnn_wave_sum", "group_sum<EGNN_WAVE>"), ("egnn_group_sum", "group_sum<G>"), ("egnn_wave_max", "group_max<EGNN_WAVE>")):
        assert re.search(alias + r"\(float v\) \{ return egnn_reduce::" + re.escape(target) + r"\(v\); \}", common), alias
    fused_bn = _read("fused_bn.hip")
    assert "block_reduce.h" not in fused_bn                    # out of scope: it takes the aliases through common.h
