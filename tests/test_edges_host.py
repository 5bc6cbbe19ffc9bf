"""Rows of C placed exactly on every class limit and table-size switch of speck_multiply_*: the edge table, the generator
that builds matrices whose rows have prescribed (len_a, ops, nnz, cmin, cmax), and their checks without a GPU.

A row of C takes its symbolic and its numeric kernel class from four integers (classify_symbolic / classify_numeric,
speck_amd/csrc/device_common.hpp): entries of the A row (len_a), products (ops), distinct columns (nnz) and reachable
column range (cmin .. cmax).  Every limit is a `<=` against a constant and every kernel is sized to just work at it.
PROBES below holds, for each such limit, rows with the last value on one side and the first on the other -- with
DIFFERENT row counts, so that the per-class counts of a call say which side went where -- and the class of every row
written LITERALLY, taken from the class tables of DESIGN.md 4.1 / 4.2 (not computed by a copy of the classifier).

Here (no GPU):
  * the generator is what it claims: per row the oracle's nnz, first and last column, and len_a / ops from A and B;
  * the real header, compiled for the host (tests/cpp/classify_probe.cpp), gives every row its literal class, under the
    options of its probe;
  * table_bits / max_nnz_of against the rule stated at their definition, in exact integers, for every nnz up to 8192;
  * the one edge no call can reach is shown unreachable with the real classifier.
tests/test_gpu_edges.py runs the same table through the kernels.
"""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_values import _dyadic, exact_spgemm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# enum order of device_common.hpp (SymClass / NumClass), by the names last_stats() reports
SYM_NAMES = ["g16", "wave256", "wave1k", "block4k", "block16k", "block32k", "bitmap256k", "bitmap1m", "numeric_first",
             "global_hash", "g8", "wave128", "r32", "r64"]
NUM_NAMES = ["direct", "g16", "wave128", "wave512", "block2k", "block8k", "dense4k", "dense16k", "global", "wave256",
             "nfcopy", "g8", "r32", "r64"]
NO_CLASS = 0xFF

# ClassifyParams of a fresh config (speck_config_create), in the order classify_probe reads them
CP_FIELDS = ["sym_bitmap_ratio", "num_dense_ratio", "num_global_passes", "num_w256", "esc16", "esc32", "esc64", "esc_fused",
             "num_g8", "sym_g8", "sym_w128", "nf_min_ops", "gh_per_window", "slice_ops"]
CP_DEFAULT = dict(sym_bitmap_ratio=32, num_dense_ratio=16, num_global_passes=4, num_w256=1, esc16=1, esc32=1, esc64=1,
                  esc_fused=0, num_g8=1, sym_g8=1, sym_w128=1, nf_min_ops=512, gh_per_window=8192, slice_ops=0)

Row = collections.namedtuple("Row", "count len_a ops nnz cmin cmax sym num share")
Probe = collections.namedtuple("Probe", "name kind rows opts cp cols")


def R(count, len_a, ops, nnz, rng, sym, num, c0=5, share=False):
    """`count` rows of C with len_a entries of A, ops products, nnz distinct columns spanning exactly [c0, c0 + rng - 1];
    sym / num: the class names the row must get (None: no class).  share: the rows reference the SAME rows of B."""
    return Row(count, len_a, ops, nnz, c0, c0 + rng - 1 if rng else c0, sym, num, share)


PROBES = []


def probe(name, kind, rows, opts=None, cp=None, cols=None):
    """opts: library options of the call (set_option); cp: what the call itself derives on top (ClassifyParams only)."""
    assert name not in [p.name for p in PROBES]
    PROBES.append(Probe(name, kind, rows, opts or {}, cp or {}, cols))


ESC_OFF = dict(esc16=0, esc32=0, esc64=0, num_g8=0, sym_g8=0)     # no register classes: rows of few A entries reach the hash classes
W = 5000          # a column range above 4096 (neither numeric-first nor NUM_D1) that 32 * ops covers from 157 products on
G8 = R(2, 2, 4, 4, W, "g8", "g8")                                  # filler rows of another class

# ---- analysis / no class ------------------------------------------------------------------------------------------------
probe("no_products_one_entry_two_entries", "analysis", [
    R(5, 3, 0, 0, 0, None, None),                  # ops == 0 with len_a > 0: three empty rows of B
    R(3, 1, 6, 6, W, None, "direct"),              # len_a 1: resolved by the analysis, NUM_DIRECT
    R(4, 2, 6, 6, W, "g8", "g8"),                  # len_a 2: the first row with a symbolic class
    R(2, 1, 0, 0, 0, None, None),                  # one entry of A onto an empty row of B
])
for n in (255, 256, 257):                          # NUM_DIRECT: one workgroup flattens 256 rows
    probe(f"direct_{n}_rows", "analysis", [R(n, 1, 5, 5, 300, None, "direct"), R(1, 1, 0, 0, 0, None, None),
                                           R(1, 1, 700, 700, W, None, "direct"), G8])

# ---- register classes (both phases) -------------------------------------------------------------------------------------
# at each ops limit two shapes: every product a column of its own, and the products onto as few columns as sorted B rows
# allow -- ceil(ops / len_a) of them, cmin and cmax among them (two columns would need B rows with a column twice)
probe("g8_ops_32_33", "register", [R(5, 8, 32, 32, W, "g8", "g8"), R(5, 8, 32, 4, W, "g8", "g8", share=True),
                                   R(3, 8, 33, 33, W, "g16", "g16"), R(3, 8, 33, 5, W, "g16", "g16")])
probe("g8_len_8_9", "register", [R(5, 8, 16, 16, W, "g8", "g8"), R(3, 9, 18, 18, W, "g16", "g16"),
                                 R(2, 8, 3, 3, W, "g8", "g8"), R(4, 9, 3, 3, W, "g16", "g16")])       # len_a > ops: empty B rows between
probe("g16_ops_64_65", "register", [R(5, 16, 64, 64, W, "g16", "g16"), R(5, 16, 64, 4, W, "g16", "g16"),
                                    R(3, 16, 65, 65, W, "r32", "r32"), R(3, 16, 65, 5, W, "r32", "r32", share=True), G8])
probe("g16_len_16_17", "register", [R(5, 16, 32, 32, W, "g16", "g16"), R(3, 17, 34, 34, W, "r32", "r32"),
                                    R(2, 17, 5, 5, W, "r32", "r32"), G8])
# cols(B) 2^26 / 2^26 + 1: the 16-lane class packs (column << 6 | product) into 32 bits -- off for the whole call beyond
probe("g16_cols_2p26", "register", [R(5, 16, 64, 64, (1 << 26) - 5, "g16", "g16"), R(3, 8, 32, 32, (1 << 26) - 5, "g8", "g8"),
                                    R(4, 16, 64, 64, 1 << 25, "g16", "g16")], cols=1 << 26)
probe("g16_cols_2p26_plus_1", "register", [R(5, 16, 64, 64, (1 << 26) - 4, "wave128", "wave128"),
                                           R(3, 8, 32, 32, (1 << 26) - 4, "g8", "g8"),
                                           R(4, 16, 64, 64, 1 << 25, "r32", "r32")], cp=dict(esc16=0), cols=(1 << 26) + 1)
probe("r32_ops_128_129", "register", [R(5, 32, 128, 128, W, "r32", "r32"), R(5, 32, 128, 4, W, "r32", "r32"),
                                      R(3, 32, 129, 129, W, "r64", "r64"), R(3, 32, 129, 5, W, "r64", "r64"), G8])
probe("r32_len_32_33", "register", [R(5, 32, 64, 64, W, "r32", "r32", c0=0), R(3, 33, 66, 66, W, "r64", "r64"),
                                    R(2, 33, 7, 7, W, "r64", "r64"), G8])
# cmax - cmin = 2^25 - 1 / 2^25: the sort key of the 32-lane class packs (column - cmin) into 25 bits
probe("r32_range_2p25", "register", [R(5, 20, 100, 100, 1 << 25, "r32", "r32"), R(3, 20, 100, 100, (1 << 25) + 1, "wave128", "wave256"),
                                     R(4, 32, 128, 4, 1 << 25, "r32", "r32", c0=0), R(2, 32, 128, 4, (1 << 25) + 1, "wave256", "wave128"), G8])
probe("r64_ops_256_257", "register", [R(5, 64, 256, 256, W, "r64", "r64"), R(5, 64, 256, 4, W, "r64", "r64"),
                                      R(3, 64, 257, 257, W, "bitmap256k", "wave512"), R(2, 64, 257, 5, W, "bitmap256k", "wave128"), G8])
probe("r64_len_64_65", "register", [R(5, 64, 128, 128, W, "r64", "r64"), R(3, 65, 130, 130, W, "wave256", "wave256"),
                                    R(2, 64, 9, 9, W, "r64", "r64"), G8])
# cmax - cmin = 2^24 - 1 / 2^24: 24 bits in the wave class
probe("r64_range_2p24", "register", [R(5, 40, 200, 200, 1 << 24, "r64", "r64"), R(3, 40, 200, 200, (1 << 24) + 1, "wave256", "wave512"),
                                     R(4, 64, 256, 4, 1 << 24, "r64", "r64", c0=0), R(2, 64, 256, 4, (1 << 24) + 1, "wave1k", "wave128"), G8])
probe("register_classes_off", "register", [R(5, 8, 32, 32, W, "wave128", "wave128"), R(3, 16, 64, 64, W, "wave128", "wave128"),
                                           R(4, 32, 128, 128, W, "wave256", "wave256"), R(2, 64, 256, 256, W, "bitmap256k", "wave512")],
      opts=ESC_OFF)
probe("g8_off", "register", [R(5, 8, 32, 32, W, "g16", "g16"), R(3, 9, 18, 18, W, "g16", "g16")], opts=dict(num_g8=0, sym_g8=0))

# ---- symbolic key sets: every product a new key (nnz == ops), range > 32 * ops so that no bitmap takes the row ------------
# (65 entries of A: beyond every register class)
probe("sym_ops_102_103", "symbolic", [R(5, 65, 102, 102, 4300, "wave128", "wave256"), R(3, 65, 103, 103, 4300, "wave256", "wave256"), G8])
probe("sym_ops_102_103_register_classes_off", "symbolic", [
    R(5, 6, 102, 102, 4300, "wave128", "wave256"), R(3, 6, 103, 103, 4300, "wave256", "wave256"), R(4, 4, 20, 20, W, "wave128", "wave128")],
      opts=ESC_OFF)
probe("sym_w128_off", "symbolic", [R(5, 65, 102, 102, 4300, "wave256", "wave256"), R(3, 65, 103, 103, 4300, "wave256", "wave256"), G8],
      opts=dict(sym_w128=0))
probe("sym_ops_204_205", "symbolic", [R(5, 65, 204, 204, 7000, "wave256", "wave512"), R(3, 65, 205, 205, 7000, "wave1k", "wave512"), G8])
probe("sym_ops_819_820", "symbolic", [R(5, 65, 819, 819, 27000, "wave1k", "block2k"), R(3, 65, 820, 820, 27000, "block4k", "block2k"),
                                      R(4, 128, 819, 7, 27000, "wave1k", "wave128"), G8])          # long probe chains onto seven keys
probe("sym_ops_3276_3277", "symbolic", [R(5, 65, 3276, 3276, 300000, "block4k", "block8k"), R(3, 65, 3277, 3277, 300000, "block16k", "block8k"), G8])
probe("sym_ops_13107_13108", "symbolic", [R(5, 65, 13107, 13107, 500000, "block16k", "global"),
                                          R(3, 65, 13108, 13108, 500000, "block32k", "global"), G8])
probe("sym_ops_26214_26215", "symbolic", [R(3, 65, 26214, 26214, 900000, "block32k", "global"),
                                          R(2, 65, 26215, 26215, 900000, "bitmap1m", "global"), G8])
# ---- symbolic bitmaps --------------------------------------------------------------------------------------------------------
probe("bitmap_rule_32_ops", "symbolic", [R(5, 65, 300, 300, 9600, "bitmap256k", "wave512"), R(3, 65, 300, 300, 9601, "wave1k", "wave512"), G8])
probe("bitmap_ratio_0", "symbolic", [R(5, 65, 300, 300, 9600, "wave1k", "wave512"), R(3, 65, 300, 300, 9601, "wave1k", "wave512"), G8],
      opts=dict(sym_bitmap_ratio=0))
# SYM_BM1: 131 072 columns per window (the second window begins at 131 073), rows up to 262 144 columns
probe("bm1_windows", "symbolic", [R(5, 65, 5000, 5000, 131072, "bitmap256k", "block8k"), R(3, 65, 5000, 5000, 131073, "bitmap256k", "block8k"),
                                  R(4, 65, 9000, 6000, 262144, "bitmap256k", "block8k"), R(2, 65, 9000, 6000, 262145, "block16k", "block8k"),
                                  R(3, 65, 14000, 6900, 262144, "bitmap256k", "block8k", c0=0), R(1, 65, 14000, 6900, 262145, "bitmap1m", "block8k"), G8])
# SYM_BM2: 2^20 columns per window
probe("bm2_windows", "symbolic", [R(3, 65, 40000, 6900, 1 << 20, "bitmap1m", "block8k"), R(2, 65, 40000, 6900, (1 << 20) + 1, "bitmap1m", "block8k"),
                                  R(2, 65, 70000, 6900, 1 << 21, "bitmap1m", "block8k", c0=0), R(1, 65, 70000, 6900, (1 << 21) + 1, "bitmap1m", "block8k"), G8])
# SYM_GH: fewer than gh_per_window (8192) products per 2^20-column window; its key set: 65 536 slots at least, load <= 1/2
probe("gh_per_window", "symbolic", [R(3, 65, 4 * 8192 - 1, 4 * 8192 - 1, 4 << 20, "global_hash", "global"),
                                    R(2, 65, 4 * 8192, 4 * 8192, 4 << 20, "bitmap1m", "global"), G8])
probe("gh_per_window_0", "symbolic", [R(3, 65, 4 * 8192 - 1, 4 * 8192 - 1, 4 << 20, "bitmap1m", "global"), G8], opts=dict(gh_per_window=0))
probe("gh_table_slots", "symbolic", [R(2, 65, 32768, 32768, (4 << 20) + 1, "global_hash", "global"),
                                     R(1, 65, 32769, 32769, (4 << 20) + 1, "global_hash", "global"),
                                     R(2, 65, 65536, 65536, (8 << 20) + 1, "global_hash", "global", c0=0),
                                     R(1, 65, 65537, 65537, (8 << 20) + 1, "global_hash", "global"), G8])
# SYM_NF: range <= 4096, >= nf_min_ops (512) products, more than one entry of A
probe("nf_range_4096_4097", "symbolic", [R(5, 65, 600, 300, 4096, "numeric_first", "nfcopy"), R(3, 65, 600, 300, 4097, "bitmap256k", "wave512"), G8])
probe("nf_ops_511_512", "symbolic", [R(5, 65, 512, 300, 4000, "numeric_first", "nfcopy"), R(3, 65, 511, 300, 4000, "bitmap256k", "dense4k"), G8])
probe("nf_len_1_2", "symbolic", [R(4, 1, 600, 600, 4000, None, "direct"), R(2, 2, 600, 300, 4000, "numeric_first", "nfcopy"), G8])
probe("nf_min_ops_0", "symbolic", [R(5, 65, 600, 400, 4096, "bitmap256k", "dense4k"), R(3, 65, 600, 300, 4097, "bitmap256k", "wave512"), G8],
      opts=dict(nf_min_ops=0))

# ---- numeric tables: 65 entries of A, range above 4096; each limit at ops == nnz and at ops = several times nnz ------------
probe("num_nnz_85_86", "numeric", [R(5, 65, 85, 85, W, "wave128", "wave128"), R(3, 65, 86, 86, W, "wave128", "wave256"),
                                   R(4, 65, 340, 85, W, "bitmap256k", "wave128"), R(2, 65, 344, 86, W, "bitmap256k", "wave256", share=True), G8])
probe("num_nnz_170_171", "numeric", [R(5, 65, 170, 170, W, "wave256", "wave256"), R(3, 65, 171, 171, W, "wave256", "wave512"),
                                     R(4, 65, 680, 170, W, "bitmap256k", "wave256"), R(2, 65, 684, 171, W, "bitmap256k", "wave512"), G8])
probe("num_w256_off", "numeric", [R(5, 65, 170, 170, W, "wave256", "wave512"), R(3, 65, 171, 171, W, "wave256", "wave512"),
                                  R(4, 65, 86, 86, W, "wave128", "wave512"), R(2, 65, 85, 85, W, "wave128", "wave128"), G8], opts=dict(num_w256=0))
probe("num_nnz_341_342", "numeric", [R(5, 65, 341, 341, W, "bitmap256k", "wave512"), R(3, 65, 342, 342, W, "bitmap256k", "block2k"),
                                     R(4, 65, 1364, 341, W, "bitmap256k", "wave512", share=True), R(2, 65, 1368, 342, W, "bitmap256k", "block2k"), G8])
probe("num_nnz_1740_1741", "numeric", [R(5, 65, 1740, 1740, 20000, "bitmap256k", "block2k"), R(3, 65, 1741, 1741, 20000, "bitmap256k", "block8k"),
                                       R(4, 65, 6960, 1740, 20000, "bitmap256k", "block2k"), R(2, 65, 6964, 1741, 20000, "bitmap256k", "block8k"), G8])
# 3481 / 3482: the half-table and the full-table launch of NUM_B8K (one class; also with the two launches in the other order:
# b8k_full_first, default 1 = the full table first in complete calls, the half table first in a reuse sequence)
_B8K_HALF = [R(5, 65, 3481, 3481, 20000, "bitmap256k", "block8k"), R(3, 65, 3482, 3482, 20000, "bitmap256k", "block8k"),
             R(3, 65, 10443, 3481, 20000, "bitmap256k", "block8k"), R(2, 65, 10446, 3482, 20000, "bitmap256k", "block8k"), G8]
probe("num_nnz_3481_3482", "numeric", _B8K_HALF)
probe("num_nnz_3481_3482_other_launch_order", "numeric", _B8K_HALF, opts=dict(b8k_full_first=2))
probe("num_nnz_6963_6964_dense", "numeric", [R(3, 65, 6963, 6963, 20000, "bitmap256k", "block8k"), R(2, 65, 6964, 6964, 20000, "bitmap256k", "dense16k"),
                                             R(4, 65, 20889, 6963, 20000, "bitmap256k", "block8k"), R(1, 65, 20892, 6964, 20000, "bitmap256k", "dense16k"), G8])
probe("num_nnz_6963_6964_global", "numeric", [R(3, 65, 6963, 6963, 100000, "bitmap256k", "block8k"), R(2, 65, 6964, 6964, 100000, "bitmap256k", "global"),
                                              R(4, 65, 20889, 6963, 100000, "bitmap256k", "block8k"), R(1, 65, 20892, 6964, 100000, "bitmap256k", "global"), G8])
# inside the classes: every nnz where table_bits changes (NUM_W128: 32 / 64 / 128 slots; NUM_B2K: 512 / 1024 / 2048)
probe("w128_table_bits", "numeric", [R(5, 3, 21, 21, W, "wave128", "wave128"), R(3, 3, 22, 22, W, "wave128", "wave128"),
                                     R(5, 3, 42, 42, W, "wave128", "wave128"), R(4, 3, 43, 43, W, "wave128", "wave128"),
                                     R(3, 3, 44, 44, W, "wave128", "wave128"), R(5, 7, 63, 21, W, "wave128", "wave128"),
                                     R(3, 11, 88, 22, W, "wave128", "wave128"), R(5, 6, 126, 42, W, "wave256", "wave128"),
                                     R(4, 3, 129, 43, W, "wave256", "wave128"), R(3, 3, 132, 44, W, "wave256", "wave128")], opts=ESC_OFF)
probe("b2k_table_bits", "numeric", [R(5, 65, 435, 435, W, "bitmap256k", "block2k"), R(3, 65, 436, 436, W, "bitmap256k", "block2k"),
                                    R(5, 65, 870, 870, W, "bitmap256k", "block2k"), R(3, 65, 871, 871, W, "bitmap256k", "block2k"),
                                    R(4, 65, 1740, 435, W, "bitmap256k", "block2k"), R(2, 65, 1744, 436, W, "bitmap256k", "block2k"),
                                    R(4, 65, 2610, 870, W, "bitmap256k", "block2k"), R(2, 65, 2613, 871, W, "bitmap256k", "block2k"), G8])

# ---- numeric sort forms and windows --------------------------------------------------------------------------------------
# NUM_W128 ranks by bitmap when cmax - cmin < 1024 (every row of the wave), by comparison beyond
probe("rank_sort_1023", "sort", [R(8, 65, 80, 80, 1024, "wave128", "wave128"), R(4, 65, 200, 30, 1024, "wave256", "wave128")])
probe("rank_sort_1024", "sort", [R(8, 65, 80, 80, 1025, "wave128", "wave128"), R(4, 65, 200, 30, 1025, "wave256", "wave128")])
probe("rank_sort_1023_1024", "sort", [R(5, 65, 80, 80, 1024, "wave128", "wave128"), R(3, 65, 80, 80, 1025, "wave128", "wave128"), G8])
# bitmap-sort windows of W1 * 1024 columns: W1 = 256 (NUM_W256), 768 (NUM_W512), 1024 (NUM_B2K), 2048 (NUM_B8K)
probe("sort_windows", "sort", [R(5, 65, 150, 150, 256 << 10, "wave256", "wave256"), R(3, 65, 150, 150, (256 << 10) + 1, "wave256", "wave256"),
                               R(5, 65, 300, 300, 768 << 10, "wave1k", "wave512"), R(3, 65, 300, 300, (768 << 10) + 1, "wave1k", "wave512"),
                               R(5, 65, 1000, 1000, 1024 << 10, "block4k", "block2k", c0=0), R(3, 65, 1000, 1000, (1024 << 10) + 1, "block4k", "block2k"),
                               R(3, 65, 4000, 4000, 2048 << 10, "block16k", "block8k"), R(2, 65, 4000, 4000, (2048 << 10) + 1, "block16k", "block8k")])
# NUM_D1 (fewer than nf_min_ops products): range 4096 / 4097, range = 16 nnz / + 1, its LDS window of 2560 columns
probe("d1_range_4096_4097", "sort", [R(5, 65, 400, 300, 4096, "bitmap256k", "dense4k"), R(3, 65, 400, 300, 4097, "bitmap256k", "wave512"), G8])
probe("d1_ratio_16_nnz", "sort", [R(5, 65, 400, 200, 3200, "bitmap256k", "dense4k"), R(3, 65, 400, 200, 3201, "bitmap256k", "wave512"), G8])
probe("d1_ratio_0", "sort", [R(5, 65, 400, 200, 3200, "bitmap256k", "wave512"), R(3, 65, 400, 200, 3201, "bitmap256k", "wave512"), G8],
      opts=dict(num_dense_ratio=0))
probe("d1_window_2560_2561", "sort", [R(5, 65, 400, 300, 2560, "bitmap256k", "dense4k"), R(3, 65, 400, 300, 2561, "bitmap256k", "dense4k"),
                                      R(2, 65, 400, 300, 2560, "bitmap256k", "dense4k", c0=0), G8])
probe("d1_heavy_nf_off", "sort", [R(4, 65, 3000, 2000, 4096, "bitmap256k", "dense4k"), R(2, 65, 6000, 2561, 2561, "bitmap256k", "dense4k"), G8],
      opts=dict(nf_min_ops=0))
# NUM_D2: windows of 16 384 columns, four of them at most (num_global_passes), NUM_G beyond
probe("d2_window_16384_16385", "sort", [R(3, 65, 14000, 7000, 16384, "bitmap256k", "dense16k"), R(2, 65, 14000, 7000, 16385, "bitmap256k", "dense16k"), G8])
probe("d2_passes_4_5", "sort", [R(3, 65, 14000, 7000, 65536, "bitmap256k", "dense16k"), R(2, 65, 14000, 7000, 65537, "bitmap256k", "global"), G8])
probe("d2_passes_1", "sort", [R(3, 65, 14000, 7000, 16384, "bitmap256k", "dense16k"), R(2, 65, 14000, 7000, 16385, "bitmap256k", "global"), G8],
      opts=dict(num_global_passes=1))
probe("d2_passes_8", "sort", [R(3, 65, 14000, 7000, 65537, "bitmap256k", "dense16k"), R(2, 65, 14000, 7000, (8 << 14) + 1, "bitmap256k", "global"), G8],
      opts=dict(num_global_passes=8))
# NUM_NFCOPY: the scratch slot holds min(range, ops) entries -- range < ops, ==, >
probe("nf_slot_min_range_ops", "sort", [R(3, 65, 2000, 1000, 1500, "numeric_first", "nfcopy"), R(4, 65, 1500, 1000, 1500, "numeric_first", "nfcopy"),
                                        R(2, 65, 1000, 800, 1500, "numeric_first", "nfcopy"), R(2, 65, 1500, 1500, 1500, "numeric_first", "nfcopy"), G8])

# ---- staging: len_a at one group width and one more; ops at the owner window of 256 products --------------------------------
probe("stage_wave_classes", "staging", [R(5, 32, 320, 100, W, "bitmap256k", "wave256"), R(3, 33, 330, 100, W, "bitmap256k", "wave256"),
                                        R(5, 64, 320, 300, W, "bitmap256k", "wave512"), R(3, 65, 325, 300, W, "bitmap256k", "wave512"),
                                        R(4, 64, 320, 300, 20000, "wave1k", "wave512"), R(2, 65, 325, 300, 20000, "wave1k", "wave512"),
                                        R(4, 32, 288, 60, W, "bitmap256k", "wave128"), R(2, 33, 297, 60, W, "bitmap256k", "wave128")])
probe("stage_block_classes", "staging", [R(4, 256, 1024, 1000, W, "bitmap256k", "block2k"), R(3, 257, 1028, 1000, W, "bitmap256k", "block2k"),
                                         R(4, 256, 1024, 1000, 40000, "block4k", "block2k"), R(3, 257, 1028, 1000, 40000, "block4k", "block2k"),
                                         R(3, 512, 4096, 4000, 20000, "bitmap256k", "block8k"), R(2, 513, 4104, 4000, 20000, "bitmap256k", "block8k"),
                                         R(3, 1024, 8192, 7000, 20000, "bitmap256k", "dense16k"), R(2, 1025, 8200, 7000, 20000, "bitmap256k", "dense16k")])
# the last B row ends exactly on a window of 256 products / one product beyond
probe("owner_window_256_257", "staging", [R(5, 128, 256, 100, W, "bitmap256k", "wave256"), R(3, 128, 257, 100, W, "bitmap256k", "wave256"),
                                          R(4, 128, 512, 100, 20000, "wave1k", "wave256"), R(2, 128, 513, 100, 20000, "wave1k", "wave256"),
                                          R(4, 256, 256, 256, W, "bitmap256k", "wave512"), R(2, 257, 257, 257, W, "bitmap256k", "wave512")])

# Edges no call can reach, and why (asserted with the real classifier in test_unreachable_edges_are_unreachable):
UNREACHABLE = {
    "SYM_GH ops 2^22 - 1 / 2^22 (kSymGhMaxOps)":
        "B has at most 2^27 columns, so a row spans at most 128 windows of 2^20 columns and the rule `fewer than gh_per_window "
        "(8192) products per window` already ends SYM_GH at 128 * 8192 = 2^20 products",
}


# ------------------------------------------------------------------------------------------------------------ the generator
def _pick(rng, k, n):
    """k distinct sorted integers of range(n)"""
    if k == 0:
        return np.zeros(0, dtype=np.int64)
    if n <= (1 << 21) or 4 * k >= n:
        return np.sort(rng.choice(n, size=k, replace=False)).astype(np.int64)
    got = np.unique(rng.integers(0, n, size=k + k // 8 + 16))
    while got.size < k:
        got = np.unique(np.concatenate([got, rng.integers(0, n, size=k)]))
    return np.sort(rng.choice(got, size=k, replace=False)).astype(np.int64)


def _b_rows(rng, r):
    """The rows of B one row of C is made of: (lengths[len_a], concatenated column ids).  The products fall on a sorted set S
    of nnz columns with S[0] = cmin, S[-1] = cmax; the `live` rows of B (all of them when ops >= len_a) share the products
    evenly and walk S round and round, so that S is covered as soon as ops >= nnz; rows of length zero lie BETWEEN them."""
    if r.ops == 0:
        return np.zeros(r.len_a, dtype=np.int64), np.zeros(0, dtype=np.int64)
    assert r.nnz <= r.ops and (r.nnz >= 2 or r.cmin == r.cmax) and r.nnz <= r.cmax - r.cmin + 1
    live = min(r.len_a, r.ops)
    ln = np.full(live, r.ops // live, dtype=np.int64)
    ln[:r.ops % live] += 1
    assert ln.max() <= r.nnz, "a sorted row of B cannot hold a column twice"
    S = np.array([r.cmin], dtype=np.int64)
    if r.nnz >= 2:
        S = np.concatenate([[r.cmin], r.cmin + 1 + _pick(rng, r.nnz - 2, r.cmax - r.cmin - 1), [r.cmax]]).astype(np.int64)
    start = np.cumsum(ln) - ln
    j = np.repeat(np.arange(live), ln)
    t = np.arange(r.ops) - np.repeat(start, ln)
    col = S[(np.repeat(start, ln) + t) % r.nnz]
    col = col[np.lexsort((col, j))]
    lengths = np.zeros(r.len_a, dtype=np.int64)
    lengths[(np.arange(live) * r.len_a) // live] = ln          # spread over the len_a entries of the A row
    return lengths, col


@functools.lru_cache(maxsize=None)
def build(name):
    """(A, B, rows) of a probe: rows[i] is the Row (count = 1) that row i of C must be; the rows are shuffled, every row of A
    owns its rows of B (consecutive ids) unless its Row says share; dyadic values: exact_spgemm is THE answer bit for bit."""
    p = next(q for q in PROBES if q.name == name)
    rng = np.random.default_rng([PROBES.index(p), 20])
    specs, b_len, b_col, a_cols = [], [], [], []
    next_b = 0
    for r in p.rows:
        for k in range(r.count):
            if k == 0 or not r.share:
                lengths, col = _b_rows(rng, r)
                first_b = next_b
                next_b += r.len_a
                b_len.append(lengths)
                b_col.append(col)
            specs.append(r._replace(count=1))
            a_cols.append(np.arange(first_b, first_b + r.len_a, dtype=np.int64))
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    a_cols = [a_cols[i] for i in order]
    b_len, b_col = np.concatenate(b_len), np.concatenate(b_col)
    cols = p.cols or int(max(r.cmax for r in p.rows)) + 4
    assert b_col.size == 0 or b_col.max() < cols
    a_ro = np.concatenate([[0], np.cumsum([c.size for c in a_cols])]).astype(np.uint32)
    a_ci = np.concatenate(a_cols).astype(np.uint32)
    A = po.HostCSR(len(specs), next_b, a_ro, a_ci, _dyadic(rng, a_ci.size, -3, 3))
    B = po.HostCSR(next_b, cols, np.concatenate([[0], np.cumsum(b_len)]).astype(np.uint32), b_col.astype(np.uint32),
                   _dyadic(rng, b_col.size, -3, 3))
    return A, B, specs


def as_dtype(M, dtype):
    return po.HostCSR(M.rows, M.cols, M.row_offsets, M.col_ids, M.data.astype(dtype))


@functools.lru_cache(maxsize=8)
def expected(name, dtype):
    A, B, _ = build(name)
    return exact_spgemm(as_dtype(A, dtype), as_dtype(B, dtype))


def class_counts(p):
    """(sym_bin_rows, num_bin_rows) a complete call on the probe must report: every class, zero where no row goes"""
    sym, num = dict.fromkeys(SYM_NAMES, 0), dict.fromkeys(NUM_NAMES, 0)
    for r in p.rows:
        if r.sym is not None:
            sym[r.sym] += r.count
        if r.num is not None:
            num[r.num] += r.count
    return sym, num


def params_of(p):
    """ClassifyParams of a call on the probe: the defaults, the probe's options, what the call derives on top"""
    cp = dict(CP_DEFAULT)
    cp.update({k: v for k, v in p.opts.items() if k in cp})
    cp.update(p.cp)
    return cp


# ------------------------------------------------------------------------------------------------------------ the header
@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("classify") / "classify_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           "-I", os.path.join(ROOT, "speck_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "classify_probe.cpp"),
                           "-o", exe])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines) and not any(o.startswith("error") for o in out), out[:3]
        return [[int(x) for x in o.split()] for o in out]
    return ask


def _classify_line(len_a, ops, nnz, cmin, cmax, cp):
    return "C " + " ".join(str(int(x)) for x in [len_a, ops, nnz, cmin, cmax] + [cp[f] for f in CP_FIELDS])


def _name(names, k):
    return None if k == NO_CLASS else names[k]


# ------------------------------------------------------------------------------------------------------------ the tests
def test_the_table_names_every_class_and_the_api_reports_them_in_enum_order():
    import speck_amd.api as api
    assert api.SYM_CLASS_NAMES == SYM_NAMES and api.NUM_CLASS_NAMES == NUM_NAMES
    sym = {r.sym for p in PROBES for r in p.rows}
    num = {r.num for p in PROBES for r in p.rows}
    assert sym == set(SYM_NAMES) | {None} and num == set(NUM_NAMES) | {None}
    for p in PROBES:      # the two sides of an edge are told apart by their row counts wherever their classes differ
        s, n = class_counts(p)
        assert sum(s.values()) == sum(r.count for r in p.rows if r.sym) and sum(n.values()) == sum(r.count for r in p.rows if r.num)


@pytest.mark.parametrize("name", [p.name for p in PROBES])
def test_generator_builds_the_rows_it_claims(name):
    A, B, specs = build(name)
    C, _ = po.spgemm(A, B)
    a_ro, b_ro, c_ro = (M.row_offsets.astype(np.int64) for M in (A, B, C))
    b_len = np.diff(b_ro)
    assert A.rows == len(specs) == C.rows and A.cols == B.rows
    for M in (A, B):      # sorted rows without duplicates: what the library requires of its inputs
        ro = M.row_offsets.astype(np.int64)
        inner = np.ones(M.nnz, dtype=bool)
        inner[ro[:-1][np.diff(ro) > 0]] = False
        assert (np.diff(M.col_ids.astype(np.int64))[inner[1:]] > 0).all() and (M.nnz == 0 or M.col_ids.max() < M.cols)
    for i, r in enumerate(specs):
        k = A.col_ids[a_ro[i]:a_ro[i + 1]].astype(np.int64)
        row = C.col_ids[c_ro[i]:c_ro[i + 1]]
        assert k.size == r.len_a, (i, r)
        assert b_len[k].sum() == r.ops, (i, r)
        assert row.size == r.nnz, (i, r, row.size)
        if r.nnz:
            assert (int(row[0]), int(row[-1])) == (r.cmin, r.cmax), (i, r, row[0], row[-1])
            live = b_len[k] > 0                                   # the range the analysis sees: first / last entry of each B row
            assert B.col_ids[b_ro[k][live]].min() == r.cmin and B.col_ids[b_ro[k + 1][live] - 1].max() == r.cmax
        if r.len_a > r.ops > 0:
            assert b_len[k][-1] == 0 and (b_len[k][:-1] > 0).any()   # empty rows of B between and behind the others
    E = expected(name, np.float64)                                # the exact reference has the oracle's structure
    assert (E.row_offsets == C.row_offsets).all() and (E.col_ids == C.col_ids).all()
    p = next(q for q in PROBES if q.name == name)
    assert B.cols <= 1 << 27 and (p.cols is None or B.cols == p.cols)


@pytest.mark.parametrize("name", [p.name for p in PROBES])
def test_header_gives_every_row_its_literal_class(classify, name):
    p = next(q for q in PROBES if q.name == name)
    cp = params_of(p)
    got = classify([_classify_line(r.len_a, r.ops, r.nnz, r.cmin, r.cmax, cp) for r in p.rows])
    for r, (s, n) in zip(p.rows, got):
        assert (_name(SYM_NAMES, s), _name(NUM_NAMES, n)) == (r.sym, r.num), (name, r, cp)


def test_probe_options_are_the_ones_the_issue_lists():
    """every option a call of the GPU module switches appears in the table, away from its default"""
    switched = {k for p in PROBES for k, v in list(p.opts.items()) + list(p.cp.items()) if k in CP_DEFAULT and v != CP_DEFAULT[k]}
    assert switched >= {"esc16", "esc32", "esc64", "num_g8", "sym_g8", "sym_w128", "num_w256", "nf_min_ops", "sym_bitmap_ratio",
                        "num_dense_ratio", "gh_per_window", "num_global_passes"}


def test_replayed_register_rows_are_booked_as_nfcopy(classify):
    """esc_fused (a replayed sequence): the register-class rows are NUM_NFCOPY, every other row keeps its class"""
    cp = dict(CP_DEFAULT, esc_fused=1)
    rows = [r for p in PROBES if not p.opts and not p.cp for r in p.rows]
    got = classify([_classify_line(r.len_a, r.ops, r.nnz, r.cmin, r.cmax, cp) for r in rows])
    for r, (s, n) in zip(rows, got):
        assert _name(SYM_NAMES, s) == r.sym
        assert _name(NUM_NAMES, n) == ("nfcopy" if r.num in ("g8", "g16", "r32", "r64") else r.num), r


def test_table_bits_and_max_nnz_of_against_the_documented_rule(classify):
    """table_bits(nnz, pct) is the smallest bits >= 1 with
         pct 67: nnz + floor(nnz / 2) <= 2^bits   (load <= 2/3 for even nnz; odd nnz up to one entry above: 43 in 64, 11 in 16, 3 in 4)
         pct 85: 100 nnz <= 85 * 2^bits
    and max_nnz_of(cap, pct) is the largest nnz at load <= 2/3 / 0.85 -- for 85 exactly the largest that gets `cap`, for 67 that
    or one less (log2(cap) even)."""
    assert classify(["K"]) == [[85, 67]]
    N = 8192
    for pct in (67, 85):
        got = [b for (b,) in classify([f"T {n} {pct}" for n in range(1, N + 1)])]
        for n, bits in zip(range(1, N + 1), got):
            fits = (lambda b: n + n // 2 <= 1 << b) if pct == 67 else (lambda b: 100 * n <= 85 * (1 << b))
            assert bits >= 1 and fits(bits) and (bits == 1 or not fits(bits - 1)), (n, pct, bits)
            assert n < 1 << bits                                    # a table never fills
            if pct == 67:
                assert 4 * n <= 3 * (1 << bits), (n, bits)          # load <= 3/4 at the worst ...
                assert n % 2 or 3 * n <= 2 * (1 << bits), (n, bits)  # ... and <= 2/3 for every even nnz
        caps = [1 << b for b in range(2, 14)]
        mx = [m for (m,) in classify([f"M {cap} {pct}" for cap in caps])]
        for cap, m in zip(caps, mx):
            log2 = cap.bit_length() - 1
            assert m == (2 * cap // 3 if pct == 67 else 85 * cap // 100)
            if m <= N:
                assert got[m - 1] == log2, (cap, pct, m)            # the class limit gets the class's capacity
            largest = max(n for n in range(1, N + 1) if got[n - 1] <= log2) if cap < N else None
            if largest is not None:
                assert largest == (m + (1 if log2 % 2 == 0 else 0) if pct == 67 else m), (cap, pct, largest, m)
    # the figures named in the table above
    bits67 = dict(zip(range(1, N + 1), [b for (b,) in classify([f"T {n} 67" for n in range(1, N + 1)])]))
    assert [bits67[n] for n in (3, 11, 21, 22, 42, 43, 44, 85)] == [2, 4, 5, 6, 6, 6, 7, 7]
    bits85 = [b for (b,) in classify([f"T {n} 85" for n in (435, 436, 870, 871, 1740, 1741, 3481, 3482, 6963, 6964)])]
    assert bits85 == [9, 10, 10, 11, 11, 12, 12, 13, 13, 14]


def test_scratch_slots_of_numeric_first_and_global_key_set_rows(classify):
    assert classify(["S 5 1504 2000", "S 5 1504 1500", "S 5 1504 1000", "S 0 4095 4096", "S 0 4095 512"]) == [[1500], [1500], [1000], [4096], [512]]
    assert classify(["G 1", "G 32767", "G 32768", "G 32769", "G 65536", "G 65537", "G 4194303", "G 4194304", "G 4294967295"]) == \
        [[65536], [65536], [65536], [131072], [131072], [262144], [8388608], [8388608], [8388608]]


def test_unreachable_edges_are_unreachable(classify):
    """SYM_GH's own limit of 2^22 products: with gh_per_window = 8192 and at most 2^27 columns the per-window rule ends the class
    at 2^20 products -- shown with the real classifier at the widest row a call accepts; the limit itself holds in the header
    (seen with a gh_per_window no shipped config has)."""
    assert len(UNREACHABLE) == 1
    widest = (0, (1 << 27) - 1)
    q = lambda ops, cp: _classify_line(65, ops, ops, widest[0], widest[1], cp)
    got = classify([q((1 << 20) - 1, CP_DEFAULT), q(1 << 20, CP_DEFAULT), q((1 << 22) - 1, CP_DEFAULT), q(1 << 22, CP_DEFAULT)])
    assert [_name(SYM_NAMES, s) for s, _ in got] == ["global_hash", "bitmap1m", "bitmap1m", "bitmap1m"]
    big = dict(CP_DEFAULT, gh_per_window=1 << 16)
    got = classify([q((1 << 22) - 1, big), q(1 << 22, big)])
    assert [_name(SYM_NAMES, s) for s, _ in got] == ["global_hash", "bitmap1m"]
