"""Rows of A placed at every POSITIONAL switch of the two integer kernels of a multiply (analysis_kernel / scan_kernel,
speck_amd/csrc/stages.hip): the layout table, the generator that builds matrices from it, and their checks without a GPU.

test_edges_host.py pins what a row becomes from its own four integers.  Here the rows are ordinary; what is exact is WHERE
they lie: which sub-chunk of R = 32 / 64 rows of which 256-row chunk of which analysis workgroup, at which entry offset of a
tile of 64 x U entries, in which scan tile at which thread.  The switches ("positional switches"):
  * a sub-chunk takes a lane per row when its longest row has <= kAnRowPathMax entries, the tile walk otherwise;
  * a sub-chunk whose longest row has > kAnCoopRowLen entries AND that holds > kAnCoopEntries * R / 32 entries goes on the
    workgroup's hub list -- which has kAnCoopMax places;
  * a workgroup bins kChunk rows per pass and carries the class places and the scratch-slot offset to the next pass;
  * a scan tile is kScanThreads x ITEMS rows (ITEMS 2 / 3 / 4 by option, 8 above 2^19 rows, 32 above 2^23), two sub-tiles
    above 2^25 rows.
A layout is a list of sub-chunks (A1 .. A4: literal (longest row, entries, path) per sub-chunk) or of placed rows (A5, A6,
S1 .. S3); build(layout, R) makes (A, B, claims) of it.  Here: the generator is what it claims (oracle), the table's
statements hold against the constants read from stages.hip, and row_chunking / scan_tiles in exact integers.
tests/test_gpu_stages.py runs the same layouts through the kernels.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from test_edges_host import CP_DEFAULT, NUM_NAMES, SYM_NAMES, R as edge_row, Row, _b_rows, _classify_line, _pick, classify  # noqa: F401
from test_gpu_values import _dyadic, exact_spgemm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CLASS = 0xFF

# ---- the constants the table is written against (test_constants_guard reads them from stages.hip) ------------------------
K = dict(kChunk=256, kAnRowPathMax=8, kAnCoopMax=64, kAnCoopRowLen=256, kAnCoopEntries=2048, U=4, kScanThreads=256,
         g_an_wide_rows=16, g_scan_small=3)
MAX_BLOCKS = 1024                    # row_chunking: at most this many analysis workgroups
SCAN_8, SCAN_32, SCAN_SUB = 1 << 19, 1 << 23, 1 << 25      # rows(A) above which a thread scans 8 / 32 rows / a tile has sub-tiles
SHAPES = (32, 64)                    # R: rows per sub-chunk (8 waves x 32, 4 waves x 64)
SPARE_LEN = 5                        # entries of the spare row of B every row of A leaves unreferenced (no row of B a
                                     #   layout references has 5 entries: moving an entry onto it changes the products)
W = 5000                             # a column range above 4096: neither numeric-first nor the dense class


def hub_entries(R):
    """E: a sub-chunk with a row of more than kAnCoopRowLen entries is a hub sub-chunk above this many entries"""
    return K["kAnCoopEntries"] * R // 32


def row_chunking(m):
    """(rows per analysis workgroup, workgroups): contiguous rows, a multiple of kChunk, at most 1024 workgroups"""
    r = -(-max(m, 1) // MAX_BLOCKS)
    r = -(-r // K["kChunk"]) * K["kChunk"]
    return r, -(-max(m, 1) // r)


def scan_shape(m, small=None):
    """(rows per thread, sub-tiles per tile, tiles) of scan_kernel"""
    items = (small or K["g_scan_small"]) if m <= SCAN_8 else (8 if m <= SCAN_32 else 32)
    sub = 1 if m <= SCAN_SUB else -(-m // SCAN_SUB)
    return items, sub, -(-max(m, 1) // (K["kScanThreads"] * items * sub))


# ---- rows -------------------------------------------------------------------------------------------------------------------
# the classed rows, with the classes test_edges_host.PROBES states for them literally (name -> Row)
KINDS = {
    "direct": edge_row(1, 1, 6, 6, W, None, "direct"),
    "g8": edge_row(1, 2, 4, 4, W, "g8", "g8"),
    "r64": edge_row(1, 64, 256, 256, W, "r64", "r64"),
    "wave128": edge_row(1, 65, 85, 85, W, "wave128", "wave128"),
    "block2k": edge_row(1, 65, 819, 819, 27000, "wave1k", "block2k"),
    "nf": edge_row(1, 65, 600, 300, 4096, "numeric_first", "nfcopy"),
    "dense4k": edge_row(1, 65, 400, 300, 4096, "bitmap256k", "dense4k"),
    "gh": edge_row(1, 65, 4 * 8192 - 1, 4 * 8192 - 1, 4 << 20, "global_hash", "global"),
}
SCAN_KINDS = ["direct", "g8", "wave128", "block2k", "nf", "dense4k"]      # S1 .. S3: six numeric classes

# a placed row: its index in A, its Row, the entries of it that point to EMPTY rows of B, and whether rows with the same
# (Row, zeros) reference the same rows of B
Placed = collections.namedtuple("Placed", "row spec zeros share")
# a sub-chunk of the table: index (rows [index R, index R + R)), longest row, entries, path ("lane" / "tile" / "hub"; None:
# the layout makes no statement; a "hub" sub-chunk that finds no place on the workgroup's list is walked by its wave)
Sub = collections.namedtuple("Sub", "index max_len entries path")
Layout = collections.namedtuple("Layout", "m placed subs opts targets")
Claims = collections.namedtuple("Claims", "m rows len_a ops mx cmin cmax nnz subs b_first")


def plain(n, zeros=(), i=0):
    """A row of n entries of A onto rows of B with 1 .. 3 entries (`zeros`: onto empty ones; "all": every entry); the column
    range differs from row to row (i), so that a minimum or maximum that leaks into a neighbour shows"""
    zeros = tuple(range(n)) if zeros == "all" else tuple(zeros)
    live = n - len(zeros)
    c0, rng = 5 + 3 * (i % 11), W - (i % 13)
    if live == 0:
        return Row(1, n, 0, 0, c0, c0, None, None, False), zeros
    ops = 3 if live == 1 else live + live // 2
    nnz = min(ops, 2000)
    return Row(1, n, ops, nnz, c0, c0 + rng - 1, None, None, False), zeros


def _sub_rows(index, R, items, at=0):
    """the rows of sub-chunk `index`: items (n or (n, zeros)) from offset `at` (negative: the last item on row R - 1)"""
    if at < 0:
        at = R - len(items)
    out = []
    for j, it in enumerate(items):
        n, zeros = (it, ()) if isinstance(it, int) else it
        if n:
            row = index * R + at + j
            out.append(Placed(row, *plain(n, zeros, row), False))
    return out


def _table(R, subs, m=None, targets=None):
    """Layout of literal sub-chunks [(max_len, entries, path, items, at)], in order from sub-chunk 0"""
    placed, table = [], []
    for index, (max_len, entries, path, items, at) in enumerate(subs):
        placed += _sub_rows(index, R, items, at)
        table.append(Sub(index, max_len, entries, path))
    return Layout(m or len(subs) * R, placed, table, {}, targets or {})


def _derived_subs(m, R, placed):
    """(max_len, entries) per non-empty sub-chunk from the SPECS of the placed rows; no statement about the path"""
    acc = {}
    for p in placed:
        mx, n = acc.get(p.row // R, (0, 0))
        acc[p.row // R] = (max(mx, p.spec.len_a), n + p.spec.len_a)
    return [Sub(i, mx, n, None) for i, (mx, n) in sorted(acc.items())]


def _kinds_at(m, R, positions, kinds, opts=None):
    pos = sorted({int(p) for p in positions if 0 <= p < m})
    placed = [Placed(p, KINDS[kinds[i % len(kinds)]], (), False) for i, p in enumerate(pos)]
    return Layout(m, placed, _derived_subs(m, R, placed), opts or {}, {})


# ---- A1: the lane-per-row path up to 8 entries, the tile walk from 9 -----------------------------------------------------------
def _row_path_8_9(R):
    return _table(R, [
        (0, 0, "lane", [], 0),
        (1, 4, "lane", [1, 0, (1, [0]), 1, 0, 0, 1], 0),
        (4, 25, "lane", [4, 0, 1, 2, 3, (4, [0]), (4, [3]), (3, "all"), 4], -1),            # one round of the U loop
        (5, 29, "lane", [5, (5, [0]), (5, [4]), (5, "all"), 0, 3, 1, 5], 3),                # two rounds
        (8, 57, "lane", [8, (8, [0]), (8, [7]), 7, 0, (8, "all"), 4, 5, 1, 8], -1),
        (9, 63, "tile", [9, (9, [0]), (9, [8]), 8, 0, (9, "all"), 1, 4, 5, 9], 0),
        (8, 18, "lane", [8, 8, 0, 2], -1),
    ], targets=dict(lane=4 * R + R - 10, tile=5 * R))


# ---- A2: tiles of 64 x U = 256 entries, 16-lane groups of the segmented reduction ---------------------------------------------
def _tile_256_257(R):
    g = lambda a, b: list(range(a, b))
    return _table(R, [
        # rows start at entry offsets 0, 15, 31 (= 15 mod 16), 48, 79, 111, 144, 207; empty rows first, two between, last
        (63, 255, "tile", [0, (15, g(0, 3)), (16, g(13, 16)), (17, "all"), 0, 0, 31, 32, 33, (63, g(16, 32)), 48, 0], 0),
        # ... at 0, 1, 16, 32, 49, 113, 178, 209; the 64-entry row has lanes 64 .. 79 of the tile onto empty rows of B
        (65, 256, "tile", [1, 15, 16, 17, (64, g(15, 31)), (65, [0, 64]), 0, 31, 47], 0),
        (64, 257, "tile", [0, 0, 32, 33, 1, 63, 64, 0, 64], 0),
        # a 300-entry row across two tiles: its entries 255, 256 and the whole group 272 .. 287 onto empty rows of B
        (300, 511, "tile", [(300, [255, 256] + g(272, 288)), 15, 17, 31, 33, 65, 50], 0),
        (300, 512, "tile", [15, (300, [0] + g(241, 257)), (1, "all"), 16, 64, 63, 53], -1),
        # 255 entries end exactly on the first tile; the longest row has kAnCoopRowLen entries
        (256, 513, "tile", [0, 1, (255, [254]), (1, "all"), 256], 0),
    ], targets=dict(tile=3 * R))


# ---- A3: whole matrices whose last sub-chunk is partial -----------------------------------------------------------------------
_TILE_LENS = [12, 0, 9, 3, 40, 1, 17, 0, 0, 8, 33, 2]
_LANE_LENS = [1, 8, 0, 3, 5, 0, 0, 7, 2, 4, 6]
PARTIAL_M = {"1": lambda R: 1, "Rm1": lambda R: R - 1, "R": lambda R: R, "Rp1": lambda R: R + 1, "255": lambda R: 255,
             "256": lambda R: 256, "257": lambda R: 257, "511": lambda R: 511, "513": lambda R: 513}


def _partial(which):
    def make(R):
        m = PARTIAL_M[which](R)
        placed, table = [], []
        for s in range(-(-m // R)):
            tile = s % 2 == 0                               # even sub-chunks walk tiles, odd ones take a lane per row
            lens = [(_TILE_LENS if tile else _LANE_LENS)[(j + s) % (12 if tile else 11)] for j in range(min(R, m - s * R))]
            lens[0] = 12 if tile else 1
            if s * R + len(lens) == m:
                lens[-1] = max(lens[-1], 2)                 # the last row of the matrix is not empty
            zeros = lambda j, n: [0] if (j % 5 == 1 and n > 1) else ([n - 1] if j % 5 == 3 and n > 1 else ())
            placed += _sub_rows(s, R, [(n, zeros(j, n)) for j, n in enumerate(lens)], 0)
            table.append(Sub(s, max(lens), sum(lens), "tile" if tile else "lane"))
        return Layout(m, placed, table, {}, {})
    return make


# ---- A4: the two thresholds of a hub sub-chunk ----------------------------------------------------------------------------------
def _hub_thresholds(R):
    E = hub_entries(R)
    n = E // 256
    hub = (E + 1, [0, 255, 256, E] + list(range(1024, 1040)))      # the row that holds E + 1 entries, some onto empty rows of B
    return _table(R, [
        (256, E + 500, "tile", [256] * (n + 1) + [244], 0),           # entries beyond E, but no row beyond kAnCoopRowLen
        (257, E, "tile", [257] + [256] * (n - 2) + [255], 0),         # a row beyond it, entries exactly E
        (257, E + 1, "hub", [257] + [256] * (n - 1), 0),
        (E + 1, E + 1, "hub", [hub], -1),                             # one row holds everything: row R - 1 of its sub-chunk
        (E + 1, E + 13, "hub", [hub, 1, 3, 0, 8], 0),                 # ... row 0, short rows behind it
        (E + 1, E + 11, "hub", [2, 8, hub], 0),                      # ... in the last, partial sub-chunk of the matrix
    ], m=5 * R + R // 2, targets=dict(hub=3 * R + R - 1, last_partial=5 * R + 2))


# ---- A5: 64, 65 and 66 hub sub-chunks in one workgroup (the list has kAnCoopMax places) ------------------------------------------
A5_M = 4194305
A5_GROUPS = {100: 64, 500: 65, 900: 66}       # workgroup -> hub sub-chunks in it


def _hub_list_64_65(R):
    E = hub_entries(R)
    per, blocks = row_chunking(A5_M)
    hub_spec, hub_zeros = plain(E + 1, [0, 300, E], 1)
    placed, table, targets = [], [], {}
    for wg, hubs in A5_GROUPS.items():
        first = wg * per // R                                       # the workgroup's sub-chunks: first .. first + per / R - 1
        for k, kind in ((0, "g8"), (per // R - 1, "wave128")):       # rows of other classes in the first and last of them
            rows = [Placed((first + k) * R + j, KINDS[kd], (), False) for j, kd in ((0, kind), (7, "direct"), (R - 1, "r64"))]
            placed += rows
            table += _derived_subs(A5_M, R, rows)
        for h in range(hubs):
            s = first + 1 + h
            at = (5 * h) % R
            rows = [Placed(s * R + at, hub_spec, hub_zeros, True)]
            rows += _sub_rows(s, R, [3], (at + 1) % R) + (_sub_rows(s, R, [1], (at + 9) % R) if h % 2 else [])
            placed += rows
            table.append(Sub(s, E + 1, E + 1 + 3 + (1 if h % 2 else 0), "hub"))
            if h in (0, 33, 65):
                targets[f"hub{hubs}_{h}"] = s * R + at
    placed.append(Placed(A5_M - 1, KINDS["direct"], (), False))     # the single row of the last workgroup
    table += _derived_subs(A5_M, R, placed[-1:])
    return Layout(A5_M, sorted(placed), sorted(table), {}, targets)


# ---- A6: rows that own a class place or a scratch slot in the second .. fourth chunk of a workgroup --------------------------
def _later_chunks(m):
    def make(R):
        per, blocks = row_chunking(m)
        chunks = per // K["kChunk"]
        # first / last row of chunk 0 .. 3 of a workgroup: every chunk holds a row with a scratch slot (nf, gh)
        first_kinds = ["nf", "g8", "nf", "wave128"]
        last_kinds = ["r64", "nf", "block2k", "nf"]
        placed = []
        for n, wg in enumerate((0, 1, (blocks - 1) // 2, blocks - 2)):
            for c in range(chunks):
                at = wg * per + c * 256
                placed.append(Placed(at, KINDS[first_kinds[c]], (), False))
                kind = "gh" if (n, c) in ((1, 0), (2, chunks - 1)) else last_kinds[c]     # two global-hash rows
                if kind != "nf" and first_kinds[c] != "nf":
                    placed.append(Placed(at + 100, KINDS["nf"], (), False))
                placed.append(Placed(at + 255, KINDS[kind], (), False))
        placed.append(Placed(m - 1, KINDS["g8"], (), False))         # the single row of the last workgroup
        return Layout(m, sorted(placed), _derived_subs(m, R, placed), {}, {})
    return make


# ---- S1 .. S3: scan tiles ----------------------------------------------------------------------------------------------------
def _scan_items(items, which):
    def make(R):
        T = K["kScanThreads"] * items
        m = {"Tm1": T - 1, "T": T, "Tp1": T + 1, "3Tp1": 3 * T + 1}[which]
        rel = [0, 1, items - 1, items, 64 * items - 1, 64 * items, T - 1]
        return _kinds_at(m, R, [t * T + p for t in range(4) for p in rel] + [m - 1], SCAN_KINDS, dict(scan_small_items=items))
    return make


def _around(xs):
    return [x + d for x in xs for d in (-1, 0, 1)]


def _scan_2p19(m):
    mid = m // 2
    mult = lambda step, x: x // step * step
    pos = _around([0, 768, 2048, mult(768, mid), mult(2048, mid), mult(768, m - 2), mult(2048, m - 2)]) + [m - 1]
    return lambda R: _kinds_at(m, R, pos, SCAN_KINDS)


def _scan_wide(m):
    pos = _around([8192, 16384, 1 << 24]) + [0, (1 << 25) - 1, 1 << 25]
    return lambda R: _kinds_at(m, R, pos, SCAN_KINDS)


LAYOUTS = collections.OrderedDict()
LAYOUTS["row_path_8_9"] = _row_path_8_9
LAYOUTS["tile_256_257"] = _tile_256_257
for _w in PARTIAL_M:
    LAYOUTS[f"partial_{_w}"] = _partial(_w)
LAYOUTS["hub_thresholds"] = _hub_thresholds
LAYOUTS["hub_list_64_65"] = _hub_list_64_65
LAYOUTS["later_chunks_262145"] = _later_chunks(262145)
LAYOUTS["later_chunks_786433"] = _later_chunks(786433)
for _i in (2, 3, 4):
    for _w in ("Tm1", "T", "Tp1", "3Tp1"):
        LAYOUTS[f"scan_items_{_i}_{_w}"] = _scan_items(_i, _w)
LAYOUTS["scan_2p19"] = _scan_2p19(1 << 19)
LAYOUTS["scan_2p19_plus_1"] = _scan_2p19((1 << 19) + 1)
LAYOUTS["scan_wide_2p25"] = _scan_wide(1 << 25)
LAYOUTS["scan_wide_2p25_plus_1"] = _scan_wide((1 << 25) + 1)

ANALYSIS = [n for n in LAYOUTS if not n.startswith("scan_")]
SCAN = [n for n in LAYOUTS if n.startswith("scan_")]
# (layout, R): the analysis layouts in both shapes, the scan layouts once (their analysis shape is the default's choice)
CASES = [(n, R) for n in ANALYSIS for R in SHAPES] + [(n, 32) for n in SCAN]
CASE_IDS = [f"{n}-R{R}" for n, R in CASES]


@functools.lru_cache(maxsize=None)
def layout(name, R):
    return LAYOUTS[name](R)


# ------------------------------------------------------------------------------------------------------------ the generator
def _rows_of_b(rng, spec, zeros):
    """(lengths[len_a], column ids) of the rows of B behind one row of A: _b_rows for the live entries, empty rows at `zeros`"""
    if not zeros:
        return _b_rows(rng, spec)
    live = spec.len_a - len(zeros)
    if live == 0:
        return np.zeros(spec.len_a, dtype=np.int64), np.zeros(0, dtype=np.int64)
    ln, col = _b_rows(rng, spec._replace(len_a=live))
    assert (ln > 0).all()
    lengths = np.zeros(spec.len_a, dtype=np.int64)
    lengths[np.setdiff1d(np.arange(spec.len_a), np.array(zeros))] = ln
    return lengths, col


def a_col_ids(first_b, len_a):
    """the column ids of a row of A over its block of len_a + 1 rows of B: the block's row len_a // 2 stays unreferenced"""
    k = first_b + np.arange(len_a, dtype=np.int64)
    k[len_a // 2:] += 1
    return k


@functools.lru_cache(maxsize=None)
def build(name, R):
    """(A, B, claims) of a layout: every row of A named by the layout is the Row it states, every other row is empty.  A row
    of A owns a block of len_a + 1 consecutive rows of B -- one of them, in the middle of the block, is a SPARE of SPARE_LEN
    entries no row references (so that one column id of A can move onto it and stay between its neighbours).  Dyadic values:
    exact_spgemm is THE answer bit for bit."""
    L = layout(name, R)
    rng = np.random.default_rng([list(LAYOUTS).index(name), R, 7])
    n = len(L.placed)
    rows = np.array([p.row for p in L.placed], dtype=np.int64)
    assert (np.diff(rows) > 0).all() and (n == 0 or rows[-1] < L.m)
    b_len, b_col, a_cols, b_first, shared = [], [], [], np.zeros(n, dtype=np.int64), {}
    mx = np.zeros(n, dtype=np.int64)
    next_b = 0
    cols = int(max([p.spec.cmax for p in L.placed] + [0])) + 4
    for i, p in enumerate(L.placed):
        key = (p.spec, p.zeros)
        if p.share and key in shared:
            b_first[i], mx[i] = shared[key]
        else:
            lengths, col = _rows_of_b(rng, p.spec, p.zeros)
            spare = p.spec.len_a // 2
            parts = np.split(col, np.cumsum(lengths)[:-1]) if p.spec.len_a > 1 else [col]
            parts.insert(spare, _pick(rng, SPARE_LEN, cols))
            b_len.append(np.insert(lengths, spare, SPARE_LEN))
            b_col.append(np.concatenate(parts))
            b_first[i], mx[i] = next_b, lengths.max()
            next_b += p.spec.len_a + 1
            if p.share:
                shared[key] = (b_first[i], mx[i])
        a_cols.append(a_col_ids(b_first[i], p.spec.len_a))
    len_a = np.array([p.spec.len_a for p in L.placed], dtype=np.int64)
    a_ro = np.zeros(L.m + 1, dtype=np.int64)
    a_ro[rows + 1] = len_a
    a_ro = np.cumsum(a_ro).astype(np.uint32)
    a_ci = np.concatenate(a_cols).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    b_len = np.concatenate(b_len) if n else np.zeros(0, dtype=np.int64)
    b_col = np.concatenate(b_col) if n else np.zeros(0, dtype=np.int64)
    A = po.HostCSR(L.m, next_b, a_ro, a_ci, _dyadic(rng, a_ci.size, -3, 3))
    B = po.HostCSR(next_b, cols, np.concatenate([[0], np.cumsum(b_len)]).astype(np.uint32), b_col.astype(np.uint32),
                   _dyadic(rng, b_col.size, -3, 3))
    ops = np.array([p.spec.ops for p in L.placed], dtype=np.int64)
    live = ops > 0                                                   # (a row without products: the analysis' neutral elements)
    claims = Claims(L.m, rows, len_a, ops, mx,
                    np.where(live, [p.spec.cmin for p in L.placed], 0xFFFFFFFF).astype(np.int64),
                    np.where(live, [p.spec.cmax for p in L.placed], 0).astype(np.int64),
                    np.array([p.spec.nnz for p in L.placed], dtype=np.int64), {s.index: s for s in L.subs}, b_first)
    return A, B, claims


def full(claims, field):
    """a per-row claim as an array over all rows of A (u32, as the analysis writes it)"""
    out = np.full(claims.m, 0xFFFFFFFF if field == "cmin" else 0, dtype=np.uint32)
    out[claims.rows] = getattr(claims, field)
    return out


def expand_rows(Cc, rows, m):
    """the product of the compacted matrix (the non-empty rows of A) as a matrix of m rows"""
    ro = np.zeros(m + 1, dtype=np.int64)
    ro[rows + 1] = np.diff(Cc.row_offsets.astype(np.int64))
    return po.HostCSR(m, Cc.cols, np.cumsum(ro).astype(np.uint32), Cc.col_ids, Cc.data)


def exact_of(A, B):
    """exact_spgemm(A, B), computed on the non-empty rows of A only"""
    lens = np.diff(A.row_offsets.astype(np.int64))
    rows = np.flatnonzero(lens)
    Ac = po.HostCSR(rows.size, A.cols, np.concatenate([[0], np.cumsum(lens[rows])]).astype(np.uint32), A.col_ids, A.data)
    return expand_rows(exact_spgemm(Ac, B), rows, A.rows)


@functools.lru_cache(maxsize=4)
def expected(name, R):
    A, B, _ = build(name, R)
    return exact_of(A, B)


def rows_of(E, r0, r1):
    """rows [r0, r1) of a host matrix as a matrix of their own"""
    ro = E.row_offsets.astype(np.int64)
    return po.HostCSR(r1 - r0, E.cols, (ro[r0:r1 + 1] - ro[r0]).astype(np.uint32), E.col_ids[ro[r0]:ro[r1]], E.data[ro[r0]:ro[r1]])


def with_entry(A, e, k):
    """A with the column id of entry e replaced"""
    col = A.col_ids.copy()
    col[e] = k
    return po.HostCSR(A.rows, A.cols, A.row_offsets, col, A.data)


def movable_entry(A, row):
    """(entry, new id) of a row of A: the entry behind the spare row of B of its block, which lies between its neighbours"""
    a0, a1 = int(A.row_offsets[row]), int(A.row_offsets[row + 1])
    e = a0 + (a1 - a0) // 2
    return e, int(A.col_ids[e]) - 1


def class_counts(claims, classify, cp=None):
    """(sym_bin_rows, num_bin_rows) a complete call must report, by the real classifier applied to the claims"""
    cp = dict(CP_DEFAULT, **(cp or {}))
    keep = claims.len_a > 0
    rows = np.stack([claims.len_a, claims.ops, claims.nnz, np.where(claims.ops > 0, claims.cmin, 0xFFFFFFFF),
                     claims.cmax], axis=1)[keep]
    uniq, count = np.unique(rows, axis=0, return_counts=True)
    sym, num = dict.fromkeys(SYM_NAMES, 0), dict.fromkeys(NUM_NAMES, 0)
    got = classify([_classify_line(*u, cp) for u in uniq.tolist()]) if len(uniq) else []
    for (s, n), c in zip(got, count.tolist()):
        if s != NO_CLASS:
            sym[SYM_NAMES[s]] += c
        if n != NO_CLASS:
            num[NUM_NAMES[n]] += c
    return sym, num


def path_of(max_len, entries, R):
    """which side of which switch a sub-chunk is on, by the constants of the table"""
    if max_len > K["kAnCoopRowLen"] and entries > hub_entries(R):
        return "hub"
    return "lane" if max_len <= K["kAnRowPathMax"] else "tile"


# ------------------------------------------------------------------------------------------------------------ the tests
def test_constants_guard():
    """the literal values the layout table is written against; whoever changes one revisits the table"""
    src = open(os.path.join(ROOT, "speck_amd", "csrc", "stages.hip")).read()

    def value(pattern):
        found = re.findall(pattern, src)
        assert len(found) == 1, (pattern, found)
        return int(found[0])
    assert value(r"constexpr int kChunk = (\d+);") == K["kChunk"] == 256
    assert value(r"constexpr u32 kAnRowPathMax = (\d+);") == K["kAnRowPathMax"] == 8
    assert value(r"constexpr u32 kAnCoopMax = (\d+);") == K["kAnCoopMax"] == 64
    assert value(r"constexpr u32 kAnCoopRowLen = (\d+),") == K["kAnCoopRowLen"] == 256
    assert value(r"kAnCoopRowLen = \d+, kAnCoopEntries = (\d+);") == K["kAnCoopEntries"] == 2048
    assert value(r"constexpr int U = (\d+);") == K["U"] == 4
    assert value(r"constexpr int kScanThreads = (\d+);") == K["kScanThreads"] == 256
    assert value(r"static u32 g_an_wide_rows = (\d+);") == K["g_an_wide_rows"] == 16
    assert value(r"static int g_scan_small = (\d+);") == K["g_scan_small"] == 3
    # the rule of the hub list and of the two paths, as the table reads them
    assert "max_len > kAnCoopRowLen && e_end - e_begin > kAnCoopEntries * (R / 32)" in src
    assert "if (at < kAnCoopMax)" in src and "if (max_len <= kAnRowPathMax)" in src
    assert "return m <= (1u << 19) ? g_scan_small : (m <= (1u << 23) ? 8 : 32);" in src
    assert "return m <= (1u << 25) ? 1u : cdiv(m, (1u << 25));" in src
    assert (SCAN_8, SCAN_32, SCAN_SUB) == (1 << 19, 1 << 23, 1 << 25)
    assert "u32 r = cdiv(m ? m : 1, 1024);" in src and MAX_BLOCKS == 1024
    assert "g_scan_small = (i == 4 || i == 2) ? i : 3;" in src


@pytest.mark.parametrize("m, per, blocks, chunks", [(262145, 512, 513, 2), (786433, 1024, 769, 4), (4194305, 4352, 964, 17),
                                                    ((1 << 25) + 1, 33024, 1017, 129)])
def test_row_chunking_in_exact_integers(m, per, blocks, chunks):
    assert row_chunking(m) == (per, blocks) and per == chunks * K["kChunk"]
    assert (blocks - 1) * per < m <= blocks * per <= m + per - 1
    assert row_chunking(262144) == (256, 1024)                       # one chunk per workgroup up to here


def test_scan_tiles_in_exact_integers():
    assert scan_shape(1 << 25) == (32, 1, 4096)                      # the chain at its capacity
    assert scan_shape((1 << 25) + 1) == (32, 2, 2049)                # two sub-tiles of 8192 rows
    assert scan_shape(1 << 19) == (3, 1, 683) and scan_shape((1 << 19) + 1) == (8, 1, 257)
    assert scan_shape(1 << 23) == (8, 1, 4096) and scan_shape((1 << 23) + 1) == (32, 1, 1025)
    for items in (2, 3, 4):
        T = 256 * items
        assert [scan_shape(m, items)[2] for m in (T - 1, T, T + 1, 3 * T + 1)] == [1, 1, 2, 4]


def test_the_classed_rows_are_what_the_edge_table_states(classify):
    got = classify([_classify_line(r.len_a, r.ops, r.nnz, r.cmin, r.cmax, CP_DEFAULT) for r in KINDS.values()])
    for r, (s, n) in zip(KINDS.values(), got):
        assert (None if s == NO_CLASS else SYM_NAMES[s], None if n == NO_CLASS else NUM_NAMES[n]) == (r.sym, r.num), r
    assert {KINDS[k].num for k in SCAN_KINDS} == {"direct", "g8", "wave128", "block2k", "nfcopy", "dense4k"}


def test_the_layouts_the_table_must_hold():
    """what the tables above promise in words, checked on the tables"""
    for R in SHAPES:
        E = hub_entries(R)
        assert E == 2048 * R // 32
        a1 = layout("row_path_8_9", R)
        assert [s.max_len for s in a1.subs] == [0, 1, 4, 5, 8, 9, 8]
        a2 = layout("tile_256_257", R)
        assert [s.entries for s in a2.subs] == [255, 256, 257, 511, 512, 513]
        a4 = layout("hub_thresholds", R)
        assert [(s.max_len, s.entries) for s in a4.subs[:4]] == [(256, E + 500), (257, E), (257, E + 1), (E + 1, E + 1)]
        assert a4.m % R == R // 2 and a4.subs[-1].path == "hub"
        a5 = layout("hub_list_64_65", R)
        per, blocks = row_chunking(A5_M)
        hubs = collections.Counter(s.index * R // per for s in a5.subs if s.path == "hub")
        assert dict(hubs) == A5_GROUPS and all(0 < wg < blocks - 1 for wg in hubs) and a5.placed[-1].row == A5_M - 1
        assert max(A5_GROUPS.values()) + 2 <= per // R
        for m in (262145, 786433):
            a6 = layout(f"later_chunks_{m}", R)
            per, blocks = row_chunking(m)
            at = {p.row: p.spec for p in a6.placed}
            assert at[m - 1].len_a and (blocks - 1) * per == m - 1
            for wg in (0, 1, (blocks - 1) // 2, blocks - 2):
                for c in range(per // 256):
                    chunk = [at.get(r) for r in range(wg * per + c * 256, wg * per + c * 256 + 256)]
                    assert chunk[0] is not None and chunk[255] is not None
                    assert any(s is not None and s.sym in ("numeric_first", "global_hash") for s in chunk)
            assert sum(p.spec.sym == "global_hash" for p in a6.placed) == 2
    for name in SCAN:
        L = layout(name, 32)
        assert len({p.spec.num for p in L.placed}) >= 5 and L.placed[-1].row == L.m - 1, name


@pytest.mark.parametrize("name, R", CASES, ids=CASE_IDS)
def test_generator_builds_the_layout_it_claims(name, R):
    A, B, claims = build(name, R)
    L = layout(name, R)
    assert A.rows == claims.m == L.m and A.cols == B.rows
    # per row: the oracle's analysis and symbolic pass against the claims
    an = po.analysis(A, B)
    assert (np.diff(A.row_offsets.astype(np.int64)) == full(claims, "len_a")).all()
    for got, field in (("row_ops", "ops"), ("row_max_ops", "mx"), ("row_col_min", "cmin"), ("row_col_max", "cmax")):
        bad = np.flatnonzero(an[got] != full(claims, field))
        assert bad.size == 0, (field, bad[:5], an[got][bad[:5]], full(claims, field)[bad[:5]])
    assert an["sum_products"] == claims.ops.sum() and an["max_row_ops"] == claims.ops.max()
    cnt, total = po.symbolic(A, B)
    assert (cnt[:-1] == full(claims, "nnz")).all() and total == claims.nnz.sum()
    E = expected(name, R)                                            # the exact reference has the oracle's structure
    assert (np.diff(E.row_offsets.astype(np.int64)) == cnt[:-1]).all()
    if A.rows <= 1 << 20:
        C, _ = po.spgemm(A, B)
        assert (C.col_ids == E.col_ids).all() and (E.data == exact_spgemm(A, B).data).all()
    # per sub-chunk: longest row and entries from A.row_offsets against the table's literal numbers, and the side of the
    # switch the table states against the constants
    ro = A.row_offsets.astype(np.int64)
    nsub = -(-A.rows // R)
    edges = np.minimum(np.arange(nsub + 1) * R, A.rows)
    entries = ro[edges[1:]] - ro[edges[:-1]]
    lens = np.zeros(nsub * R, dtype=np.int64)
    lens[:A.rows] = np.diff(ro)
    max_len = lens.reshape(nsub, R).max(axis=1)
    stated = np.zeros(nsub, dtype=bool)
    for s in claims.subs.values():
        assert (int(max_len[s.index]), int(entries[s.index])) == (s.max_len, s.entries), s
        assert s.path is None or s.path == path_of(s.max_len, s.entries, R), s
        stated[s.index] = True
    assert not entries[~stated].any()                                # every sub-chunk the table does not name is empty
    # every row's movable entry: onto a spare row of B, between its neighbours, with another length than the row it leaves
    b_len = np.diff(B.row_offsets.astype(np.int64))
    for row in L.targets.values():
        e, k = movable_entry(A, row)
        a0, a1 = int(ro[row]), int(ro[row + 1])
        assert (e == a0 or A.col_ids[e - 1] < k) and k < A.col_ids[e] and b_len[k] == SPARE_LEN != b_len[A.col_ids[e]]


@pytest.mark.parametrize("name, R", [c for c in CASES if c[0] in ("hub_list_64_65", "later_chunks_786433", "scan_wide_2p25_plus_1")],
                         ids=lambda x: str(x))
def test_class_counts_of_the_large_layouts(classify, name, R):
    _, _, claims = build(name, R)
    sym, num = class_counts(claims, classify)
    assert sum(sym.values()) == (claims.len_a > 1).sum() - ((claims.len_a > 1) & (claims.ops == 0)).sum()
    assert sum(num.values()) == (claims.ops > 0).sum()
    if name == "hub_list_64_65":
        assert sum(A5_GROUPS.values()) in num.values()               # the hub rows are one class of their own
