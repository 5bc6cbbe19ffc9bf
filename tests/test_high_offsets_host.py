"""The premises of tests/test_gpu_high_offsets_side.py, without a GPU: pure numpy over the matrices, lists and placements
that file uses and the constants the package exports.  Every case is what its name says -- the row around 2^31 goes to the
kernel the class setting names, the last row at the top ends at 0xFFFFFFFF within one trip of every kernel that walks it,
extract's list makes tiles that more rows touch than LDS holds, every list names the rows that matter -- and the numpy
statements the GPU file compares the device with agree with an entry-by-entry count on the view's short rows."""
import math

import numpy as np
import pytest

import speck_amd as sa
import test_gpu_high_offsets_side as SIDE
from test_extract_host import numpy_extract
from test_gpu_high_offsets import COLS, T, TWO31, TWO32, base_of, check_premise, structure, twin_base
from test_sample_host import WITH, WITHOUT, brute_sample, numpy_sample
from test_topk_host import MODES, bits, brute_topk, numpy_topk

PLACES = ("low", "straddle", "above", "top")
LDS_ROWS = 4096                            # the rows of a tile whose ends extract.hip keeps in LDS (kTileRows)
SHORT = 60                                 # the rows the brute-force counts take: 0 .. 60 entries each
TOPK = (sa.TOPK_GROUP_MAX, sa.TOPK_LDS_MAX)
SAMPLE = (sa.SAMPLE_GROUP_MAX, sa.SAMPLE_LDS_MAX)


def offsets(where):
    ro = structure()[0].astype(np.int64)
    return ro + base_of(where, int(ro[-1]))


def test_the_constants_are_the_ones_the_cases_were_laid_out_for():
    assert TOPK == (256, 4096) and SAMPLE == (256, 4096)
    assert sa.SAMPLE_TILE_ENTRIES == sa.EXTRACT_TILE_ENTRIES == sa.SOFTMAX_TILE_ENTRIES == T == 4096 and sa.COO_TILE_ENTRIES == 2048
    assert SIDE.TK.CLASSES == {"group": TOPK, "lds": (0, TOPK[1]), "long": (0, 0)}
    assert SIDE.SP.CLASSES == {"group": SAMPLE, "lds": (0, SAMPLE[1]), "long": (0, 0)}
    assert SIDE.EX.LDS_ROWS == LDS_ROWS and SIDE.EX.T == sa.EXTRACT_TILE_ENTRIES


def test_every_placement_is_what_its_name_says_and_the_twin_keeps_the_place_in_the_tile():
    for where in PLACES:
        a = offsets(where)
        check_premise(where, a)
        assert twin_base(int(a[0])) % T == a[0] % T and twin_base(int(a[0])) + (a[-1] - a[0]) < 1 << 24
        for tile in (T, sa.COO_TILE_ENTRIES):
            assert a[0] % tile and a[-1] % tile                                        # a partial first and last tile
    a = offsets("top")
    assert a[-1] == 0xFFFFFFFF
    for tile in (sa.SOFTMAX_TILE_ENTRIES, sa.EXTRACT_TILE_ENTRIES, sa.SAMPLE_TILE_ENTRIES, sa.COO_TILE_ENTRIES):
        assert (a[-1] // tile + 1) * tile == TWO32                                     # the last tile ends at 2^32


@pytest.mark.parametrize("limits, classes", [(TOPK, SIDE.TK.CLASSES), (SAMPLE, SIDE.SP.CLASSES)], ids=["topk", "sample"])
def test_the_row_around_2_31_goes_through_every_kernel(limits, classes):
    """at `straddle` ONE row has start < 2^31 < end; k = 40 keeps it whole (the copy kernel), k = 5 cuts it, and the class
    setting decides which of the three kernels ranks it"""
    inside, long_row, last, empty = SIDE.marked_rows()
    a = offsets("straddle")
    assert a[inside] < TWO31 < a[inside + 1]
    n = int(a[inside + 1] - a[inside])
    assert SIDE.KS == (5, 40) and 5 < n <= 40
    for cls, setting in classes.items():
        assert SIDE.class_of(n, 40, setting, limits) == "copy"
        assert SIDE.class_of(n, 5, setting, limits) == cls
    # the long row is cut at both k and is a long row under every setting
    n_long = int(a[long_row + 1] - a[long_row])
    assert n_long == 70 * T + 3 and all(SIDE.class_of(n_long, k, s, limits) == "long" for k in SIDE.KS for s in classes.values())
    # the short rows split between the copy kernel and two group widths at both k under the default setting
    lens = np.diff(a)
    for k in SIDE.KS:
        assert ((lens > 0) & (lens <= k)).sum() > 20
        assert ((lens > k) & (lens <= limits[0] // 8)).sum() > 20 or k > limits[0] // 8
        assert ((lens > max(k, limits[0] // 8)) & (lens <= limits[0] // 4)).sum() > 20


@pytest.mark.parametrize("limits, classes", [(TOPK, SIDE.TK.CLASSES), (SAMPLE, SIDE.SP.CLASSES)], ids=["topk", "sample"])
def test_at_the_top_the_last_row_ends_at_the_last_offset_within_one_trip_of_every_kernel(limits, classes):
    inside, long_row, last, empty = SIDE.marked_rows()
    a = offsets("top")
    assert a[last + 1] == 0xFFFFFFFF and (a[last + 1:] == 0xFFFFFFFF).all() and a[0] >= TWO31
    n = int(a[last + 1] - a[last])
    for trip in (256, 1024, 4096):                                                     # the copy tile, a row kernel's threads, a tile
        assert a[last] + trip > TWO32 - 1 and n < trip
    assert 5 < n <= 40
    for cls, setting in classes.items():
        assert SIDE.class_of(n, 40, setting, limits) == "copy" and SIDE.class_of(n, 5, setting, limits) == cls


def test_every_list_names_the_rows_that_matter():
    inside, long_row, last, empty = SIDE.marked_rows()
    lens = np.diff(structure()[0].astype(np.int64))
    assert lens[empty] == 0 and lens[last] > 0 and (lens[last + 1:] == 0).all() and lens[long_row] == 70 * T + 3
    for rows in (SIDE.row_list(), SIDE.sparse_list()):
        assert (rows == inside).sum() >= 2 and (rows == last).sum() >= 2 and rows[-1] == last
        assert long_row in rows and empty in rows and rows.min() >= 0 and rows.max() < len(lens)
    m, out_cols = SIDE.column_map()
    assert len(m) == COLS and (m < 0).sum() == COLS // 3 and out_cols == COLS - COLS // 3
    assert np.array_equal(m[m >= 0], np.arange(out_cols))
    ci = structure()[1]
    assert 0.3 < (m[ci] < 0).mean() < 0.36                                             # a third of the view's entries is dropped


def tiles_of(rows, where):
    """per tile of gross entries of extract's list: (first row, rows it touches) as tile_rows_load finds them, and the
    absolute source entry of every gross entry"""
    a = offsets(where)
    glen = a[rows + 1] - a[rows]
    G = np.concatenate([[0], np.cumsum(glen)])
    tile = sa.EXTRACT_TILE_ENTRIES
    e0 = np.arange(0, G[-1], tile)
    e1 = np.minimum(e0 + tile, G[-1])
    first = np.searchsorted(G[1:], e0, side="right")                                   # the first row whose end lies beyond e0
    final = np.searchsorted(G[1:], e1 - 1, side="right")
    src = np.repeat(a[rows] - G[:-1], glen) + np.arange(G[-1])
    return first, final - first + 1, src, G


def test_the_list_with_empty_rows_makes_tiles_that_more_rows_touch_than_lds_holds():
    rows = SIDE.sparse_list()
    inside, long_row, last, empty = SIDE.marked_rows()
    first, nr, src, G = tiles_of(rows, "straddle")
    tile = sa.EXTRACT_TILE_ENTRIES
    # the first tile: the row around 2^31, 5000 empty rows, that row again, the start of the long row -- and source entry 2^31
    assert first[0] == 0 and nr[0] == 5003 > LDS_ROWS and TWO31 in src[:tile]
    assert (src[:tile] < TWO31).any() and (src[:tile] > TWO31).any()
    # the tile the first copy of the long row ends in: 4500 empty rows and the second copy
    at = int(np.nonzero(rows == long_row)[0][0])
    t = int((G[at + 1] - 1) // tile)
    assert nr[t] == 4502 > LDS_ROWS and first[t] == at and G[at + 1] % tile
    assert (np.delete(nr, [0, t]) <= 3).all() and len(nr) == 141
    # the other list stays within LDS: both branches are taken
    assert (tiles_of(SIDE.row_list(), "straddle")[1] <= LDS_ROWS).all()
    # at the top the sources end at the last entry of the store
    assert tiles_of(rows, "top")[2].max() == 0xFFFFFFFE and tiles_of(rows, "top")[2][-1] == 0xFFFFFFFE


def test_the_long_row_is_split_over_71_tiles_at_every_placement():
    long_row = SIDE.marked_rows()[1]
    for where in PLACES:
        a = offsets(where)
        tile = sa.SOFTMAX_TILE_ENTRIES
        assert (a[long_row + 1] - 1) // tile - a[long_row] // tile + 1 == 71
        split = ((a[1:] > a[:-1]) & (a[:-1] // tile != (np.maximum(a[1:], 1) - 1) // tile)).sum()
        assert split >= 2                                                              # the long row and a short one on a tile edge


# ---------------------------------------------------------------------------------------------------- the numpy statements
def short_view(dtype, values):
    """the first SHORT rows of the view (0 .. 60 entries, empty ones among them) with the GPU file's values"""
    H = values(dtype)
    ro = H.row_offsets[:SHORT + 1].astype(np.int64)
    assert ro[0] == 0 and (np.diff(ro) == 0).any() and np.diff(ro).max() > 40
    return ro, H.col_ids[:ro[-1]], H.data[:ro[-1]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_topk_is_the_count_of_beaters_on_the_short_rows(dtype):
    ro, col, val = short_view(dtype, SIDE.tagged_matrix)
    assert np.isnan(val).any() and len(np.unique(bits(val))) < len(val)                # NaNs and ties go in
    for mode in MODES.values():
        for k in SIDE.KS:
            new_ro, ci, vb, info = numpy_topk(ro, col, val, k, mode)
            kept, ties = brute_topk(ro, val, k, mode)
            assert np.array_equal(ci, col[kept]) and np.array_equal(vb, bits(val)[kept]) and info["ties_cut"] == ties
            assert np.array_equal(np.diff(new_ro.astype(np.int64)), np.minimum(np.diff(ro), k))


@pytest.mark.parametrize("mode", [WITHOUT, WITH])
def test_numpy_sample_is_the_count_of_smaller_keys_on_the_short_rows(mode):
    ro, col, val = short_view(np.float64, SIDE.tagged_matrix)
    rows = np.concatenate([np.random.default_rng(5).integers(0, SHORT, size=30), [7, 7, SHORT - 1]])
    for k in SIDE.KS:
        for picks in (None, rows):
            new_ro, ci, vb, info, pos = numpy_sample(ro, col, val, k, SIDE.SEED, picks, mode, SIDE.ROW_BASE)
            named = range(SHORT) if picks is None else picks
            want_pos, want_lens = brute_sample(ro, k, SIDE.SEED, named, mode, SIDE.ROW_BASE)
            assert np.array_equal(pos, want_pos) and np.array_equal(np.diff(new_ro.astype(np.int64)), want_lens)
            assert np.array_equal(ci, col[want_pos]) and np.array_equal(vb, bits(val)[want_pos])


def test_numpy_extract_is_the_loop_over_the_named_rows():
    ro, col, val = short_view(np.float32, SIDE.tagged_matrix)
    cmap, out_cols = SIDE.column_map()
    rows = np.concatenate([np.random.default_rng(6).integers(0, SHORT, size=30), [7, 7, SHORT - 1, SHORT - 1]])
    for picks in (None, rows):
        for m in (None, cmap):
            new_ro, ci, vb, info = numpy_extract(ro, col, val, picks, m, COLS, out_cols if m is not None else COLS)
            want_ro, want_ci, want_vb = [0], [], []
            for r in (range(SHORT) if picks is None else picks):
                for e in range(int(ro[r]), int(ro[r + 1])):
                    if m is None or m[col[e]] >= 0:
                        want_ci.append(int(col[e]) if m is None else int(m[col[e]]))
                        want_vb.append(int(bits(val)[e]))
                want_ro.append(len(want_ci))
            assert new_ro.tolist() == want_ro and ci.tolist() == want_ci and vb.tolist() == want_vb
            assert info["nnz_out"] == len(want_ci) and info["rows_out"] == len(want_ro) - 1


def test_the_row_of_every_entry_is_the_loop_over_the_rows():
    ro, _, _ = short_view(np.float64, SIDE.tagged_matrix)
    want = [r + SIDE.ROW_BASE for r in range(SHORT) for _ in range(int(ro[r]), int(ro[r + 1]))]
    assert (np.repeat(np.arange(SHORT), np.diff(ro)) + SIDE.ROW_BASE).tolist() == want


@pytest.mark.parametrize("mode", ["normalized", "exp"])
def test_numpy_softmax_is_the_sum_entry_by_entry(mode):
    ro, col, val = short_view(np.float64, SIDE.softmax_matrix)
    H = sa.HostCSR(SHORT, COLS, ro.astype(np.uint32), col, val)
    out, m, s = SIDE.SM.numpy_forward(H, -1.0, mode)
    for r in range(SHORT):
        x = [-1.0 * float(v) for v in val[ro[r]:ro[r + 1]]]
        if not x:
            assert m[r] == -np.inf and s[r] == 0
            continue
        e = [math.exp(v - max(x)) for v in x]
        total = math.fsum(e)
        want = np.array(e if mode == "exp" else [v / total for v in e])
        assert m[r] == max(x) and abs(s[r] - total) <= len(x) * 2.0 ** -52 * total
        assert np.allclose(out[ro[r]:ro[r + 1]], want, rtol=(len(x) + 4) * 2.0 ** -52, atol=0)


def test_the_transposed_product_and_the_row_sums_are_the_loops_over_the_entries():
    ro, col, val = short_view(np.float32, lambda dtype: SIDE.view_matrix(dtype))
    H = sa.HostCSR(SHORT, COLS, ro.astype(np.uint32), col, val)
    X = SIDE.B32.ints((SHORT, 3), 51)
    S = SIDE.SPT.at_x(H, X.astype(np.float64))
    want = np.zeros((COLS, 3))
    for r in range(SHORT):
        for e in range(int(ro[r]), int(ro[r + 1])):
            want[col[e]] += float(val[e]) * X[r].astype(np.float64)
    assert np.array_equal(S, want)
    Xc = SIDE.B32.ints((COLS, 3), 61)
    rows = np.zeros((SHORT, 3))
    for r in range(SHORT):
        for e in range(int(ro[r]), int(ro[r + 1])):
            rows[r] += float(val[e]) * Xc[col[e]].astype(np.float64)
    assert np.array_equal(SIDE.B32.row_sums(H, Xc), rows)


# ---------------------------------------------------------------------------------------------------- counters relative to the matrix
def test_a_matrix_within_one_step_of_2_32_entries_is_refused_before_anything_runs():
    """three loops count entries RELATIVE to the matrix in 32 bits: expand_rows_kernel of the transpose and of the plan
    creation (a wave of 64 a step) and the j0 loops of the copy kernels of topk and sample (1024 a step).  A counter that is
    within one step of 2^32 passes its end and starts over: such a matrix is refused on the host, from the struct alone --
    the buffers below hold 64 words and nothing follows them"""
    import ctypes
    import test_sample_host as SH
    import test_topk_host as TH
    from speck_amd import _lib
    L = _lib.load()
    words = np.zeros(64, dtype=np.uint64)
    at = words.ctypes.data
    ref = ctypes.byref
    OVERFLOW = 5
    for over in ((1 << 32) - 63, (1 << 32) - 1):
        A, At = TH._a(4, 6, over, at), TH._a(9, 9, 9, at)
        before = bytes(At)
        for fn in (L.speck_transpose_f64, L.speck_transpose_f32):
            assert fn(None, ref(A), ref(At)) == OVERFLOW and bytes(At) == before
        h = ctypes.c_void_p()
        assert L.speck_tplan_create(None, ref(A), ref(h), None) == OVERFLOW and not h
    for over in ((1 << 32) - 1023, (1 << 32) - 1):
        A, C = TH._a(4, 6, over, at), TH._a(9, 9, 9, at)
        before = bytes(C)
        for fn in (L.speck_topk_f64, L.speck_topk_f32):
            assert fn(None, ref(A), ref(TH._params(2)), ref(C), None) == OVERFLOW and bytes(C) == before
        for fn in (L.speck_sample_f64, L.speck_sample_f32):
            assert fn(None, ref(A), ref(SH._params(2, 4)), ref(C), None) == OVERFLOW and bytes(C) == before
    assert not words.any()
