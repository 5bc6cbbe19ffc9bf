"""The three device utilities around the multiply -- compare, transpose, device copy -- at their own switches: the generators,
the expectations and the mirrored constants, checked without a GPU.  tests/test_gpu_utilities.py runs them through the kernels.

  * transpose (speck_amd/csrc/extras.hip) is a stable LSD radix sort of (column, position): 8 bits per pass, tiles of
    TRANSPOSE_TILE entries of which a wave owns TRANSPOSE_WAVE_SHARE in steps of 64 lanes, TRANSPOSE_BLOCKS workgroups that
    each own a run of whole tiles (slice_begin), ping-pong buffers.  Its expectation is numpy's stable argsort of the column
    ids; the values of every input are the entries' input positions, so that an order that is not stable shows.
  * compare runs one wave per row, 64 entries per step, at most COMPARE_MAX_WAVES waves per trip of its row loop.
  * the device copy runs at most COPY_MAX_THREADS threads, a word per thread and trip.
Every expectation here is numpy on the host arrays; nothing is computed with the library.
"""
import functools
import os
import re

import numpy as np
import pytest

import speck_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, BLOCKS, SHARE = sa.TRANSPOSE_TILE, sa.TRANSPOSE_BLOCKS, sa.TRANSPOSE_WAVE_SHARE
GRID_THREADS = 2048 * 256            # iota / gather / offsets kernels of the transpose: the threads of their launch

# ---- entry counts of the transpose: the 64-lane step, a wave's share, a tile, two tiles, one tile per workgroup / two ----
ENTRY_COUNTS_SMALL = [1, 63, 64, 65, SHARE - 1, SHARE, SHARE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
ENTRY_COUNTS_LARGE = [BLOCKS * TILE - 1, BLOCKS * TILE, BLOCKS * TILE + 1, (BLOCKS + BLOCKS // 2) * TILE + 7]
# ---- column counts: both sides of every change of the number of digit passes ---------------------------------------------
COLS_CASES = [1, 2, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 1 << 27]
COMPARE_ROW_LENGTHS = [1, 63, 64, 65, 128, 129, 1000]
COMPARE_ROW_COUNTS = [sa.COMPARE_MAX_WAVES - 1, sa.COMPARE_MAX_WAVES, sa.COMPARE_MAX_WAVES + 1, 70001]


def host(rows, cols, lens, ci, dtype=np.float64):
    """HostCSR of row lengths and flat column ids; the values are the entries' positions"""
    ro = np.zeros(rows + 1, dtype=np.uint32)
    np.cumsum(lens, dtype=np.uint32, out=ro[1:])
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    assert int(ro[-1]) == ci.size and (ci.size == 0 or int(ci.max()) < cols)
    return sa.HostCSR(rows, cols, ro, ci, np.arange(ci.size, dtype=dtype))


def with_values(H, data):
    return sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, data)


def positions(H, dtype):
    """H with its values = entry positions in `dtype` (float32 holds them exactly below 2^24)"""
    assert dtype == np.float64 or H.nnz <= 1 << 24
    return with_values(H, np.arange(H.nnz, dtype=dtype))


def row_index(H):
    return np.repeat(np.arange(H.rows, dtype=np.uint32), np.diff(H.row_offsets.astype(np.int64)))


def sorted_in_rows(lens, ci):
    """the column ids ascending inside every row (what a transpose gives back)"""
    row = np.repeat(np.arange(len(lens)), lens)
    return ci[np.lexsort((ci, row))]


def lengths(nnz, rng, longest=5):
    """row lengths 0 .. longest that sum to exactly nnz: row and entry boundaries do not coincide"""
    lens = rng.integers(0, longest + 1, size=nnz // 2 + 8)
    while int(lens.sum()) < nnz:
        lens = np.concatenate([lens, rng.integers(0, longest + 1, size=lens.size)])
    cum = np.cumsum(lens)
    last = int(np.searchsorted(cum, nnz))                      # the first row at which the sum reaches nnz
    lens = lens[:last + 1].copy()
    lens[last] -= int(cum[last]) - nnz
    return lens


# ---- the expectation -----------------------------------------------------------------------------------------------------
def transpose_expect(H):
    """(offsets, column ids, values) of the transpose of H (offsets from 0): the stable sort of its entries by column"""
    assert int(H.row_offsets[0]) == 0
    order = np.argsort(H.col_ids, kind="stable")
    t_ro = np.zeros(H.cols + 1, dtype=np.uint32)
    np.cumsum(np.bincount(H.col_ids, minlength=H.cols), dtype=np.uint32, out=t_ro[1:])
    return t_ro, row_index(H)[order], H.data[order]


def expected_transpose(H):
    t_ro, t_ci, t_da = transpose_expect(H)
    return sa.HostCSR(H.cols, H.rows, t_ro, t_ci, t_da)


def positions_in_transpose(H):
    """where the transpose holds each entry of H: the values of the transpose of (the transpose with ITS positions as values)"""
    order = np.argsort(H.col_ids, kind="stable")
    inverse = np.empty(H.nnz, dtype=np.int64)
    inverse[order] = np.arange(H.nnz)
    return inverse.astype(np.float64)


def same_bytes(a, b):
    """a.tobytes() == b.tobytes() of two arrays of one type, without the two copies"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u)))


def same_matrix(got, ro, ci, da):
    return same_bytes(got.row_offsets, ro) and same_bytes(got.col_ids, ci) and same_bytes(got.data, da)


# ---- mirrors of the host-side arithmetic of extras.hip ---------------------------------------------------------------------
def slice_begin(n, b):
    """the first entry of workgroup b: whole tiles, the same number for every workgroup"""
    tiles = -(-n // TILE)
    per = -(-tiles // BLOCKS)
    return min(b * per * TILE, n)


def digit_passes(cols):
    bits = 1
    while bits < 32 and (1 << bits) < max(cols, 1):
        bits += 1
    return -(-bits // 8)


# ---- transpose inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def entry_count_case(nnz, cols=300):
    rng = np.random.default_rng(1000 + nnz % 977)
    lens = lengths(nnz, rng)
    return host(len(lens), cols, lens, sorted_in_rows(lens, rng.integers(0, cols, size=nnz)))


@functools.lru_cache(maxsize=None)
def digit_case(cols, nnz=5000):
    """columns 0 and cols - 1 present, the other entries in the middle half of the range: empty columns at both ends"""
    rng = np.random.default_rng(2000 + cols % 977)
    lens = lengths(nnz, rng, 8)
    if cols < 4:
        ci = rng.integers(0, cols, size=nnz)
    else:
        ci = rng.integers(cols // 4, cols - cols // 4, size=nnz)
    ci[17], ci[nnz - 40] = 0, cols - 1
    return host(len(lens), cols, lens, sorted_in_rows(lens, ci))


@functools.lru_cache(maxsize=None)
def equal_digit_cases():
    rng = np.random.default_rng(31)
    n = 5000
    lens = lengths(n, rng)
    cases = {
        # every key equal: all 64 lanes are peers in every step, across three tiles
        "one_column": host(n, 1, np.ones(n, dtype=np.int64), np.zeros(n)),
        # two peer groups of 32 interleaved lane by lane
        "two_alternating": host(len(lens), 2, lens, np.arange(n) % 2),
        "ends_of_a_digit": host(len(lens), 256, lens, 255 * rng.integers(0, 2, size=n)),
        # four passes of which three see the digit 0 only: they must keep the order of the first
        "low_digit_only": host(len(lens), (1 << 24) + 1, lens, sorted_in_rows(lens, rng.integers(0, 256, size=n))),
    }
    # a hub column of 10 000 entries among 20 000 scattered ones
    rows = cols = 12000
    lens = np.bincount(rng.integers(0, rows, size=20000), minlength=rows)
    lens[:10000] += 1
    ci = rng.integers(0, cols, size=30000)
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ci[first[:10000]] = 777
    cases["hub_column"] = host(rows, cols, lens, sorted_in_rows(lens, ci))
    cases["hub_row"] = positions(expected_transpose(cases["hub_column"]), np.float64)       # ... and back
    return cases


@functools.lru_cache(maxsize=None)
def row_cases():
    rng = np.random.default_rng(47)
    cases = {}
    for rows in (sa.COMPARE_MAX_WAVES - 1, sa.COMPARE_MAX_WAVES, sa.COMPARE_MAX_WAVES + 1):
        # (expand_rows_kernel is launched like compare_kernel: at most 8192 workgroups of four waves)
        cases[f"one_entry_rows_{rows}"] = host(rows, 300, np.ones(rows, dtype=np.int64), rng.integers(0, 300, size=rows))
    cases["one_row_70000"] = host(1, 1000, np.array([70000]), np.sort(rng.integers(0, 1000, size=70000)))
    lens = np.array([0, 0, 0, 5, 0, 1, 0, 0, 0, 0, 130, 0, 2, 0, 0, 64, 0, 0, 0, 0, 0, 3, 0, 0])
    cases["empty_rows"] = host(len(lens), 40, lens, sorted_in_rows(lens, rng.integers(0, 40, size=int(lens.sum()))))
    cases["no_rows"] = host(0, 7, np.zeros(0, dtype=np.int64), np.zeros(0))
    for cols, nnz in ((GRID_THREADS - 1, GRID_THREADS), (GRID_THREADS, GRID_THREADS + 1)):
        lens = lengths(nnz, rng)
        cases[f"cols_plus_1_{cols + 1}"] = host(len(lens), cols, lens, sorted_in_rows(lens, rng.integers(0, cols, size=nnz)))
    return cases


@functools.lru_cache(maxsize=None)
def view_base():
    """(matrix, r0, r1, c0, c1): row_offsets[r0] is odd and not 0; rows [c0, c1) have all their entries in column 17"""
    rng = np.random.default_rng(53)
    lens = lengths(2500, rng)
    ci = rng.integers(0, 300, size=2500)
    H = host(len(lens), 300, lens, ci)
    c0, c1 = 600, 660
    ci[int(H.row_offsets[c0]):int(H.row_offsets[c1])] = 17
    H = host(len(lens), 300, lens, sorted_in_rows(lens, ci))
    r0 = next(r for r in range(100, H.rows) if H.row_offsets[r] % 2 == 1 and lens[r])
    return H, r0, r0 + 300, c0, c1


def view_slice(H, r0, r1, dtype=None):
    """what rows [r0, r1) of H are on their own: offsets from 0, their entries, the values as they are in H"""
    e0, e1 = int(H.row_offsets[r0]), int(H.row_offsets[r1])
    da = H.data[e0:e1] if dtype is None else H.data[e0:e1].astype(dtype)
    return sa.HostCSR(r1 - r0, H.cols, (H.row_offsets[r0:r1 + 1] - H.row_offsets[r0]).astype(np.uint32),
                      H.col_ids[e0:e1].copy(), da.copy())


def any_bits(n, dtype, seed=8):
    """n values of arbitrary bit patterns (NaN payloads, subnormals, both zeros, infinities among them)"""
    u = np.uint64 if dtype == np.float64 else np.uint32
    v = np.random.default_rng(seed).integers(0, np.iinfo(u).max, size=n, dtype=u, endpoint=True)
    v[:6] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(dtype).tiny / 4], dtype=dtype).view(u)
    return v.view(dtype)


# ---- compare inputs --------------------------------------------------------------------------------------------------------
def dyadic_values(n, dtype=np.float64):
    """1 + j / 4096: exact in both value types, every neighbour different"""
    return (1.0 + (np.arange(n) % 4096) / 4096.0).astype(dtype)


@functools.lru_cache(maxsize=None)
def compare_rows_matrix(dtype=np.float64):
    lens = np.array(COMPARE_ROW_LENGTHS)
    ci = np.concatenate([2 * np.arange(n) for n in lens])           # even columns: id + 1 is a column no entry has
    H = host(len(lens), 4096, lens, ci)
    return with_values(H, dyadic_values(H.nnz, dtype))


def plant_positions(length):
    return sorted({p for p in (0, 63, 64, length - 1) if p < length})


def planted(H, places, kind):
    """H with one column id (kind "col") or one value (kind "val") changed at each (row, position) of `places`"""
    ci, da = H.col_ids.copy(), H.data.copy()
    for row, pos in places:
        j = int(H.row_offsets[row]) + pos
        assert j < int(H.row_offsets[row + 1])
        if kind == "col":
            ci[j] += 1
        else:
            da[j] += 1
    return sa.HostCSR(H.rows, H.cols, H.row_offsets, ci, da)


@functools.lru_cache(maxsize=None)
def two_entry_rows(rows):
    ci = np.stack([2 * (np.arange(rows) % 500), 2 * (np.arange(rows) % 500) + 1000], axis=1).ravel()
    H = host(rows, 4096, np.full(rows, 2), ci)
    return with_values(H, dyadic_values(H.nnz))


def planted_rows(rows):
    """five rows: the first, one of the first trip, the middle, the first row of the second trip or next to the end, the last"""
    return sorted({0, 8191, rows // 2, min(sa.COMPARE_MAX_WAVES, rows - 2), rows - 1})


def shifted_pair(rows=200, longer=37, shorter=121):
    """(A, B, differing rows): in B row `longer` has one entry more and row `shorter` one less.  Every entry is (7, 1.0):
    the rows between the two hold the same entries in A and in B and differ by their place alone"""
    lens = 3 + np.arange(rows) % 4
    n = int(lens.sum())
    A = with_values(host(rows, 4096, lens, np.full(n, 7)), np.ones(n))
    lens_b = lens.copy()
    lens_b[longer] += 1
    lens_b[shorter] -= 1
    B = with_values(host(rows, 4096, lens_b, A.col_ids), A.data)
    a, b = A.row_offsets.astype(np.int64), B.row_offsets.astype(np.int64)
    differ = (a[:-1] - a[0] != b[:-1] - b[0]) | (np.diff(a) != np.diff(b))
    return A, B, int(np.count_nonzero(differ))


# ---- device copy inputs ----------------------------------------------------------------------------------------------------
def copy_entries_case(nnz, dtype):
    """nnz entries in 1000 rows"""
    lens = np.full(1000, nnz // 1000)
    lens[:nnz % 1000] += 1
    return positions(host(1000, 4096, lens, np.arange(nnz) % 4096), dtype)


def copy_rows_case(rows):
    """1000 one-entry rows spread over `rows` rows"""
    lens = np.zeros(rows, dtype=np.int64)
    lens[np.linspace(0, rows - 1, 1000).astype(np.int64)] = 1
    return host(rows, 4096, lens, np.arange(1000))


# ================================================================================================================ the checks
def _constexpr(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_mirrored_constants_are_the_ones_in_the_sources():
    extras = open(os.path.join(ROOT, "speck_amd", "csrc", "extras.hip")).read()
    line = next(ln for ln in extras.splitlines() if ln.startswith("constexpr int kRadixThreads"))
    threads, items, blocks = (_constexpr(line, k) for k in ("kRadixThreads", "kRadixItems", "kRadixBlocks"))
    assert (threads, items, blocks) == (256, 8, 1024)
    assert re.search(r"kRadixTile\s*=\s*kRadixThreads\s*\*\s*kRadixItems\s*;", extras)
    assert sa.TRANSPOSE_TILE == threads * items and sa.TRANSPOSE_BLOCKS == blocks and sa.TRANSPOSE_WAVE_SHARE == 64 * items
    # compare_kernel and expand_rows_kernel: (rows + 3) / 4 workgroups of 256 threads = four waves, at most 8192
    caps = re.findall(r"u32 blocks = \(rows \+ 3\) / 4;\s*if \(blocks > (\d+)\) blocks = (\d+);", extras)
    assert caps == [("8192", "8192")] * 2
    assert len(re.findall(r"dim3\(blocks(?: \? blocks : 1)?\), dim3\(256\)", extras)) == 2
    assert sa.COMPARE_MAX_WAVES == 8192 * 256 // 64
    # the three grid-stride kernels of the transpose
    assert len(re.findall(r"dim3\(2048\), dim3\(256\)", extras)) == 3 and GRID_THREADS == 2048 * 256
    dcsr = open(os.path.join(ROOT, "speck_amd", "csrc", "dcsr.hip")).read()
    m = re.search(r"std::min<u64>\(\(work \+ 255\) / 256, (\d+)\)\), dim3\(256\)", dcsr)
    assert m and int(m.group(1)) == 8192
    assert sa.COPY_MAX_THREADS == 8192 * 256


@pytest.mark.parametrize("nnz", ENTRY_COUNTS_SMALL + ENTRY_COUNTS_LARGE)
def test_entry_count_generator_is_exact(nnz):
    H = entry_count_case(nnz)
    lens = np.diff(H.row_offsets.astype(np.int64))
    assert H.nnz == nnz == H.col_ids.size and H.cols == 300 and 0 <= lens.min() and lens.max() <= 5
    assert nnz < 64 or (lens == 0).any() and len(set(lens.tolist())) == 6
    row = row_index(H).astype(np.int64)
    assert (np.diff(row * 300 + H.col_ids) >= 0).all()            # ascending inside every row: the transpose of its
    assert same_bytes(H.data, np.arange(nnz, dtype=np.float64))   # transpose is the matrix itself


def test_entry_counts_stand_on_the_switches_of_the_sort():
    assert ENTRY_COUNTS_SMALL == [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 4097]
    assert ENTRY_COUNTS_LARGE == [1024 * 2048 - 1, 1024 * 2048, 1024 * 2048 + 1, 1536 * 2048 + 7]
    held = lambda n: np.array([slice_begin(n, b + 1) - slice_begin(n, b) for b in range(BLOCKS)])   # noqa: E731
    for n in ENTRY_COUNTS_SMALL + ENTRY_COUNTS_LARGE:
        assert held(n).sum() == n and slice_begin(n, BLOCKS) == n
    h = held(BLOCKS * TILE - 1)
    assert (h[:-1] == TILE).all() and h[-1] == TILE - 1          # one tile each, the last one short
    assert (held(BLOCKS * TILE) == TILE).all()
    h = held(BLOCKS * TILE + 1)                                   # two tiles each: half of the grid is idle
    assert (h[:512] == 2 * TILE).all() and h[512] == 1 and (h[513:] == 0).all()
    h = held(1536 * TILE + 7)
    assert (h[:768] == 2 * TILE).all() and h[768] == 7 and (h[769:] == 0).all()
    assert (held(TILE + 1)[:3] == [TILE, 1, 0]).all()


def test_column_counts_stand_on_both_sides_of_every_pass_count():
    assert [digit_passes(c) for c in COLS_CASES] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 4]
    for cols in COLS_CASES:
        H = digit_case(cols)
        assert H.nnz == 5000 and H.cols == cols
        count = np.bincount(H.col_ids, minlength=cols) if cols <= 1 << 24 else None
        assert 0 in H.col_ids and cols - 1 in H.col_ids
        if cols >= 255:                                           # empty columns next to both ends
            assert H.col_ids[(H.col_ids != 0) & (H.col_ids != cols - 1)].min() >= cols // 4 > 1
            assert H.col_ids[(H.col_ids != 0) & (H.col_ids != cols - 1)].max() < cols - cols // 4 < cols - 1
        if count is not None and cols >= 255:
            assert count[1] == 0 and count[cols - 2] == 0


def test_the_expectation_is_the_transpose():
    """transpose_expect against the dense transpose, written out: 4 x 5 with an empty row, an empty column, a full row"""
    D = np.array([[0, 3, 0, 0, 7], [0, 0, 0, 0, 0], [1, 2, 0, 4, 5], [0, 9, 0, 0, 0]], dtype=np.float64)
    r, c = np.nonzero(D)
    H = sa.HostCSR(4, 5, np.array([0, 2, 2, 6, 7], dtype=np.uint32), c.astype(np.uint32), D[r, c])
    t_ro, t_ci, t_da = transpose_expect(H)
    rt, ct = np.nonzero(D.T)
    assert t_ro.tolist() == [0, 1, 4, 4, 5, 7] and (t_ci == ct).all() and (t_da == D.T[rt, ct]).all()
    # duplicates inside a row keep their input order
    H = host(2, 3, np.array([3, 2]), np.array([1, 1, 0, 1, 1]))
    t_ro, t_ci, t_da = transpose_expect(H)
    assert t_ro.tolist() == [0, 1, 5, 5] and t_ci.tolist() == [0, 0, 0, 1, 1] and t_da.tolist() == [2, 0, 1, 3, 4]
    # there and back on an input with ascending rows
    A = entry_count_case(513)
    B = expected_transpose(positions(expected_transpose(A), np.float64))
    assert same_matrix(B, A.row_offsets, A.col_ids, positions_in_transpose(A))


def test_equal_digit_row_and_view_cases_are_what_they_claim():
    E = equal_digit_cases()
    assert E["one_column"].rows == 5000 > 2 * TILE and E["one_column"].cols == 1
    assert (E["two_alternating"].col_ids == np.arange(5000) % 2).all()
    assert set(E["ends_of_a_digit"].col_ids.tolist()) == {0, 255} and E["ends_of_a_digit"].cols == 256
    assert E["low_digit_only"].col_ids.max() < 256 and digit_passes(E["low_digit_only"].cols) == 4
    assert np.bincount(E["hub_column"].col_ids)[777] >= 10000 and E["hub_column"].nnz == 30000
    assert np.diff(E["hub_row"].row_offsets.astype(np.int64)).max() >= 10000
    R = row_cases()
    assert R["one_row_70000"].rows == 1 and R["no_rows"].rows == 0 and R["no_rows"].nnz == 0
    lens = np.diff(R["empty_rows"].row_offsets.astype(np.int64))
    assert lens[0] == 0 and lens[-1] == 0 and (lens[6:10] == 0).all()
    assert sorted(R[k].cols + 1 for k in R if k.startswith("cols_plus_1")) == [GRID_THREADS, GRID_THREADS + 1]
    assert sorted(R[k].nnz for k in R if k.startswith("cols_plus_1")) == [GRID_THREADS, GRID_THREADS + 1]
    H, r0, r1, c0, c1 = view_base()
    assert H.row_offsets[r0] % 2 == 1 and r1 <= H.rows
    assert (H.col_ids[int(H.row_offsets[c0]):int(H.row_offsets[c1])] == 17).all() and H.row_offsets[c1] > H.row_offsets[c0]


def test_compare_inputs_differ_exactly_where_planted():
    M = compare_rows_matrix()
    assert np.diff(M.row_offsets.astype(np.int64)).tolist() == COMPARE_ROW_LENGTHS
    assert [plant_positions(n) for n in (1, 63, 64, 65, 1000)] == [[0], [0, 62], [0, 63], [0, 63, 64], [0, 63, 64, 999]]
    for row, n in enumerate(COMPARE_ROW_LENGTHS):
        for pos in plant_positions(n):
            X, Y = planted(M, [(row, pos)], "col"), planted(M, [(row, pos)], "val")
            j = int(M.row_offsets[row]) + pos
            assert np.flatnonzero(X.col_ids != M.col_ids).tolist() == [j] and same_bytes(X.data, M.data)
            assert np.flatnonzero(Y.data != M.data).tolist() == [j] and same_bytes(Y.col_ids, M.col_ids)
    assert COMPARE_ROW_COUNTS == [32767, 32768, 32769, 70001]
    for rows in COMPARE_ROW_COUNTS:
        p = planted_rows(rows)
        assert len(p) == 5 and p[0] == 0 and p[-1] == rows - 1 and two_entry_rows(rows).nnz == 2 * rows
        assert rows <= sa.COMPARE_MAX_WAVES or sa.COMPARE_MAX_WAVES in p
    A, B, differ = shifted_pair()
    assert A.nnz == B.nnz and A.rows == B.rows and differ == 121 - 37 + 1


def test_the_bounds_are_exact_in_binary():
    """the value checks of test_gpu_utilities.py sit on the bound itself: every quantity is a dyadic number"""
    x, y = 1.0, 1.0 + 2.0 ** -40
    assert y - x == 2.0 ** -40 and 2.0 ** -40 * 1.0 + 1e-300 == 2.0 ** -40 and 2.0 ** -41 + 1e-300 == 2.0 ** -41
    assert 2.0 ** -37 * 2.0 ** -3 + 1e-300 == 2.0 ** -40 and 2.0 ** -38 * 2.0 ** -3 + 1e-300 == 2.0 ** -41
    assert 2.0 ** -41 * y + 1e-300 < y - x <= 2.0 ** -39 * y + 1e-300        # the relative form: max(|x|, |y|) = y
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    d = float(up) - float(one)
    assert d == 2.0 ** -23 and 2.0 ** -25 * float(up) + 1e-300 < d <= 2.0 ** -23 * float(up) + 1e-300


def test_copy_cases_stand_on_the_thread_count():
    T = sa.COPY_MAX_THREADS
    for nnz in (T - 1, T, T + 1):
        H = copy_entries_case(nnz, np.float32)
        assert H.nnz == nnz and H.rows == 1000 and H.data.dtype == np.float32
    for rows in (T - 2, T - 1, T):
        H = copy_rows_case(rows)
        assert H.rows + 1 in (T - 1, T, T + 1) and H.nnz == 1000
