"""speck_select_* on the GPU (speck_amd/csrc/select.hip).  The expectation is a few lines of numpy: the row of every entry,
the boolean keep vector of the predicates, the kept entries per row summed into offsets.  Offsets, column ids AND values
are compared bit for bit (the values as raw bytes: NaN payloads and -0.0 count)."""
import ctypes as C_

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po
from conftest import random_csr

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSORTED = 1, 8
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TOL64 = 1e-12                # the bounds of tests/test_gpu_masked.py
TOL32 = 4.0 * 2.0 ** -23
DTYPES = [np.float64, np.float32]
TILES = sa.SELECT_TILE_ROWS
LONG_AVG = sa.SELECT_LONG_ROW_AVG


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def host(rows, cols, ro, ci, data):
    return sa.HostCSR(rows, cols, np.asarray(ro, dtype=np.uint32), np.asarray(ci, dtype=np.uint32), np.asarray(data))


def from_lengths(lens, cols, seed, dtype=np.float64):
    """rows of the given lengths, columns drawn with replacement (unsorted, duplicates as they fall), values of any sign
    with a tenth of them zero"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    v = (0.5 + rng.random(n)) * rng.choice([-1.0, 1.0], size=n)
    v[rng.random(n) < 0.1] = 0.0
    return host(len(lens), cols, ro, rng.integers(0, cols, size=n), v.astype(dtype))


def canonical(H, dtype=None):
    return host(H.rows, H.cols, H.row_offsets, H.col_ids, H.data if dtype is None else H.data.astype(dtype))


def row_of_entries(H):
    return np.repeat(np.arange(H.rows, dtype=np.int64), np.diff(H.row_offsets.astype(np.int64)))


def keys(H):
    base = int(H.row_offsets[0])
    return row_of_entries(H) * H.cols + H.col_ids[base:base + H.nnz].astype(np.int64)


def reference(H, band=None, abs_gt=None, pattern=None, negate=(), row_base=0):
    """(row_offsets, col_ids, data, rows unchanged) of the filtered matrix"""
    base = int(H.row_offsets[0])
    ci, v = H.col_ids[base:base + H.nnz], H.data[base:base + H.nnz]
    row = row_of_entries(H)
    keep = np.ones(H.nnz, dtype=bool)
    if band is not None:
        d = ci.astype(np.int64) - (row_base + row)
        lo, hi = (INT64_MIN if band[0] is None else band[0]), (INT64_MAX if band[1] is None else band[1])
        keep &= ((d >= lo) & (d <= hi)) != ("band" in negate)
    if abs_gt is not None:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.abs(v.astype(np.float64)) <= np.float64(abs_gt)) != ("abs" in negate)
    if pattern is not None:
        keep &= np.isin(row * H.cols + ci.astype(np.int64), keys(pattern)) != ("pattern" in negate)
    kept_per_row = np.bincount(row[keep], minlength=H.rows)
    ro = np.zeros(H.rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(kept_per_row)
    unchanged = int((kept_per_row == np.diff(H.row_offsets.astype(np.int64))).sum())
    return ro, ci[keep], v[keep], unchanged


def same(got, want, info=None, nnz_in=None):
    ro, ci, v, unchanged = want
    assert got.nnz == len(ci)
    assert got.row_offsets.tobytes() == ro.tobytes(), "row_offsets differ"
    assert got.col_ids.tobytes() == ci.tobytes(), "col_ids differ"
    assert got.data.dtype == v.dtype and got.data.tobytes() == v.tobytes(), "values differ"
    if info is not None:
        assert (info.kept, info.nnz_out, info.rows_unchanged) == (len(ci), len(ci), unchanged)
        assert info.dropped == nnz_in - len(ci)


def check(cfg, H, dA=None, dPattern=None, matOut=None, **pred):
    """one call held against the numpy reference of the same predicates"""
    dA = dA or sa.dCSR.from_host(H)
    kwargs = dict(pred)
    if "pattern" in pred:
        kwargs["pattern"] = dPattern or sa.dCSR.from_host(pred["pattern"])
    dC, info = sa.select(dA, cfg, matOut=matOut, **kwargs)
    got = dC.to_host()
    assert dC.dtype == H.data.dtype and (got.rows, got.cols) == (H.rows, H.cols)
    same(got, reference(H, **pred), info, H.nnz)
    return dC, info, got


def median_abs(H):
    return float(np.median(np.abs(H.data))) if H.nnz else 0.0


# ---------------------------------------------------------------------------------------------------- 1: sizes at the seams
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nnz", [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193])
def test_entry_counts_at_the_word_and_tile_boundaries(cfg, dtype, nnz):
    """the four keep bytes of a word (0 .. 5 entries), the 4096 entries of a compaction tile"""
    rng = np.random.default_rng(nnz)
    cuts = np.sort(rng.integers(0, nnz + 1, size=6))
    H = from_lengths(np.diff(np.concatenate([[0], cuts, [nnz]])), 97, 100 + nnz, dtype)
    assert H.nnz == nnz
    _, info, _ = check(cfg, H, abs_gt=median_abs(H))
    assert nnz < 3 or 0 < info.kept < nnz
    check(cfg, H)                                           # no predicate: a copy
    check(cfg, H, abs_gt=0.0, negate=("abs",))              # the zeros alone
    check(cfg, H, band=(None, 40), abs_gt=median_abs(H))


ROW_COUNTS = sorted({1023, 1024, 1025, 2049} | {T + d for T in TILES for d in (-1, 0, 1)})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("long_rows", [False, True])
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_at_the_tile_and_scan_boundaries(cfg, dtype, long_rows, rows):
    """the 1024 rows of a workgroup of the scan; the rows of a tile of the marking pass, in the kernel that walks tiles of
    that size and in the other one (the average row length picks it)"""
    rng = np.random.default_rng(rows)
    lens = rng.integers(LONG_AVG, LONG_AVG + 17, size=rows) if long_rows else rng.integers(0, 6, size=rows)
    H = from_lengths(lens, 3000, 200 + rows, dtype)
    assert (H.nnz // rows >= LONG_AVG) == long_rows
    _, info, _ = check(cfg, H, band=(-1500, 0), abs_gt=0.0)
    assert 0 < info.kept < H.nnz and info.rows_unchanged < rows
    assert long_rows or info.rows_unchanged > 0
    check(cfg, H, pattern=canonical(random_csr(rows, 3000, 2, 300 + rows)), negate=("pattern",), abs_gt=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_long_row_between_short_ones(cfg, dtype):
    lens = np.full(41, 3)
    lens[20] = 10_000                                       # several compaction tiles, and its tile of the marking pass alone
    H = from_lengths(lens, 50_000, 7, dtype)
    _, info, got = check(cfg, H, abs_gt=median_abs(H))
    assert 1000 < got.row_offsets[21] - got.row_offsets[20] < 9000
    check(cfg, H, band=(None, 20_000))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_first_last_and_everywhere(cfg, dtype):
    lens = np.array([0, 0, 0, 5, 2, 0, 7, 1, 0, 0])
    H = from_lengths(lens, 30, 11, dtype)
    _, info, _ = check(cfg, H, band=(0, None))
    assert info.rows_unchanged >= 6
    E = from_lengths(np.zeros(300, dtype=np.int64), 30, 12, dtype)
    for pred in ({}, {"band": (0, 0)}, {"abs_gt": 1.0}, {"pattern": canonical(random_csr(300, 30, 3, 13))}):
        _, info, got = check(cfg, E, **pred)
        assert got.nnz == 0 and (got.row_offsets == 0).all() and info.rows_unchanged == 300


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_row_and_a_single_column(cfg, dtype):
    wide = from_lengths([5000], 5000, 21, dtype)
    check(cfg, wide, band=(100, 4000), abs_gt=0.0)
    tall = from_lengths(np.random.default_rng(22).integers(0, 3, size=5000), 1, 23, dtype)
    _, info, _ = check(cfg, tall, band=(None, -2500))
    assert 0 < info.kept < tall.nnz
    check(cfg, tall, abs_gt=median_abs(tall), negate=("abs",))


# ---------------------------------------------------------------------------------------------------- 2: BAND
def rect(dtype):
    return canonical(random_csr(200, 317, 12, 31, empty_row_frac=0.05), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [-3, -1, 0, 1, 3])
def test_tril_and_triu_against_scipy(cfg, dtype, k):
    H = rect(dtype)
    S = sp.csr_matrix((H.data, H.col_ids, H.row_offsets.astype(np.int64)), shape=(H.rows, H.cols))
    dA = sa.dCSR.from_host(H)
    for ours, theirs, band in ((sa.tril, sp.tril, (None, k)), (sa.triu, sp.triu, (k, None))):
        got = ours(dA, cfg, k=k).to_host()
        want = theirs(S, k=k, format="csr")
        want.sort_indices()
        assert 0 < want.nnz < S.nnz
        assert got.row_offsets.tobytes() == want.indptr.astype(np.uint32).tobytes()
        assert got.col_ids.tobytes() == want.indices.astype(np.uint32).tobytes()
        assert got.data.tobytes() == want.data.astype(dtype).tobytes()
        same(got, reference(H, band=band))


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_diagonal_off_diagonal_open_and_empty(cfg, dtype):
    H = rect(dtype)
    dA = sa.dCSR.from_host(H)
    _, info, _ = check(cfg, H, dA=dA, band=(0, 0))
    assert 0 < info.kept <= 200
    _, off, _ = check(cfg, H, dA=dA, band=(0, 0), negate=("band",))
    assert off.kept == H.nnz - info.kept
    _, everything, _ = check(cfg, H, dA=dA, band=(None, None))
    assert everything.kept == H.nnz and everything.rows_unchanged == H.rows
    _, nothing, got = check(cfg, H, dA=dA, band=(INT64_MIN + 1, INT64_MIN + 1))
    assert nothing.kept == 0 and (got.row_offsets == 0).all()
    _, info, _ = check(cfg, H, dA=dA, band=(INT64_MIN + 1, INT64_MIN + 1), negate=("band",))
    assert info.kept == H.nnz
    check(cfg, H, dA=dA, band=(-5, 9))
    check(cfg, H, dA=dA, band=(INT64_MAX, INT64_MAX))


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_on_a_row_range_view_with_row_base(cfg, dtype):
    H = canonical(random_csr(300, 300, 9, 41), dtype)
    dA = sa.dCSR.from_host(H)
    full = reference(H, band=(-2, 1))
    for r0, r1 in ((0, 300), (100, 220), (299, 300), (7, 7)):
        dC, info = sa.select(dA.row_view(r0, r1), cfg, band=(-2, 1), row_base=r0)
        got = dC.to_host()
        a, b = int(full[0][r0]), int(full[0][r1])
        assert got.rows == r1 - r0 and got.row_offsets.tobytes() == (full[0][r0:r1 + 1] - full[0][r0]).astype(np.uint32).tobytes()
        assert got.col_ids.tobytes() == full[1][a:b].tobytes() and got.data.tobytes() == full[2][a:b].tobytes()
        assert info.kept == b - a
    # ... and without row_base the view is a matrix of its own
    V = host(120, 300, H.row_offsets[100:221], H.col_ids, H.data)
    check(cfg, V, dA=dA.row_view(100, 220), band=(-2, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_at_the_column_limit(cfg, dtype):
    """cols = 2^27: the signed difference at both ends"""
    cols = 1 << 27
    H = host(3, cols, [0, 2, 2, 4], [cols - 1, 0, 0, cols - 1], np.array([1, 2, 3, 4], dtype=dtype))
    dA = sa.dCSR.from_host(H)
    kept = {}
    for band in ((None, 0), (0, None), (cols - 1, cols - 1), (-2, -2), (None, -3), (cols, None), (1 - cols, cols - 1)):
        _, info, got = check(cfg, H, dA=dA, band=band)
        kept[band] = list(got.data)
    assert kept[(None, 0)] == [2, 3] and kept[(0, None)] == [1, 2, 4] and kept[(cols - 1, cols - 1)] == [1]
    assert kept[(-2, -2)] == [3] and kept[(None, -3)] == [] and kept[(cols, None)] == [] and len(kept[(1 - cols, cols - 1)]) == 4
    # the same matrix as the LAST rows of a larger one
    check(cfg, H, dA=dA, band=(None, 0), row_base=cols - 3)


# ---------------------------------------------------------------------------------------------------- 3: ABS
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("negate", [(), ("abs",)])
@pytest.mark.parametrize("t", [0.0, 0.5, float("inf")])
def test_abs_on_special_values(cfg, dtype, negate, t):
    tt = dtype(t)
    payload = np.array([0x7FF8_0000_0000_1234 if dtype == np.float64 else 0x7FC0_1234],
                       dtype=np.uint64 if dtype == np.float64 else np.uint32).view(dtype)[0]
    row = np.array([np.nan, payload, np.inf, -np.inf, 0.0, -0.0, np.nextafter(dtype(0), dtype(1)), -tt, tt,
                    np.nextafter(tt, dtype(np.inf)), -np.nextafter(dtype(0), dtype(1))], dtype=dtype)
    n = len(row)
    H = host(3, 16, [0, n, n, 2 * n], np.concatenate([np.arange(n), np.arange(n)[::-1]]), np.concatenate([row, row[::-1]]))
    _, info, got = check(cfg, H, abs_gt=t, negate=negate)
    nans = int(np.isnan(got.data).sum())
    assert nans == (0 if negate else 4)                          # a filter does not hide a NaN; its complement drops it
    if t == 0.0:                                                 # (-t and t are zeros here: four of them in a row)
        zeros = got.data[got.data == 0]
        assert len(zeros) == (8 if negate else 0) and int(np.signbit(zeros).sum()) == (4 if negate else 0)
        assert info.kept == (8 if negate else 2 * n - 8)
    if t == float("inf"):
        assert info.kept == (2 * n - 4 if negate else 4)         # nothing exceeds +inf: only the NaNs are "not <="
    if t == 0.5:
        assert (dtype(0.5) in got.data) == bool(negate) and (np.nextafter(tt, dtype(np.inf)) in got.data) != bool(negate)


def test_abs_threshold_is_compared_in_double_for_float():
    cfg = sa.spECKConfig.initialize(0)
    try:
        v = np.float32(0.1)
        assert float(v) > 0.1
        H = host(1, 4, [0, 4], [0, 1, 2, 3], np.array([v, -v, np.nextafter(v, np.float32(0)), 0.25], dtype=np.float32))
        _, _, got = check(cfg, H, abs_gt=0.1)                    # float32(0.1) lies above the double 0.1
        assert list(got.col_ids) == [0, 1, 3]
        _, _, got = check(cfg, H, abs_gt=float(v))               # ... and not above itself
        assert list(got.col_ids) == [3]
        _, _, got = check(cfg, H, abs_gt=0.1, negate=("abs",))
        assert list(got.col_ids) == [2]
    finally:
        cfg.cleanup()


# ---------------------------------------------------------------------------------------------------- 4: PATTERN
def shuffled_with_duplicates(H, seed, dtype):
    """every row of H shuffled, a third of its entries repeated with another value"""
    rng = np.random.default_rng(seed)
    ro, ci, va = [0], [], []
    for r in range(H.rows):
        a, b = int(H.row_offsets[r]), int(H.row_offsets[r + 1])
        c = H.col_ids[a:b]
        c = np.concatenate([c, c[rng.random(b - a) < 0.33]])
        c = c[rng.permutation(len(c))]
        ci.append(c)
        va.append(rng.standard_normal(len(c)))
        ro.append(ro[-1] + len(c))
    return host(H.rows, H.cols, ro, np.concatenate(ci), np.concatenate(va).astype(dtype))


def pattern_from_rows(rows_cols, cols):
    ro = np.zeros(len(rows_cols) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([len(c) for c in rows_cols])
    ci = np.concatenate(rows_cols).astype(np.uint32) if len(rows_cols) else np.zeros(0, np.uint32)
    return host(len(rows_cols), cols, ro, ci, np.ones(len(ci)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("negate", [(), ("pattern",)])
def test_pattern_on_unsorted_rows_with_duplicates(cfg, dtype, negate):
    A = shuffled_with_duplicates(random_csr(400, 250, 14, 51, empty_row_frac=0.05), 52, dtype)
    M = canonical(random_csr(400, 250, 60, 53, empty_row_frac=0.1))
    dA = sa.dCSR.from_host(A)
    _, info, _ = check(cfg, A, dA=dA, pattern=M, negate=negate)
    assert 0 < info.kept < A.nnz
    # the brackets: an empty pattern, the pattern of A itself, one dense row
    empty = pattern_from_rows([np.zeros(0, np.uint32)] * 400, 250)
    _, info, _ = check(cfg, A, dA=dA, pattern=empty, negate=negate)
    assert info.kept == (A.nnz if negate else 0)
    own = sp.csr_matrix((np.ones(A.nnz), A.col_ids, A.row_offsets.astype(np.int64)), shape=(400, 250))
    own.sum_duplicates()
    own = host(400, 250, own.indptr, own.indices, own.data)
    _, info, _ = check(cfg, A, dA=dA, pattern=own, negate=negate)
    assert info.kept == (0 if negate else A.nnz)
    r = int(np.argmax(np.diff(A.row_offsets.astype(np.int64))))
    dense = pattern_from_rows([np.arange(250) if i == r else np.zeros(0, np.uint32) for i in range(400)], 250)
    _, info, _ = check(cfg, A, dA=dA, pattern=dense, negate=negate)
    row_len = int(A.row_offsets[r + 1] - A.row_offsets[r])
    assert info.kept == (A.nnz - row_len if negate else row_len)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("negate", [(), ("pattern",)])
def test_pattern_rows_of_one_and_of_5000_entries(cfg, dtype, negate):
    """the first and the last probe of the search"""
    cols = 12_000
    long_row = np.arange(1000, 11_000, 2)                                    # 5000 even columns
    assert len(long_row) == 5000
    M = pattern_from_rows([np.array([77]), long_row, np.array([0]), np.array([cols - 1])], cols)
    a_rows = [np.array([76, 77, 78, 77, 0, cols - 1]),
              np.array([999, 1000, 1001, 10_998, 10_999, 11_000, 6000, 6001, 0, cols - 1, 1000, 10_998]),
              np.array([1, 0, cols - 1]), np.array([cols - 2, cols - 1, 0])]
    ro = np.concatenate([[0], np.cumsum([len(c) for c in a_rows])])
    ci = np.concatenate(a_rows)
    A = host(4, cols, ro, ci, np.arange(1, len(ci) + 1).astype(dtype))
    _, info, got = check(cfg, A, pattern=M, negate=negate)
    if not negate:
        assert list(got.col_ids) == [77, 77, 1000, 10_998, 6000, 1000, 10_998, 0, cols - 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pattern_without_values_and_on_views(cfg, dtype):
    A = shuffled_with_duplicates(random_csr(300, 200, 10, 61), 62, dtype)
    M = canonical(random_csr(300, 200, 40, 63))
    dA, dM = sa.dCSR.from_host(A), sa.dCSR.from_host(M)
    bare = sa.dCSR.from_device(M.rows, M.cols, M.nnz, dM._c.row_offsets, dM._c.col_ids, None, keep=dM)   # data == NULL
    want = reference(A, pattern=M)
    for negate in ((), ("pattern",)):
        check(cfg, A, dA=dA, dPattern=bare, pattern=M, negate=negate)
        full = reference(A, pattern=M, negate=negate)
        for r0, r1 in ((0, 150), (150, 300), (37, 38), (10, 290)):
            dC, info = sa.select(dA.row_view(r0, r1), cfg, pattern=dM.row_view(r0, r1), negate=negate)
            got = dC.to_host()
            a, b = int(full[0][r0]), int(full[0][r1])
            assert got.row_offsets.tobytes() == (full[0][r0:r1 + 1] - full[0][r0]).astype(np.uint32).tobytes()
            assert got.col_ids.tobytes() == full[1][a:b].tobytes() and got.data.tobytes() == full[2][a:b].tobytes()
            assert info.kept == b - a
    assert 0 < len(want[1]) < A.nnz


# ---------------------------------------------------------------------------------------------------- 5: combination
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_predicates_in_one_call_equal_three_calls(cfg, dtype):
    A = shuffled_with_duplicates(random_csr(500, 400, 12, 71), 72, dtype)
    A.data[::7] = 0
    M = canonical(random_csr(500, 400, 100, 73))
    dA, dM = sa.dCSR.from_host(A), sa.dCSR.from_host(M)
    t = 0.6
    one, info, got = check(cfg, A, dA=dA, dPattern=dM, band=(-150, 30), abs_gt=t, pattern=M, negate=("pattern",))
    assert 0 < info.kept < A.nnz
    step, i1 = sa.select(dA, cfg, band=(-150, 30))
    step, i2 = sa.select(step, cfg, abs_gt=t)
    step, i3 = sa.select(step, cfg, pattern=dM, negate=("pattern",))
    assert A.nnz > i1.kept > i2.kept > i3.kept == info.kept
    seq = step.to_host()
    assert seq.row_offsets.tobytes() == got.row_offsets.tobytes() and seq.col_ids.tobytes() == got.col_ids.tobytes()
    assert seq.data.tobytes() == got.data.tobytes()


# ---------------------------------------------------------------------------------------------------- 6: with the rest of the library
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_behind_the_multiply_is_the_masked_product(cfg, dtype):
    """the sentence of the masked product's contract, on the device: speck_multiply_* followed by "keep (i,j) in M" has bit
    for bit the offsets and column ids of SPECK_MASK_STRUCTURE; the values against the oracle, within the multiply's bound"""
    A, B = random_csr(300, 300, 8, 81), random_csr(300, 300, 8, 82)
    M = random_csr(300, 300, 60, 83, signed=False)
    as_t = lambda H: po.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, H.data.astype(dtype))
    dA, dB, dM = (sa.dCSR.from_host(canonical(H, dtype)) for H in (A, B, M))
    dFull = sa.dCSR(dtype)
    sa.MultiplyspECK(dA, dB, dFull, cfg)
    dSel, info = sa.select(dFull, cfg, pattern=dM)
    dMasked, minfo = sa.multiply_masked(dA, dB, dM, cfg)
    sel, masked = dSel.to_host(), dMasked.to_host()
    assert 0 < sel.nnz < dFull.nnz and info.nnz_out == minfo.nnz_out
    assert sel.row_offsets.tobytes() == masked.row_offsets.tobytes()
    assert sel.col_ids.tobytes() == masked.col_ids.tobytes()
    R, ab = po.spgemm_f64_of(as_t(A), as_t(B))
    in_m = np.isin(keys(R), keys(M))
    assert sel.col_ids.tobytes() == R.col_ids[in_m].tobytes()
    tol = TOL32 if dtype == np.float32 else TOL64
    for got in (sel, masked):
        assert (np.abs(got.data.astype(np.float64) - R.data[in_m]) <= tol * ab[in_m] + 1e-300).all()
    # the complement: what the product holds outside M
    dRest, rest = sa.select(dFull, cfg, pattern=dM, negate=("pattern",))
    assert rest.kept == dFull.nnz - info.kept and dRest.to_host().col_ids.tobytes() == R.col_ids[~in_m].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_triangles_with_the_triangle_made_on_the_device(cfg, dtype):
    P = sp.random(300, 300, density=4 / 300, random_state=91, format="csr")
    S = ((P + P.T) != 0).astype(np.float64).tocsr()
    S.sort_indices()
    Ls = sp.tril(S, k=-1).tocsr()
    triangles = int(((Ls @ Ls).multiply(Ls)).sum())
    assert triangles > 0
    dS = sa.dCSR.from_host(host(300, 300, S.indptr, S.indices, S.data.astype(dtype)))
    dL = sa.tril(dS, cfg, k=-1)
    assert dL.nnz == Ls.nnz
    dC, info = sa.multiply_masked(dL, dL, dL, cfg)
    assert info.hits == triangles and float(dC.to_host().data.astype(np.float64).sum()) == float(triangles)


# ---------------------------------------------------------------------------------------------------- 7: ownership of C
def test_output_buffers_are_reused_as_the_multiply_reuses_them(cfg):
    H = canonical(random_csr(300, 200, 12, 101))
    dA = sa.dCSR.from_host(H)
    dC, info1, _ = check(cfg, H, dA=dA, band=(None, 0))
    ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets)
    dC, info, _ = check(cfg, H, dA=dA, matOut=dC, band=(None, 0))            # same result size: nothing re-allocated
    assert (dC._c.data, dC._c.col_ids, dC._c.row_offsets) == ptrs and info.nnz_out == info1.nnz_out
    dC, info2, _ = check(cfg, H, dA=dA, matOut=dC, band=(1, None))           # another size: data / col_ids only
    assert info2.nnz_out != info1.nnz_out
    assert dC._c.row_offsets == ptrs[2] and dC._c.data != ptrs[0] and dC._c.col_ids != ptrs[1]
    dC, info3, got = check(cfg, H, dA=dA, matOut=dC, band=(500, None))       # nothing left: as the masked product does it
    assert info3.nnz_out == 0 and dC.nnz == 0 and dC._c.row_offsets == ptrs[2] and (got.row_offsets == 0).all()
    assert dC._c.data and dC._c.col_ids                                      # (buffers of one entry)
    empty = (dC._c.data, dC._c.col_ids)
    dC, _, _ = check(cfg, H, dA=dA, matOut=dC, band=(600, None))             # 0 entries again: kept
    assert (dC._c.data, dC._c.col_ids) == empty
    other = canonical(random_csr(120, 200, 12, 102))
    dC, _, _ = check(cfg, other, matOut=dC, abs_gt=1.0)                      # another row count: row_offsets too
    assert dC.rows == 120
    H32 = canonical(H, np.float32)
    dC, _, _ = check(cfg, H32, matOut=dC, abs_gt=1.0)                        # a matOut of the other dtype is reset
    assert dC.dtype == np.float32


# ---------------------------------------------------------------------------------------------------- 8: refusals write nothing
def _update(d, ro=None, ci=None):
    assert _lib.load().speck_dcsr_update(C_.byref(d._c), ro.ctypes.data if ro is not None else None,
                                         ci.ctypes.data if ci is not None else None, None, 8) == 0


@pytest.mark.parametrize("guard", [0, 4096])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_is_written(guard, dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        if guard:
            cfg.set_option("guard_bytes", guard)
        A = canonical(random_csr(700, 500, 10, 111, empty_row_frac=0.05), dtype)
        M = canonical(random_csr(700, 500, 30, 112))
        r = next(i for i in range(350, 700) if A.row_offsets[i + 1] - A.row_offsets[i] >= 4)
        a_ro_desc = A.row_offsets.copy()
        a_ro_desc[r], a_ro_desc[r + 1] = A.row_offsets[r + 1], A.row_offsets[r]
        a_ro_far = A.row_offsets.copy()
        a_ro_far[-1] = A.nnz + 5                                          # the last offset beyond nnz
        a_ro_wild = A.row_offsets.copy()
        a_ro_wild[r + 1:] = 0xFFFFFF00
        a_col = A.col_ids.copy()
        a_col[int(A.row_offsets[r]) + 1] = A.cols                         # a column id == cols
        m = next(i for i in range(350, 700) if M.row_offsets[i + 1] - M.row_offsets[i] >= 8)
        m0 = int(M.row_offsets[m])
        equal, descending, beyond = M.col_ids.copy(), M.col_ids.copy(), M.col_ids.copy()
        equal[m0 + 3] = equal[m0 + 2]
        descending[m0 + 2], descending[m0 + 3] = M.col_ids[m0 + 3], M.col_ids[m0 + 2]
        beyond[int(M.row_offsets[m + 1]) - 1] = M.cols                    # (still ascending: only the range is wrong)
        m_ro_desc = M.row_offsets.copy()
        m_ro_desc[m], m_ro_desc[m + 1] = M.row_offsets[m + 1], M.row_offsets[m]
        cases = [("A", a_ro_desc, None, ERR_INVALID), ("A", a_ro_far, None, ERR_INVALID), ("A", a_ro_wild, None, ERR_INVALID),
                 ("A", None, a_col, ERR_INVALID), ("M", None, equal, ERR_UNSORTED), ("M", None, descending, ERR_UNSORTED),
                 ("M", None, beyond, ERR_UNSORTED), ("M", m_ro_desc, None, ERR_INVALID)]
        sentinel_n = 1234
        for which, h_ro, h_ci, status in cases:
            d = {"A": sa.dCSR.from_host(A), "M": sa.dCSR.from_host(M)}
            _update(d[which], h_ro, h_ci)
            preds = [dict(pattern=d["M"]), dict(pattern=d["M"], negate=("pattern",), band=(None, 0), abs_gt=0.7)]
            if which == "A":
                preds += [dict(), dict(band=(0, None)), dict(abs_gt=0.7)]
            for pred in preds:
                dC = sa.dCSR(dtype)
                dC.alloc(A.rows, A.cols, sentinel_n)
                s_ro = np.full(A.rows + 1, 0xABABABAB, dtype=np.uint32)
                s_ci = np.full(sentinel_n, 0xCDCDCDCD, dtype=np.uint32)
                s_da = np.full(sentinel_n, -77.25, dtype=dtype)
                assert _lib.load().speck_dcsr_update(C_.byref(dC._c), s_ro.ctypes.data, s_ci.ctypes.data, s_da.ctypes.data,
                                                     np.dtype(dtype).itemsize) == 0
                before = bytes(dC._c)
                with pytest.raises(sa.SpeckError) as e:
                    sa.select(d["A"], cfg, matOut=dC, **pred)
                assert e.value.status == status, (which, status)        # (not 3: no canary zone was touched either)
                assert bytes(dC._c) == before                            # the struct: sizes and the three pointers
                got = dC.to_host()
                assert got.row_offsets.tobytes() == s_ro.tobytes() and got.col_ids.tobytes() == s_ci.tobytes()
                assert got.data.tobytes() == s_da.tobytes()
        # the config serves the valid input afterwards, canary zones intact
        check(cfg, A, pattern=M, band=(None, 0), abs_gt=0.7)
    finally:
        if guard:
            cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


# ---------------------------------------------------------------------------------------------------- 9: canary zones, reuse, stream
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        lens = np.random.default_rng(121).integers(0, 9, size=1500)
        lens[700] = 9000
        A = from_lengths(lens, 2000, 122, dtype)
        M = canonical(random_csr(1500, 2000, 20, 123))
        dA = sa.dCSR.from_host(A)
        for pred in (dict(band=(None, -1)), dict(abs_gt=median_abs(A)), dict(pattern=M), dict(pattern=M, negate=("pattern",)),
                     dict(), dict(band=(-100, 100), abs_gt=0.0, pattern=M)):
            check(cfg, A, dA=dA, **pred)                                 # (a touched zone is status 3)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_a_select_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.08, 7, signed=True)
    S = po.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data)
    R, ab = po.spgemm(S, S)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()

    def multiply_matches():
        sa.MultiplyspECK(dS, dS, dC, cfg)
        got = dC.to_host()
        assert got.nnz == R.nnz and got.row_offsets.tobytes() == R.row_offsets.tobytes()
        assert got.col_ids.tobytes() == R.col_ids.tobytes() and (np.abs(got.data - R.data) <= TOL64 * ab + 1e-300).all()

    multiply_matches()
    multiply_matches()
    assert cfg.last_stats()["replayed"]
    multiply_matches()
    dOut = sa.dCSR()
    for pred in (dict(band=(None, -1)), dict(abs_gt=1.0), dict(pattern=h)):
        check(cfg, h, dA=dS, dPattern=dS, matOut=dOut, **pred)
        multiply_matches()
        assert cfg.last_stats()["replayed"] == 1
    check(cfg, dC.to_host(), dA=dC, abs_gt=1.0)                           # ... and of the product itself, where it lies
    multiply_matches()
    assert cfg.last_stats()["replayed"] == 1


def test_runs_on_the_callers_stream(cfg):
    """the columns of A are written by a copy on the caller's stream right before the call: ordering against the producer
    is by the stream alone"""
    A = canonical(random_csr(2000, 900, 15, 131))
    M = canonical(random_csr(2000, 900, 15, 132))
    dev = torch.device("cuda:0")
    t_ro = torch.from_numpy(A.row_offsets.view(np.int32).copy()).to(dev)
    t_va = torch.from_numpy(A.data.copy()).to(dev)
    t_ci = torch.full((A.nnz,), 900, dtype=torch.int32, device=dev)          # not a valid matrix until the producer has run
    t_real = torch.from_numpy(A.col_ids.view(np.int32).copy()).to(dev)
    dA = sa.dCSR.from_device(A.rows, A.cols, A.nnz, t_ro.data_ptr(), t_ci.data_ptr(), t_va.data_ptr(), keep=(t_ro, t_ci, t_va))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(200_000_000)          # ~0.1 s: whatever does not wait for the stream sees an invalid matrix
            t_ci.copy_(t_real, non_blocking=True)
        _, info, _ = check(cfg, A, dA=dA, band=(None, 0), pattern=M, negate=("pattern",))
        assert 0 < info.kept < A.nnz
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()
