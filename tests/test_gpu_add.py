"""speck_add_* on the GPU (speck_amd/csrc/add.hip).  The expectation is a few lines of numpy: the keys row * cols + col of
both operands, np.union1d for the union, np.searchsorted to place the values, alpha * a.astype(f64) + beta * b.astype(f64)
cast to the value type where both operands hold an entry and the one product alone elsewhere.  (Not scipy's A + B: that
drops the entries that cancel.)  Offsets and column ids are compared bit for bit, the values as raw bytes -- except that a
NaN matches any NaN --, the info counters against the same key sets."""
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
TOL64 = 1e-12                # the bounds of tests/test_gpu_masked.py
TOL32 = 4.0 * 2.0 ** -23
DTYPES = [np.float64, np.float32]
TILES = sa.ADD_TILE_ROWS
LONG_AVG = sa.ADD_LONG_ROW_AVG
ENTRY_TILE = sa.ADD_TILE_ENTRIES
COEFFS = [(1.0, 1.0), (1.0, -1.0), (2.5, -0.5), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def host(rows, cols, ro, ci, data):
    return sa.HostCSR(rows, cols, np.asarray(ro, dtype=np.uint32), np.asarray(ci, dtype=np.uint32), np.asarray(data))


def values(n, rng, dtype):
    return ((0.5 + rng.random(n)) * rng.choice([-1.0, 1.0], size=n)).astype(dtype)


def from_rows(rows_cols, cols, seed, dtype=np.float64):
    """a matrix from one ascending column list per row"""
    rng = np.random.default_rng(seed)
    ro = np.zeros(len(rows_cols) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([len(c) for c in rows_cols])
    ci = np.concatenate([np.asarray(c, dtype=np.uint32) for c in rows_cols]) if len(rows_cols) else np.zeros(0, np.uint32)
    return host(len(rows_cols), cols, ro, ci, values(len(ci), rng, dtype))


def from_lengths(lens, cols, seed, dtype=np.float64):
    """rows of the given lengths, strictly ascending columns drawn without replacement"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max(initial=0) <= cols
    if len(lens) * cols <= 1 << 22:      # every row at once: the lens[r] columns of row r with the smallest random rank
        rank = np.argsort(np.argsort(rng.random((len(lens), cols)), axis=1), axis=1)
        ci = np.nonzero(rank < lens[:, None])[1]
    else:
        ci = np.concatenate([np.sort(rng.choice(cols, size=int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)])
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    return host(len(lens), cols, ro, ci, values(len(ci), rng, dtype))


def spread(nnz, rows, seed):
    """nnz entries cut into `rows` rows at random places"""
    cuts = np.sort(np.random.default_rng(seed).integers(0, nnz + 1, size=rows - 1))
    return np.diff(np.concatenate([[0], cuts, [nnz]]))


def with_dtype(H, dtype):
    return host(H.rows, H.cols, H.row_offsets, H.col_ids, H.data.astype(dtype))


def entries(H):
    """(keys, values) of the entries the rows of H hold; H may be a row-range view with absolute offsets"""
    a, b = int(H.row_offsets[0]), int(H.row_offsets[-1])
    row = np.repeat(np.arange(H.rows, dtype=np.int64), np.diff(H.row_offsets.astype(np.int64)))
    return row * H.cols + H.col_ids[a:b].astype(np.int64), H.data[a:b]


def reference(A, B, alpha=1.0, beta=1.0):
    """(row_offsets, col_ids, data, (only_a, only_b, both)) of alpha A + beta B"""
    dtype = A.data.dtype
    (ka, va), (kb, vb) = entries(A), entries(B)
    assert (np.diff(ka) > 0).all() and (np.diff(kb) > 0).all()
    ku = np.union1d(ka, kb)
    pa, pb = np.searchsorted(ku, ka), np.searchsorted(ku, kb)
    in_a, in_b = np.zeros(len(ku), dtype=bool), np.zeros(len(ku), dtype=bool)
    in_a[pa], in_b[pb] = True, True
    xa, xb = np.zeros(len(ku)), np.zeros(len(ku))
    with np.errstate(all="ignore"):
        xa[pa] = np.float64(alpha) * va.astype(np.float64)       # each product rounded to double
        xb[pb] = np.float64(beta) * vb.astype(np.float64)
        v = np.where(in_a & in_b, xa + xb, np.where(in_a, xa, xb)).astype(dtype)   # the sum to double, once to T
    ro = np.zeros(A.rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(np.bincount(ku // max(A.cols, 1), minlength=A.rows))
    both = int((in_a & in_b).sum())
    return ro, (ku % max(A.cols, 1)).astype(np.uint32), v, (len(ka) - both, len(kb) - both, both)


def same(got, want, info=None):
    ro, ci, v, counts = want
    assert got.nnz == len(ci)
    assert got.row_offsets.tobytes() == ro.tobytes(), "row_offsets differ"
    assert got.col_ids.tobytes() == ci.tobytes(), "col_ids differ"
    assert got.data.dtype == v.dtype
    nan = np.isnan(v)
    assert (np.isnan(got.data) == nan).all(), "NaNs differ"
    assert got.data[~nan].tobytes() == v[~nan].tobytes(), "values differ"
    if info is not None:
        assert (info.only_a, info.only_b, info.both) == counts
        assert info.nnz_out == len(ci) == sum(counts)


def check(cfg, A, B, alpha=1.0, beta=1.0, dA=None, dB=None, matOut=None):
    """one call held against the numpy reference"""
    dA = dA or sa.dCSR.from_host(A)
    dB = dB or sa.dCSR.from_host(B)
    dC, info = sa.add(dA, dB, cfg, alpha=alpha, beta=beta, matOut=matOut)
    got = dC.to_host()
    assert dC.dtype == A.data.dtype and (got.rows, got.cols) == (A.rows, A.cols)
    same(got, reference(A, B, alpha, beta), info)
    return dC, info, got


# ---------------------------------------------------------------------------------------------------- 1: sizes at the seams
SEAM_NNZ = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193]
SEAM_COLS = 9000
_seam = {}


def seam_operand(which, nnz, dtype):
    """the operand of `nnz` entries over 7 rows: made once, never changed"""
    key = (which, nnz)
    if key not in _seam:
        _seam[key] = from_lengths(spread(nnz, 7, 10 * nnz + which), SEAM_COLS, 1000 + 10 * nnz + which)
        assert _seam[key].nnz == nnz
    return with_dtype(_seam[key], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nnz_a", SEAM_NNZ)
def test_entry_counts_at_the_word_and_tile_boundaries(cfg, dtype, nnz_a):
    """the four match bytes of a word (0 .. 5 entries), the 4096 entries of a tile of the write pass, in A and in B
    independently"""
    A = seam_operand(0, nnz_a, dtype)
    dA = sa.dCSR.from_host(A)
    overlap = 0
    for nnz_b in SEAM_NNZ:
        _, info, _ = check(cfg, A, seam_operand(1, nnz_b, dtype), 2.5, -0.5, dA=dA)
        overlap += info.both
    assert nnz_a < 4095 or overlap > 0


ROW_COUNTS = sorted({1023, 1024, 1025, 2049} | {T + d for T in TILES + (ENTRY_TILE,) for d in (-1, 0, 1)})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("long_rows", [False, True])
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_at_the_tile_and_scan_boundaries(cfg, dtype, long_rows, rows):
    """the 1024 rows of a workgroup of the scan; the rows of a tile of the marking pass, in the kernel that walks tiles of
    that size and in the other one (the average row length picks it); as many rows as a tile of the write pass has entries"""
    rng = np.random.default_rng(rows)
    cols = 60 if long_rows else 12
    lo, hi = (LONG_AVG // 2, LONG_AVG // 2 + 9) if long_rows else (0, 6)
    A = from_lengths(rng.integers(lo, hi, size=rows), cols, 200 + rows, dtype)
    B = from_lengths(rng.integers(lo, hi, size=rows), cols, 300 + rows, dtype)
    assert ((A.nnz + B.nnz) // rows >= LONG_AVG) == long_rows
    _, info, _ = check(cfg, A, B, 1.0, -1.0)
    assert info.both > 0 and info.only_a > 0 and info.only_b > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_long_row_between_short_ones(cfg, dtype):
    """one row of 9 000 + 7 000 entries, about half of them in both: the tiles of the write pass cut the row, and the waves
    around it cut rows"""
    A, B = long_row_pair(dtype)
    _, info, got = check(cfg, A, B, 2.5, -0.5)
    assert 3000 < info.both < 4500
    assert got.row_offsets[151] - got.row_offsets[150] > 12_000


def long_row_pair(dtype):
    rng = np.random.default_rng(7)
    cols = 20_000
    a_long = np.sort(rng.choice(cols, size=9000, replace=False))
    outside = np.setdiff1d(np.arange(cols), a_long)
    b_long = np.sort(np.concatenate([rng.choice(a_long, size=3500, replace=False), rng.choice(outside, size=3500, replace=False)]))
    rows_a = [np.sort(rng.choice(40, size=int(k), replace=False)) for k in rng.integers(0, 9, size=300)]
    rows_b = [np.sort(rng.choice(40, size=int(k), replace=False)) for k in rng.integers(0, 9, size=300)]
    rows_a[150], rows_b[150] = a_long, b_long
    return from_rows(rows_a, cols, 8, dtype), from_rows(rows_b, cols, 9, dtype)


# ---------------------------------------------------------------------------------------------------- 2: overlap laws
def law_rows(law, n, rng):
    """(columns of A, columns of B) of a row of about 2 n entries that follows the law; cols = 4 n + 2"""
    if law == "disjoint":
        p = rng.permutation(4 * n)
        return np.sort(p[:n]), np.sort(p[n:2 * n])
    if law == "identical":
        c = np.sort(rng.choice(4 * n, size=n, replace=False))
        return c, c
    if law in ("b_in_a", "a_in_b"):
        big = np.sort(rng.choice(4 * n, size=n, replace=False))
        small = np.sort(rng.choice(big, size=max(n // 2, 1), replace=False))
        return (big, small) if law == "b_in_a" else (small, big)
    if law == "interleaved":
        return np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2)
    if law == "b_before_a":
        return np.arange(2 * n, 3 * n), np.arange(0, n)
    if law == "b_after_a":
        return np.arange(0, n), np.arange(2 * n, 3 * n)
    if law == "a_empty":
        return np.zeros(0, np.int64), np.sort(rng.choice(4 * n, size=n, replace=False))
    if law == "b_empty":
        return np.sort(rng.choice(4 * n, size=n, replace=False)), np.zeros(0, np.int64)
    assert law == "both_empty"
    return np.zeros(0, np.int64), np.zeros(0, np.int64)


LAWS = ["disjoint", "identical", "b_in_a", "a_in_b", "interleaved", "b_before_a", "b_after_a", "a_empty", "b_empty", "both_empty"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("law", LAWS + ["mixed"])
def test_overlap_laws_in_one_row_and_across_rows(cfg, dtype, law):
    rng = np.random.default_rng(LAWS.index(law) if law in LAWS else 99)
    n_max = 70
    for rows in (1, 90):
        pairs = [law_rows(law if law in LAWS else LAWS[rng.integers(len(LAWS))], int(rng.integers(1, n_max + 1)), rng)
                 for _ in range(rows)]
        if law == "mixed" and rows > 1:                  # empty first and last rows
            pairs[0] = pairs[-1] = law_rows("both_empty", 1, rng)
        A = from_rows([p[0] for p in pairs], 4 * n_max + 2, 21, dtype)
        B = from_rows([p[1] for p in pairs], 4 * n_max + 2, 22, dtype)
        for alpha, beta in ((1.0, 1.0), (2.5, -0.5)):
            _, info, _ = check(cfg, A, B, alpha, beta)
        if law == "identical":
            assert info.both == A.nnz == B.nnz and info.only_a == info.only_b == 0
        if law in ("disjoint", "interleaved", "b_before_a", "b_after_a"):
            assert info.both == 0 and info.nnz_out == A.nnz + B.nnz
        if law == "b_in_a":
            assert info.both == B.nnz and info.only_b == 0
        if law == "a_in_b":
            assert info.both == A.nnz and info.only_a == 0
        if law == "both_empty":
            assert info.nnz_out == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_row_and_a_single_column(cfg, dtype):
    wide_a, wide_b = from_lengths([3000], 5000, 31, dtype), from_lengths([2500], 5000, 32, dtype)
    _, info, _ = check(cfg, wide_a, wide_b, 1.0, -1.0)
    assert 0 < info.both < 2500
    rng = np.random.default_rng(33)
    tall_a, tall_b = from_lengths(rng.integers(0, 2, size=5000), 1, 34, dtype), from_lengths(rng.integers(0, 2, size=5000), 1, 35, dtype)
    _, info, _ = check(cfg, tall_a, tall_b, 2.5, -0.5)
    assert info.both > 0 and info.only_a > 0 and info.only_b > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_and_last_column_at_the_column_limit(cfg, dtype):
    cols = 1 << 27
    A = host(4, cols, [0, 2, 3, 3, 4], [0, cols - 1, 0, cols - 1], np.array([1, 2, 3, 4], dtype=dtype))
    B = host(4, cols, [0, 2, 3, 4, 4], [0, cols - 1, cols - 1, 0], np.array([10, 20, 30, 40], dtype=dtype))
    _, info, got = check(cfg, A, B)
    assert list(got.col_ids) == [0, cols - 1, 0, cols - 1, 0, cols - 1] and list(got.data) == [11, 22, 3, 30, 40, 4]
    assert (info.only_a, info.only_b, info.both) == (2, 2, 2)


# ---------------------------------------------------------------------------------------------------- 3: values
def random_pair(dtype, rows=400, cols=250, seed=41):
    return (with_dtype(random_csr(rows, cols, 14, seed, empty_row_frac=0.05), dtype),
            with_dtype(random_csr(rows, cols, 10, seed + 1, empty_row_frac=0.1), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_coefficients(cfg, dtype):
    A, B = random_pair(dtype)
    dA, dB = sa.dCSR.from_host(A), sa.dCSR.from_host(B)
    patterns = set()
    for alpha, beta in COEFFS:
        _, info, got = check(cfg, A, B, alpha, beta, dA=dA, dB=dB)
        patterns.add((got.row_offsets.tobytes(), got.col_ids.tobytes()))
        assert info.both > 0 and info.only_a > 0 and info.only_b > 0
    assert len(patterns) == 1                               # a zero coefficient removes nothing


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_minus_a_keeps_every_entry_as_plus_zero(cfg, dtype):
    A, _ = random_pair(dtype, seed=51)
    _, info, got = check(cfg, A, A, 1.0, -1.0)
    assert got.nnz == A.nnz and info.both == A.nnz
    assert got.col_ids.tobytes() == A.col_ids.tobytes() and got.row_offsets.tobytes() == A.row_offsets.tobytes()
    assert (got.data == 0).all() and not np.signbit(got.data).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_device_matrix_passed_twice(cfg, dtype):
    A, _ = random_pair(dtype, seed=61)
    dA = sa.dCSR.from_host(A)
    _, info, got = check(cfg, A, A, dA=dA, dB=dA)
    assert info.both == A.nnz and got.data.tobytes() == (A.data + A.data).tobytes()
    check(cfg, A, A, 2.5, -0.5, dA=dA, dB=dA)


def test_f32_products_and_sum_stay_in_double_until_the_one_rounding(cfg):
    """alpha a = 1 + 2^-24 is exact in double and a tie in float: rounded to float on its own it falls to 1, and b = 2^-30
    is lost; kept in double the sum lies above the tie and rounds up"""
    alpha, beta = 1.0 + 2.0 ** -24, 1.0
    a, b = np.array([1.0, 1.0, 3.0], dtype=np.float32), np.array([2.0 ** -30, 7.0], dtype=np.float32)
    A = host(1, 4, [0, 3], [0, 1, 3], a)
    B = host(1, 4, [0, 2], [0, 2], b)
    once = (alpha * a[:1].astype(np.float64) + beta * b[:1].astype(np.float64)).astype(np.float32)
    twice = (alpha * a[:1].astype(np.float64)).astype(np.float32) + (beta * b[:1].astype(np.float64)).astype(np.float32)
    assert once[0] != twice[0] and once[0] == np.float32(1.0 + 2.0 ** -23) and twice[0] == np.float32(1.0)
    _, _, got = check(cfg, A, B, alpha, beta)
    assert got.data[0] == once[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_and_subnormal_values(cfg, dtype):
    inf, nan = np.inf, np.nan
    tiny = np.finfo(dtype).tiny                              # the smallest normal
    sub = np.nextafter(dtype(0), dtype(1))                   # the smallest subnormal
    #            both ......................................................................... | A alone ....... | B alone
    a = [inf, -inf, inf, nan, 1.0, -0.0, -0.0, 0.0, inf, tiny, sub, 3 * sub, tiny, -tiny, 1.0] + [inf, nan, -0.0, sub, tiny]
    b = [inf, -inf, -inf, 1.0, nan, -0.0, 0.0, -0.0, 0.0, -tiny / 2, sub, -sub, -tiny, tiny / 4, inf] + [-inf, nan, -0.0, sub, -tiny]
    nb, na = 15, 5
    A = host(2, 64, [0, nb + na, nb + na], np.concatenate([np.arange(nb), 20 + np.arange(na)]), np.array(a, dtype=dtype))
    B = host(2, 64, [0, nb + na, nb + na], np.concatenate([np.arange(nb), 40 + np.arange(na)]), np.array(b, dtype=dtype))
    dA, dB = sa.dCSR.from_host(A), sa.dCSR.from_host(B)
    for alpha, beta in COEFFS + [(0.5, 0.5), (0.25, 1.0), (-1.0, -1.0)]:
        _, _, got = check(cfg, A, B, alpha, beta, dA=dA, dB=dB)
        v = got.data
        if (alpha, beta) == (1.0, 1.0):
            assert np.isnan(v[2]) and np.isinf(v[0])                          # inf + (-inf); inf + inf
            assert v[5] == 0 and np.signbit(v[5]) and not np.signbit(v[6])    # -0 + -0 = -0, -0 + 0 = +0
            assert v[9] == tiny / 2 and v[10] == 2 * sub and v[11] == 2 * sub  # sums in the subnormal range
            assert v[13] != 0 and abs(v[13]) < tiny
            assert np.signbit(v[nb + 2]) and v[nb + 3] == sub                 # an entry of one operand alone: as it was
        if alpha == 0.0:
            assert np.isnan(v[0]) and np.isnan(v[nb])                         # 0 * inf shields nothing
        if (alpha, beta) == (0.5, 0.5):
            assert v[nb + 4] == tiny / 2                                      # a product in the subnormal range
            assert v[12] == 0


# ---------------------------------------------------------------------------------------------------- 4: views
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_range_views_with_their_own_bases(cfg, dtype):
    A, B = random_pair(dtype, rows=300, cols=200, seed=71)
    dA, dB = sa.dCSR.from_host(A), sa.dCSR.from_host(B)
    for r0, r1 in ((0, 300), (100, 220), (299, 300), (7, 7), (150, 300)):
        VA = host(r1 - r0, A.cols, A.row_offsets[r0:r1 + 1], A.col_ids, A.data)
        VB = host(r1 - r0, B.cols, B.row_offsets[r0:r1 + 1], B.col_ids, B.data)
        assert r0 in (0, 7) or VA.row_offsets[0] != VB.row_offsets[0]
        _, info, got = check(cfg, VA, VB, 2.5, -0.5, dA=dA.row_view(r0, r1), dB=dB.row_view(r0, r1))
        assert got.row_offsets[0] == 0
    # ... and a view of one operand beside the other one whole
    VA = host(120, A.cols, A.row_offsets[100:221], A.col_ids, A.data)
    B120 = with_dtype(random_csr(120, 200, 10, 73), dtype)
    check(cfg, VA, B120, dA=dA.row_view(100, 220))
    check(cfg, B120, VA, dB=dA.row_view(100, 220))


# ---------------------------------------------------------------------------------------------------- 5: with the rest of the library
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_product_plus_its_operand(cfg, dtype):
    """add(multiply(S, S), S): the pattern against the oracle's product and the numpy union, the product's values within
    the bound of tests/test_gpu_masked.py, and the sum bit for bit what numpy makes of the product as the device holds it"""
    h = sa.gen_matrix("scircuit", 0.05, 7, signed=True)
    S = po.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data.astype(dtype))
    R, ab = po.spgemm_f64_of(S, S)
    dS, dP = sa.dCSR.from_host(S), sa.dCSR(dtype)
    sa.MultiplyspECK(dS, dS, dP, cfg)
    P = dP.to_host()
    assert P.row_offsets.tobytes() == R.row_offsets.tobytes() and P.col_ids.tobytes() == R.col_ids.tobytes()
    tol = TOL32 if dtype == np.float32 else TOL64
    assert (np.abs(P.data.astype(np.float64) - R.data) <= tol * ab + 1e-300).all()
    dC, info = sa.add(dP, dS, cfg)
    got = dC.to_host()
    same(got, reference(P, S), info)
    want = reference(host(R.rows, R.cols, R.row_offsets, R.col_ids, R.data), with_dtype(S, np.float64))
    assert got.row_offsets.tobytes() == want[0].tobytes() and got.col_ids.tobytes() == want[1].tobytes()
    assert info.both > 0 and info.only_a > 0
    # C is a valid input of the multiply, as the operand whose rows it checks
    dD = sa.dCSR(dtype)
    sa.MultiplyspECK(dS, dC, dD, cfg)
    D = dD.to_host()
    R2, _ = po.spgemm_f64_of(S, po.HostCSR(got.rows, got.cols, got.row_offsets, got.col_ids, got.data))
    assert D.row_offsets.tobytes() == R2.row_offsets.tobytes() and D.col_ids.tobytes() == R2.col_ids.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_symmetrize_then_triangles(cfg, dtype):
    P = sp.random(300, 300, density=4 / 300, random_state=91, format="csr")
    P.data[:] = 1.0
    P.sort_indices()
    S = ((P + P.T) != 0).astype(np.float64).tocsr()
    S.sort_indices()
    Ls = sp.tril(S, k=-1).tocsr()
    triangles = int(((Ls @ Ls).multiply(Ls)).sum())
    assert triangles > 0
    HP = host(300, 300, P.indptr, P.indices, P.data.astype(dtype))
    dS = sa.symmetrize(sa.dCSR.from_host(HP), cfg)
    got = dS.to_host()
    assert got.row_offsets.tobytes() == S.indptr.astype(np.uint32).tobytes()
    assert got.col_ids.tobytes() == S.indices.astype(np.uint32).tobytes()
    keys, _ = entries(got)
    assert np.array_equal(np.sort((keys % 300) * 300 + keys // 300), keys)          # the pattern is symmetric
    T = sp.csr_matrix((got.data, got.col_ids, got.row_offsets.astype(np.int64)), shape=(300, 300))
    assert (T != T.T).nnz == 0 and got.data.tobytes() == (P + P.T).tocsr().data.astype(dtype).tobytes()
    dL = sa.tril(dS, cfg, k=-1)
    assert dL.nnz == Ls.nnz
    _, info = sa.multiply_masked(dL, dL, dL, cfg)
    assert info.hits == triangles


# ---------------------------------------------------------------------------------------------------- 6: ownership of C
def test_output_buffers_are_reused_as_the_multiply_reuses_them(cfg):
    A, B = random_pair(np.float64, rows=300, cols=200, seed=101)
    dA, dB = sa.dCSR.from_host(A), sa.dCSR.from_host(B)
    dC, info1, _ = check(cfg, A, B, dA=dA, dB=dB)
    ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets)
    dC, info, _ = check(cfg, A, B, 2.0, 3.0, dA=dA, dB=dB, matOut=dC)       # same result size: nothing re-allocated
    assert (dC._c.data, dC._c.col_ids, dC._c.row_offsets) == ptrs and info.nnz_out == info1.nnz_out
    dC, info2, _ = check(cfg, A, A, dA=dA, dB=dA, matOut=dC)                 # another size: data / col_ids only
    assert info2.nnz_out != info1.nnz_out
    assert dC._c.row_offsets == ptrs[2] and dC._c.data != ptrs[0] and dC._c.col_ids != ptrs[1]
    E = from_lengths(np.zeros(300, dtype=np.int64), 200, 102)
    dC, info3, got = check(cfg, E, E, matOut=dC)                             # nothing at all
    assert info3.nnz_out == 0 and dC.nnz == 0 and dC._c.row_offsets == ptrs[2] and (got.row_offsets == 0).all()
    assert dC._c.data and dC._c.col_ids                                      # (buffers of one entry)
    empty = (dC._c.data, dC._c.col_ids)
    dC, _, _ = check(cfg, E, E, 0.0, 0.0, matOut=dC)                         # 0 entries again: kept
    assert (dC._c.data, dC._c.col_ids) == empty
    A120, B120 = random_pair(np.float64, rows=120, cols=200, seed=103)
    dC, _, _ = check(cfg, A120, B120, matOut=dC)                             # another row count: row_offsets too
    assert dC.rows == 120
    dC, _, _ = check(cfg, with_dtype(A, np.float32), with_dtype(B, np.float32), matOut=dC)   # the other dtype: reset
    assert dC.dtype == np.float32 and dC.rows == 300


# ---------------------------------------------------------------------------------------------------- 7: refusals write nothing
def _update(d, ro=None, ci=None):
    assert _lib.load().speck_dcsr_update(C_.byref(d._c), ro.ctypes.data if ro is not None else None,
                                         ci.ctypes.data if ci is not None else None, None, 8) == 0


def hostile(H):
    """[(row_offsets or None, col_ids or None, status)]: what the pass has to refuse in an operand"""
    r = next(i for i in range(350, 700) if H.row_offsets[i + 1] - H.row_offsets[i] >= 8)
    r0 = int(H.row_offsets[r])
    ro_desc = H.row_offsets.copy()
    ro_desc[r], ro_desc[r + 1] = H.row_offsets[r + 1], H.row_offsets[r]
    ro_far = H.row_offsets.copy()
    ro_far[-1] = H.nnz + 5                                            # the last offset beyond nnz
    ro_wild = H.row_offsets.copy()
    ro_wild[r + 1:] = 0xFFFFFF00
    beyond, equal, descending = H.col_ids.copy(), H.col_ids.copy(), H.col_ids.copy()
    beyond[int(H.row_offsets[r + 1]) - 1] = H.cols                    # (still ascending: only the range is wrong)
    equal[r0 + 3] = equal[r0 + 2]
    descending[r0 + 2], descending[r0 + 3] = H.col_ids[r0 + 3], H.col_ids[r0 + 2]
    return [(ro_desc, None, ERR_INVALID), (ro_far, None, ERR_INVALID), (ro_wild, None, ERR_INVALID),
            (None, beyond, ERR_UNSORTED), (None, equal, ERR_UNSORTED), (None, descending, ERR_UNSORTED)]


@pytest.mark.parametrize("guard", [0, 4096])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_is_written(guard, dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        if guard:
            cfg.set_option("guard_bytes", guard)
        A = with_dtype(random_csr(700, 500, 10, 111, empty_row_frac=0.05), dtype)
        B = with_dtype(random_csr(700, 500, 12, 112, empty_row_frac=0.05), dtype)
        sentinel_n = 1234
        for which, H in (("A", A), ("B", B)):
            for h_ro, h_ci, status in hostile(H):
                d = {"A": sa.dCSR.from_host(A), "B": sa.dCSR.from_host(B)}
                _update(d[which], h_ro, h_ci)
                dC = sa.dCSR(dtype)
                dC.alloc(A.rows, A.cols, sentinel_n)
                s_ro = np.full(A.rows + 1, 0xABABABAB, dtype=np.uint32)
                s_ci = np.full(sentinel_n, 0xCDCDCDCD, dtype=np.uint32)
                s_da = np.full(sentinel_n, -77.25, dtype=dtype)
                assert _lib.load().speck_dcsr_update(C_.byref(dC._c), s_ro.ctypes.data, s_ci.ctypes.data, s_da.ctypes.data,
                                                     np.dtype(dtype).itemsize) == 0
                before = bytes(dC._c)
                with pytest.raises(sa.SpeckError) as e:
                    sa.add(d["A"], d["B"], cfg, alpha=2.5, beta=-0.5, matOut=dC)
                assert e.value.status == status, (which, status)        # (not 3: no canary zone was touched either)
                assert bytes(dC._c) == before                            # the struct: sizes and the three pointers
                got = dC.to_host()
                assert got.row_offsets.tobytes() == s_ro.tobytes() and got.col_ids.tobytes() == s_ci.tobytes()
                assert got.data.tobytes() == s_da.tobytes()
        # the config serves the valid pair afterwards, canary zones intact
        check(cfg, A, B, 2.5, -0.5)
    finally:
        if guard:
            cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


# ---------------------------------------------------------------------------------------------------- 8: canary zones, reuse, stream
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        A, B = long_row_pair(dtype)
        check(cfg, A, B, 2.5, -0.5)                                      # (a touched zone is status 3)
        for nnz_a in SEAM_NNZ:
            for nnz_b in SEAM_NNZ:
                check(cfg, seam_operand(0, nnz_a, dtype), seam_operand(1, nnz_b, dtype))
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_an_add_between_two_multiplies_keeps_the_reuse_sequence(cfg):
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
    Sh = host(h.rows, h.cols, h.row_offsets, h.col_ids, h.data)
    check(cfg, Sh, Sh, 1.0, -1.0, dA=dS, dB=dS, matOut=dOut)
    multiply_matches()
    assert cfg.last_stats()["replayed"] == 1
    check(cfg, dC.to_host(), Sh, dA=dC, dB=dS, matOut=dOut)               # ... and of the product itself, where it lies
    multiply_matches()
    assert cfg.last_stats()["replayed"] == 1


def test_runs_on_the_callers_stream(cfg):
    """the columns of B are written by a copy on the caller's stream right before the call: ordering against the producer
    is by the stream alone"""
    A, B = random_pair(np.float64, rows=2000, cols=900, seed=131)
    dev = torch.device("cuda:0")
    t_ro = torch.from_numpy(B.row_offsets.view(np.int32).copy()).to(dev)
    t_va = torch.from_numpy(B.data.copy()).to(dev)
    t_ci = torch.full((B.nnz,), 900, dtype=torch.int32, device=dev)          # not a valid matrix until the producer has run
    t_real = torch.from_numpy(B.col_ids.view(np.int32).copy()).to(dev)
    dB = sa.dCSR.from_device(B.rows, B.cols, B.nnz, t_ro.data_ptr(), t_ci.data_ptr(), t_va.data_ptr(), keep=(t_ro, t_ci, t_va))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(200_000_000)          # ~0.1 s: whatever does not wait for the stream sees an invalid matrix
            t_ci.copy_(t_real, non_blocking=True)
        _, info, _ = check(cfg, A, B, 2.5, -0.5, dB=dB)
        assert info.both > 0
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config(dtype):
    A, B = random_pair(dtype, seed=141)
    _, info, _ = check(None, A, B, 1.0, -1.0)
    assert info.both > 0
