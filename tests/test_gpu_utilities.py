"""compare, transpose and the device copy at every lane, tile and pass edge (inputs and expectations: test_utilities_host.py).

Everything is bit-exact: results are compared as raw bytes with numpy's stable sort / the host slices, mismatch counts with the
number of rows planted.  The values of a transposed matrix are the entries' input positions, so an unstable order shows; the
bound checks of compare use dyadic numbers that sit on the bound itself.
"""
import ctypes as C

import numpy as np
import pytest

import speck_amd as sa
from speck_amd import _lib
import test_utilities_host as U

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
_ids = lambda d: np.dtype(d).name   # noqa: E731


@pytest.fixture(scope="module")
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


def check_transpose(cfg, H, dtype=np.float64):
    """one transpose call on H with the entries' positions as values, against the stable sort"""
    H = U.positions(H, dtype)
    T = sa.transpose(sa.dCSR.from_host(H), cfg)
    assert (T.rows, T.cols, T.nnz) == (H.cols, H.rows, H.nnz)
    got = T.to_host()
    t_ro, t_ci, t_da = U.transpose_expect(H)
    assert U.same_bytes(got.row_offsets, t_ro)
    assert U.same_bytes(got.col_ids, t_ci)
    assert U.same_bytes(got.data, t_da)


# ================================================================================================================= transpose
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("nnz", U.ENTRY_COUNTS_SMALL)
def test_transpose_entry_counts(cfg, nnz, dtype):
    check_transpose(cfg, U.entry_count_case(nnz), dtype)


@pytest.mark.parametrize("nnz", U.ENTRY_COUNTS_LARGE)
def test_transpose_entry_counts_at_the_slice_switch(cfg, nnz):
    """one tile per workgroup / two tiles and an idle half of the grid (float64 only: positions beyond 2^24 stay distinct)"""
    check_transpose(cfg, U.entry_count_case(nnz))


@pytest.mark.parametrize("nnz", U.ENTRY_COUNTS_SMALL + U.ENTRY_COUNTS_LARGE)
def test_transpose_of_the_transpose_is_the_matrix(cfg, nnz):
    """the expected transpose as the input (300 rows, hub rows of thousands of entries at size): one call gives A back"""
    A = U.entry_count_case(nnz)
    T = U.positions(U.expected_transpose(A), np.float64)
    got = sa.transpose(sa.dCSR.from_host(T), cfg).to_host()
    # (T's values are T's positions: every entry of A comes back with the place it had in T)
    assert U.same_matrix(got, A.row_offsets, A.col_ids, U.positions_in_transpose(A))


# (one value type at 2^27 columns, 512 MB of offsets: the passes do not see the values)
@pytest.mark.parametrize("cols,dtype", [(c, d) for c in U.COLS_CASES for d in DTYPES if c < 1 << 27 or d == np.float64],
                         ids=lambda v: str(v) if isinstance(v, int) else _ids(v))
def test_transpose_digit_passes(cfg, cols, dtype):
    check_transpose(cfg, U.digit_case(cols), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["one_column", "two_alternating", "ends_of_a_digit", "low_digit_only", "hub_column",
                                  "hub_row"])
def test_transpose_equal_digits(cfg, name, dtype):
    check_transpose(cfg, U.equal_digit_cases()[name], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["one_entry_rows_32767", "one_entry_rows_32768", "one_entry_rows_32769", "one_row_70000",
                                  "empty_rows", "no_rows", "cols_plus_1_524288", "cols_plus_1_524289"])
def test_transpose_rows(cfg, name, dtype):
    check_transpose(cfg, U.row_cases()[name], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("which", ["odd_base", "no_rows", "one_column"])
def test_transpose_of_a_row_view(cfg, which, dtype):
    H, r0, r1, c0, c1 = U.view_base()
    a, b = {"odd_base": (r0, r1), "no_rows": (r0, r0), "one_column": (c0, c1)}[which]
    H = U.positions(H, dtype)
    dH = sa.dCSR.from_host(H)
    assert H.row_offsets[a] > 0
    S = U.view_slice(H, a, b)                                     # (its values: the positions in H, base included)
    T = sa.transpose(dH.row_view(a, b), cfg)
    assert (T.rows, T.cols, T.nnz) == (S.cols, S.rows, S.nnz)
    t_ro, t_ci, t_da = U.transpose_expect(S)
    assert U.same_matrix(T.to_host(), t_ro, t_ci, t_da)
    assert U.same_matrix(dH.to_host(), H.row_offsets, H.col_ids, H.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_transpose_moves_any_bit_pattern(cfg, dtype):
    A = U.entry_count_case(U.TILE + 1)
    H = U.with_values(A, U.any_bits(A.nnz, dtype))
    got = sa.transpose(sa.dCSR.from_host(H), cfg).to_host()
    t_ro, t_ci, t_da = U.transpose_expect(H)
    assert U.same_matrix(got, t_ro, t_ci, t_da)


# =================================================================================================================== compare
def mismatches(cfg, a, b, compare_data, rel_tol=1e-12):
    """*h_mismatches of speck_compare_f64 / _f32"""
    n = C.c_uint64(0xDEAD)
    L = _lib.load()
    fn = L.speck_compare_f32 if a.dtype == np.float32 else L.speck_compare_f64
    assert fn(cfg._h, C.byref(a._c), C.byref(b._c), int(compare_data), float(rel_tol), C.byref(n)) == 0
    return int(n.value)


def ones_like(H):
    return U.with_values(H, np.ones(H.nnz))


@pytest.mark.parametrize("row", range(len(U.COMPARE_ROW_LENGTHS)), ids=[str(n) for n in U.COMPARE_ROW_LENGTHS])
def test_compare_finds_one_entry_at_every_lane_step(cfg, row):
    M = U.compare_rows_matrix()
    dM, dS = sa.dCSR.from_host(M), sa.dCSR.from_host(ones_like(M))
    assert mismatches(cfg, dM, sa.dCSR.from_host(M), 1) == 0
    assert sa.compare_bounded(dM, sa.dCSR.from_host(M), dS, cfg) == (0, 0)
    for pos in U.plant_positions(U.COMPARE_ROW_LENGTHS[row]):
        dX = sa.dCSR.from_host(U.planted(M, [(row, pos)], "col"))
        dY = sa.dCSR.from_host(U.planted(M, [(row, pos)], "val"))
        for a, b in ((dM, dX), (dX, dM)):
            assert mismatches(cfg, a, b, 1) == 1, pos
            assert mismatches(cfg, a, b, 0) == 1, pos
            assert sa.compare_bounded(a, b, dS, cfg) == (1, 0), pos
        for a, b in ((dM, dY), (dY, dM)):
            assert mismatches(cfg, a, b, 1) == 1, pos
            assert mismatches(cfg, a, b, 0) == 0, pos            # values are not looked at
            assert sa.compare_bounded(a, b, dS, cfg) == (0, 1), pos
            assert not sa.compare(a, b, cfg, compare_data=True) and sa.compare(a, b, cfg)


def test_compare_float32_finds_one_entry_at_every_lane_step(cfg):
    M = U.compare_rows_matrix(np.float32)
    dM = sa.dCSR.from_host(M)
    assert mismatches(cfg, dM, sa.dCSR.from_host(M), 1) == 0
    for row, n in enumerate(U.COMPARE_ROW_LENGTHS):
        pos = U.plant_positions(n)[-1]
        assert mismatches(cfg, dM, sa.dCSR.from_host(U.planted(M, [(row, pos)], "col")), 1) == 1, n
        dY = sa.dCSR.from_host(U.planted(M, [(row, pos)], "val"))
        assert mismatches(cfg, dM, dY, 1) == 1 and mismatches(cfg, dM, dY, 0) == 0, n


@pytest.mark.parametrize("rows", U.COMPARE_ROW_COUNTS)
def test_compare_counts_rows_in_every_trip_of_the_row_loop(cfg, rows):
    M = U.two_entry_rows(rows)
    dM, dS = sa.dCSR.from_host(M), sa.dCSR.from_host(ones_like(M))
    assert mismatches(cfg, dM, sa.dCSR.from_host(M), 1) == 0
    singles = [rows - 1] + ([sa.COMPARE_MAX_WAVES] if rows > sa.COMPARE_MAX_WAVES + 1 else [])
    for r in singles:
        dX = sa.dCSR.from_host(U.planted(M, [(r, 1)], "col"))
        dY = sa.dCSR.from_host(U.planted(M, [(r, 0)], "val"))
        assert mismatches(cfg, dM, dX, 0) == 1 and sa.compare_bounded(dM, dX, dS, cfg) == (1, 0), r
        assert mismatches(cfg, dM, dY, 1) == 1 and sa.compare_bounded(dM, dY, dS, cfg) == (0, 1), r
    five = U.planted_rows(rows)
    X = U.planted(U.planted(M, [(r, 0) for r in five[0::2]], "col"), [(r, 1) for r in five[1::2]], "val")
    dX = sa.dCSR.from_host(X)
    assert mismatches(cfg, dM, dX, 1) == 5 and mismatches(cfg, dX, dM, 1) == 5
    assert mismatches(cfg, dM, dX, 0) == 3
    assert sa.compare_bounded(dM, dX, dS, cfg) == (3, 2)


def test_compare_counts_the_rows_between_two_moved_offsets(cfg):
    A, B, differ = U.shifted_pair()
    dA, dB = sa.dCSR.from_host(A), sa.dCSR.from_host(B)
    for data in (0, 1):
        assert mismatches(cfg, dA, dB, data) == differ and mismatches(cfg, dB, dA, data) == differ
    assert sa.compare_bounded(dA, dB, sa.dCSR.from_host(ones_like(A)), cfg) == (differ, 0)


def test_compare_scale_with_one_entry_moved_is_a_structure_mismatch(cfg):
    """the scale matrix has the rows and nnz of the reference; the entry it moves makes two rows of another length"""
    A, B, _ = U.shifted_pair(longer=37, shorter=38)
    dA = sa.dCSR.from_host(A)
    moved = int(np.count_nonzero(np.diff(A.row_offsets.astype(np.int64)) != np.diff(B.row_offsets.astype(np.int64))))
    assert moved == 2
    assert sa.compare_bounded(dA, sa.dCSR.from_host(A), sa.dCSR.from_host(ones_like(B)), cfg) == (moved, 0)
    assert sa.compare_bounded(dA, sa.dCSR.from_host(A), sa.dCSR.from_host(ones_like(A)), cfg) == (0, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_compare_of_row_views(cfg, dtype):
    rows, r0, r1 = 400, 101, 301
    lens = np.full(rows, 3)
    ci = ((np.arange(rows)[:, None] * 7 + np.arange(3)[None, :] * 1000) % 4096).ravel()      # no two rows alike
    H = U.positions(U.host(rows, 4096, lens, ci), dtype)
    dH = sa.dCSR.from_host(H)
    view, own = dH.row_view(r0, r1), dH.row_view(r0, r1).copy()
    S = sa.dCSR.from_host(ones_like(U.view_slice(H, r0, r1)))
    for a, b in ((view, own), (own, view), (view, view)):
        assert mismatches(cfg, a, b, 1) == 0
        if dtype == np.float64:
            assert sa.compare_bounded(a, b, S, cfg) == (0, 0)
    near = dH.row_view(r0 + 1, r1 + 1).copy()                   # the same shape, nnz and relative offsets
    for a, b in ((view, near), (near, view)):
        # (columns and values differ in every row: a row is counted once, as a row of another pattern)
        assert mismatches(cfg, a, b, 1) == r1 - r0 and mismatches(cfg, a, b, 0) == r1 - r0
        if dtype == np.float64:
            assert sa.compare_bounded(a, b, S, cfg) == (r1 - r0, 0)
    # the neighbouring range of one column pattern: the values alone differ, in every row
    same_cols = U.with_values(U.host(rows, 4096, lens, np.tile([5, 6, 7], rows)), H.data)
    dG = sa.dCSR.from_host(same_cols)
    a, b = dG.row_view(r0, r1), dG.row_view(r0 + 1, r1 + 1).copy()
    assert mismatches(cfg, a, b, 0) == 0 and mismatches(cfg, b, a, 0) == 0
    assert mismatches(cfg, a, b, 1) == r1 - r0 and mismatches(cfg, b, a, 1) == r1 - r0


def _pair(x, y, scale=1.0, dtype=np.float64):
    """three one-entry 1 x 1 matrices: x, y and the scale"""
    one = lambda v: sa.dCSR.from_host(sa.HostCSR(1, 1, np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32),  # noqa: E731
                                                 np.array([v], dtype=dtype)))
    return one(x), one(y), one(scale)


def test_compare_bound_in_exact_arithmetic(cfg):
    x, y = 1.0, 1.0 + 2.0 ** -40
    for a, b in ((x, y), (y, x)):
        dX, dY, dS = _pair(a, b)
        assert sa.compare_bounded(dX, dY, dS, cfg, tol=2.0 ** -40) == (0, 0)       # |x - y| = tol * scale: within
        assert sa.compare_bounded(dX, dY, dS, cfg, tol=2.0 ** -41) == (0, 1)
        dX, dY, dS = _pair(a, b, scale=2.0 ** -3)
        assert sa.compare_bounded(dX, dY, dS, cfg, tol=2.0 ** -37) == (0, 0)
        assert sa.compare_bounded(dX, dY, dS, cfg, tol=2.0 ** -38) == (0, 1)
        # relative to max(|x|, |y|): a factor 2 on either side of the difference
        assert mismatches(cfg, dX, dY, 1, 2.0 ** -39) == 0 and mismatches(cfg, dX, dY, 1, 2.0 ** -41) == 1
        assert mismatches(cfg, dX, dY, 0, 2.0 ** -41) == 0


def test_compare_float32_one_ulp(cfg):
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    for a, b in ((one, up), (up, one)):
        dX, dY, _ = _pair(a, b, dtype=np.float32)
        assert mismatches(cfg, dX, dY, 1, 2.0 ** -23) == 0
        assert mismatches(cfg, dX, dY, 1, 2.0 ** -25) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_compare_early_outs(cfg, dtype):
    lens = np.array([2, 0, 3, 1])
    H = U.positions(U.host(4, 9, lens, np.array([0, 4, 1, 2, 8, 3])), dtype)
    dH = sa.dCSR.from_host(H)
    other_cols = sa.HostCSR(4, 10, H.row_offsets, H.col_ids, H.data)
    other_rows = U.positions(U.host(5, 9, np.append(lens, 0), H.col_ids), dtype)
    other_nnz = U.positions(U.host(4, 9, lens + [0, 0, 0, 1], np.append(H.col_ids, 5)), dtype)
    for X in (other_cols, other_rows, other_nnz):
        dX = sa.dCSR.from_host(X)
        for data in (0, 1):
            assert mismatches(cfg, dH, dX, data) > 0 and mismatches(cfg, dX, dH, data) > 0
        assert not sa.compare(dH, dX, cfg)
    none = U.positions(U.host(0, 9, np.zeros(0, dtype=np.int64), np.zeros(0)), dtype)
    assert mismatches(cfg, sa.dCSR.from_host(none), sa.dCSR.from_host(none), 1) == 0
    empty = U.positions(U.host(70, 9, np.zeros(70, dtype=np.int64), np.zeros(0)), dtype)
    assert mismatches(cfg, sa.dCSR.from_host(empty), sa.dCSR.from_host(empty), 1) == 0
    assert sa.compare(sa.dCSR.from_host(empty), sa.dCSR.from_host(empty), cfg, compare_data=True)


# =============================================================================================================== device copy
def check_copy(src, expect, padding=0):
    """copy() of `src` holds `expect` byte for byte, with the rows and nnz of the source"""
    d = src.copy(padding) if padding else src.copy()
    assert (d.rows, d.cols, d.nnz) == (expect.rows, expect.cols, expect.nnz) == (src.rows, src.cols, src.nnz)
    assert d._c.row_offsets != src._c.row_offsets and d._c.col_ids != src._c.col_ids and d._c.data != src._c.data
    got = d.to_host()
    assert got.data.dtype == expect.data.dtype
    assert U.same_matrix(got, expect.row_offsets, expect.col_ids, expect.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_copy_of_a_matrix_and_of_a_view_with_an_odd_base(dtype):
    H0, r0, r1, _, _ = U.view_base()
    H = U.with_values(H0, U.any_bits(H0.nnz, dtype, seed=9))
    dH = sa.dCSR.from_host(H)
    check_copy(dH, H)
    check_copy(dH, H, padding=3)
    view = dH.row_view(r0, r1)
    assert H.row_offsets[r0] % 2 == 1
    for a, b in ((r0, r1), (r0, r0), (H.rows - 1, H.rows), (0, r0)):
        check_copy(dH.row_view(a, b), U.view_slice(H, a, b))
        check_copy(dH.row_view(a, b), U.view_slice(H, a, b), padding=3)
    assert (view.rows, view.nnz) == (r1 - r0, int(H.row_offsets[r1]) - int(H.row_offsets[r0]))
    assert U.same_matrix(dH.to_host(), H.row_offsets, H.col_ids, H.data)       # the source is what it was


@pytest.mark.parametrize("dtype,nnz", [(np.float32, sa.COPY_MAX_THREADS - 1), (np.float32, sa.COPY_MAX_THREADS),
                                       (np.float32, sa.COPY_MAX_THREADS + 1), (np.float64, sa.COPY_MAX_THREADS // 2 - 1),
                                       (np.float64, sa.COPY_MAX_THREADS // 2), (np.float64, sa.COPY_MAX_THREADS // 2 + 1)])
def test_copy_at_the_thread_count_in_value_words(dtype, nnz):
    """nnz x (value size / 4) words of values around the 2 097 152 threads of the launch: one trip / a second one"""
    H = U.copy_entries_case(nnz, dtype)
    dH = sa.dCSR.from_host(H)
    check_copy(dH, H)
    check_copy(dH.row_view(1, H.rows), U.view_slice(H, 1, H.rows))
    assert U.same_matrix(dH.to_host(), H.row_offsets, H.col_ids, H.data)


@pytest.mark.parametrize("rows", [sa.COPY_MAX_THREADS - 2, sa.COPY_MAX_THREADS - 1, sa.COPY_MAX_THREADS])
def test_copy_at_the_thread_count_in_offsets(rows):
    H = U.copy_rows_case(rows)
    dH = sa.dCSR.from_host(H)
    check_copy(dH, H)
    check_copy(dH, H, padding=3)
    half = rows // 2 + 1
    check_copy(dH.row_view(half, rows), U.view_slice(H, half, rows))
    assert U.same_matrix(dH.to_host(), H.row_offsets, H.col_ids, H.data)


# ======================================================================================================= download of a view
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_download_of_a_row_view_is_the_download_of_its_copy(dtype):
    H0, r0, r1, _, _ = U.view_base()
    H = U.with_values(H0, U.any_bits(H0.nnz, dtype, seed=10))
    dH = sa.dCSR.from_host(H)
    for a, b in ((0, r0), (r0, r1), (H.rows - 1, H.rows), (r0, r0), (0, 0), (H.rows, H.rows), (0, H.rows)):
        view = dH.row_view(a, b)
        got, S, through_copy = view.to_host(), U.view_slice(H, a, b), view.copy().to_host()
        assert (got.rows, got.cols, got.nnz) == (S.rows, S.cols, S.nnz), (a, b)
        assert U.same_matrix(got, S.row_offsets, S.col_ids, S.data), (a, b)
        assert U.same_matrix(got, through_copy.row_offsets, through_copy.col_ids, through_copy.data), (a, b)
    assert H.row_offsets[H.rows - 1] > 0 and H.row_offsets[r0] > 0
    # the C call with some of the host arrays absent: the entries still start at the view's first offset
    view, S = dH.row_view(r0, r1), U.view_slice(H, r0, r1)
    ci, da = np.zeros(S.nnz, dtype=np.uint32), np.zeros(S.nnz, dtype=dtype)
    L = _lib.load()
    assert L.speck_dcsr_download(C.byref(view._c), None, ci.ctypes.data, None, da.itemsize) == 0
    assert L.speck_dcsr_download(C.byref(view._c), None, None, da.ctypes.data, da.itemsize) == 0
    assert U.same_bytes(ci, S.col_ids) and U.same_bytes(da, S.data)
    assert U.same_matrix(dH.to_host(), H.row_offsets, H.col_ids, H.data)       # an owner: as before
