"""speck_multiply_masked_* on the GPU (speck_amd/csrc/masked.hip).  Every expectation is computed without the library under
test: the full product of the CPU oracle (with its sum|a*b| array) filtered by the mask's pattern in numpy, the products
from the oracle's analysis, the hits as the sum over the mask of pattern(A) @ pattern(B) in scipy (integers in float64:
exact).  Offsets and column ids are compared bit for bit, EVERY value against the project's bound."""
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
GROUP_MAX, LDS_MAX = sa.MASK_GROUP_MAX, sa.MASK_LDS_MAX
ERR_INVALID, ERR_UNSORTED = 1, 8
TOL64 = 1e-12
TOL32 = 4.0 * 2.0 ** -23   # fp32 against the product formed in fp64 (tests/test_gpu_parity.py)
DTYPES = [np.float64, np.float32]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def as_dtype(H, dtype):
    return po.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, H.data.astype(dtype))


def to_dev(H):
    return sa.dCSR.from_host(sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, H.data))


def pattern(H):
    """scipy matrix of ones on the pattern of H (duplicates would add up: there are none in a canonical matrix)"""
    base = int(H.row_offsets[0])
    return sp.csr_matrix((np.ones(H.nnz), H.col_ids[base:base + H.nnz], H.row_offsets.astype(np.int64) - base),
                         shape=(H.rows, H.cols))


def mask_from_rows(rows_cols, cols):
    ro = np.zeros(len(rows_cols) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([len(c) for c in rows_cols])
    ci = np.concatenate(rows_cols).astype(np.uint32) if len(rows_cols) else np.zeros(0, np.uint32)
    return po.HostCSR(len(rows_cols), cols, ro, ci, np.ones(len(ci)))


def keys(H):
    ro = H.row_offsets.astype(np.int64)
    base = int(ro[0])
    return np.repeat(np.arange(H.rows, dtype=np.int64), np.diff(ro)) * H.cols + H.col_ids[base:base + H.nnz].astype(np.int64)


class Expect:
    """what the masked product of A, B on M has to be, from the oracle's full product"""

    def __init__(self, A, B, M):
        R, ab = po.spgemm_f64_of(A, B)                 # fp32 inputs: their product formed in fp64
        kR, kM = keys(R), keys(M)                      # both ascending: rows ascend, columns ascend inside a row
        pos = np.minimum(np.searchsorted(kR, kM), max(len(kR) - 1, 0))
        found = (kR[pos] == kM) if len(kR) else np.zeros(len(kM), dtype=bool)
        m_row = kM // M.cols
        self.rows, self.cols = A.rows, B.cols
        # FULL_PATTERN: M's pattern, the product where there is one, +0.0 elsewhere
        self.full_ro = (M.row_offsets - M.row_offsets[0]).astype(np.uint32)
        self.full_ci = (kM % M.cols).astype(np.uint32)
        self.full_data = np.where(found, R.data[pos] if len(kR) else 0.0, 0.0)
        self.full_ab = np.where(found, ab[pos] if len(kR) else 0.0, 0.0)
        self.found = found
        # STRUCTURE: the entries of the full product that lie in M
        self.ro = np.zeros(A.rows + 1, dtype=np.uint32)
        self.ro[1:] = np.cumsum(np.bincount(m_row[found], minlength=A.rows))
        self.ci = self.full_ci[found]
        self.data = self.full_data[found]
        self.ab = self.full_ab[found]
        # the statistics
        len_a, len_m = np.diff(A.row_offsets.astype(np.int64)), np.diff(M.row_offsets.astype(np.int64))
        self.work = (len_a > 0) & (len_m > 0)
        self.row_ops = po.analysis(A, B)["row_ops"].astype(np.int64)
        self.products = int(self.row_ops[self.work].sum())
        counts = (pattern(A) @ pattern(B)).multiply(pattern(M)).tocsr()
        self.row_hits = np.asarray(counts.sum(axis=1)).ravel().astype(np.int64)
        self.hits = int(self.row_hits.sum())
        self.rows_idle = int((~self.work).sum())
        self.len_m = len_m

    def classes(self, group_max=GROUP_MAX, lds_max=LDS_MAX):
        """rows with work per class: group / LDS / global"""
        n = self.len_m[self.work]
        g = int((n <= group_max).sum())
        l = int(((n > group_max) & (n <= lds_max)).sum())
        return (g, l, len(n) - g - l)


def close(got, ref, ab, dtype):
    tol = TOL32 if dtype == np.float32 else TOL64
    g, r = got.astype(np.float64), ref.astype(np.float64)
    special = ~np.isfinite(r)
    with np.errstate(invalid="ignore"):
        ok = np.where(special, (np.isnan(g) & np.isnan(r)) | (g == r),
                      np.abs(g - r) <= tol * np.where(special, 0.0, ab) + 1e-300)
    return bool(ok.all())


def check(cfg, A, B, M, dtype, full, X=None, dC=None, views=None):
    """run one call and hold the result and the statistics against X (an Expect of the same inputs)"""
    A, B = as_dtype(A, dtype), as_dtype(B, dtype)
    X = X or Expect(A, B, M)
    dA, dB, dM = views or (to_dev(A), to_dev(B), to_dev(M))
    dC, info = sa.multiply_masked(dA, dB, dM, cfg, matOut=dC, full_pattern=full)
    got = dC.to_host()
    assert dC.dtype == np.dtype(dtype) and got.data.dtype == np.dtype(dtype)
    assert (got.rows, got.cols) == (X.rows, X.cols)
    ro, ci, data, ab = (X.full_ro, X.full_ci, X.full_data, X.full_ab) if full else (X.ro, X.ci, X.data, X.ab)
    assert got.nnz == len(ci) == info.nnz_out
    assert got.row_offsets.tobytes() == ro.tobytes(), "row_offsets differ"
    assert got.col_ids.tobytes() == ci.tobytes(), "col_ids differ"
    assert close(got.data, data, ab, dtype), "values beyond the bound"
    assert info.rows_idle == X.rows_idle and info.products == X.products and info.hits == X.hits
    assert sum(info.rows_class) == X.rows - X.rows_idle
    return dC, info, got


def random_mask(rows, cols, per_row, seed, empty_row_frac=0.0):
    return random_csr(rows, cols, per_row, seed, signed=False, empty_row_frac=empty_row_frac)


# ---------------------------------------------------------------------------------------------------- 1: every class, at its edges
def edge_case(seed=3, cols=20_000, inner=300):
    """mask rows of 0, 1, 2, 4 L and 4 L + 1 entries for every group width, the limits of the three classes and the limit
    + 1 (1024 / 1025: where the LDS class changes its workgroup size), one row well beyond, in shuffled row order; A and B
    dense enough (a row of A B holds about a quarter of the columns) that every class sees hits and misses"""
    rng = np.random.default_rng(seed)
    short = [0, 1, 2] + [4 * L + d for L in (8, 16, 32, 64) for d in (0, 1)] + [GROUP_MAX, GROUP_MAX + 1, 1024, 1025]
    lengths = short * 3 + [LDS_MAX, LDS_MAX + 1, LDS_MAX, LDS_MAX + 1, 3 * LDS_MAX]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    M = mask_from_rows([np.sort(rng.choice(cols, size=n, replace=False)) for n in lengths], cols)
    A = random_csr(len(lengths), inner, 12, seed + 1, empty_row_frac=0.08)
    B = random_csr(inner, cols, 500, seed + 2)
    return A, B, M


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_every_class_at_its_edges(cfg, dtype, full):
    A, B, M = edge_case()
    X = Expect(as_dtype(A, dtype), as_dtype(B, dtype), M)
    # the input is not degenerate: in every class some products hit and some miss, some mask entries are produced and
    # some are not; some rows have a mask row but no row of A
    cls = np.where(X.len_m <= GROUP_MAX, 0, np.where(X.len_m <= LDS_MAX, 1, 2))
    produced = np.add.reduceat(np.concatenate([X.found, [False]]).astype(np.int64),
                               np.minimum(M.row_offsets[:-1], M.nnz).astype(np.int64))
    produced[X.len_m == 0] = 0
    for k in range(3):
        rows = X.work & (cls == k)
        assert rows.any()
        assert 0 < X.row_hits[rows].sum() < X.row_ops[rows].sum()
        assert 0 < produced[rows].sum() < X.len_m[rows].sum()
    assert ((X.len_m > 0) & ~X.work).any() and (X.len_m == 0).any()
    _, info, _ = check(cfg, A, B, M, dtype, full, X=X)
    assert all(n > 0 for n in info.rows_class)
    assert info.rows_class == X.classes()


# ---------------------------------------------------------------------------------------------------- 2: one matrix, every class
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_the_same_rows_forced_through_each_class(cfg, dtype, full):
    A, B = random_csr(300, 200, 9, 21, empty_row_frac=0.05), random_csr(200, 900, 40, 22)
    M = random_mask(300, 900, 30, 23, empty_row_frac=0.05)
    X = Expect(as_dtype(A, dtype), as_dtype(B, dtype), M)
    assert 0 < X.hits < X.products and 0 < X.found.sum() < M.nnz
    results = []
    for group_max, lds_max in ((0, 0), (0, LDS_MAX), (GROUP_MAX, LDS_MAX)):
        cfg.set_option("mask_group_max", group_max)
        cfg.set_option("mask_lds_max", lds_max)
        _, info, got = check(cfg, A, B, M, dtype, full, X=X)
        assert info.rows_class == X.classes(group_max, lds_max)
        assert info.rows_class[{(0, 0): 2, (0, LDS_MAX): 1}.get((group_max, lds_max), 0)] == X.rows - X.rows_idle
        results.append(got)
    for other in results[1:]:
        assert other.row_offsets.tobytes() == results[0].row_offsets.tobytes()
        assert other.col_ids.tobytes() == results[0].col_ids.tobytes()


def test_class_limits_are_clamped_to_what_the_kernels_support(cfg):
    A, B, M = edge_case(seed=5)
    cfg.set_option("mask_group_max", 10 * GROUP_MAX)
    cfg.set_option("mask_lds_max", 10 * LDS_MAX)
    _, info, _ = check(cfg, A, B, M, np.float64, False)
    assert info.rows_class[2] > 0 and info.rows_class[1] > 0


# ---------------------------------------------------------------------------------------------------- 3: masks that bracket the semantics
@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_equal_to_the_pattern_of_the_product_gives_the_product(cfg, dtype):
    A, B = as_dtype(random_csr(500, 400, 7, 31), dtype), as_dtype(random_csr(400, 600, 9, 32), dtype)
    R, ab = po.spgemm_f64_of(A, B)
    M = po.HostCSR(R.rows, R.cols, R.row_offsets, R.col_ids, np.ones(R.nnz))
    for full in (False, True):
        dC, info, got = check(cfg, A, B, M, dtype, full)
        assert got.nnz == R.nnz and info.hits == info.products
        assert got.row_offsets.tobytes() == R.row_offsets.tobytes() and got.col_ids.tobytes() == R.col_ids.tobytes()
    if dtype == np.float64:   # ... and against the library's own full product, through its own bounded comparison
        dFull = sa.dCSR()
        sa.MultiplyspECK(to_dev(A), to_dev(B), dFull, cfg)
        dAbs = to_dev(po.HostCSR(R.rows, R.cols, R.row_offsets, R.col_ids, ab))
        assert sa.compare_bounded(dFull, dC, dAbs, cfg, tol=2 * TOL64) == (0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_mask(cfg, dtype):
    A, B = random_csr(100, 80, 5, 41), random_csr(80, 120, 6, 42)
    M = mask_from_rows([np.zeros(0, np.uint32)] * 100, 120)
    for full in (False, True):
        _, info, got = check(cfg, A, B, M, dtype, full)
        assert info.nnz_out == 0 and got.nnz == 0 and (got.row_offsets == 0).all() and info.rows_idle == 100
        assert info.products == 0 and info.hits == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_disjoint_from_the_product(cfg, dtype):
    A, B = random_csr(200, 150, 6, 51), random_csr(150, 400, 8, 52)
    R, _ = po.spgemm(A, B)
    rng = np.random.default_rng(53)
    rows_cols = []
    for r in range(R.rows):
        free = np.setdiff1d(np.arange(400), R.col_ids[int(R.row_offsets[r]):int(R.row_offsets[r + 1])])
        rows_cols.append(np.sort(rng.choice(free, size=min(len(free), int(rng.integers(0, 300))), replace=False)))
    M = mask_from_rows(rows_cols, 400)
    assert M.nnz > 0 and max(len(c) for c in rows_cols) > GROUP_MAX
    _, info, got = check(cfg, A, B, M, dtype, False)
    assert info.nnz_out == 0 and info.hits == 0 and info.products > 0 and (got.row_offsets == 0).all()
    _, info, got = check(cfg, A, B, M, dtype, True)
    assert info.nnz_out == M.nnz and (got.data == 0).all() and not np.signbit(got.data).any()   # +0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [300, LDS_MAX + 500])
def test_mask_with_dense_rows(cfg, dtype, cols):
    """rows of M that hold every column of B (LDS class / global-memory class), among ordinary ones"""
    A, B = random_csr(60, 90, 8, 61), random_csr(90, cols, cols // 12, 62)
    rng = np.random.default_rng(63)
    rows_cols = [np.arange(cols) if r % 7 == 0 else np.sort(rng.choice(cols, size=int(rng.integers(0, 40)), replace=False))
                 for r in range(60)]
    M = mask_from_rows(rows_cols, cols)
    for full in (False, True):
        _, info, _ = check(cfg, A, B, M, dtype, full)
        assert info.rows_class[1 if cols <= LDS_MAX else 2] > 0 and 0 < info.hits < info.products


@pytest.mark.parametrize("dtype", DTYPES)
def test_cancelling_products_stay_as_an_explicit_zero(cfg, dtype):
    # C(0,2) = 3*5 + (-3)*5 = 0.0: structural, the entry stays; C(1,2) = 2*5
    A = po.HostCSR(2, 3, [0, 2, 3], [0, 1, 0], np.array([3.0, -3.0, 2.0]))
    B = po.HostCSR(3, 4, [0, 2, 3, 4], [1, 2, 2, 0], np.array([7.0, 5.0, 5.0, 1.0]))
    M = mask_from_rows([np.array([0, 2, 3]), np.array([2])], 4)
    _, info, got = check(cfg, A, B, M, dtype, False)
    assert got.nnz == 2 and list(got.col_ids) == [2, 2] and list(got.data) == [0.0, 10.0]
    assert (info.products, info.hits) == (5, 3)
    _, _, got = check(cfg, A, B, M, dtype, True)
    assert list(got.data) == [0.0, 0.0, 0.0, 10.0] and not np.signbit(got.data).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_reach_exactly_the_entries_they_should(cfg, dtype):
    A, B = random_csr(150, 100, 6, 71, signed=False), random_csr(100, 200, 10, 72, signed=False)
    data = B.data.copy()
    i_nan, i_inf = int(B.row_offsets[17]), int(B.row_offsets[58]) + 1      # one entry of row 17, one of row 58
    assert B.row_offsets[18] > i_nan and B.row_offsets[59] > i_inf
    data[i_nan], data[i_inf] = np.nan, np.inf
    B = po.HostCSR(B.rows, B.cols, B.row_offsets, B.col_ids, data)
    R, _ = po.spgemm(A, B)
    assert np.isnan(R.data).any() and np.isinf(R.data).any()
    keep = np.random.default_rng(73).random(R.nnz) < 0.7                    # most of the product's pattern ...
    extra = random_mask(150, 200, 8, 74)                                    # ... and entries beside it
    M = po.HostCSR.from_scipy(sp.csr_matrix((keep.astype(np.float64), R.col_ids, R.row_offsets.astype(np.int64)),
                                            shape=(150, 200)) + pattern(extra))
    M = po.HostCSR(M.rows, M.cols, M.row_offsets, M.col_ids, np.ones(M.nnz))
    X = Expect(as_dtype(A, dtype), as_dtype(B, dtype), M)
    assert np.isnan(X.data).any() and np.isinf(X.data).any() and np.isfinite(X.data).sum() > X.data.size // 2
    for full in (False, True):
        _, _, got = check(cfg, A, B, M, dtype, full, X=X)
        ref = X.full_data if full else X.data
        assert (np.isnan(got.data) == np.isnan(ref)).all() and (np.isinf(got.data) == np.isinf(ref)).all()


# ---------------------------------------------------------------------------------------------------- 4: stand-ins
STANDINS = [("scircuit", 0.08, 76_124, 76_124, 8_614, 6_667), ("mac_econ", 0.08, 99_467, 26_030, 41_320, 20_663),
            ("cant", 0.1, 385_985, 385_985, 2_097_101, 187_765), ("webbase", 0.04, 114_157, 41_934, 111_586, 25_822)]


def standin(kind, scale):
    h = sa.gen_matrix(kind, scale, 7, signed=True)
    return po.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,scale,nnz_m,nnz_c,triangles,nnz_t", STANDINS)
def test_standin_squared_on_its_own_pattern(cfg, dtype, kind, scale, nnz_m, nnz_c, triangles, nnz_t):
    S = standin(kind, scale)
    assert S.nnz == nnz_m
    for full in (False, True):
        _, info, _ = check(cfg, S, S, S, dtype, full)
        assert info.nnz_out == (nnz_m if full else nnz_c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,scale,nnz_m,nnz_c,triangles,nnz_t", STANDINS)
def test_standin_triangles(cfg, dtype, kind, scale, nnz_m, nnz_c, triangles, nnz_t):
    """A = B = M = L, the strictly lower triangle of pattern(S + S^T) with unit values: sum(C) = hits = the triangles"""
    P = pattern(standin(kind, scale))
    Ls = sp.tril(((P + P.T) > 0).astype(np.float64), k=-1).tocsr()
    assert int(((Ls @ Ls).multiply(Ls)).sum()) == triangles                 # scipy's count
    L = po.HostCSR.from_scipy(Ls)
    _, info, got = check(cfg, L, L, L, dtype, False)
    assert info.nnz_out == nnz_t < L.nnz
    assert info.hits == triangles and float(got.data.astype(np.float64).sum()) == float(triangles)
    _, info, got = check(cfg, L, L, L, dtype, True)
    assert info.nnz_out == L.nnz and float(got.data.astype(np.float64).sum()) == float(triangles)


# ---------------------------------------------------------------------------------------------------- 5: views
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_row_range_views_of_a_and_m(cfg, dtype, full):
    A, B, M = edge_case(seed=9)
    A, B = as_dtype(A, dtype), as_dtype(B, dtype)
    X = Expect(A, B, M)
    dA, dB, dM = to_dev(A), to_dev(B), to_dev(M)
    rows = A.rows
    for bounds in ([0, rows // 2, rows], [0, 5, 6, rows - 3, rows], [0, rows // 3, 2 * rows // 3, rows]):
        ro, ci, da = [np.zeros(1, np.uint32)], [], []
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            dC, info = sa.multiply_masked(dA.row_view(r0, r1), dB, dM.row_view(r0, r1), cfg, full_pattern=full)
            got = dC.to_host()
            assert got.rows == r1 - r0 and got.row_offsets[0] == 0 and info.nnz_out == got.nnz
            ro.append(got.row_offsets[1:] + ro[-1][-1])
            ci.append(got.col_ids)
            da.append(got.data)
        ro, ci, da = np.concatenate(ro).astype(np.uint32), np.concatenate(ci), np.concatenate(da)
        want = (X.full_ro, X.full_ci, X.full_data, X.full_ab) if full else (X.ro, X.ci, X.data, X.ab)
        assert ro.tobytes() == want[0].tobytes() and ci.tobytes() == want[1].tobytes()
        assert close(da, want[2], want[3], dtype)


# ---------------------------------------------------------------------------------------------------- 6: refusals write nothing
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
        A, B, M = edge_case(seed=13)
        A, B = as_dtype(A, dtype), as_dtype(B, dtype)
        rows = A.rows
        r = next(i for i in range(rows // 2, rows) if M.row_offsets[i + 1] - M.row_offsets[i] >= 8)
        m0 = int(M.row_offsets[r])
        equal, descending, beyond = M.col_ids.copy(), M.col_ids.copy(), M.col_ids.copy()
        equal[m0 + 3] = equal[m0 + 2]
        descending[m0 + 2], descending[m0 + 3] = M.col_ids[m0 + 3], M.col_ids[m0 + 2]
        last = int(M.row_offsets[r + 1]) - 1
        beyond[last] = B.cols                                   # (still ascending: only the range is wrong)
        m_ro_desc = M.row_offsets.copy()
        m_ro_desc[r], m_ro_desc[r + 1] = M.row_offsets[r + 1], M.row_offsets[r]
        m_ro_far = M.row_offsets.copy()
        m_ro_far[r + 1:] = 0xFFFFFF00
        ra = next(i for i in range(rows) if A.row_offsets[i + 1] > A.row_offsets[i])
        a_bad = A.col_ids.copy()
        a_bad[int(A.row_offsets[ra + 1]) - 1] = B.rows
        a_far = A.col_ids.copy()
        a_far[int(A.row_offsets[ra])] = 0xFFFFFFF0
        b_unsorted = B.col_ids.copy()
        b0 = int(B.row_offsets[B.rows // 2])
        b_unsorted[b0], b_unsorted[b0 + 1] = B.col_ids[b0 + 1], B.col_ids[b0]
        cases = [("M", None, equal, ERR_UNSORTED), ("M", None, descending, ERR_UNSORTED), ("M", None, beyond, ERR_UNSORTED),
                 ("M", m_ro_desc, None, ERR_INVALID), ("M", m_ro_far, None, ERR_INVALID),
                 ("A", None, a_bad, ERR_INVALID), ("A", None, a_far, ERR_INVALID), ("B", None, b_unsorted, ERR_UNSORTED)]
        X = Expect(A, B, M)
        sentinel_n = len(X.ci)                                  # C allocated at a plausible size, filled with a sentinel
        for which, h_ro, h_ci, status in cases:
            d = {"A": to_dev(A), "B": to_dev(B), "M": to_dev(M)}
            _update(d[which], h_ro, h_ci)
            for full in (False, True):
                dC = sa.dCSR(dtype)
                dC.alloc(rows, B.cols, sentinel_n)
                s_ro = np.full(rows + 1, 0xABABABAB, dtype=np.uint32)
                s_ci = np.full(sentinel_n, 0xCDCDCDCD, dtype=np.uint32)
                s_da = np.full(sentinel_n, -77.25, dtype=dtype)
                assert _lib.load().speck_dcsr_update(C_.byref(dC._c), s_ro.ctypes.data, s_ci.ctypes.data, s_da.ctypes.data,
                                                     np.dtype(dtype).itemsize) == 0
                before = bytes(dC._c)
                with pytest.raises(sa.SpeckError) as e:
                    sa.multiply_masked(d["A"], d["B"], d["M"], cfg, matOut=dC, full_pattern=full)
                assert e.value.status == status, (which, status)    # (not 3: no canary zone was touched either)
                assert bytes(dC._c) == before                        # the struct: sizes and the three pointers
                got = dC.to_host()
                assert got.row_offsets.tobytes() == s_ro.tobytes() and got.col_ids.tobytes() == s_ci.tobytes()
                assert got.data.tobytes() == s_da.tobytes()
        # the config serves the valid input afterwards, canary zones intact
        for full in (False, True):
            check(cfg, A, B, M, dtype, full, X=X)
    finally:
        if guard:
            cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


# ---------------------------------------------------------------------------------------------------- 7: output reuse rules
def test_output_buffers_are_reused_as_the_multiply_reuses_them(cfg):
    A, B = random_csr(300, 200, 9, 81), random_csr(200, 500, 20, 82)
    M1, M2 = random_mask(300, 500, 40, 83), random_mask(300, 500, 25, 84)
    dC, info1, _ = check(cfg, A, B, M1, np.float64, False)
    ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets)
    dC, info, _ = check(cfg, A, B, M1, np.float64, False, dC=dC)             # same result size: nothing re-allocated
    assert (dC._c.data, dC._c.col_ids, dC._c.row_offsets) == ptrs and info.nnz_out == info1.nnz_out
    dC, info2, _ = check(cfg, A, B, M2, np.float64, False, dC=dC)            # another mask: data / col_ids only
    assert info2.nnz_out != info1.nnz_out
    assert dC._c.row_offsets == ptrs[2] and dC._c.data != ptrs[0] and dC._c.col_ids != ptrs[1]
    dC, info3, _ = check(cfg, A, B, M2, np.float64, True, dC=dC)             # ... and the other mode, another size again
    assert info3.nnz_out == M2.nnz and dC._c.row_offsets == ptrs[2]
    dC, _, _ = check(cfg, A, B, M2, np.float32, True, dC=dC)                 # a matOut of the other dtype is reset
    assert dC.dtype == np.float32
    dC, _, _ = check(cfg, A, B, M2, np.float64, False, dC=dC)
    assert dC.dtype == np.float64


# ---------------------------------------------------------------------------------------------------- 8: the multiply is not disturbed
def test_a_masked_call_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    S = standin("scircuit", 0.08)
    R, ab = po.spgemm(S, S)
    dS, dC = to_dev(S), sa.dCSR()

    def multiply_matches():
        sa.MultiplyspECK(dS, dS, dC, cfg)
        got = dC.to_host()
        assert got.nnz == R.nnz and got.row_offsets.tobytes() == R.row_offsets.tobytes()
        assert got.col_ids.tobytes() == R.col_ids.tobytes() and (np.abs(got.data - R.data) <= TOL64 * ab + 1e-300).all()

    multiply_matches()
    multiply_matches()
    assert cfg.last_stats()["replayed"]
    X = Expect(S, S, S)
    multiply_matches()
    dM = sa.dCSR()
    for full in (False, True):
        check(cfg, S, S, S, np.float64, full, X=X, dC=dM, views=(dS, dS, dS))
        multiply_matches()
        assert cfg.last_stats()["replayed"]


# ---------------------------------------------------------------------------------------------------- 9: stream, canary zones
@pytest.mark.parametrize("full", [False, True])
def test_runs_on_the_callers_stream(cfg, full):
    """the mask's columns are written by a copy on the caller's stream right before the call: ordering against the
    producer is by the stream alone"""
    A, B, M = edge_case(seed=17)
    X = Expect(A, B, M)
    dev = torch.device("cuda:0")
    t_ro = torch.from_numpy(M.row_offsets.view(np.int32).copy()).to(dev)
    t_ci = torch.zeros(M.nnz, dtype=torch.int32, device=dev)               # not a valid mask until the producer has run
    t_real = torch.from_numpy(M.col_ids.view(np.int32).copy()).to(dev)
    dM = sa.dCSR.from_device(M.rows, M.cols, M.nnz, t_ro.data_ptr(), t_ci.data_ptr(), None, keep=(t_ro, t_ci))
    dA, dB = to_dev(A), to_dev(B)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(200_000_000)          # ~0.1 s: whatever does not wait for the stream sees an invalid mask
            t_ci.copy_(t_real, non_blocking=True)
        _, info, _ = check(cfg, A, B, M, np.float64, full, X=X, views=(dA, dB, dM))
        assert all(n > 0 for n in info.rows_class)
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        A, B, M = edge_case(seed=19)
        for full in (False, True):
            _, info, _ = check(cfg, A, B, M, dtype, full)
            assert all(n > 0 for n in info.rows_class)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()

# ---------------------------------------------------------------------------------------------------- 10: the scans at their edges
def scan_case(rows, last_row_cols=7):
    """A: one entry per row, column r mod 16, value r mod 7 + 1.  B: 16 x 8, row k holds columns k mod 8 and (k + 3) mod 8
    (ascending) with the values 2 k + 1 and 2 k + 2.  M: columns 0 .. 3 in every row, 0 .. last_row_cols - 1 in the last
    one.  C = the mask entries that meet the B row of their row's entry of A, a * b: exact in either precision.  Built and
    expected without a Python loop over the rows."""
    r = np.arange(rows)
    A = po.HostCSR(rows, 16, np.arange(rows + 1, dtype=np.uint32), (r % 16).astype(np.uint32), (r % 7 + 1).astype(np.float64))
    k = np.arange(16)
    b_ci = np.sort(np.stack([k % 8, (k + 3) % 8], axis=1), axis=1)
    b_va = np.stack([2 * k + 1, 2 * k + 2], axis=1).astype(np.float64)
    B = po.HostCSR(16, 8, (2 * np.arange(17)).astype(np.uint32), b_ci.ravel().astype(np.uint32), b_va.ravel())
    dense_b = np.zeros((16, 8))
    dense_b[k[:, None], b_ci] = b_va
    m_len = np.full(rows, 4)
    m_len[-1] = last_row_cols
    m_ro = np.zeros(rows + 1, dtype=np.uint32)
    m_ro[1:] = np.cumsum(m_len)
    m_row = np.repeat(r, m_len)
    m_ci = (np.arange(int(m_ro[-1])) - m_ro[:-1].astype(np.int64)[m_row]).astype(np.uint32)
    M = po.HostCSR(rows, 8, m_ro, m_ci, np.ones(len(m_ci)))
    b_at = dense_b[m_row % 16, m_ci]
    hit = b_at != 0
    e_ro = np.zeros(rows + 1, dtype=np.uint32)
    e_ro[1:] = np.cumsum(np.bincount(m_row[hit], minlength=rows))
    return A, B, M, (e_ro, m_ci[hit], (A.data[m_row] * b_at)[hit])


def check_scan_case(cfg, dtype, rows, last_row_cols=7):
    A, B, M, (e_ro, e_ci, e_va) = scan_case(rows, last_row_cols)
    dC, info = sa.multiply_masked(to_dev(as_dtype(A, dtype)), to_dev(as_dtype(B, dtype)), to_dev(M), cfg)
    got = dC.to_host()
    assert (got.rows, got.cols, got.nnz) == (rows, 8, len(e_ci))
    assert info.nnz_out == len(e_ci) and info.hits == len(e_ci) and info.products == 2 * rows
    assert got.row_offsets.tobytes() == e_ro.tobytes(), "row_offsets differ"
    assert got.col_ids.tobytes() == e_ci.tobytes(), "col_ids differ"
    assert got.data.dtype == np.dtype(dtype) and got.data.tobytes() == e_va.astype(dtype).tobytes(), "values differ"


SCAN_ROWS = [1023, 1024, 1025, 2049, 1024 * 1024 + 1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", SCAN_ROWS)
def test_structure_scans_across_workgroup_boundaries(cfg, dtype, rows):
    """Both scans of the STRUCTURE finish at their boundaries: 1024 rows per workgroup of the row scan (one short, exact,
    one more, two and a row, more than 1024 workgroups: the second trip over the workgroup sums) and, with nnz(M) =
    4 rows + 3, the same for the 4096-entry tiles of the compaction -- 4 194 311 entries at the largest: past 1024 tiles and
    no multiple of four, so the last word of hit bytes is masked."""
    check_scan_case(cfg, dtype, rows)


@pytest.mark.parametrize("nnz_m", [4095, 4096, 4097])
def test_structure_compaction_at_the_first_tile_boundary(cfg, nnz_m):
    check_scan_case(cfg, np.float64, 1024, last_row_cols=4 + nnz_m - 4096)


def test_structure_scans_with_canary_zones():
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        check_scan_case(cfg, np.float64, 1025)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()
