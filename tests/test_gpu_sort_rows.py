"""speck_sort_rows_* on the GPU (speck_amd/csrc/sort_rows.hip): every expectation is computed here with numpy -- per row
np.argsort(cols, kind="stable"), for the merged case np.add.reduceat over the sorted runs in float64 -- never with the
library itself.  Results of the stable sort are compared as raw bytes."""
import ctypes as C_

import numpy as np
import pytest
import torch

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po
from conftest import random_csr

pytestmark = pytest.mark.gpu
REG_MAX, LDS_MAX = sa.SORT_REG_MAX, sa.SORT_LDS_MAX
ERR_INVALID, ERR_UNSORTED = 1, 8


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def assemble(rows_cols, rows_vals, dtype):
    ro = np.zeros(len(rows_cols) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([len(c) for c in rows_cols])
    ci = np.concatenate(rows_cols).astype(np.uint32) if rows_cols else np.zeros(0, np.uint32)
    va = np.concatenate(rows_vals).astype(dtype) if rows_vals else np.zeros(0, dtype)
    return ro, ci, va


def upload(ro, ci, va, cols):
    return sa.dCSR.from_host(sa.HostCSR(len(ro) - 1, cols, ro, ci, va))


def expect_keep(ro, ci, va):
    """every row: the stable sort of itself by column id"""
    eci, eva = ci.copy(), va.copy()
    for r in range(len(ro) - 1):
        a, b = int(ro[r]), int(ro[r + 1])
        p = np.argsort(ci[a:b], kind="stable")
        eci[a:b], eva[a:b] = ci[a:b][p], va[a:b][p]
    return eci, eva


def expect_sum(ro, ci, va):
    """... then every run of equal columns one entry: the float64 sum of the run (and the run's sum of |v|)"""
    sci, sva = expect_keep(ro, ci, va)
    oro = np.zeros_like(ro)
    oci, osum, oabs = [], [], []
    for r in range(len(ro) - 1):
        a, b = int(ro[r]), int(ro[r + 1])
        c, v = sci[a:b], sva[a:b].astype(np.float64)
        if b > a:
            heads = np.flatnonzero(np.concatenate(([True], c[1:] != c[:-1])))
            oci.append(c[heads])
            osum.append(np.add.reduceat(v, heads))
            oabs.append(np.add.reduceat(np.abs(v), heads))
            oro[r + 1] = oro[r] + len(heads)
        else:
            oro[r + 1] = oro[r]
    cat = lambda x, t: np.concatenate(x).astype(t) if x else np.zeros(0, t)
    return oro, cat(oci, np.uint32), cat(osum, np.float64), cat(oabs, np.float64)


def strictly_ascending_rows(ro, ci):
    return sum(1 for r in range(len(ro) - 1) if (np.diff(ci[int(ro[r]):int(ro[r + 1])].astype(np.int64)) > 0).all())


def same_bytes(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def edge_matrix(dtype, seed=5, cols=100_000, long_row=20_000):
    """row lengths 0, 1, 2, 4 L and 4 L + 1 for L = 8 .. 64, the LDS cap and the cap + 1, one row well beyond it; each
    length shuffled, reversed, already sorted, and sorted but for the last entry; every value distinct"""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 2] + [4 * L + d for L in (8, 16, 32, 64) for d in (0, 1)] + [LDS_MAX, LDS_MAX + 1, long_row]
    rows_cols = []
    for n in lengths:
        for pattern in range(4):
            c = np.sort(rng.choice(cols, size=n, replace=False))
            if pattern == 0:
                c = rng.permutation(c)
            elif pattern == 1:
                c = c[::-1]
            elif pattern == 3:
                c = np.roll(c, -1)      # ascending, then the smallest column
            rows_cols.append(c)
    order = rng.permutation(len(rows_cols))
    rows_cols = [rows_cols[i] for i in order]
    nnz = sum(len(c) for c in rows_cols)
    vals = np.arange(1, nnz + 1, dtype=np.float64)   # < 2^24: distinct in float32 as well
    ro, ci, va = assemble(rows_cols, [vals], dtype)
    return ro, ci, va, cols


def duplicate_matrix(dtype, value_fn, seed=9, cols=50_000):
    """rows of every class whose columns repeat: up to 1 024 copies of a column"""
    rng = np.random.default_rng(seed)
    rows_cols = []
    plan = [(3, [2]), (6, [3, 2]), (20, [5, 1, 1, 7]), (40, [31, 2]), (60, [64, 64]), (10, [200]), (100, [255, 3]),
            (50, [1024]), (300, [1024, 1024, 17]), (3000, [1024, 500, 2, 2, 2]), (LDS_MAX, [1024] * 4), (0, [2]), (0, [])]
    for distinct, copies in plan * 3:
        c = rng.choice(cols, size=distinct + len(copies), replace=False)
        row = np.concatenate([c[:distinct]] + [np.full(m, c[distinct + i]) for i, m in enumerate(copies)])
        rows_cols.append(rng.permutation(row))
    for _ in range(40):                               # short rows over a handful of columns
        n = int(rng.integers(1, 120))
        rows_cols.append(rng.integers(1000, 1000 + max(2, n // 3), size=n))
    nnz = sum(len(c) for c in rows_cols)
    ro, ci, va = assemble(rows_cols, [value_fn(rng, nnz)], dtype)
    return ro, ci, va, cols


# ---------------------------------------------------------------------------------------------------- stable sort
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stable_sort_is_bit_exact_through_every_class(cfg, dtype):
    ro, ci, va, cols = edge_matrix(dtype)
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg)
    got = d.to_host()
    eci, eva = expect_keep(ro, ci, va)
    assert d.nnz == len(ci) and info.nnz_out == len(ci) and info.duplicates == 0
    assert same_bytes(got.row_offsets, ro)
    assert same_bytes(got.col_ids, eci)
    assert same_bytes(got.data, eva)
    assert all(k > 0 for k in info.rows_sorted), info
    planted = strictly_ascending_rows(ro, ci)
    assert info.rows_in_order == planted and sum(info.rows_sorted) == len(ro) - 1 - planted, info
    # a second call finds a canonical matrix: nothing to do, nothing changes
    again = sa.sort_rows(d, cfg)
    assert again.rows_in_order == len(ro) - 1 and sum(again.rows_sorted) == 0
    got = d.to_host()
    assert same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)


@pytest.mark.parametrize("reg_max,lds_max,empty", [(0, LDS_MAX, (0,)), (0, 0, (0, 1)), (40, 100, ()), (REG_MAX, 0, (1,))])
def test_the_same_rows_forced_through_each_class(cfg, reg_max, lds_max, empty):
    ro, ci, va, cols = edge_matrix(np.float64, seed=6, long_row=9000)
    cfg.set_option("sort_reg_max", reg_max)
    cfg.set_option("sort_lds_max", lds_max)
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg)
    got = d.to_host()
    eci, eva = expect_keep(ro, ci, va)
    assert same_bytes(got.row_offsets, ro) and same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)
    for k in range(3):
        assert (info.rows_sorted[k] == 0) == (k in empty), (info, empty)


def test_class_limits_are_clamped_to_what_the_kernels_support(cfg):
    ro, ci, va, cols = edge_matrix(np.float64, seed=7, long_row=9000)
    cfg.set_option("sort_reg_max", 1 << 20)
    cfg.set_option("sort_lds_max", 1 << 30)
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg)
    got = d.to_host()
    eci, eva = expect_keep(ro, ci, va)
    assert same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)
    assert all(k > 0 for k in info.rows_sorted)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_short_row_that_spans_every_column(cfg, dtype):
    """columns 0 and cols - 1 with cols = 2^27: the register key cannot hold the range"""
    cols = 1 << 27
    rng = np.random.default_rng(3)
    rows_cols = [np.array([cols - 1, 0]), np.array([cols - 1, 5, 0, cols - 2, 7]), rng.permutation(np.arange(0, cols, cols // 200)),
                 np.array([9, 3, 5]), np.array([cols - 1]), np.array([cols - 1, cols - 3, cols - 2]),
                 np.array([(1 << 24) - 2, 0]), np.array([(1 << 24) - 1, 0]), np.array([1 << 24, 0])]
    nnz = sum(len(c) for c in rows_cols)
    ro, ci, va = assemble(rows_cols, [np.arange(1, nnz + 1, dtype=np.float64)], dtype)
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg)
    got = d.to_host()
    eci, eva = expect_keep(ro, ci, va)
    assert same_bytes(got.row_offsets, ro) and same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)
    assert info.rows_in_order == 1 and sum(info.rows_sorted) == len(rows_cols) - 1


# ---------------------------------------------------------------------------------------------------- duplicates
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("limits", [(REG_MAX, LDS_MAX), (0, LDS_MAX), (0, 0)])
def test_duplicates_kept_stay_in_input_order(cfg, dtype, limits):
    """the values are the entries' input positions: inside a run of equal columns they must ascend"""
    ro, ci, va, cols = duplicate_matrix(dtype, lambda rng, n: np.arange(n, dtype=np.float64))
    cfg.set_option("sort_reg_max", limits[0])
    cfg.set_option("sort_lds_max", limits[1])
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg)
    got = d.to_host()
    eci, eva = expect_keep(ro, ci, va)
    assert same_bytes(got.row_offsets, ro) and same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)
    oro, _, _, _ = expect_sum(ro, ci, va)
    assert info.duplicates == len(ci) - int(oro[-1]) and info.nnz_out == len(ci) and d.nnz == len(ci)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("limits", [(REG_MAX, LDS_MAX), (0, LDS_MAX), (0, 0)])
def test_duplicates_summed_exactly(cfg, dtype, limits):
    """integers in [-64, 64], at most 1 024 copies: every partial sum is below 2^17 and exact in any order"""
    def values(rng, n):
        return rng.integers(-64, 65, size=n).astype(np.float64)
    ro, ci, va, cols = duplicate_matrix(dtype, values)
    # an entry that cancels to zero and stays: the first row holds its duplicated column twice
    a, b = int(ro[0]), int(ro[1])
    twice = np.flatnonzero(ci[a:b] == np.bincount(ci[a:b]).argmax()) + a
    assert len(twice) == 2
    va[twice[0]], va[twice[1]] = 5, -5
    cfg.set_option("sort_reg_max", limits[0])
    cfg.set_option("sort_lds_max", limits[1])
    d = upload(ro, ci, va, cols)
    info = sa.sort_rows(d, cfg, sum_duplicates=True)
    oro, oci, osum, _ = expect_sum(ro, ci, va)
    got = d.to_host()
    assert d.nnz == int(oro[-1]) and info.nnz_out == d.nnz and info.duplicates == len(ci) - d.nnz
    assert same_bytes(got.row_offsets, oro)
    assert same_bytes(got.col_ids, oci)
    assert same_bytes(got.data, osum.astype(dtype))
    first = got.data[int(oro[0]):int(oro[1])][got.col_ids[int(oro[0]):int(oro[1])] == ci[twice[0]]]
    assert len(first) == 1 and first[0] == 0
    # the result is canonical: a multiply's input check would take it, a second call has nothing to do
    again = sa.sort_rows(d, cfg, sum_duplicates=True)
    assert again.rows_in_order == len(ro) - 1 and again.duplicates == 0 and again.nnz_out == d.nnz


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_duplicates_summed_random_values(cfg, dtype):
    def values(rng, n):
        return (0.5 + rng.random(n)) * rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.integers(-8, 9, size=n)
    ro, ci, va, cols = duplicate_matrix(dtype, values, seed=21)
    d = upload(ro, ci, va, cols)
    sa.sort_rows(d, cfg, sum_duplicates=True)
    oro, oci, osum, oabs = expect_sum(ro, ci, va)
    got = d.to_host()
    assert same_bytes(got.row_offsets, oro) and same_bytes(got.col_ids, oci)
    if dtype == np.float64:
        err = np.abs(got.data - osum)
        print("fp64: max |got - ref| / sum|v| =", float((err / np.maximum(oabs, 1e-300)).max()))
        assert (err <= 1e-12 * oabs).all()
    else:
        ref = osum.astype(np.float32)
        lo, hi = np.nextafter(ref, np.float32(-np.inf)), np.nextafter(ref, np.float32(np.inf))
        print("fp32: entries off the rounded float64 sum:", int((got.data != ref).sum()), "of", len(ref))
        assert ((got.data == ref) | (got.data == lo) | (got.data == hi)).all()


# ---------------------------------------------------------------------------------------------------- the scan at its edges
def two_entry_rows(rows):
    """every row two entries, by r mod 3: (5, 3) out of order, (4, 4) a duplicate to merge, (1, 2) in order; the values
    1 .. 2 rows.  Returns the matrix and what SUM_DUPLICATES has to leave, both built without a Python loop."""
    kind = np.arange(rows) % 3
    ci = np.array([[5, 3], [4, 4], [1, 2]], dtype=np.uint32)[kind].ravel()
    va = np.arange(1, 2 * rows + 1, dtype=np.float64)
    ro = (2 * np.arange(rows + 1)).astype(np.uint32)
    first, second = va[0::2], va[1::2]
    e_ci = np.array([[3, 5], [4, 4], [1, 2]], dtype=np.uint32)[kind]
    e_va = np.stack([np.where(kind == 0, second, np.where(kind == 1, first + second, first)),
                     np.where(kind == 0, first, second)], axis=1)
    keep = np.ones((rows, 2), dtype=bool)
    keep[kind == 1, 1] = False                                   # the merged row keeps one entry
    e_ro = np.zeros(rows + 1, dtype=np.uint32)
    e_ro[1:] = np.cumsum(keep.sum(axis=1))
    return (ro, ci, va), (e_ro, e_ci[keep], e_va[keep]), kind


SCAN_ROWS = [1023, 1024, 1025, 2049, 1024 * 1024 + 1]


@pytest.mark.parametrize("rows", SCAN_ROWS)
def test_compaction_scan_across_workgroup_boundaries(cfg, rows):
    """The new row offsets come from a device-wide scan of 1024 rows per workgroup whose workgroup sums are scanned 1024
    at a time: one row short of a workgroup, exactly one, one more, two and a row, and one more than 1024 workgroups (the
    second trip of the loop over the sums).  Integers below 2^23: every sum is exact."""
    (ro, ci, va), (e_ro, e_ci, e_va), kind = two_entry_rows(rows)
    merged = int((kind == 1).sum())
    d = upload(ro, ci, va, 8)
    info = sa.sort_rows(d, cfg, sum_duplicates=True)
    got = d.to_host()
    assert d.nnz == 2 * rows - merged and info.nnz_out == d.nnz and info.duplicates == merged
    assert info.rows_in_order == int((kind == 2).sum()) and sum(info.rows_sorted) == rows - info.rows_in_order
    assert same_bytes(got.row_offsets, e_ro)
    assert same_bytes(got.col_ids, e_ci)
    assert same_bytes(got.data, e_va)
    again = sa.sort_rows(d, cfg, sum_duplicates=True)
    assert again.rows_in_order == rows and again.duplicates == 0 and again.nnz_out == d.nnz and sum(again.rows_sorted) == 0


# ---------------------------------------------------------------------------------------------------- views
def test_row_range_view(cfg):
    ro, ci, va, cols = duplicate_matrix(np.float64, lambda rng, n: np.arange(n, dtype=np.float64), seed=33)
    rows = len(ro) - 1
    r0, r1 = rows // 3, 2 * rows // 3
    assert ro[r0] != 0
    d = upload(ro, ci, va, cols)
    view = d.row_view(r0, r1)
    info = sa.sort_rows(view, cfg)
    got = d.to_host()
    a, b = int(ro[r0]), int(ro[r1])
    eci, eva = expect_keep(ro, ci, va)
    assert same_bytes(got.row_offsets, ro)
    assert same_bytes(got.col_ids[:a], ci[:a]) and same_bytes(got.col_ids[b:], ci[b:])
    assert same_bytes(got.data[:a], va[:a]) and same_bytes(got.data[b:], va[b:])
    assert same_bytes(got.col_ids[a:b], eci[a:b]) and same_bytes(got.data[a:b], eva[a:b])
    assert info.duplicates > 0 and view.nnz == b - a
    # SUM_DUPLICATES on a view that does not start at entry 0, duplicates present: refused, nothing changes
    d2 = upload(ro, ci, va, cols)
    view2 = d2.row_view(r0, r1)
    with pytest.raises(sa.SpeckError) as e:
        sa.sort_rows(view2, cfg, sum_duplicates=True)
    assert e.value.status == ERR_INVALID
    got = d2.to_host()
    assert same_bytes(got.row_offsets, ro) and same_bytes(got.col_ids, ci) and same_bytes(got.data, va)
    assert view2.nnz == b - a
    # ... without duplicates the flag changes nothing and a view is fine
    ro3, ci3, va3, cols3 = edge_matrix(np.float64, seed=8, long_row=6000)
    rows3 = len(ro3) - 1
    d3 = upload(ro3, ci3, va3, cols3)
    lo, hi = 10, rows3 - 10
    assert ro3[lo] != 0
    sa.sort_rows(d3.row_view(lo, hi), cfg, sum_duplicates=True)
    got = d3.to_host()
    eci, eva = expect_keep(ro3, ci3, va3)
    a, b = int(ro3[lo]), int(ro3[hi])
    assert same_bytes(got.row_offsets, ro3)
    assert same_bytes(got.col_ids[a:b], eci[a:b]) and same_bytes(got.data[a:b], eva[a:b])
    assert same_bytes(got.col_ids[:a], ci3[:a]) and same_bytes(got.col_ids[b:], ci3[b:])
    assert same_bytes(got.data[:a], va3[:a]) and same_bytes(got.data[b:], va3[b:])


# ---------------------------------------------------------------------------------------------------- rejected inputs
@pytest.mark.parametrize("guard", [0, 4096])
def test_hostile_input_is_refused_and_nothing_is_written(guard):
    """rejected inputs, not faults: a column id >= cols, a descending row_offsets, an offset beyond nnz"""
    cfg = sa.spECKConfig.initialize(0)
    try:
        if guard:
            cfg.set_option("guard_bytes", guard)
        ro, ci, va, cols = edge_matrix(np.float64, seed=11, long_row=6000)
        rows, nnz = len(ro) - 1, len(ci)
        mid = rows // 2
        while ro[mid + 1] == ro[mid]:
            mid += 1
        bad_col = ci.copy()
        bad_col[int(ro[mid])] = cols
        descending = ro.copy()
        descending[mid], descending[mid + 1] = ro[mid + 1], ro[mid]
        beyond = ro.copy()
        beyond[-1] = nnz + 5
        far = ro.copy()
        far[mid + 1:] = 0xFFFFFF00
        for h_ro, h_ci in ((ro, bad_col), (descending, ci), (beyond, ci), (far, ci)):
            d = upload(ro, ci, va, cols)
            assert _lib.load().speck_dcsr_update(C_.byref(d._c), h_ro.ctypes.data, h_ci.ctypes.data, None, 8) == 0
            for sum_duplicates in (False, True):
                with pytest.raises(sa.SpeckError) as e:
                    sa.sort_rows(d, cfg, sum_duplicates=sum_duplicates)
                assert e.value.status == ERR_INVALID     # (not 3: no canary zone was touched either)
                got = d.to_host()
                assert d.nnz == nnz
                assert same_bytes(got.row_offsets, h_ro) and same_bytes(got.col_ids, h_ci) and same_bytes(got.data, va)
        # the config serves a valid input afterwards, canary zones intact
        d = upload(ro, ci, va, cols)
        sa.sort_rows(d, cfg, sum_duplicates=True)
        eci, eva = expect_keep(ro, ci, va)
        got = d.to_host()
        assert same_bytes(got.col_ids, eci) and same_bytes(got.data, eva)
    finally:
        if guard:
            cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_duplicates_summed_with_canary_zones():
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        ro, ci, va, cols = duplicate_matrix(np.float64, lambda rng, n: rng.integers(-64, 65, size=n).astype(np.float64), seed=41)
        for limits in ((REG_MAX, LDS_MAX), (0, 0)):
            cfg.set_option("sort_reg_max", limits[0])
            cfg.set_option("sort_lds_max", limits[1])
            d = upload(ro, ci, va, cols)
            sa.sort_rows(d, cfg, sum_duplicates=True)
            oro, oci, osum, _ = expect_sum(ro, ci, va)
            got = d.to_host()
            assert same_bytes(got.row_offsets, oro) and same_bytes(got.col_ids, oci) and same_bytes(got.data, osum)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


# ---------------------------------------------------------------------------------------------------- the point of it all
def shuffled_rows(B, rng, duplicate_fraction=0.0):
    """every row's entries in random order; a fraction of them split into two entries v = v1 + v2 (exactly)"""
    ro = B.row_offsets.astype(np.int64)
    row_of = np.repeat(np.arange(B.rows), np.diff(ro))
    ci, va = B.col_ids, B.data
    if duplicate_fraction:
        pick = rng.random(B.nnz) < duplicate_fraction
        v1 = (va * 0.5).astype(np.float32).astype(np.float64)   # short mantissa; v - v1 is exact (within a factor 2 of v1)
        v2 = va - v1
        assert (v1 + v2 == va).all()
        row_of = np.concatenate([row_of, row_of[pick]])
        ci = np.concatenate([ci, ci[pick]])
        va = np.concatenate([np.where(pick, v1, va), v2[pick]])
    order = np.lexsort((rng.random(len(ci)), row_of))
    new_ro = np.zeros(B.rows + 1, dtype=np.uint32)
    new_ro[1:] = np.cumsum(np.bincount(row_of, minlength=B.rows))
    return new_ro, ci[order].astype(np.uint32), va[order]


def _inputs(kind):
    if kind == "random":
        return random_csr(400, 300, 6, 1), random_csr(300, 500, 8, 2)
    h = sa.gen_matrix(kind, {"scircuit": 0.05, "webbase": 0.02}[kind], 7, signed=True)
    A = po.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data)
    return A, A


@pytest.mark.parametrize("kind", ["random", "scircuit", "webbase"])
@pytest.mark.parametrize("duplicates", [False, True])
def test_a_shuffled_b_is_refused_and_multiplies_after_sort_rows(cfg, kind, duplicates):
    A, B = _inputs(kind)
    rng = np.random.default_rng(77)
    s_ro, s_ci, s_va = shuffled_rows(B, rng, 0.1 if duplicates else 0.0)
    dA = sa.dCSR.from_host(sa.HostCSR(A.rows, A.cols, A.row_offsets, A.col_ids, A.data))
    dB = upload(s_ro, s_ci, s_va, B.cols)
    dC = sa.dCSR()
    with pytest.raises(sa.SpeckError) as e:
        sa.MultiplyspECK(dA, dB, dC, cfg)
    assert e.value.status == ERR_UNSORTED            # today's behaviour, and it stays
    info = sa.sort_rows(dB, cfg, sum_duplicates=duplicates)
    assert dB.nnz == B.nnz and info.nnz_out == B.nnz and info.duplicates == len(s_ci) - B.nnz
    if kind == "webbase":
        assert info.rows_sorted[1] + info.rows_sorted[2] > 0, info     # long rows are in B
    sa.MultiplyspECK(dA, dB, dC, cfg)
    R, ab = po.spgemm(A, B)
    got = dC.to_host()
    assert got.nnz == R.nnz and same_bytes(got.row_offsets, R.row_offsets) and same_bytes(got.col_ids, R.col_ids)
    assert (np.abs(got.data - R.data) <= 1e-12 * ab + 1e-300).all()


# ---------------------------------------------------------------------------------------------------- caller's stream
def test_sort_rows_runs_on_the_callers_stream(cfg):
    """the columns are written by a torch kernel on the caller's stream right before the call: ordering against the
    producer is by the stream alone"""
    ro, ci, va, cols = edge_matrix(np.float64, seed=13, long_row=9000)
    eci, eva = expect_keep(ro, ci, va)
    dev = torch.device("cuda:0")
    t_ro = torch.from_numpy(ro.view(np.int32).copy()).to(dev)
    t_ci = torch.from_numpy(eci.view(np.int32).copy()).to(dev)      # canonical until the producer has run
    t_va = torch.from_numpy(va.copy()).to(dev)
    t_shuffled = torch.from_numpy(ci.view(np.int32).copy()).to(dev)
    d = sa.dCSR.from_device(len(ro) - 1, cols, len(ci), t_ro.data_ptr(), t_ci.data_ptr(), t_va.data_ptr(),
                            keep=(t_ro, t_ci, t_va), host_row_offsets=ro)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(200_000_000)          # ~0.1 s: whatever does not wait for the stream sees canonical rows
            t_ci.copy_(t_shuffled, non_blocking=True)
        info = sa.sort_rows(d, cfg)
        assert sum(info.rows_sorted) > 0
        assert same_bytes(t_ci.cpu().numpy().view(np.uint32), eci)
        assert same_bytes(t_va.cpu().numpy(), eva)
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()
