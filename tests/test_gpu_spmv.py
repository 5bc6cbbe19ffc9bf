"""speck_spmv_* on the GPU (speck_amd/csrc/spmv.hip): y = alpha A x + beta y.  The expectation is numpy / math.fsum in this
file: with integer values every order gives the same bits, so equality (every sum stays below 2^53); for real values the
bound of any summation order, (g_n + 2^-53) sum|t| with g_n = n 2^-53 / (1 - n 2^-53) and t = a.astype(f64) * x[col] -- the
extra ulp is the reference's own rounding.  The epilogue alpha * s + beta * y0 is numpy's, bit for bit.  T = 4096 entries
per tile below."""
import ctypes as C_
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
DTYPES = [np.float64, np.float32]
T = sa.SPMV_TILE_ENTRIES
U = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
COLS = 3000


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def mk(lens, data, cols=COLS, seed=1):
    """rows of the given lengths over `data`; column ids random in [0, cols), duplicates allowed, unsorted"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = np.random.default_rng(seed).integers(0, cols, size=len(data)).astype(np.uint32)
    return sa.HostCSR(len(lens), cols, ro, ci, np.asarray(data))


def ints(n, seed, dtype=np.float64):
    return np.random.default_rng(seed).integers(-1024, 1025, size=n).astype(dtype)


def real_values(n, seed, dtype=np.float64):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.random(n)) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(dtype)


def terms(H, x):
    with np.errstate(invalid="ignore"):
        return H.data.astype(np.float64) * np.asarray(x, dtype=np.float64)[H.col_ids.astype(np.int64)]


def row_sums(H, x):
    """numpy's row sums of the terms (exact for integers); +0.0 for a row without entries"""
    t = terms(H, x)
    ro = H.row_offsets.astype(np.int64)
    s = np.zeros(H.rows)
    full = np.nonzero(ro[1:] > ro[:-1])[0]
    with np.errstate(invalid="ignore"):
        if len(full):
            s[full] = np.add.reduceat(t, ro[:-1][full])
    return s


def counts(ro):
    """what speck_spmv_info reports, counted on the host (ro absolute)"""
    ro = np.asarray(ro, dtype=np.int64)
    s, e = ro[:-1], ro[1:]
    full = e > s
    nnz = int(ro[-1] - ro[0]) if len(ro) else 0
    return (int((~full).sum()), int(((e[full] - 1) // T > s[full] // T).sum()),
            int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0, nnz)


def check_info(info, ro):
    assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == counts(ro), (info, counts(ro))


def tv(a):
    """a float64 vector on the device (one element at least, so that it has an address)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(1)).to(DEV)


def sentinel(n):
    return torch.from_numpy(np.full(max(n, 1), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)


def host(t, n=None):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a if n is None else a[:n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True)


def run(cfg, dA, x, alpha=1.0, beta=0.0, y0=None):
    """one call into a y that lives in a torch tensor: (y on the host, info); without y0 the tensor holds the sentinel"""
    y = sentinel(dA.rows) if y0 is None else tv(y0)
    out, info = sa.spmv(dA, x, cfg, alpha=alpha, beta=beta, y=y.data_ptr() if dA.rows == 0 else y[:max(dA.rows, 1)])
    assert out is None
    return host(y, dA.rows), info


def edge_lens():
    """case 1: (row lengths) laid out against the tile edges; the comments give the entries a row holds"""
    return ([0,                # an empty first row
             T,                # [0, T): a row that is a tile
             0,                # an empty row exactly at T
             1,                # [T, T + 1): the first entry of a tile
             T - 3,            # [T + 1, 2T - 2)
             1,                # [2T - 2, 2T - 1): ends at T - 1 of its tile
             1,                # [2T - 1, 2T): the last entry of a tile
             0,                # an empty row exactly at 2T
             T - 1,            # [2T, 3T - 1)
             2 * T + 2,        # [3T - 1, 5T + 1): four tiles, two of them wholly inside
             99,               # [5T + 1, 5T + 100)
             T - 50,           # [5T + 100, 6T + 50): split ...
             T - 40,           # [6T + 50, 7T + 10): ... and split: the two meet in tile 6
             T - 10]           # [7T + 10, 8T)
            + [0] * 5000 +     # more rows without entries than a tile has entries, between two tiles
            [5,                # [8T, 8T + 5)
             2,                # [8T + 5, 8T + 7)
             0])               # an empty last row


_CACHE = {}


def edge_case(dtype):
    """(H, x, row sums by numpy), computed once"""
    key = ("edge", np.dtype(dtype).name)
    if key not in _CACHE:
        lens = edge_lens()
        H = mk(lens, ints(sum(lens), 11, dtype), seed=12)
        x = ints(COLS, 13)
        s = row_sums(H, x)
        assert np.abs(terms(H, x)).sum() < 2.0 ** 53
        for a in (H.row_offsets, H.col_ids, H.data, x, s):
            a.setflags(write=False)
        _CACHE[key] = (H, x, s)
    return _CACHE[key]


def real_case(dtype):
    """cases 2 and 3: row lengths from 0 to 3T; (H, x, fsum per row, sum|t| per row), computed once"""
    key = ("real", np.dtype(dtype).name)
    if key not in _CACHE:
        rng = np.random.default_rng(5)
        lens = [T - 1, 1, 7, 0, 100, T, T + 1, 3 * T, 0, 2 * T + 5, 33, 1000, 3 * T - 1, 17, 0, 0, 2, T + T // 2]
        lens += [int(v) for v in rng.integers(0, 60, size=400)]
        H = mk(lens, real_values(sum(lens), 6, dtype), seed=7)
        x = real_values(COLS, 8)
        t = terms(H, x)
        ro = H.row_offsets.astype(np.int64)
        want = np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])])
        mags = np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])])
        for a in (H.row_offsets, H.col_ids, H.data, x, want, mags):
            a.setflags(write=False)
        _CACHE[key] = (H, x, want, mags)
    return _CACHE[key]


def on_torch(H, ro=None, col=None, nnz=None, r0=0, r1=None, shift=0):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz, a view; shift = 1 puts
    a dummy entry in front of data and col_ids and advances both pointers by one element"""
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    r1 = H.rows if r1 is None else r1
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    va = np.concatenate([np.full(shift, 77, dtype=H.data.dtype), H.data, np.zeros(1, dtype=H.data.dtype)])
    ci = np.concatenate([np.zeros(shift, dtype=np.uint32), np.asarray(col, dtype=np.uint32), np.zeros(1, dtype=np.uint32)])
    t_va = torch.from_numpy(va).to(DEV)
    t_ci = torch.from_numpy(ci.view(np.int32)).to(DEV)
    if nnz is None:
        nnz = int(H.row_offsets[r1]) - int(H.row_offsets[r0])
    return sa.dCSR.from_device(r1 - r0, H.cols, nnz, t_ro.data_ptr() + 4 * r0, t_ci.data_ptr() + 4 * shift,
                               t_va.data_ptr() + H.data.itemsize * shift, dtype=H.data.dtype, keep=(t_ro, t_va, t_ci))


# ---------------------------------------------------------------------------------------------------- 1: tile edges, exact
COEFFS = [(1.0, 0.0), (2.0, -3.0), (0.0, 1.0)]


def check_edge(cfg, dA, dtype):
    H, x, s = edge_case(dtype)
    dx = tv(x)
    y0 = ints(H.rows, 14)
    for alpha, beta in COEFFS:
        got, info = run(cfg, dA, dx, alpha, beta, y0 if beta else None)
        want = alpha * s + beta * y0 if beta else alpha * s
        assert np.array_equal(got, want), (alpha, beta, np.nonzero(got != want)[0][:8])
        check_info(info, H.row_offsets)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_at_every_tile_edge(cfg, dtype):
    H, _, _ = edge_case(dtype)
    ro = H.row_offsets.astype(np.int64)
    assert {T - 1, 0, 1} <= set((ro % T).tolist()) and T in ro and 2 * T in ro and 8 * T in ro
    assert counts(ro) == (5004, 3, 9, 8 * T + 7)
    check_edge(cfg, sa.dCSR.from_host(H), dtype)


# ---------------------------------------------------------------------------------------------------- 2: views; 3: the bound
def allowance(n, mag):
    n = np.asarray(n, dtype=np.float64)
    return (n * U / (1.0 - n * U) + U) * mag


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_gives_the_rows_of_the_whole_and_two_calls_the_same_bytes(cfg, dtype):
    H, x, _, _ = real_case(dtype)
    ro = H.row_offsets.astype(np.int64)
    dA, dx = sa.dCSR.from_host(H), tv(x)
    whole, info = run(cfg, dA, dx)
    again, _ = run(cfg, dA, dx)
    assert bits(whole).tobytes() == bits(again).tobytes()
    check_info(info, ro)
    r_odd = next(r for r in range(1, H.rows) if ro[r] % 2 == 1 and ro[r] % T != T - 1 and ro[r + 1] > ro[r])
    r_tile = next(r for r in range(1, H.rows) if ro[r] % T == 0 and ro[r] > 0 and ro[r + 1] > ro[r])
    r_last = next(r for r in range(1, H.rows) if ro[r] % T == T - 1 and ro[r + 1] > ro[r])
    r_mid = next(r for r in range(H.rows - 1, 0, -1) if ro[r] % T and ro[r] // T > ro[r_odd] // T + 2)
    for a, b in ((r_odd, H.rows), (r_tile, H.rows), (r_last, H.rows), (r_odd, r_mid), (r_tile, r_mid), (0, r_mid)):
        got, info = run(cfg, dA.row_view(a, b), dx)
        assert bits(got).tobytes() == bits(whole[a:b]).tobytes(), (a, b)
        check_info(info, ro[a:b + 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_values_within_the_bound_of_any_order(cfg, dtype):
    H, x, want, mags = real_case(dtype)
    ro = H.row_offsets.astype(np.int64)
    got, _ = run(cfg, sa.dCSR.from_host(H), tv(x))
    err = np.abs(got - want)
    print("largest error / allowance:", float(np.max(err / np.maximum(allowance(ro[1:] - ro[:-1], mags), 1e-300))))
    ok = err <= allowance(ro[1:] - ro[:-1], mags)
    assert ok.all(), (np.nonzero(~ok)[0][:8], err[~ok][:8])


# ---------------------------------------------------------------------------------------------------- 4: the epilogue, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_epilogue_is_numpys_bit_for_bit(cfg, dtype):
    H, x, _, _ = real_case(dtype)
    dA, dx = sa.dCSR.from_host(H), tv(x)
    s, _ = run(cfg, dA, dx)
    rng = np.random.default_rng(40)
    y0 = rng.choice([-1.0, 1.0], size=H.rows) * (0.5 + rng.random(H.rows))        # (1e300 y0 stays finite: no inf - inf)
    for alpha, beta in ((0.3, 0.0), (-1.7, 0.9), (1e300, 1e300)):
        got, _ = run(cfg, dA, dx, alpha, beta, y0)
        with np.errstate(over="ignore"):
            want = alpha * s + beta * y0
        assert not np.isnan(want).any()
        assert bits(got).tobytes() == bits(want).tobytes(), (alpha, beta, np.nonzero(bits(got) != bits(want))[0][:8])
        if alpha == 1e300:
            assert np.isinf(want).any() and np.isfinite(want).any()                # overflow to inf included


# ---------------------------------------------------------------------------------------------------- 5: the tree of reduce
def test_the_same_tree_as_reduce_of_the_column_scaled_matrix(cfg):
    for H, x in (edge_case(np.float64)[:2], real_case(np.float64)[:2]):
        dA, dx = sa.dCSR.from_host(H), tv(x)
        got, _ = run(cfg, dA, dx)
        scaled, _ = sa.scale(dA, cfg, col=dx)
        want, _, _ = sa.reduce(scaled, cfg, "sum", total=False)
        assert np.array_equal(got, want, equal_nan=True)
        both = ~(np.isnan(got) | np.isnan(want))
        assert (bits(got)[both] == bits(want)[both]).all()


# ---------------------------------------------------------------------------------------------------- 6: beta = 0 does not read y
@pytest.mark.parametrize("dtype", DTYPES)
def test_beta_zero_does_not_read_y_and_a_nan_of_y_stays_in_its_row(cfg, dtype):
    H, x, s = edge_case(dtype)
    dA, dx = sa.dCSR.from_host(H), tv(x)
    got, _ = run(cfg, dA, dx, 1.0, 0.0, None)                                      # y holds the payload NaN everywhere
    assert not np.isnan(got).any() and np.array_equal(got, s)
    y0 = ints(H.rows, 15)
    ks = [0, 1, 9, H.rows - 3, H.rows - 1]                                         # empty, a whole tile, four tiles, five entries, empty
    y0[ks] = np.nan
    got, _ = run(cfg, dA, dx, 1.0, 1.0, y0)
    assert np.nonzero(np.isnan(got))[0].tolist() == ks
    assert same(got, s + y0)


# ---------------------------------------------------------------------------------------------------- 7: special values
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_land_in_the_rows_that_reference_them(cfg, dtype):
    lens = [3, 2, 0, 5, 2 * T + 10, 4, 1, 6]
    ro = np.concatenate([[0], np.cumsum(lens)])
    n = int(ro[-1])
    rng = np.random.default_rng(70)
    data = rng.integers(1, 100, size=n).astype(dtype)
    col = rng.integers(10, 50, size=n).astype(np.uint32)                           # nobody references 7 or 9 by chance
    x = ints(50, 71)
    x[7], x[9] = np.nan, np.inf
    col[ro[0] + 1] = 7                                                             # row 0: a NaN of x
    col[ro[1]] = 9
    data[ro[1]] = 0.0                                                              # row 1: 0 * inf
    col[ro[3] + 4] = 9                                                             # row 3: 12 * inf = inf, no NaN
    data[ro[3] + 4] = 12
    col[ro[4] + T + T // 2] = 7                                                    # row 4: a NaN of x in a tile inside the row
    data[ro[5] + 2] = np.nan                                                       # row 5: a NaN of A
    H = sa.HostCSR(len(lens), 50, ro.astype(np.uint32), col, data)
    got, _ = run(cfg, sa.dCSR.from_host(H), tv(x))
    want = row_sums(H, x)
    assert np.nonzero(np.isnan(want))[0].tolist() == [0, 1, 4, 5] and want[3] == np.inf
    assert same(got, want), (got[:8], want[:8])


# ---------------------------------------------------------------------------------------------------- 8: hostile input
def hostile(H):
    """(offsets, column ids, declared nnz, first row, last row) -- one change each"""
    ro, rows, nnz = H.row_offsets, H.rows, H.nnz
    assert nnz % T and ro[6] - ro[5] == 1 and ro[5] == 2 * T - 2 and ro[9] == 3 * T - 1 and ro[10] == 5 * T + 1
    for bad_id in (H.cols, 0xFFFFFFFF):
        # entry 0, T - 1, T, the last entry of the partial last tile, a one-entry row, the middle of a split row
        for p in (0, T - 1, T, nnz - 1, 2 * T - 2, 4 * T + T // 2):
            col = H.col_ids.copy()
            col[p] = bad_id
            yield ro, col, nnz, 0, rows
    bad = ro.copy()
    bad[1024] = bad[1025] + 1                                      # a descending pair
    yield bad, None, nnz, 0, rows
    yield ro, None, nnz + 1, 0, rows                               # the last offset is short of nnz
    a, b = 3, rows - 2                                             # a view whose second row starts below its base
    bad = ro.copy()
    bad[a] = bad[a + 1] + 1
    yield bad, None, int(ro[b]) - int(ro[a]), a, b


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_of_y_is_written(cfg, dtype):
    H, x, s = edge_case(dtype)
    good, dx = sa.dCSR.from_host(H), tv(x)
    L = _lib.load()
    fn = L.speck_spmv_f32 if dtype == np.float32 else L.speck_spmv_f64
    y0 = ints(H.rows, 16)
    for k, (ro, col, nnz, a, b) in enumerate(hostile(H)):
        dA = on_torch(H, ro=ro, col=col, nnz=nnz, r0=a, r1=b)
        y = sentinel(b - a)
        info = _lib.CSpmvInfo(7, 7, 7, 7)
        alpha, beta = COEFFS[k % 2]
        torch.cuda.synchronize()
        rc = fn(cfg._h, alpha, C_.byref(dA._c), dx.data_ptr(), beta, y.data_ptr(), C_.byref(info))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, k
        assert (bits(host(y)) == SENTINEL_BITS).all(), k
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == (0, 0, 0, 0), k
        got, _ = run(cfg, good, dx, 2.0, -3.0, y0)                 # the config serves a valid call right after
        assert np.array_equal(got, 2.0 * s - 3.0 * y0), k


# ---------------------------------------------------------------------------------------------------- 9: alignment
@pytest.mark.parametrize("dtype", DTYPES)
def test_arrays_off_the_16_byte_boundary(cfg, dtype):
    H, _, _ = edge_case(dtype)
    dA = on_torch(H, shift=1)
    assert dA._c.data % 16 and dA._c.col_ids % 16
    check_edge(cfg, dA, dtype)


# ---------------------------------------------------------------------------------------------------- 10: degenerate
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_shapes(cfg, dtype):
    x = ints(COLS, 17)
    dx = tv(x)
    # no row: nothing is written
    none = sa.HostCSR(0, COLS, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))
    y = sentinel(4)
    out, info = sa.spmv(sa.dCSR.from_host(none), dx, cfg, alpha=2.0, beta=0.0, y=y.data_ptr())
    assert out is None and (bits(host(y)) == SENTINEL_BITS).all()
    assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == (0, 0, 0, 0)
    # no entry: y = alpha (+0.0) + beta y
    hollow = mk([0] * 5, np.zeros(0, dtype=dtype))
    y0 = np.array([1.0, -2.0, 0.0, 4.5, -0.0])
    got, info = run(cfg, sa.dCSR.from_host(hollow), dx, 3.0, 2.0, y0)
    assert bits(got).tobytes() == bits(3.0 * 0.0 + 2.0 * y0).tobytes()
    check_info(info, hollow.row_offsets)
    # rows without entries only, more than a workgroup's: +0.0, whatever y held
    hollow = mk([0] * 3000, np.zeros(0, dtype=dtype))
    got, info = run(cfg, sa.dCSR.from_host(hollow), dx)
    assert (bits(got) == 0).all()
    check_info(info, hollow.row_offsets)
    # one row of 3T + 1 entries; 70 000 rows of one entry: more rows than any tile has entries
    for lens in ([3 * T + 1], [1] * 70000):
        H = mk(lens, ints(sum(lens), 18, dtype), seed=19)
        got, info = run(cfg, sa.dCSR.from_host(H), dx)
        assert np.array_equal(got, row_sums(H, x)), len(lens)
        check_info(info, H.row_offsets)


# ---------------------------------------------------------------------------------------------------- 11: plumbing
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config_and_a_result_of_the_librarys_own(cfg, dtype):
    H, x, s = edge_case(dtype)
    dA, dx = sa.dCSR.from_host(H), tv(x)
    check_edge(None, dA, dtype)
    for c in (None, cfg):
        out, info = sa.spmv(dA, dx, c, alpha=-2.0)                                 # y=None: downloaded from a library buffer
        assert np.array_equal(out, -2.0 * s)
        check_info(info, H.row_offsets)
        out, _ = sa.spmv(dA, dx.data_ptr(), c)                                     # x as a plain device address
        assert np.array_equal(out, s)


def test_x_and_y_side_by_side_in_one_buffer(cfg):
    """two ranges that touch share no byte: y right behind x and right in front of it are served, one element closer is
    refused with nothing written"""
    H, x, s = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    for y_first in (False, True):
        buf = sentinel(COLS + H.rows)
        dx, dy = (buf[H.rows:], buf[:H.rows]) if y_first else (buf[:COLS], buf[COLS:])
        dx.copy_(tv(x))
        sa.spmv(dA, dx, cfg, y=dy)
        assert np.array_equal(host(dy), s) and np.array_equal(host(dx), x)
    buf = sentinel(COLS + H.rows)
    buf[:COLS].copy_(tv(x))
    with pytest.raises(sa.SpeckError) as e:
        sa.spmv(dA, buf[:COLS], cfg, y=buf[COLS - 1:COLS - 1 + H.rows])
    assert e.value.status == ERR_INVALID
    assert np.array_equal(host(buf[:COLS]), x) and (bits(host(buf[COLS:])) == SENTINEL_BITS).all()


def test_wrong_vectors_are_refused_in_python(cfg):
    H, x, _ = edge_case(np.float64)
    dA, dx = sa.dCSR.from_host(H), tv(x)
    y = torch.zeros(H.rows, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        sa.spmv(dA, dx.float(), cfg)
    with pytest.raises(ValueError):
        sa.spmv(dA, dx[:-1], cfg)
    with pytest.raises(ValueError):
        sa.spmv(dA, torch.zeros(2 * COLS, dtype=torch.float64, device=DEV)[::2], cfg)
    with pytest.raises(ValueError):
        sa.spmv(dA, dx, cfg, y=y.float())
    with pytest.raises(ValueError):
        sa.spmv(dA, dx, cfg, y=y[1:])
    with pytest.raises(ValueError):
        sa.spmv(dA, dx, cfg, beta=1.0)                                             # nothing to read
    assert not host(y).any()


def test_runs_on_the_callers_stream(cfg):
    """x is written by a copy on the caller's stream right before the call: ordering against the producer is by the
    stream alone"""
    H, x, s = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    real, dx = tv(x), tv(np.zeros(COLS))
    y = sentinel(H.rows)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream multiplies zeros
            dx.copy_(real, non_blocking=True)
        sa.spmv(dA, dx, cfg, y=y)
        assert np.array_equal(host(y), s)
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        check_edge(cfg, sa.dCSR.from_host(edge_case(dtype)[0]), dtype)             # (a touched zone is status 3)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_a_spmv_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.08, 7, signed=True)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()
    for _ in range(3):
        sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"]
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1
    x = real_values(h.cols, 21)
    out, _ = sa.spmv(dS, tv(x), cfg)
    t = terms(h, x)
    ro = h.row_offsets.astype(np.int64)
    want = np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])])
    mags = np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])])
    assert (np.abs(out - want) <= allowance(ro[1:] - ro[:-1], mags)).all()
    sa.spmv(dC, tv(x), cfg)                                                        # ... and of the product itself, where it lies
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1


# ---------------------------------------------------------------------------------------------------- 12: a power iteration
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_power_iteration_stays_on_the_device(cfg, dtype):
    n = 2000
    S = sp.random(n, n, density=6 / n, random_state=120, format="csr")
    S.sort_indices()
    G = ((S + S.T) != 0).astype(np.float64).tocsr()
    deg = np.asarray(G.sum(axis=1)).ravel()
    assert 0 < deg.max() <= 100
    P = sp.diags(1.0 / np.maximum(deg, 1.0)).dot(G).tocsr()                        # (1 / deg is one rounding, as on the device)
    P.data = P.data.astype(dtype).astype(np.float64)
    x0 = 1.0 + np.random.default_rng(121).random(n)
    ref = x0 / np.linalg.norm(x0)
    for _ in range(10):
        ref = P @ ref
        ref = ref / np.linalg.norm(ref)

    HS = sa.HostCSR(n, n, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.astype(dtype))
    dP, _ = sa.normalize_rows(sa.pattern_ones(sa.symmetrize(sa.dCSR.from_host(HS), cfg), cfg), cfg)
    x = tv(x0)
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)                                             # torch's normalisation and the product: one queue
    try:
        with torch.cuda.stream(stream):
            x /= torch.linalg.vector_norm(x)
            for _ in range(10):
                sa.spmv(dP, x, cfg, y=y)
                torch.div(y, torch.linalg.vector_norm(y), out=x)
            got = host(x)
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    rel2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("relative difference after ten steps:", rel, rel2)
    assert rel <= 1e-12 and rel2 <= 1e-12
