"""speck_spmm_* on the GPU (speck_amd/csrc/spmm.hip): Y = alpha A X + beta Y with k right-hand sides in padded row-major
blocks.  The expectation is numpy / math.fsum in this file: with integer values every order gives the same bits, so
equality (every sum stays below 2^53); for real values the bound of any summation order, (g_n + 2^-53) sum|t| with
g_n = n 2^-53 / (1 - n 2^-53) and t = a.astype(f64) * X[col, c] -- the extra ulp is the reference's own rounding -- and,
the defining property, byte equality of every column with speck_spmv_* on contiguous copies of that column.  Every Y lives
in a frame filled with a payload NaN: the padding between its rows and what lies behind the last row must still hold the
payload after every call.  T = 4096 entries per tile below; CB is the number of columns the tile kernel takes per round."""
import ctypes as C_
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_DIM_LIMIT = 1, 2
DTYPES = [np.float64, np.float32]
T = sa.SPMV_TILE_ENTRIES
CB = sa.SPMM_COLUMN_BLOCK              # the columns whose gathers the tile kernel has in flight together
KS = sorted({1, 2, 3, CB, CB + 1, 2 * CB + 1, 9})
U = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
COLS = 3000
TAIL = 8                                # payload words behind the last row of a frame


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


def ints(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).integers(-1024, 1025, size=shape).astype(dtype)


def real_values(shape, seed, dtype=np.float64):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(dtype)


def terms(H, x):
    """the terms of one column"""
    with np.errstate(invalid="ignore"):
        return H.data.astype(np.float64) * np.asarray(x, dtype=np.float64)[H.col_ids.astype(np.int64)]


def row_sums(H, X):
    """numpy's row sums of the terms, column by column (exact for integers); +0.0 for a row without entries"""
    ro = H.row_offsets.astype(np.int64)
    S = np.zeros((H.rows, X.shape[1]))
    full = np.nonzero(ro[1:] > ro[:-1])[0]
    with np.errstate(invalid="ignore"):
        for c in range(X.shape[1]):
            if len(full):
                S[full, c] = np.add.reduceat(terms(H, X[:, c]), ro[:-1][full])
    return S


def counts(ro, k):
    """what speck_spmm_info reports, counted on the host (ro absolute)"""
    ro = np.asarray(ro, dtype=np.int64)
    s, e = ro[:-1], ro[1:]
    full = e > s
    nnz = int(ro[-1] - ro[0]) if len(ro) else 0
    return (int((~full).sum()), int(((e[full] - 1) // T > s[full] // T).sum()),
            int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0, nnz, nnz * k)


def as_tuple(info):
    return (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms)


def check_info(info, ro, k):
    assert as_tuple(info) == counts(ro, k), (info, counts(ro, k))


def tv(a):
    """a float64 vector on the device (one element at least, so that it has an address)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return torch.from_numpy(a.copy() if a.size else np.zeros(1)).to(DEV)


def frame(n, ld, k, vals=None, lead=0):
    """(buffer, block): a device buffer of the payload NaN that holds an n x k block in rows ld apart, `lead` words from its
    start and TAIL words from its end; the block is the torch view [:, :k] of those rows and holds vals"""
    buf = torch.from_numpy(np.full(lead + n * ld + TAIL, SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
    blk = buf[lead:lead + n * ld].view(n, ld)[:, :k]
    if vals is not None and n and k:
        blk.copy_(torch.from_numpy(np.array(vals, dtype=np.float64)).to(DEV))
    return buf, blk


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True)


def read_frame(buf, n, ld, k, lead=0):
    """the n x k block of a frame on the host, after checking that every other word still holds the payload"""
    full = host(buf)
    rows = full[lead:lead + n * ld].reshape(n, ld)
    assert (bits(full[:lead]) == SENTINEL_BITS).all(), "in front of Y"
    assert (bits(rows[:, k:]) == SENTINEL_BITS).all(), "the padding of Y"
    assert (bits(full[lead + n * ld:]) == SENTINEL_BITS).all(), "behind the last row of Y"
    return rows[:, :k].copy()


def run(cfg, dA, X, alpha=1.0, beta=0.0, Y0=None, ldx=None, ldy=None, x_lead=0):
    """one call on padded blocks (ldx = k + 3, ldy = k + 2 unless given) passed as torch column slices: (Y on the host,
    info); without Y0 the block holds the payload too"""
    k = X.shape[1]
    ldx = k + 3 if ldx is None else ldx
    ldy = k + 2 if ldy is None else ldy
    xb, xs = frame(dA.cols, ldx, k, X, lead=x_lead)
    yb, ys = frame(dA.rows, ldy, k, Y0)
    out, info = sa.spmm(dA, xs, cfg, alpha=alpha, beta=beta, Y=ys)
    assert out is None
    assert bits(host(xb)).tobytes() == bits(host(frame(dA.cols, ldx, k, X, lead=x_lead)[0])).tobytes(), "X was written"
    return read_frame(yb, dA.rows, ldy, k), info


def edge_lens():
    """(row lengths) laid out against the tile edges; the comments give the entries a row holds"""
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
K_MAX = max(KS)


def edge_case(dtype):
    """(H, X of K_MAX columns, row sums by numpy), computed once; a test with k columns takes the first k"""
    key = ("edge", np.dtype(dtype).name)
    if key not in _CACHE:
        lens = edge_lens()
        H = mk(lens, ints(sum(lens), 11, dtype), seed=12)
        X = ints((COLS, K_MAX), 13)
        S = row_sums(H, X)
        for c in range(K_MAX):
            assert np.abs(terms(H, X[:, c])).sum() < 2.0 ** 53
        for a in (H.row_offsets, H.col_ids, H.data, X, S):
            a.setflags(write=False)
        _CACHE[key] = (H, X, S)
    return _CACHE[key]


REAL_K = 5


def real_case(dtype):
    """row lengths from 0 to 3T, real values; (H, X of REAL_K columns, fsum per row and column, sum|t| likewise), once"""
    key = ("real", np.dtype(dtype).name)
    if key not in _CACHE:
        rng = np.random.default_rng(5)
        lens = [T - 1, 1, 7, 0, 100, T, T + 1, 3 * T, 0, 2 * T + 5, 33, 1000, 3 * T - 1, 17, 0, 0, 2, T + T // 2]
        lens += [int(v) for v in rng.integers(0, 60, size=400)]
        H = mk(lens, real_values(sum(lens), 6, dtype), seed=7)
        X = real_values((COLS, REAL_K), 8)
        ro = H.row_offsets.astype(np.int64)
        want, mags = np.zeros((H.rows, 3)), np.zeros((H.rows, 3))
        for c in range(3):                                                         # (the bound test takes three columns)
            t = terms(H, X[:, c])
            want[:, c] = [math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])]
            mags[:, c] = [math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])]
        for a in (H.row_offsets, H.col_ids, H.data, X, want, mags):
            a.setflags(write=False)
        _CACHE[key] = (H, X, want, mags)
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


def check_edge(cfg, dA, dtype, ks=KS, **layout):
    H, X, S = edge_case(dtype)
    for k in ks:
        Y0 = ints((H.rows, k), 14)
        for alpha, beta in COEFFS:
            got, info = run(cfg, dA, X[:, :k], alpha, beta, Y0 if beta else None, **layout)
            want = alpha * S[:, :k] + beta * Y0 if beta else alpha * S[:, :k]
            assert np.array_equal(got, want), (k, alpha, beta, np.argwhere(got != want)[:8])
            check_info(info, H.row_offsets, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_k_around_the_block_width_exact_with_the_padding_untouched(cfg, dtype):
    H, _, _ = edge_case(dtype)
    ro = H.row_offsets.astype(np.int64)
    assert {T - 1, 0, 1} <= set((ro % T).tolist()) and T in ro and 2 * T in ro and 8 * T in ro
    assert counts(ro, 2) == (5004, 3, 9, 8 * T + 7, 2 * (8 * T + 7))
    assert {1, 2, 3, 9} <= set(KS)
    check_edge(cfg, sa.dCSR.from_host(H), dtype)


# ---------------------------------------------------------------------------------------------------- 2: column c is spmv
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_column_is_spmv_bit_for_bit_and_two_calls_give_the_same_bytes(cfg, dtype):
    H, X, _, _ = real_case(dtype)
    dA = sa.dCSR.from_host(H)
    rng = np.random.default_rng(40)
    Y0 = rng.choice([-1.0, 1.0], size=(H.rows, REAL_K)) * (0.5 + rng.random((H.rows, REAL_K)))
    for alpha, beta in ((1.0, 0.0), (-1.7, 0.9)):
        got, info = run(cfg, dA, X, alpha, beta, Y0 if beta else None)
        again, _ = run(cfg, dA, X, alpha, beta, Y0 if beta else None)
        assert bits(got).tobytes() == bits(again).tobytes()
        check_info(info, H.row_offsets, REAL_K)
        assert not np.isnan(got).any()
        for c in range(REAL_K):
            y = tv(Y0[:, c])
            sa.spmv(dA, tv(X[:, c]), cfg, alpha=alpha, beta=beta, y=y)
            col = host(y)
            assert bits(got[:, c]).tobytes() == bits(col).tobytes(), (alpha, beta, c, np.nonzero(bits(got[:, c]) != bits(col))[0][:8])


# ---------------------------------------------------------------------------------------------------- 3: views
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_writes_the_rows_of_the_whole_at_y_plus_r0_ldy(cfg, dtype):
    H, X, _, _ = real_case(dtype)
    k, ldy = 3, 5
    ro = H.row_offsets.astype(np.int64)
    dA = sa.dCSR.from_host(H)
    whole, _ = run(cfg, dA, X[:, :k], ldy=ldy)
    r_odd = next(r for r in range(1, H.rows) if ro[r] % 2 == 1 and ro[r] % T != T - 1 and ro[r + 1] > ro[r])
    r_tile = next(r for r in range(1, H.rows) if ro[r] % T == 0 and ro[r] > 0 and ro[r + 1] > ro[r])
    r_last = next(r for r in range(1, H.rows) if ro[r] % T == T - 1 and ro[r + 1] > ro[r])
    r_mid = next(r for r in range(H.rows - 1, 0, -1) if ro[r] % T and ro[r] // T > ro[r_odd] // T + 2)
    _, xs = frame(COLS, k + 3, k, X[:, :k])
    for a, b in ((r_odd, H.rows), (r_tile, H.rows), (r_last, H.rows), (r_odd, r_mid), (r_tile, r_mid), (0, r_mid)):
        yb, ys = frame(H.rows, ldy, k)                                             # the frame of the WHOLE result
        assert ys[a:b].data_ptr() == ys.data_ptr() + 8 * a * ldy
        _, info = sa.spmm(dA.row_view(a, b), xs, cfg, Y=ys[a:b])
        got = read_frame(yb, H.rows, ldy, k)
        assert bits(got[a:b]).tobytes() == bits(whole[a:b]).tobytes(), (a, b)
        assert (bits(got[:a]) == SENTINEL_BITS).all() and (bits(got[b:]) == SENTINEL_BITS).all(), (a, b)
        check_info(info, ro[a:b + 1], k)


# ---------------------------------------------------------------------------------------------------- 4: the bound
def allowance(n, mag):
    n = np.asarray(n, dtype=np.float64)[:, None]
    return (n * U / (1.0 - n * U) + U) * mag


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_values_within_the_bound_of_any_order(cfg, dtype):
    H, X, want, mags = real_case(dtype)
    ro = H.row_offsets.astype(np.int64)
    got, _ = run(cfg, sa.dCSR.from_host(H), X[:, :3])
    err = np.abs(got - want)
    print("largest error / allowance:", float(np.max(err / np.maximum(allowance(ro[1:] - ro[:-1], mags), 1e-300))))
    ok = err <= allowance(ro[1:] - ro[:-1], mags)
    assert ok.all(), (np.argwhere(~ok)[:8], err[~ok][:8])


# ---------------------------------------------------------------------------------------------------- 5: special values
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_land_in_their_column_of_the_rows_that_reference_them(cfg, dtype):
    lens = [3, 2, 0, 5, 2 * T + 10, 4, 1, 6]
    ro = np.concatenate([[0], np.cumsum(lens)])
    n = int(ro[-1])
    rng = np.random.default_rng(70)
    data = rng.integers(1, 100, size=n).astype(dtype)
    col = rng.integers(10, 50, size=n).astype(np.uint32)                           # nobody references 7 or 9 by chance
    X = ints((50, 3), 71)
    X[7, 1], X[9, 2] = np.nan, np.inf                                              # ONE element each
    col[ro[0] + 1] = 7                                                             # row 0: the NaN, in column 1
    col[ro[1]] = 9
    data[ro[1]] = 0.0                                                              # row 1: 0 * inf, in column 2
    col[ro[3] + 4] = 9                                                             # row 3: 12 * inf = inf in column 2, no NaN
    data[ro[3] + 4] = 12
    col[ro[4] + T + T // 2] = 7                                                    # row 4, split over three tiles: the NaN in a tile inside
    H = sa.HostCSR(len(lens), 50, ro.astype(np.uint32), col, data)
    dA = sa.dCSR.from_host(H)
    got, _ = run(cfg, dA, X)
    want = row_sums(H, X)
    assert np.argwhere(np.isnan(want)).tolist() == [[0, 1], [1, 2], [4, 1]] and want[3, 2] == np.inf
    assert np.isfinite(want[:, 0]).all() and np.isinf(want).sum() == 1
    assert same(got, want), (got[:8], want[:8])

    # beta = 0: Y held the payload NaN in every word and is not read
    clean = ints((50, 3), 72)
    got, _ = run(cfg, dA, clean, 1.0, 0.0, None)
    assert not np.isnan(got).any() and np.array_equal(got, row_sums(H, clean))
    # beta = 1: a NaN of Y0 stays in its element
    Y0 = ints((H.rows, 3), 73)
    at = [(0, 2), (2, 0), (4, 1), (7, 2)]                                          # (row 2 holds no entry, row 4 is split)
    for i, c in at:
        Y0[i, c] = np.nan
    got, _ = run(cfg, dA, clean, 1.0, 1.0, Y0)
    assert [tuple(p) for p in np.argwhere(np.isnan(got)).tolist()] == at
    assert same(got, row_sums(H, clean) + Y0)


# ---------------------------------------------------------------------------------------------------- 6: hostile input
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
    H, X, S = edge_case(dtype)
    k, ldx, ldy = 3, 6, 5
    good = sa.dCSR.from_host(H)
    _, xs = frame(COLS, ldx, k, X[:, :k])
    L = _lib.load()
    fn = L.speck_spmm_f32 if dtype == np.float32 else L.speck_spmm_f64
    Y0 = ints((H.rows, k), 16)
    cases = list(hostile(H))
    assert len(cases) == 15
    for n, (ro, col, nnz, a, b) in enumerate(cases):
        dA = on_torch(H, ro=ro, col=col, nnz=nnz, r0=a, r1=b)
        yb, ys = frame(b - a, ldy, k)
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)
        alpha, beta = COEFFS[n % 2]
        torch.cuda.synchronize()
        rc = fn(cfg._h, alpha, C_.byref(dA._c), xs.data_ptr(), ldx, k, beta, ys.data_ptr(), ldy, C_.byref(info))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, n
        assert (bits(host(yb)) == SENTINEL_BITS).all(), n          # every word, padding included
        assert as_tuple(info) == (0, 0, 0, 0, 0), n
        got, _ = run(cfg, good, X[:, :k], 2.0, -3.0, Y0)           # the config serves a valid call right after
        assert np.array_equal(got, 2.0 * S[:, :k] - 3.0 * Y0), n


# ---------------------------------------------------------------------------------------------------- 7: alignment
@pytest.mark.parametrize("dtype", DTYPES)
def test_arrays_and_blocks_off_the_16_byte_boundary(cfg, dtype):
    H, _, _ = edge_case(dtype)
    dA = on_torch(H, shift=1)
    assert dA._c.data % 16 and dA._c.col_ids % 16
    check_edge(cfg, dA, dtype, ks=(2, 3))                                          # data and col_ids advanced by one element
    good = sa.dCSR.from_host(H)
    assert frame(COLS, 5, 2, lead=1)[1].data_ptr() % 16 == 8
    check_edge(cfg, good, dtype, ks=(2, 5), ldx=7, x_lead=1)                       # X one double off, rows an odd number apart
    assert frame(COLS, 8, 2)[1].data_ptr() % 16 == 0
    check_edge(cfg, good, dtype, ks=(2, 5), ldx=8, ldy=6)                          # X on 16 bytes, rows an even number apart


# ---------------------------------------------------------------------------------------------------- 8: degenerate
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_shapes(cfg, dtype):
    X = ints((COLS, 2), 17)
    _, xs = frame(COLS, 5, 2, X)
    H, _, _ = edge_case(dtype)
    # k == 0: nothing is written, info is zero
    yb, ys = frame(H.rows, 4, 2)
    out, info = sa.spmm(sa.dCSR.from_host(H), xs.data_ptr(), cfg, alpha=2.0, Y=ys.data_ptr(), k=0, ldx=5, ldy=4)
    assert out is None and (bits(host(yb)) == SENTINEL_BITS).all() and as_tuple(info) == (0, 0, 0, 0, 0)
    # no row: nothing is written
    none = sa.HostCSR(0, COLS, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))
    out, info = sa.spmm(sa.dCSR.from_host(none), xs, cfg, alpha=2.0, Y=ys.data_ptr(), ldy=4)
    assert out is None and (bits(host(yb)) == SENTINEL_BITS).all() and as_tuple(info) == (0, 0, 0, 0, 0)
    # no entry: Y = alpha (+0.0) + beta Y, signed zeros included
    hollow = mk([0] * 5, np.zeros(0, dtype=dtype))
    Y0 = np.array([[1.0, -0.0], [-2.0, 0.0], [0.0, -0.0], [4.5, 1e-300], [-0.0, -7.0]])
    got, info = run(cfg, sa.dCSR.from_host(hollow), X, 3.0, 2.0, Y0)
    assert bits(got).tobytes() == bits(3.0 * 0.0 + 2.0 * Y0).tobytes()
    check_info(info, hollow.row_offsets, 2)
    # rows without entries only, more than a workgroup's: +0.0, whatever Y held
    hollow = mk([0] * 3000, np.zeros(0, dtype=dtype))
    got, info = run(cfg, sa.dCSR.from_host(hollow), X)
    assert (bits(got) == 0).all()
    check_info(info, hollow.row_offsets, 2)
    # one row of 3T + 1 entries; 70 000 rows of one entry: more rows than any tile has entries
    for lens in ([3 * T + 1], [1] * 70000):
        M = mk(lens, ints(sum(lens), 18, dtype), seed=19)
        got, info = run(cfg, sa.dCSR.from_host(M), X)
        assert np.array_equal(got, row_sums(M, X)), len(lens)
        check_info(info, M.row_offsets, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_most_right_hand_sides_and_one_more(cfg, dtype):
    k = sa.SPMM_MAX_RHS
    M = mk([2, 0, 3], ints(5, 20, dtype), cols=7, seed=21)
    dA = sa.dCSR.from_host(M)
    X = ints((7, k + 1), 22)
    Y0 = ints((3, k), 23)
    got, info = run(cfg, dA, X[:, :k], 2.0, -3.0, Y0)
    assert np.array_equal(got, 2.0 * row_sums(M, X[:, :k]) - 3.0 * Y0)
    check_info(info, M.row_offsets, k)
    _, xs = frame(7, k + 1, k + 1, X)
    yb, ys = frame(3, k + 1, k + 1)
    with pytest.raises(sa.SpeckError) as e:
        sa.spmm(dA, xs, cfg, Y=ys)
    assert e.value.status == ERR_DIM_LIMIT
    assert (bits(host(yb)) == SENTINEL_BITS).all()


# ---------------------------------------------------------------------------------------------------- 9: plumbing
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_config_a_result_of_the_librarys_own_raw_addresses_and_a_column_slice(cfg, dtype):
    H, X, S = edge_case(dtype)
    dA = sa.dCSR.from_host(H)
    check_edge(None, dA, dtype, ks=(3,))
    k = 5
    Z = torch.from_numpy(ints((COLS, 8), 24)).to(DEV)
    Z[:, 2:7].copy_(torch.from_numpy(X[:, :k].copy()).to(DEV))
    for c in (None, cfg):
        out, info = sa.spmm(dA, Z[:, 2:7], c, alpha=-2.0)                          # Y=None: downloaded; X a column slice
        assert out.shape == (H.rows, k) and np.array_equal(out, -2.0 * S[:, :k])
        check_info(info, H.row_offsets, k)
        yb, ys = frame(H.rows, 9, k)                                               # raw addresses with k and ld
        out, _ = sa.spmm(dA, Z.data_ptr() + 16, c, Y=ys.data_ptr(), k=k, ldx=8, ldy=9)
        assert out is None and np.array_equal(read_frame(yb, H.rows, 9, k), S[:, :k])
        out, _ = sa.spmm(dA, torch.from_numpy(X[:, :2].copy()).to(DEV), c)         # contiguous: ld = k
        assert np.array_equal(out, S[:, :2])


def test_x_and_y_side_by_side_in_one_buffer(cfg):
    """two spans that touch share no byte: Y right behind X's last element and right in front of X are served, one element
    closer is refused with nothing written"""
    H, X, S = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    k, ldx, ldy = 3, 5, 4
    x_span, y_span = (COLS - 1) * ldx + k, (H.rows - 1) * ldy + k

    def layout(x_at, y_at):
        buf, _ = frame(x_span + y_span, 1, 1)
        xs = torch.as_strided(buf, (COLS, k), (ldx, 1), x_at)
        xs.copy_(torch.from_numpy(X[:, :k].copy()).to(DEV))
        return buf, buf.data_ptr() + 8 * x_at, buf.data_ptr() + 8 * y_at

    for x_at, y_at in ((0, x_span), (y_span, 0)):
        buf, px, py = layout(x_at, y_at)
        sa.spmm(dA, px, cfg, Y=py, k=k, ldx=ldx, ldy=ldy)
        full = host(buf)
        assert np.array_equal(torch.as_strided(torch.from_numpy(full), (H.rows, k), (ldy, 1), y_at).numpy(), S[:, :k])
        assert np.array_equal(torch.as_strided(torch.from_numpy(full), (COLS, k), (ldx, 1), x_at).numpy(), X[:, :k])
    for x_at, y_at in ((0, x_span - 1), (y_span - 1, 0)):
        buf, px, py = layout(x_at, y_at)
        before = bits(host(buf)).copy()
        with pytest.raises(sa.SpeckError) as e:
            sa.spmm(dA, px, cfg, Y=py, k=k, ldx=ldx, ldy=ldy)
        assert e.value.status == ERR_INVALID
        assert np.array_equal(bits(host(buf)), before)


def test_wrong_blocks_are_refused_in_python(cfg):
    H, X, _ = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    dX = torch.from_numpy(X[:, :4].copy()).to(DEV)
    Y = torch.zeros((H.rows, 4), dtype=torch.float64, device=DEV)
    for bad in (dX.float(), dX[:-1], dX.t().contiguous().t(), dX[:, ::2], dX[:, 0]):
        with pytest.raises(ValueError, match="spmm: X"):
            sa.spmm(dA, bad, cfg)
    for bad in (Y.float(), Y[1:], Y[:, :3], Y.t().contiguous().t()):
        with pytest.raises(ValueError, match="spmm: Y"):
            sa.spmm(dA, dX, cfg, Y=bad)
    with pytest.raises(ValueError):
        sa.spmm(dA, dX, cfg, beta=1.0)                                             # nothing to read
    assert not host(Y).any()


def test_runs_on_the_callers_stream(cfg):
    """X is written by a copy on the caller's stream right before the call: ordering against the producer is by the
    stream alone"""
    H, X, S = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    real, dX = torch.from_numpy(X[:, :3].copy()).to(DEV), torch.zeros((COLS, 3), dtype=torch.float64, device=DEV)
    yb, ys = frame(H.rows, 4, 3)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream multiplies zeros
            dX.copy_(real, non_blocking=True)
        sa.spmm(dA, dX, cfg, Y=ys)
        assert np.array_equal(read_frame(yb, H.rows, 4, 3), S[:, :3])
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        check_edge(cfg, sa.dCSR.from_host(edge_case(dtype)[0]), dtype, ks=(1, 3, 9))   # (a touched zone is status 3)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_a_spmm_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.08, 7, signed=True)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()
    for _ in range(3):
        sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"]
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1
    X = real_values((h.cols, 3), 21)
    dX = torch.from_numpy(X).to(DEV)
    out, _ = sa.spmm(dS, dX, cfg)
    ro = h.row_offsets.astype(np.int64)
    for c in range(3):
        t = terms(h, X[:, c])
        want = np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])])
        mags = np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])])
        assert (np.abs(out[:, c] - want) <= allowance(ro[1:] - ro[:-1], mags[:, None])[:, 0]).all(), c
    sa.spmm(dC, dX, cfg)                                                           # ... and of the product itself, where it lies
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1


# ---------------------------------------------------------------------------------------------------- 10: a block power iteration
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_block_power_iteration_stays_on_the_device(cfg, dtype):
    n, k = 2000, 4
    S = sp.random(n, n, density=6 / n, random_state=120, format="csr")
    S.sort_indices()
    G = ((S + S.T) != 0).astype(np.float64).tocsr()
    deg = np.asarray(G.sum(axis=1)).ravel()
    assert 0 < deg.max() <= 100
    P = sp.diags(1.0 / np.maximum(deg, 1.0)).dot(G).tocsr()                        # (1 / deg is one rounding, as on the device)
    P.data = P.data.astype(dtype).astype(np.float64)
    X0 = 1.0 + np.random.default_rng(121).random((n, k))
    ref = X0 / np.linalg.norm(X0, axis=0)
    for _ in range(10):
        ref = P @ ref
        ref = ref / np.linalg.norm(ref, axis=0)

    HS = sa.HostCSR(n, n, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.astype(dtype))
    dP, _ = sa.normalize_rows(sa.pattern_ones(sa.symmetrize(sa.dCSR.from_host(HS), cfg), cfg), cfg)
    X = torch.from_numpy(X0.copy()).to(DEV)
    Y = torch.empty_like(X)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)                                             # torch's normalisation and the product: one queue
    try:
        with torch.cuda.stream(stream):
            X /= torch.linalg.vector_norm(X, dim=0)
            for _ in range(10):
                sa.spmm(dP, X, cfg, Y=Y)
                torch.div(Y, torch.linalg.vector_norm(Y, dim=0), out=X)
            got = host(X)
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()
    rel = float(np.max(np.abs(got - ref) / np.max(np.abs(ref), axis=0)))
    rel2 = float(np.max(np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)))
    print("relative difference after ten steps (max, 2-norm; the worst column):", rel, rel2)
    assert rel <= 1e-12 and rel2 <= 1e-12
