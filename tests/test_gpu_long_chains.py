"""Rows that span many entry tiles, and matrices of many tiles, through speck_reduce_*, speck_spmv_* and speck_spmm_*
(speck_amd/csrc/tile_combine.hpp: chain_finish, totals_finish; spmm.hip: spmm_finish_kernel).  chain_finish gives lane l of a
wave the whole tiles i+1+l, i+1+l+64, ... inside a row: with fewer than 65 of them its second trip never runs, with fewer
than 64 most lanes carry the identity.  totals_finish walks the tile records 256 at a time.  spmm_finish_kernel finds
(tile, column) of a wave by a division by max_tiles.  The shapes here put rows of 0, 1, 63, 64, 65, 128 and 129 whole tiles
between the tile they start and the tile they end in, and matrices of exactly 256, 257, 512 and 513 tiles.

The expectation is numpy / math.fsum, through the helpers of test_gpu_reduce.py, test_gpu_spmv.py and test_gpu_spmm.py:
integer values in [-1024, 1024] so that every order of summation gives the same bits and the comparison is equality; for
real values the bound of any order, (g_n + 2^-53) sum|t|.  T = 4096 entries per tile below."""
import math
import struct

import numpy as np
import pytest

import speck_amd as sa
import test_gpu_reduce as R
import test_gpu_spmm as M
import test_gpu_spmv as V
from test_gpu_reduce import cfg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
T = sa.REDUCE_TILE_ENTRIES
assert T == sa.SPMV_TILE_ENTRIES
CB = sa.SPMM_COLUMN_BLOCK
OPS, SUMS = R.OPS, R.SUMS
COLS = V.COLS
MIDDLE = [0, 1, 63, 64, 65, 128, 129]           # whole tiles inside a long row: it touches two more
ENDS = [1001, 2049, 777, 3001, 3585, 15, 2501]   # where in its last tile each long row ends (odd)
SPMM_KS = [1, 3, CB + 1]
K_MAX = max(SPMM_KS)

_CACHE = {}


# ---------------------------------------------------------------------------------------------------- the shapes
def chain_lens():
    """(row lengths, the indices of the long rows): short rows of 0..60 entries, some empty, in front of, between and
    behind seven long rows; a long row starts at an odd position inside a tile and ends at an odd position ENDS[i] of the
    tile MIDDLE[i] + 1 further on"""
    rng = np.random.default_rng(77)
    lens, long_rows, pos = [], [], 0
    for mid, end in zip(MIDDLE, ENDS):
        short = [int(v) for v in rng.integers(0, 61, size=30)]
        short[3] = short[17] = 0
        lens += short
        pos += sum(short)
        if pos % 2 == 0:
            lens.append(7)
            pos += 7
        stop = (pos // T + mid + 1) * T + end
        long_rows.append(len(lens))
        lens.append(stop - pos)
        pos = stop
    short = [int(v) for v in rng.integers(0, 61, size=80)]   # (so many that the tile kernel's grid, max_tiles, is odd)
    short[5] = 0
    return lens + short, long_rows


def check_chain_premise(ro, long_rows):
    """the constructed offsets have the tile counts this file is about"""
    ro = np.asarray(ro, dtype=np.int64)
    touched = [int((ro[r + 1] - 1) // T - ro[r] // T + 1) for r in long_rows]
    assert touched == [2, 3, 65, 66, 67, 130, 131], touched
    s, e = ro[:-1], ro[1:]
    for r in long_rows:
        assert ro[r] % T % 2 == 1 and ro[r + 1] % T % 2 == 1, r                    # starts and ends mid-tile, at an odd position
        first, last = ro[r] // T, (ro[r + 1] - 1) // T
        whole = (e > s) & (s // T == (e - 1) // T)                                 # rows that lie in one tile
        assert (whole & (s // T == first)).any() and (whole & (s // T == last)).any(), r
    assert (e == s).sum() >= 15 and 1_850_000 < ro[-1] < 1_950_000 and ro[-1] % T


def chain_case(dtype, real=False):
    """(H, long rows, x, X of K_MAX columns), once per value type: the chain-length matrix with integer or real values"""
    key = ("chain", np.dtype(dtype).name, real)
    if key not in _CACHE:
        lens, long_rows = chain_lens()
        n = sum(lens)
        if real:
            H = V.mk(lens, V.real_values(n, 6, dtype), seed=7)
            X = M.real_values((COLS, K_MAX), 8)
        else:
            H = V.mk(lens, V.ints(n, 11, dtype), seed=12)
            X = M.ints((COLS, K_MAX), 13)
            for c in range(K_MAX):
                assert np.abs(V.terms(H, X[:, c])).sum() < 2.0 ** 53
        check_chain_premise(H.row_offsets, long_rows)
        x = np.ascontiguousarray(X[:, 0])
        for a in (H.row_offsets, H.col_ids, H.data, x, X):
            a.setflags(write=False)
        _CACHE[key] = (H, long_rows, x, X)
    return _CACHE[key]


def tiles_case(dtype, tiles):
    """a matrix that touches exactly `tiles` tiles, the last one in part: rows of about 100 entries"""
    key = ("tiles", np.dtype(dtype).name, tiles)
    if key not in _CACHE:
        rng = np.random.default_rng(tiles)
        nnz = (tiles - 1) * T + 1234
        lens = rng.integers(90, 111, size=nnz // 90 + 1)
        lens = lens[:int(np.searchsorted(np.cumsum(lens), nnz))].tolist()
        lens.append(nnz - sum(lens))
        H = V.mk(lens, V.ints(nnz, 20 + tiles, dtype), seed=21)
        x = V.ints(COLS, 22)
        assert 0 < lens[-1] <= 110 and R.counts(H.row_offsets)["tiles"] == tiles and nnz % T
        for a in (H.row_offsets, H.col_ids, H.data, x):
            a.setflags(write=False)
        _CACHE[key] = (H, x)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- 1: chain lengths, exact
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_of_rows_with_up_to_129_whole_tiles_inside(cfg, dtype):
    H, _, _, _ = chain_case(dtype)
    assert R.counts(H.row_offsets)["rows_split"] >= 7
    R.check_exact(cfg, H)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmv_of_rows_with_up_to_129_whole_tiles_inside(cfg, dtype):
    H, _, x, _ = chain_case(dtype)
    dA, dx = sa.dCSR.from_host(H), V.tv(x)
    s = V.row_sums(H, x)
    y0 = V.ints(H.rows, 14)
    for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
        got, info = V.run(cfg, dA, dx, alpha, beta, y0 if beta else None)
        want = alpha * s + beta * y0 if beta else alpha * s
        assert np.array_equal(got, want), (alpha, beta, np.nonzero(got != want)[0][:8])
        V.check_info(info, H.row_offsets)


@pytest.mark.parametrize("k", SPMM_KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_of_rows_with_up_to_129_whole_tiles_inside(cfg, dtype, k):
    """max_tiles k is no multiple of the waves of a workgroup for k = 1 and 3, and k = CB + 1 leaves one column alone
    behind a block, k = 3 one behind a pair; padded ldx = k + 3, ldy = k + 2 inside payload-NaN frames"""
    H, _, _, X = chain_case(dtype)
    max_tiles = -(-H.nnz // T) + 1                                                 # entry_tiles_at_most of entry_tiles.hpp
    assert max_tiles % 2 == 1 and (max_tiles * k) % 4
    dA = sa.dCSR.from_host(H)
    S = M.row_sums(H, X[:, :k])
    Y0 = M.ints((H.rows, k), 15)
    for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
        got, info = M.run(cfg, dA, X[:, :k], alpha, beta, Y0 if beta else None)
        want = alpha * S + beta * Y0 if beta else alpha * S
        assert np.array_equal(got, want), (k, alpha, beta, np.argwhere(got != want)[:8])
        M.check_info(info, H.row_offsets, k)
        for c in range(k):                                                         # every column is spmv of that column
            col, _ = V.run(cfg, dA, V.tv(X[:, c]), alpha, beta, Y0[:, c] if beta else None)
            assert V.bits(got[:, c]).tobytes() == V.bits(col).tobytes(), (k, c)


# ---------------------------------------------------------------------------------------------------- 2: tile counts of the totals
@pytest.mark.parametrize("tiles", [256, 257, 512, 513])
@pytest.mark.parametrize("dtype", DTYPES)
def test_totals_over_256_257_512_and_513_tiles(cfg, dtype, tiles):
    H, x = tiles_case(dtype, tiles)
    want = R.counts(H.row_offsets)
    assert want["tiles"] == tiles and want["rows_split"] > 0.95 * tiles            # (nearly every tile edge cuts a row)
    dA = R.check_exact(cfg, H)                                                     # every op: rows, total, info
    got, info = V.run(cfg, dA, V.tv(x))
    assert np.array_equal(got, V.row_sums(H, x))
    assert (info.rows_split, info.tiles) == (want["rows_split"], tiles)
    X = np.ascontiguousarray(np.stack([x, x[::-1], -x], axis=1))
    got, info = M.run(cfg, dA, X)
    assert np.array_equal(got, M.row_sums(H, X))
    assert (info.rows_split, info.tiles) == (want["rows_split"], tiles)


# ---------------------------------------------------------------------------------------------------- 3: views
def chain_views(H, long_rows):
    """(a, b): from the 131-tile row to the end -- the view's first tile is not tile 0, t_first > 0 in chain_finish --,
    from the start to where the 67-tile row begins, and from the 66-tile row to the end of the 130-tile row"""
    ro = H.row_offsets.astype(np.int64)
    views = [(long_rows[6], H.rows), (0, long_rows[4]), (long_rows[3], long_rows[5] + 1)]
    assert ro[views[0][0]] // T > 300 and ro[views[0][0]] % T
    assert ro[views[1][1]] % T and ro[views[1][1]] < ro[-1] // 2
    assert ro[views[2][0]] // T > 0 and ro[views[2][1]] % T
    return views


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_into_the_chain_matrix_gives_the_rows_of_the_whole(cfg, dtype):
    H, long_rows, x, X = chain_case(dtype, real=True)
    ro = H.row_offsets.astype(np.int64)
    dA, dx = sa.dCSR.from_host(H), V.tv(x)
    k, ldy = 3, 5
    _, xs = M.frame(COLS, k + 3, k, X[:, :k])
    whole_r = {op: sa.reduce(dA, cfg, op)[0] for op in OPS}
    whole_v, _ = V.run(cfg, dA, dx)
    whole_m, _ = M.run(cfg, dA, X[:, :k], ldy=ldy)
    for a, b in chain_views(H, long_rows):
        view = dA.row_view(a, b)
        for op in OPS:
            rows, total, info = sa.reduce(view, cfg, op)
            assert rows.view(np.uint64).tobytes() == whole_r[op][a:b].view(np.uint64).tobytes(), (op, a, b)
            R.check_info(info, ro[a:b + 1])
            t = R.terms_of(H.data[ro[a]:ro[b]], op)
            if op in SUMS:
                assert abs(total - math.fsum(t)) <= R.allowance(len(t), math.fsum(np.abs(t))), (op, a, b)
            else:
                assert R.same(total, R.ref_exact([0, len(t)], H.data[ro[a]:ro[b]], op)[1]), (op, a, b)
        got, info = V.run(cfg, view, dx)
        assert V.bits(got).tobytes() == V.bits(whole_v[a:b]).tobytes(), (a, b)
        V.check_info(info, ro[a:b + 1])
        yb, ys = M.frame(H.rows, ldy, k)                                           # the frame of the WHOLE result
        _, info = sa.spmm(view, xs, cfg, Y=ys[a:b])
        got = M.read_frame(yb, H.rows, ldy, k)
        assert M.bits(got[a:b]).tobytes() == M.bits(whole_m[a:b]).tobytes(), (a, b)
        assert (M.bits(got[:a]) == M.SENTINEL_BITS).all() and (M.bits(got[b:]) == M.SENTINEL_BITS).all(), (a, b)
        M.check_info(info, ro[a:b + 1], k)


# ---------------------------------------------------------------------------------------------------- 4: real values
def fsum_rows(t, ro):
    return (np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])]),
            np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_values_within_the_bound_of_any_order_and_reproducible(cfg, dtype):
    H, _, x, X = chain_case(dtype, real=True)
    ro = H.row_offsets.astype(np.int64)
    n = ro[1:] - ro[:-1]
    dA = sa.dCSR.from_host(H)
    for op in OPS:
        rows, total, info = sa.reduce(dA, cfg, op)
        again, total2, _ = sa.reduce(dA, cfg, op)
        assert rows.view(np.uint64).tobytes() == again.view(np.uint64).tobytes(), op
        assert struct.pack("<d", total) == struct.pack("<d", total2), op
        R.check_info(info, ro)
        t = R.terms_of(H.data, op)
        if op in SUMS:
            want, mags = fsum_rows(t, ro)
            ok = np.abs(rows - want) <= R.allowance(n, mags)
            assert ok.all(), (op, np.nonzero(~ok)[0][:8])
            assert abs(total - math.fsum(t)) <= R.allowance(len(t), math.fsum(np.abs(t))), (op, total)
        else:
            want_rows, want_total = R.ref_exact(ro, H.data, op)
            assert R.same(rows, want_rows) and R.same(total, want_total), op
    k = 3
    got, _ = M.run(cfg, dA, X[:, :k])
    again, _ = M.run(cfg, dA, X[:, :k])
    assert M.bits(got).tobytes() == M.bits(again).tobytes()
    for c in range(k):
        want, mags = fsum_rows(V.terms(H, X[:, c]), ro)
        col, _ = V.run(cfg, dA, V.tv(X[:, c]))
        col2, _ = V.run(cfg, dA, V.tv(X[:, c]))
        assert V.bits(col).tobytes() == V.bits(col2).tobytes(), c
        ok = np.abs(col - want) <= V.allowance(n, mags)
        assert ok.all(), (c, np.nonzero(~ok)[0][:8])
        assert M.bits(got[:, c]).tobytes() == V.bits(col).tobytes(), c            # (so spmm is within the bound too)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_in_a_middle_tile_of_the_131_tile_row_comes_out_of_that_row_alone(cfg, dtype):
    H, long_rows, _, _ = chain_case(dtype, real=True)
    ro = H.row_offsets.astype(np.int64)
    r = long_rows[6]
    at = int(ro[r]) + 70 * T + 123                                                 # a lane's second trip: whole tile 69 or 70 of the row
    tile = at // T - ro[r] // T
    assert 65 <= tile - 1 < 129 and at // T < (ro[r + 1] - 1) // T
    data = H.data.copy()
    data[at] = np.nan
    Hn = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, data)
    dA = sa.dCSR.from_host(Hn)
    for op in OPS:
        rows, total, _ = sa.reduce(dA, cfg, op)
        assert np.nonzero(np.isnan(rows))[0].tolist() == [r] and math.isnan(total), op
        if op not in SUMS:
            assert R.same(rows, R.ref_exact(ro, data, op)[0]), op
    clean = {op: sa.reduce(sa.dCSR.from_host(H), cfg, op)[0] for op in SUMS}      # a sum: every other row as without the NaN
    for op in SUMS:
        rows, _, _ = sa.reduce(dA, cfg, op)
        keep = np.arange(H.rows) != r
        assert rows[keep].view(np.uint64).tobytes() == clean[op][keep].view(np.uint64).tobytes(), op
