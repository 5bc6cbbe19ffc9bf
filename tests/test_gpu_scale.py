"""speck_scale_* on the GPU (speck_amd/csrc/scale.hip).  The expectation is numpy in this file:
    (((alpha * g(a.astype(f64))) (.) l[row]) (.) r[col]).astype(T)
There is no summation, so EVERY comparison of values is equality: the bits where the expectation is not a NaN, a NaN where
it is one.  T = 4096 entries per tile below."""
import ctypes as C_
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
DTYPES = [np.float64, np.float32]
MAPS = ["identity", "abs", "square", "one"]
MODES = [None, "mul", "div"]
T = sa.SCALE_TILE_ENTRIES
U = 2.0 ** -53
DEV = "cuda:0"
COLS = 777


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def edge_lens():
    """(row lengths) laid out against the tile edges -- the layout of the reduction's tests, and a block of T rows of one
    entry behind it; the comments give the entries a row holds"""
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
             2]                # [8T + 5, 8T + 7)
            + [1] * T +        # [8T + 7, 9T + 7): T rows of one entry, a tile's worth
            [0])               # an empty last row
LONG_ROW, SHORT_ROW, FIRST_EMPTY = 9, 10, 14   # the row over four tiles, the 99 entries behind it, the 5000 empty rows


def real_values(n, seed, dtype):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.random(n)) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(dtype)


def vector(n, seed):
    """random reals of mixed sign, none of them zero"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=n) * (0.1 + rng.random(n)) * 10.0 ** rng.uniform(-1, 1, size=n)


def mk(lens, data, cols=COLS, seed=1):
    """rows of the given lengths over `data`; random column ids below cols: unsorted, with duplicates"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = np.random.default_rng(seed).integers(0, cols, size=len(data)).astype(np.uint32)
    return sa.HostCSR(len(lens), cols, ro, ci, np.asarray(data))


_EDGE = {}


def edge_matrix(dtype):
    key = np.dtype(dtype).name
    if key not in _EDGE:
        lens = edge_lens()
        H = mk(lens, real_values(sum(lens), 11, dtype))
        _EDGE[key] = (H, vector(H.rows, 12), vector(H.cols, 13))
    return _EDGE[key]


def expected(data, rows_of, cols_of, dtype, alpha=1.0, map="identity", l=None, row=None, r=None, col=None):
    """the chain of the contract in numpy; rows_of / cols_of: the row (inside the matrix) and the column of every entry"""
    with np.errstate(all="ignore"):
        x = np.asarray(data).astype(np.float64)
        x = np.abs(x) if map == "abs" else x * x if map == "square" else np.ones_like(x) if map == "one" else x
        x = np.float64(alpha) * x
        if row == "mul":
            x = x * l[rows_of]
        elif row == "div":
            x = x / l[rows_of]
        if col == "mul":
            x = x * r[cols_of]
        elif col == "div":
            x = x / r[cols_of]
        return x.astype(dtype)


def rows_of(ro):
    ro = np.asarray(ro, dtype=np.int64)
    return np.repeat(np.arange(len(ro) - 1), ro[1:] - ro[:-1])


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        got[~nan].tobytes() == want[~nan].tobytes()


def first_difference(got, want):
    bad = ~((got.view(np.uint8).reshape(len(got), -1) == want.view(np.uint8).reshape(len(want), -1)).all(axis=1)
            | (np.isnan(got) & np.isnan(want)))
    i = np.nonzero(bad)[0]
    return (len(i), i[:6], got[i[:6]], want[i[:6]])


def tiles_of(ro, with_rows):
    ro = np.asarray(ro, dtype=np.int64)
    return int((ro[-1] - 1) // T - ro[0] // T + 1) if with_rows and ro[-1] > ro[0] else 0


def check_info(info, want, ro, with_rows):
    assert (info.entries, info.nonfinite, info.tiles) == (len(want), int((~np.isfinite(want)).sum()), tiles_of(ro, with_rows)), info


def dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(DEV)


def call(A, cfg, l_t, r_t, row, col, **kw):
    return sa.scale(A, cfg, row=l_t if row else None, col=r_t if col else None, row_div=row == "div", col_div=col == "div", **kw)


def on_torch(H, ro=None, ci=None, nnz=None):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz"""
    pad = 8   # (a declared nnz beyond the entries is looked at before it is refused: it stays inside the tensors)
    t_ro = torch.from_numpy(np.ascontiguousarray(H.row_offsets if ro is None else ro).view(np.int32).copy()).to(DEV)
    t_ci = torch.from_numpy(np.concatenate([H.col_ids if ci is None else ci, np.zeros(pad, np.uint32)]).view(np.int32)).to(DEV)
    t_va = torch.from_numpy(np.concatenate([H.data, np.zeros(pad, H.data.dtype)])).to(DEV)
    return sa.dCSR.from_device(H.rows, H.cols, H.nnz if nnz is None else nnz, t_ro.data_ptr(), t_ci.data_ptr(), t_va.data_ptr(),
                               dtype=H.data.dtype, keep=(t_ro, t_ci, t_va))


def values_of(dA):
    """the entries of an on_torch matrix as they are on the device now"""
    return dA._keep[2].cpu().numpy()[:-8]


# ---------------------------------------------------------------------------------------------------- 1: tile edges
def test_the_layout_meets_every_tile_edge():
    ro = np.concatenate([[0], np.cumsum(edge_lens())])
    assert {T - 1, 0, 1} <= set((ro % T).tolist()) and T in ro and 2 * T in ro and 8 * T in ro
    assert ro[LONG_ROW] == 3 * T - 1 and ro[LONG_ROW + 1] == 5 * T + 1 and ro[FIRST_EMPTY] == ro[FIRST_EMPTY + 5000] == 8 * T
    assert ro[-1] == 9 * T + 7 and (np.diff(ro)[-T - 1:-1] == 1).all()


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "new"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_map_and_mode_at_every_tile_edge(cfg, dtype, inplace):
    H, l, r = edge_matrix(dtype)
    ro = H.row_offsets
    rw, cl = rows_of(ro), H.col_ids.astype(np.int64)
    l_t, r_t = dev(l), dev(r)
    alpha = -1.7
    dA = None
    for map in MAPS:
        for row in MODES:
            for col in MODES:
                if dA is None or inplace:
                    dA = sa.dCSR.from_host(H)
                want = expected(H.data, rw, cl, dtype, alpha, map, l, row, r, col)
                C, info = call(dA, cfg, l_t, r_t, row, col, alpha=alpha, map=map, inplace=inplace)
                assert (C is dA) == inplace
                G = C.to_host()
                assert same(G.data, want), (map, row, col, first_difference(G.data, want))
                # in place the structure keeps its bytes; a new matrix has the offsets from 0 and the ids bit for bit
                assert G.row_offsets.tobytes() == ro.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes(), (map, row, col)
                assert (G.rows, G.cols, C.nnz) == (H.rows, H.cols, H.nnz)
                check_info(info, want, ro, row is not None)
                if not inplace:
                    assert dA.to_host().data.tobytes() == H.data.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_smallest_matrices(cfg, dtype):
    l_t, r_t = dev([3.0, -0.5, 7.0]), dev([2.0])
    for lens, data in (([1], [-3.0]), ([0, 0, 0], []), ([0, 2, 0], [5.0, -1.5])):
        H = mk(lens, np.array(data, dtype=dtype), cols=1)
        for inplace in (True, False):
            for row in MODES:
                dA = sa.dCSR.from_host(H)
                C, info = call(dA, cfg, l_t[:H.rows].contiguous(), r_t, row, "div", alpha=0.25, inplace=inplace)
                want = expected(H.data, rows_of(H.row_offsets), H.col_ids, dtype, 0.25, "identity", np.array([3.0, -0.5, 7.0]), row,
                                np.array([2.0]), "div")
                G = C.to_host()
                assert same(G.data, want) and G.row_offsets.tobytes() == H.row_offsets.tobytes()
                check_info(info, want, H.row_offsets, row is not None)
    empty = sa.HostCSR(0, 1, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))     # rows == 0
    dA = sa.dCSR.from_host(empty)
    _, info = sa.scale(dA, cfg, alpha=2.0, inplace=True)
    assert (info.entries, info.nonfinite, info.tiles) == (0, 0, 0)
    C, info = sa.scale(dA, cfg, alpha=2.0)
    assert (C.rows, C.nnz, info.entries) == (0, 0, 0) and C.to_host().row_offsets.tolist() == [0]


# ---------------------------------------------------------------------------------------------------- 2: views
def view_cases():
    """(first row, last row + 1): an odd absolute base and an end inside a tile; from inside a tile to the end; the long row
    alone (tiles wholly inside it); the 99 entries inside one tile of ... ; empty rows only"""
    return [(4, FIRST_EMPTY + 5000 + 1), (SHORT_ROW, len(edge_lens())), (LONG_ROW, LONG_ROW + 1), (SHORT_ROW, SHORT_ROW + 1),
            (FIRST_EMPTY + 10, FIRST_EMPTY + 4000)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_in_place_touches_its_entries_only(cfg, dtype):
    H, l, r = edge_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    rw, cl = rows_of(ro), H.col_ids.astype(np.int64)
    r_t = dev(r)
    for a, b in view_cases():
        lo, hi = ro[a], ro[b]
        assert a == FIRST_EMPTY + 10 or (lo % 2 == 1 and hi % T != 0 and hi > lo)
        lv = vector(b - a, 100 + a)                          # indexed from the view's first row
        lv_t = dev(lv)
        for row, col, map in (("div", None, "identity"), ("mul", "mul", "abs"), (None, None, "square"), (None, "div", "identity")):
            dA = sa.dCSR.from_host(H)
            view = dA.row_view(a, b)
            assert view.nnz == hi - lo
            _, info = call(view, cfg, lv_t, r_t, row, col, alpha=3.0, map=map, inplace=True)
            want = expected(H.data[lo:hi], rw[lo:hi] - a, cl[lo:hi], dtype, 3.0, map, lv, row, r, col)
            G = dA.to_host()
            assert same(G.data[lo:hi], want), (a, b, row, col, first_difference(G.data[lo:hi], want))
            assert G.data[:lo].tobytes() == H.data[:lo].tobytes() and G.data[hi:].tobytes() == H.data[hi:].tobytes(), (a, b, row, col)
            assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
            check_info(info, want, ro[a:b + 1], row is not None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_into_a_new_matrix(cfg, dtype):
    H, l, r = edge_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    rw, cl = rows_of(ro), H.col_ids.astype(np.int64)
    dA, r_t = sa.dCSR.from_host(H), dev(r)
    for a, b in view_cases():
        lo, hi = ro[a], ro[b]
        lv = vector(b - a, 200 + a)
        lv_t = dev(lv)
        for row, col in (("mul", "div"), (None, None)):
            C, info = call(dA.row_view(a, b), cfg, lv_t, r_t, row, col, alpha=0.5)
            want = expected(H.data[lo:hi], rw[lo:hi] - a, cl[lo:hi], dtype, 0.5, "identity", lv, row, r, col)
            G = C.to_host()
            assert same(G.data, want), (a, b, row, col, first_difference(G.data, want))
            assert G.row_offsets.tobytes() == (ro[a:b + 1] - lo).astype(np.uint32).tobytes()
            assert G.col_ids.tobytes() == H.col_ids[lo:hi].tobytes() and (G.rows, G.cols) == (b - a, H.cols)
            check_info(info, want, ro[a:b + 1], row is not None)
    assert dA.to_host().data.tobytes() == H.data.tobytes()


# ---------------------------------------------------------------------------------------------------- 3: special values
def specials(dtype):
    fi = np.finfo(dtype)
    return np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, 3 * float(fi.smallest_subnormal), np.inf, -np.inf,
                     np.nan, fi.max, -fi.max, fi.tiny, 1.0, -1.0], dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_in_the_entries(cfg, dtype):
    """zeros of both signs, subnormals, infinities and NaNs sprinkled over the edge matrix, its first and last entry among
    them: through every map, with and without the vectors"""
    H, l, r = edge_matrix(dtype)
    rng = np.random.default_rng(77)
    data = H.data.copy()
    at = np.concatenate([[0, H.nnz - 1, T - 1, T, 4 * T + 5], rng.integers(0, H.nnz, size=150)])
    data[at] = specials(dtype)[np.arange(len(at)) % len(specials(dtype))]
    H2 = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, data)
    rw, cl = rows_of(H.row_offsets), H.col_ids.astype(np.int64)
    l_t, r_t = dev(l), dev(r)
    for map in MAPS:
        for row, col, alpha in ((None, None, 1.0), ("mul", "div", -2.5), ("div", None, 1.0), (None, "mul", 0.0)):
            dA = sa.dCSR.from_host(H2)
            _, info = call(dA, cfg, l_t, r_t, row, col, alpha=alpha, map=map, inplace=True)
            want = expected(data, rw, cl, dtype, alpha, map, l, row, r, col)
            got = dA.to_host().data
            assert same(got, want), (map, row, col, first_difference(got, want))
            check_info(info, want, H.row_offsets, row is not None)
            if map == "one" and alpha == 1.0 and row is None:
                assert (got == 1.0).all() and info.nonfinite == 0            # a NaN entry becomes 1.0
            if map == "abs" and alpha == 1.0 and row is None:
                assert not np.signbit(got[data == 0]).any()                  # |-0.0| is +0.0
            if map == "identity" and alpha == 1.0 and row is None:
                assert info.nonfinite == int((~np.isfinite(data)).sum()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_underflow_division_by_zero_and_nan_in_the_vectors(cfg, dtype):
    fi = np.finfo(dtype)
    big, small = float(fi.max) / 2, float(fi.tiny) * 4
    #        row 0: overflow to inf         row 1: into the subnormals          row 2: l = 0       row 3: l = NaN   row 4: l = inf
    rows = [[big, -big, 1.0, fi.max],      [small, -small, 3 * small, 1.0],   [1.0, -2.0, 0.0, -0.0], [1.0, 0.0],  [np.inf, 5.0, -np.inf]]
    lens = [len(x) for x in rows]
    data = np.array([x for row in rows for x in row], dtype=dtype)
    H = mk(lens, data, cols=4, seed=5)
    rw, cl = rows_of(H.row_offsets), H.col_ids.astype(np.int64)
    l = np.array([0.25, 64.0, 0.0, np.nan, np.inf])
    r = np.array([1.0, -0.0, np.nan, 2.0 ** -30])
    l_t, r_t = dev(l), dev(r)
    seen = set()
    for alpha in (1.0, 0.0, -0.0, np.inf, 2.0 ** -20, 8.0):
        for row in MODES:
            for col in MODES:
                for map in ("identity", "square"):
                    dA = sa.dCSR.from_host(H)
                    _, info = call(dA, cfg, l_t, r_t, row, col, alpha=alpha, map=map, inplace=True)
                    want = expected(data, rw, cl, dtype, alpha, map, l, row, r, col)
                    got = dA.to_host().data
                    assert same(got, want), (alpha, row, col, map, first_difference(got, want))
                    assert info.nonfinite == int((~np.isfinite(want)).sum()) and info.entries == H.nnz
                    if np.isinf(want[:3]).any() and np.isfinite(alpha) and row == "div":
                        seen.add("an overflow to inf")
                    sub = want[np.isfinite(want) & (want != 0)]
                    if (np.abs(sub) < fi.tiny).any():
                        seen.add("a subnormal result")
                    if row == "div" and np.isinf(want[8:10]).all() and np.isnan(want[10:12]).all():
                        seen.add("x / 0 and 0 / 0")
                    if alpha == 0.0 and map == "identity" and row is None and col is None and np.isnan(want[-1]) and np.isnan(want[-3]):
                        seen.add("0 * inf")
    assert seen == {"an overflow to inf", "a subnormal result", "x / 0 and 0 / 0", "0 * inf"}, seen


# ---------------------------------------------------------------------------------------------------- 4: one vector, both sides
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_array_as_row_and_column_vector(cfg, dtype):
    """the GCN form D S D: scipy's diags(d) @ S @ diags(d) makes (d_i a) d_j, the same chain of roundings"""
    n = 3000
    S = sp.random(n, n, density=12 / n, random_state=4, format="csr", data_rvs=lambda k: real_values(k, 8, np.float64))
    S = S.astype(dtype)
    S.sort_indices()
    assert S.nnz > 2 * T
    d = vector(n, 21)
    want = (sp.diags(d) @ S.astype(np.float64) @ sp.diags(d)).tocsr()
    want.sort_indices()
    assert np.array_equal(want.indices, S.indices) and np.array_equal(want.indptr, S.indptr)
    H = sa.HostCSR(n, n, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data)
    d_t = dev(d)
    for inplace in (True, False):
        dA = sa.dCSR.from_host(H)
        C, info = sa.scale(dA, cfg, row=d_t, col=d_t, inplace=inplace)
        G = C.to_host()
        assert same(G.data, want.data.astype(dtype)) and G.col_ids.tobytes() == H.col_ids.tobytes()
        assert info.nonfinite == 0 and info.entries == S.nnz


# ---------------------------------------------------------------------------------------------------- 5: refusals on the device
def hostile(H, which):
    """(offsets, column ids, declared nnz, whether the column ids have to be read for the refusal)"""
    ro, ci, rows, nnz = H.row_offsets, H.col_ids, H.rows, H.nnz
    if which == "descending":
        bad = ro.copy()
        bad[1023] = bad[1024] + 1
        return bad, ci, nnz, False
    if which == "beyond":
        bad = ro.copy()
        bad[rows] = nnz + 5
        return bad, ci, nnz, False
    if which == "short":
        return ro, ci, nnz + 1, False
    at = {"id first tile": 3, "id middle tile": 4 * T + 17, "id last tile": nnz - 1}[which]
    bad = ci.copy()
    bad[at] = H.cols
    return ro, bad, nnz, True


HOSTILE = ["descending", "beyond", "short", "id first tile", "id middle tile", "id last tile"]


@pytest.mark.parametrize("which", HOSTILE)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_is_written(cfg, dtype, which):
    H, l, r = edge_matrix(dtype)
    ro, ci, nnz, by_id = hostile(H, which)
    l_t, r_t = dev(l), dev(r)
    lens = edge_lens()
    lens[0], lens[1] = lens[1], lens[0]
    other = mk(lens, real_values(H.nnz, 55, dtype), seed=56)       # C before the call: A's shape, so its buffers would be re-used
    assert (other.rows, other.nnz) == (H.rows, H.nnz) and other.row_offsets[1] != H.row_offsets[1]
    L = _lib.load()
    fn = L.speck_scale_f32 if dtype == np.float32 else L.speck_scale_f64
    for row, col in ((None, "mul"), ("div", "mul"), ("mul", None), (None, None)):
        for new in (False, True):
            if by_id and col is None and not new:
                continue                                            # (the ids are not read: accepted, below)
            dA = on_torch(H, ro=ro, ci=ci, nnz=nnz)
            dC = sa.dCSR.from_host(other)
            ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            p = _lib.CScaleParams()
            p.map, p.alpha = sa.MAP_ABS, 2.0
            p.row_mode = {None: 0, "mul": 1, "div": 2}[row]
            p.col_mode = {None: 0, "mul": 1, "div": 2}[col]
            p.d_row = l_t.data_ptr() if row else None
            p.d_col = r_t.data_ptr() if col else None
            info = _lib.CScaleInfo(9, 9, 9)
            torch.cuda.synchronize()
            rc = fn(cfg._h, C_.byref(dA._c), C_.byref(p), C_.byref(dC._c) if new else None, C_.byref(info))
            torch.cuda.synchronize()
            assert rc == ERR_INVALID, (which, row, col, new)
            assert (info.entries, info.nonfinite, info.tiles) == (0, 0, 0)
            assert values_of(dA).tobytes() == H.data.tobytes(), (which, row, col, new)
            assert ptrs == (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            G = dC.to_host()
            assert G.data.tobytes() == other.data.tobytes() and G.col_ids.tobytes() == other.col_ids.tobytes() and \
                G.row_offsets.tobytes() == other.row_offsets.tobytes(), (which, row, col, new)
    # the config serves a valid call right after
    dA = sa.dCSR.from_host(H)
    sa.scale(dA, cfg, row=l_t, row_div=True, inplace=True)
    assert same(dA.to_host().data, expected(H.data, rows_of(H.row_offsets), None, dtype, l=l, row="div"))


@pytest.mark.parametrize("which", HOSTILE[3:])
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_ids_that_are_not_read_may_hold_anything(cfg, dtype, which):
    H, l, r = edge_matrix(dtype)
    ro, ci, nnz, _ = hostile(H, which)
    l_t = dev(l)
    for row in (None, "mul"):
        dA = on_torch(H, ci=ci)
        _, info = call(dA, cfg, l_t, None, row, None, alpha=-3.0, inplace=True)
        torch.cuda.synchronize()
        want = expected(H.data, rows_of(ro), None, dtype, -3.0, "identity", l, row)
        assert same(values_of(dA), want) and dA._keep[1].cpu().numpy().view(np.uint32)[:H.nnz].tobytes() == ci.tobytes()
        check_info(info, want, ro, row is not None)
        none = sa.dCSR.from_device(H.rows, H.cols, H.nnz, dA._c.row_offsets, None, dA._c.data, dtype=dtype, keep=dA._keep)
        sa.scale(none, cfg, alpha=-1.0 / 3.0, inplace=True)          # ... or be missing
        torch.cuda.synchronize()
        assert same(values_of(dA), expected(want, None, None, dtype, -1.0 / 3.0))


# ---------------------------------------------------------------------------------------------------- 6: housekeeping
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config(dtype):
    H, l, r = edge_matrix(dtype)
    l_t, r_t = dev(l), dev(r)
    rw, cl = rows_of(H.row_offsets), H.col_ids.astype(np.int64)
    for row, col, inplace in (("div", "mul", True), (None, "div", False), ("mul", None, False)):
        dA = sa.dCSR.from_host(H)
        C, info = call(dA, None, l_t, r_t, row, col, alpha=1.5, map="abs", inplace=inplace)
        want = expected(H.data, rw, cl, dtype, 1.5, "abs", l, row, r, col)
        assert same(C.to_host().data, want)
        check_info(info, want, H.row_offsets, row is not None)


def test_runs_on_the_callers_stream(cfg):
    """the values and the row vector are written by copies on the caller's stream right before the call: ordering against
    the producer is by the stream alone"""
    H, l, r = edge_matrix(np.float64)
    dA = on_torch(H)
    t_va = dA._keep[2]
    real, l_real = t_va.clone(), dev(l)
    t_va.zero_()
    l_t = torch.ones_like(l_real)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream scales zeros by ones
            t_va.copy_(real, non_blocking=True)
            l_t.copy_(l_real, non_blocking=True)
        sa.scale(dA, cfg, row=l_t, row_div=True, inplace=True)
        with torch.cuda.stream(s):
            got = values_of(dA)
        assert same(got, expected(H.data, rows_of(H.row_offsets), None, np.float64, l=l, row="div"))
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    H, l, r = edge_matrix(dtype)
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        l_t, r_t = dev(l), dev(r)
        rw, cl = rows_of(H.row_offsets), H.col_ids.astype(np.int64)
        for row, col, inplace in (("div", "mul", True), ("mul", "mul", False), (None, "mul", True), (None, None, False)):
            dA = sa.dCSR.from_host(H)                                          # (allocated with zones: A's are checked in place)
            C, _ = call(dA, cfg, l_t, r_t, row, col, inplace=inplace)         # (a touched zone is status 3)
            assert same(C.to_host().data, expected(H.data, rw, cl, dtype, 1.0, "identity", l, row, r, col))
            a, b = LONG_ROW, FIRST_EMPTY + 2                                   # a view with an odd base: the narrow form
            view = sa.dCSR.from_host(H).row_view(a, b)
            call(view, cfg, l_t[a:b].contiguous(), r_t, row, col, inplace=inplace)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_a_scale_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.05, 7, signed=True)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()
    for _ in range(3):
        sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"]
    sa.MultiplyspECK(dS, dS, dC, cfg)
    without = cfg.last_stats()["replayed"]
    first = dC.to_host()
    l_t = dev(vector(h.rows, 9))
    dN, _ = sa.scale(dC, cfg, row=l_t, col=l_t, row_div=True)                  # of the product, into a new matrix ...
    sa.scale(dN, cfg, alpha=2.0, map="square", inplace=True)                   # ... and in place, of that
    sa.normalize_rows(dC.copy(), cfg, inplace=True)
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == without == 1
    again = dC.to_host()                                                       # (the product sums through atomics: last bits move)
    assert again.col_ids.tobytes() == first.col_ids.tobytes() and np.allclose(again.data, first.data, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_matout_keeps_the_buffers_that_fit(cfg, dtype):
    H, l, r = edge_matrix(dtype)
    dA = sa.dCSR.from_host(H)
    C, _ = sa.scale(dA, cfg, alpha=2.0)
    ptrs = (C._c.row_offsets, C._c.col_ids, C._c.data)
    C2, _ = sa.scale(dA, cfg, alpha=-4.0, map="abs", matOut=C)                 # same rows, same nnz: nothing re-allocated
    assert C2 is C and ptrs == (C._c.row_offsets, C._c.col_ids, C._c.data)
    assert same(C.to_host().data, expected(H.data, None, None, dtype, -4.0, "abs"))
    lens = edge_lens()
    lens[1] -= 7                                                               # same rows, another nnz: the offsets stay
    H2 = mk(lens, real_values(sum(lens), 3, dtype))
    sa.scale(sa.dCSR.from_host(H2), cfg, matOut=C)
    assert C._c.row_offsets == ptrs[0] and (C.rows, C.nnz) == (H2.rows, H2.nnz)
    G = C.to_host()
    assert G.data.tobytes() == H2.data.tobytes() and G.col_ids.tobytes() == H2.col_ids.tobytes() and \
        G.row_offsets.tobytes() == H2.row_offsets.tobytes()
    data_ptrs = (C._c.col_ids, C._c.data)
    H3 = mk([H2.nnz - 3, 1, 0, 2], H2.data, cols=COLS + 5)                     # other rows, the same nnz: data and ids stay
    sa.scale(sa.dCSR.from_host(H3), cfg, alpha=0.5, matOut=C)
    assert data_ptrs == (C._c.col_ids, C._c.data) and (C.rows, C.cols, C.nnz) == (4, COLS + 5, H3.nnz)
    G = C.to_host()
    assert same(G.data, expected(H3.data, None, None, dtype, 0.5)) and G.row_offsets.tobytes() == H3.row_offsets.tobytes()
    other = sa.dCSR(np.float32 if dtype == np.float64 else np.float64)         # a matOut of the other value type is reset
    C4, _ = sa.scale(dA, cfg, matOut=other)
    assert C4 is other and other.dtype == np.dtype(dtype) and other.to_host().data.tobytes() == H.data.tobytes()


def test_the_caller_that_includes_scale_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_scale.cpp")
    out = str(tmp_path / "caller_scale")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "scale caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)


# ---------------------------------------------------------------------------------------------------- 7: workflows
def standin(dtype, seed=3):
    h = sa.gen_matrix("scircuit", 0.05, seed, signed=True)
    return sa.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data.astype(dtype))


def as_scipy(H):
    return sp.csr_matrix((H.data, H.col_ids.astype(np.int64), H.row_offsets.astype(np.int64)), shape=(H.rows, H.cols))


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalised_rows_of_a_product_sum_to_one(cfg, dtype):
    """every row with an entry: |sum|y| - 1| <= g_n + u + u_T, n the row's length, g_n = n u / (1 - n u), u = 2^-53: the bound
    of the reduction that is checked, the rounding of the division and the rounding to T (u_T = 2^-53 for double: g_n + 2 u;
    2^-24 for float)"""
    dS, dP = sa.dCSR.from_host(standin(dtype)), sa.dCSR(dtype)
    sa.MultiplyspECK(dS, dS, dP, cfg)
    dN, info = sa.normalize_rows(dP, cfg, "abs_sum")
    assert info.entries == dP.nnz and info.nonfinite == 0
    sums, _, rinfo = sa.reduce(dN, cfg, "abs_sum")
    ro = dN.to_host().row_offsets.astype(np.int64)
    n = (ro[1:] - ro[:-1]).astype(np.float64)
    full = n > 0
    assert full.sum() > 1000 and rinfo.rows_empty == int((~full).sum())
    u_t = U if dtype == np.float64 else 2.0 ** -24
    err = np.abs(sums[full] - 1.0)
    print("largest |sum - 1| / bound:", float((err / (n[full] * U / (1 - n[full] * U) + U + u_t)).max()))
    assert (err <= n[full] * U / (1 - n[full] * U) + U + u_t).all()
    assert (sums[~full] == 0.0).all()
    same_in_place, _ = sa.normalize_rows(dP, cfg, "abs_sum", inplace=True)     # in place: the same bits
    assert same_in_place is dP and dP.to_host().data.tobytes() == dN.to_host().data.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_triangle_count_of_a_weighted_graph(cfg, dtype):
    P = sp.random(300, 300, density=4 / 300, random_state=91, format="csr", data_rvs=lambda k: real_values(k, 92, np.float64))
    P.sort_indices()
    S = ((P + P.T) != 0).astype(np.float64).tocsr()
    Ls = sp.tril(S, k=-1).tocsr()
    per_row = np.asarray((Ls @ Ls).multiply(Ls).sum(axis=1)).ravel()
    triangles = int(per_row.sum())
    assert triangles > 0
    HP = sa.HostCSR(300, 300, P.indptr.astype(np.uint32), P.indices.astype(np.uint32), P.data.astype(dtype))
    dL = sa.tril(sa.symmetrize(sa.dCSR.from_host(HP), cfg), cfg, k=-1)         # weighted: w_ij + w_ji
    dOne = sa.pattern_ones(dL, cfg)
    assert (dOne.to_host().data == 1.0).all() and dOne.nnz == dL.nnz == Ls.nnz
    dC, minfo = sa.multiply_masked(dOne, dOne, dOne, cfg)
    rows, total, _ = sa.reduce(dC, cfg, "sum")
    assert total == minfo.hits == triangles and np.array_equal(rows, per_row)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_mcl_step(cfg, dtype):
    """expansion S S, inflation v v, the columns normalised by their sums (transpose, normalize_rows, transpose).  Equality
    from the product's own values on; the product itself against scipy within the multiply's bound, and the column sums --
    the one summation of the chain -- within the reduction's, then taken as the device made them."""
    H = standin(dtype, seed=5)
    dS, dP = sa.dCSR.from_host(H), sa.dCSR(dtype)
    sa.MultiplyspECK(dS, dS, dP, cfg)
    P = dP.to_host()
    S64 = as_scipy(sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, H.data.astype(np.float64)))
    ref = (S64 @ S64).tocsr()
    ref.sort_indices()
    ab = (abs(S64) @ abs(S64)).tocsr()
    ab.sort_indices()
    assert P.col_ids.tobytes() == ref.indices.astype(np.uint32).tobytes() and P.row_offsets.tobytes() == ref.indptr.astype(np.uint32).tobytes()
    tol = 1e-12 if dtype == np.float64 else 4.0 * 2.0 ** -23
    assert (np.abs(P.data.astype(np.float64) - ref.data) <= tol * ab.data + 1e-300).all()

    dQ, _ = sa.scale(dP, cfg, map="square")
    dQt = sa.transpose(dQ, cfg)
    sums, _, _ = sa.reduce(dQt, cfg, "abs_sum")
    dNt, info = sa.normalize_rows(dQt, cfg, "abs_sum")
    dM = sa.transpose(dNt, cfg)

    q = expected(P.data, None, None, dtype, map="square")
    Qt = as_scipy(sa.HostCSR(P.rows, P.cols, P.row_offsets, P.col_ids, q)).T.tocsr()
    Qt.sort_indices()
    Gt = dQt.to_host()
    assert Gt.col_ids.tobytes() == Qt.indices.astype(np.uint32).tobytes() and Gt.data.tobytes() == Qt.data.tobytes()
    n = np.diff(Qt.indptr).astype(np.float64)
    exact = np.array([math.fsum(np.abs(Qt.data[a:b]).astype(np.float64)) for a, b in zip(Qt.indptr[:-1], Qt.indptr[1:])])
    assert (np.abs(sums - exact) <= (n * U / (1 - n * U) + U) * exact).all()
    nt = expected(Qt.data, rows_of(Qt.indptr), None, dtype, l=sums, row="div")
    assert same(dNt.to_host().data, nt) and info.nonfinite == int((~np.isfinite(nt)).sum())
    M = as_scipy(sa.HostCSR(Qt.shape[0], Qt.shape[1], Qt.indptr.astype(np.uint32), Qt.indices.astype(np.uint32), nt)).T.tocsr()
    M.sort_indices()
    G = dM.to_host()
    assert G.col_ids.tobytes() == P.col_ids.tobytes() and G.row_offsets.tobytes() == P.row_offsets.tobytes()
    assert same(G.data, M.data)
