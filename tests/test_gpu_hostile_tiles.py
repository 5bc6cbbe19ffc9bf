"""The edges of the tile offset check (speck_amd/csrc/row_tiles.hpp) through the four operations that stand on it: the row
sort, the masked product, the filter and the addition.  The hostile-offset cases of their own test files put the fault in
the middle of one short tile; here a descending pair of row offsets sits on the first row of a tile, on its last row, on
the first row of the next tile and on the last row of the matrix, the last offset lies beyond nnz, and an offset of a
row-range view lies below the view's first one -- in every operand the operation checks itself, at both tile sizes.
Every case is refused with SPECK_ERR_INVALID, leaves the output as it was byte for byte, and the config serves a valid
call afterwards.  The helpers and the references are those of the four files."""
import ctypes as C_
import os
import re

import numpy as np
import pytest

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po
import test_gpu_add as t_add
import test_gpu_masked as t_masked
import test_gpu_select as t_select
import test_gpu_sort_rows as t_sort

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speck_amd", "csrc")


def constants(header):
    """the unsigned constants of a header of the library: {name: value}"""
    text = open(os.path.join(CSRC, header)).read()
    found = re.findall(r"\b(k\w+) = (1u << )?(\d+)[,;]", text)
    return {name: (1 << int(n)) if shift else int(n) for name, shift, n in found}


MASK, SORT = constants("masked.hpp"), constants("sort_rows.hpp")
TILE_LONG, TILE_SHORT = sa.SELECT_TILE_ROWS       # rows per tile where rows are long / short: one pair for the three
LONG_AVG = sa.SELECT_LONG_ROW_AVG
assert sa.ADD_TILE_ROWS == (TILE_LONG, TILE_SHORT) == (MASK["kMaskTileRowsLong"], MASK["kMaskTileRowsShort"])
assert sa.ADD_LONG_ROW_AVG == LONG_AVG == MASK["kMaskLongRowAvg"]
SORT_TILE = SORT["kSortTileRows"]                 # the row sort's, for every matrix of fewer than kSortTileLongRows rows
# rows = 2 tiles + 3; entries per row and operand far on either side of LONG_AVG / 2
SHAPES = {"short_rows": (TILE_SHORT, 4, 64), "long_rows": (TILE_LONG, 40, 128)}
_made = {}


def operand(shape, which, dtype=np.float64):
    """operand `which` of a shape: no empty row, rows strictly ascending; made once, never changed"""
    tile, per_row, cols = SHAPES[shape]
    key = (shape, which)
    if key not in _made:
        seed = 1000 * sorted(SHAPES).index(shape) + which
        lens = np.random.default_rng(seed).integers(per_row - 2, per_row + 3, size=2 * tile + 3)
        _made[key] = t_add.from_lengths(lens, cols, seed + 500)
        assert (np.diff(_made[key].row_offsets.astype(np.int64)) > 0).all()
    return t_add.with_dtype(_made[key], dtype)


def picks_long_tile(shape, *operands):
    tile, _, _ = SHAPES[shape]
    long_rows = sum(H.nnz for H in operands) // operands[0].rows >= LONG_AVG
    assert long_rows == (tile == TILE_LONG)


def hostile_offsets(H, tile):
    """[(row_offsets, view)]: what the offset check has to refuse; view: the rows the call sees, None for all"""
    ro = H.row_offsets
    cases = []
    for r in (0, tile - 1, tile, H.rows - 1):
        assert ro[r + 1] > ro[r]
        bad = ro.copy()
        bad[r], bad[r + 1] = ro[r + 1], ro[r]                    # descending
        cases.append((bad, None))
    bad = ro.copy()
    bad[-1] = H.nnz + 5                                          # the last offset beyond nnz
    cases.append((bad, None))
    bad = ro.copy()
    assert ro[1] > 0
    bad[1 + tile + tile // 2] = ro[1] - 1                        # in the second tile of rows 1 .. : below the view's first
    cases.append((bad, (1, H.rows)))
    return cases


def _update_offsets(d, ro):
    assert _lib.load().speck_dcsr_update(C_.byref(d._c), ro.ctypes.data, None, None, 8) == 0


class Sentinels:
    """a C of plausible size filled with sentinels"""

    def __init__(self, dtype, rows, cols, n=1234):
        self.dC = sa.dCSR(dtype)
        self.dC.alloc(rows, cols, n)
        self.ro = np.full(rows + 1, 0xABABABAB, dtype=np.uint32)
        self.ci = np.full(n, 0xCDCDCDCD, dtype=np.uint32)
        self.da = np.full(n, -77.25, dtype=dtype)
        assert _lib.load().speck_dcsr_update(C_.byref(self.dC._c), self.ro.ctypes.data, self.ci.ctypes.data, self.da.ctypes.data,
                                             np.dtype(dtype).itemsize) == 0
        self.before = bytes(self.dC._c)

    def untouched(self):
        assert bytes(self.dC._c) == self.before                  # the struct: sizes and the three pointers
        got = self.dC.to_host()
        assert got.row_offsets.tobytes() == self.ro.tobytes() and got.col_ids.tobytes() == self.ci.tobytes()
        assert got.data.tobytes() == self.da.tobytes()


def refusals(cfg, operands, checked, rowwise, tile, dtype, out_cols, call):
    """every hostile case of every checked operand: `call(devices, dC)` raises INVALID and C keeps its sentinels"""
    for which in checked:
        for bad, view in hostile_offsets(operands[which], tile):
            d = {k: sa.dCSR.from_host(H) for k, H in operands.items()}
            _update_offsets(d[which], bad)
            if view:
                d = {k: (x.row_view(*view) if k in rowwise else x) for k, x in d.items()}
            out = Sentinels(dtype, d[which].rows, out_cols)
            with pytest.raises(sa.SpeckError) as e:
                call(d, out.dC)
            assert e.value.status == ERR_INVALID, (which, view)  # (not 3: no canary zone was touched either)
            out.untouched()


@pytest.fixture(params=[0, 4096])
def cfg(request):
    c = sa.spECKConfig.initialize(0)
    if request.param:
        c.set_option("guard_bytes", request.param)
    yield c
    if request.param:
        c.set_option("guard_bytes", 0)
    c.cleanup()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_select_refuses_offsets_at_the_tile_edges(cfg, shape, dtype):
    A, P = operand(shape, 0, dtype), operand(shape, 1)
    picks_long_tile(shape, A, P)
    refusals(cfg, {"A": A, "P": P}, ("A", "P"), ("A", "P"), SHAPES[shape][0], dtype, A.cols,
             lambda d, dC: sa.select(d["A"], cfg, matOut=dC, pattern=d["P"]))
    t_select.check(cfg, A, pattern=P)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_add_refuses_offsets_at_the_tile_edges(cfg, shape):
    A, B = operand(shape, 0), operand(shape, 1)
    picks_long_tile(shape, A, B)
    refusals(cfg, {"A": A, "B": B}, ("A", "B"), ("A", "B"), SHAPES[shape][0], np.float64, A.cols,
             lambda d, dC: sa.add(d["A"], d["B"], cfg, alpha=2.5, beta=-0.5, matOut=dC))
    t_add.check(cfg, A, B, 2.5, -0.5)


_expect = {}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_masked_refuses_offsets_at_the_tile_edges(cfg, shape, dtype):
    A, M = operand(shape, 0, dtype), operand(shape, 1)
    B = t_add.from_lengths(np.random.default_rng(3).integers(1, 8, size=A.cols), A.cols, 4, dtype)
    picks_long_tile(shape, A, M)
    for full in (False, True):
        refusals(cfg, {"A": A, "B": B, "M": M}, ("A", "M"), ("A", "M"), SHAPES[shape][0], dtype, B.cols,
                 lambda d, dC: sa.multiply_masked(d["A"], d["B"], d["M"], cfg, matOut=dC, full_pattern=full))
    as_po = lambda H: po.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, H.data)
    if (shape, dtype) not in _expect:
        _expect[shape, dtype] = t_masked.Expect(as_po(A), as_po(B), as_po(M))
    for full in (False, True):
        t_masked.check(cfg, as_po(A), as_po(B), as_po(M), dtype, full, X=_expect[shape, dtype])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sort_rows_refuses_offsets_at_the_tile_edges(cfg, shape):
    """every row reversed: there is work in every tile.  The matrix itself stays as it was"""
    H = operand(shape, 0)
    assert H.rows < SORT["kSortTileLongRows"]
    ro = H.row_offsets.astype(np.int64)
    row = np.repeat(np.arange(H.rows), np.diff(ro))
    mirror = ro[row] + ro[row + 1] - 1 - np.arange(H.nnz)
    ci, va = H.col_ids[mirror], H.data[mirror]
    for bad, view in hostile_offsets(H, SORT_TILE):
        d = t_sort.upload(H.row_offsets, ci, va, H.cols)
        _update_offsets(d, bad)
        for sum_duplicates in (False, True):
            with pytest.raises(sa.SpeckError) as e:
                sa.sort_rows(d.row_view(*view) if view else d, cfg, sum_duplicates=sum_duplicates)
            assert e.value.status == ERR_INVALID
            got = d.to_host()
            assert d.nnz == H.nnz
            assert t_sort.same_bytes(got.row_offsets, bad) and t_sort.same_bytes(got.col_ids, ci) and t_sort.same_bytes(got.data, va)
    d = t_sort.upload(H.row_offsets, ci, va, H.cols)
    sa.sort_rows(d, cfg, sum_duplicates=True)
    got = d.to_host()
    assert t_sort.same_bytes(got.row_offsets, H.row_offsets)
    assert t_sort.same_bytes(got.col_ids, H.col_ids) and t_sort.same_bytes(got.data, H.data)
