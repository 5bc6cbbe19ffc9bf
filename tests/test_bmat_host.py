"""speck_bmat_* without a GPU: the contract as numpy (numpy_bmat: what tests/test_gpu_bmat.py compares the device with)
against scipy, speck_bmat_layout -- the host half of the call -- through ctypes, the declarations, the exports, the ctypes
mirrors and the Python info class, a C++ caller that includes BMat.h only, the argument checks that come before anything
touches a device, the Python wrappers' refusals, and the loud failure where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import speck_amd
from speck_amd import _lib
from test_extract_host import Block, _header, _kinds, _mat, _no_device_status, _struct_fields, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 0, 1, 2, 5
INFO_FIELDS = ["blocks", "rows_out", "cols_out", "nnz_out", "pieces", "rows_empty", "max_row_entries"]
NOT_BUILT = ("blocks of mixed value type", "pattern-only blocks", "overlapping placements that add", "a fused sort", "a Kronecker product",
             "the batch vector itself", "a plan reused across calls", "writing into a region of an existing C")


# ---------------------------------------------------------------------------------------------------- the contract
def numpy_bmat(cells, block_rows, block_cols, row_sizes=None, col_sizes=None, vdtype=np.float64):
    """C = bmat(grid) as the header states it: (row_offsets, col_ids, the values' bits, info, row origins, column origins).
    cells: (block_row, block_col, H) in any order, H with rows, cols, row_offsets (a view's absolute ones are fine), col_ids
    and data.  Row i of block row g: row i of every block of the line in ascending block column, ids shifted, values as
    bits, in input order -- nothing sorted, summed or dropped."""
    h = [None] * block_rows if row_sizes is None else [int(v) for v in row_sizes]
    w = [None] * block_cols if col_sizes is None else [int(v) for v in col_sizes]
    assert len(h) == block_rows and len(w) == block_cols
    assert len({(g, q) for g, q, _ in cells}) == len(cells), "a cell named twice"
    for g, q, H in cells:
        h[g] = H.rows if h[g] is None else h[g]
        w[q] = H.cols if w[q] is None else w[q]
        assert (H.rows, H.cols) == (h[g], w[q]), "a block that disagrees with its line"
    assert None not in h and None not in w, "a line with neither a block nor a size"
    R0 = np.concatenate([[0], np.cumsum(h)]).astype(np.int64)
    C0 = np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
    nnz = sum(int(H.row_offsets[-1]) - int(H.row_offsets[0]) for _, _, H in cells)
    width = np.dtype(vdtype).itemsize
    ro = np.zeros(R0[-1] + 1, dtype=np.int64)
    ci = np.zeros(nnz, dtype=np.int64)
    vb = np.zeros(nnz, dtype=np.uint64 if width == 8 else np.uint32)
    at, pieces = 0, 0
    for g in range(block_rows):
        line = sorted(((q, H) for gg, q, H in cells if gg == g), key=lambda c: c[0])
        nb, rows = len(line), np.arange(h[g])
        lens = np.zeros((h[g], nb), dtype=np.int64)
        for k, (_, H) in enumerate(line):
            lens[:, k] = np.diff(H.row_offsets.astype(np.int64))
        G = at + np.concatenate([[0], np.cumsum(lens.reshape(-1))])          # the scan of the line's piece lengths
        for k, (q, H) in enumerate(line):
            o = H.row_offsets.astype(np.int64)
            src = np.arange(o[0], o[-1])
            dst = np.repeat(G[rows * nb + k] - o[:-1], lens[:, k]) + src     # piece (i, k) starts at G[i nb + k]
            assert np.dtype(H.data.dtype) == np.dtype(vdtype)
            ci[dst] = H.col_ids[src].astype(np.int64) + C0[q]
            vb[dst] = bits(H.data)[src]
        ro[R0[g]:R0[g + 1]] = G[rows * nb] if nb else at
        at, pieces = int(G[-1]), pieces + h[g] * nb
    ro[-1] = at
    assert at == nnz
    row_len = np.diff(ro)
    info = dict(blocks=len(cells), rows_out=int(R0[-1]), cols_out=int(C0[-1]), nnz_out=nnz, pieces=pieces,
                rows_empty=int((row_len == 0).sum()), max_row_entries=int(row_len.max()) if len(row_len) else 0)
    return ro.astype(np.uint32), ci.astype(np.uint32), vb, info, R0, C0


def grid_cells(grid):
    """a list of lists with None for a zero block -> (cells, block_rows, block_cols)"""
    return [(g, q, H) for g, line in enumerate(grid) for q, H in enumerate(line) if H is not None], len(grid), len(grid[0]) if grid else 0


def host_of(S):
    S = S.tocsr()
    return speck_amd.HostCSR(S.shape[0], S.shape[1], S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.astype(np.float64))


def _random_csr(rows, cols, per_row, seed):
    rng = np.random.default_rng(seed)
    S = sp.random(rows, cols, density=min(1.0, per_row / max(cols, 1)), format="csr", random_state=rng, dtype=np.float64)
    S.data = rng.integers(1, 100, size=S.nnz).astype(np.float64)
    S.sort_indices()
    return S


def _same(got, W):
    W = W.tocsr()
    W.sort_indices()
    ro, ci, vb = got[:3]
    return (len(ro) - 1, got[3]["cols_out"]) == W.shape and np.array_equal(ro, W.indptr) and np.array_equal(ci, W.indices) and \
        np.array_equal(vb.view(np.float64), W.data)


def test_numpy_statement_is_scipys_bmat_on_canonical_blocks():
    A, B, D = _random_csr(40, 30, 5, 1), _random_csr(40, 17, 3, 2), _random_csr(25, 17, 4, 3)
    E, Z = _random_csr(25, 30, 2, 4), _random_csr(0, 30, 1, 5)
    for grid in ([[A, B], [E, D]], [[A, None], [None, D]], [[A, B], [None, D]], [[None, B], [E, None]], [[A, B]], [[A], [E], [Z]]):
        cells, br, bc = grid_cells([[None if S is None else host_of(S) for S in line] for line in grid])
        got = numpy_bmat(cells, br, bc)
        assert _same(got, sp.bmat(grid, format="csr")), grid
        assert got[3]["nnz_out"] == sum(S.nnz for line in grid for S in line if S is not None)
        assert got[3]["pieces"] == sum(line[[S is not None for S in line].index(True)].shape[0] * sum(S is not None for S in line)
                                       for line in grid)


def test_numpy_statement_is_scipys_vstack_hstack_and_block_diag():
    mats = [_random_csr(r, 23, 4, 10 + r) for r in (7, 0, 31, 1)]
    got = numpy_bmat([(g, 0, host_of(S)) for g, S in enumerate(mats)], 4, 1)
    assert _same(got, sp.vstack(mats)) and got[4].tolist() == [0, 7, 7, 38, 39] and got[3]["pieces"] == 39
    mats = [_random_csr(19, c, 3, 20 + c) for c in (5, 0, 40, 1)]
    got = numpy_bmat([(0, q, host_of(S)) for q, S in enumerate(mats)], 1, 4)
    assert _same(got, sp.hstack(mats)) and got[5].tolist() == [0, 5, 5, 45, 46] and got[3]["pieces"] == 4 * 19
    mats = [_random_csr(r, c, 2, 30 + r) for r, c in ((4, 6), (0, 3), (5, 0), (9, 9), (1, 1))]
    got = numpy_bmat([(i, i, host_of(S)) for i, S in enumerate(mats)], 5, 5)
    assert _same(got, sp.block_diag(mats)) and got[3]["pieces"] == 19
    assert got[4].tolist() == [0, 4, 4, 9, 18, 19] and got[5].tolist() == [0, 6, 9, 9, 18, 19]


def test_numpy_statement_keeps_input_order_where_scipy_sorts_and_sums():
    # THE difference to scipy.sparse.bmat: rows that are unsorted and hold an id twice stay as they are, entry for entry --
    # scipy's conversion to CSR sorts every row and sums equal ids.  (Sorted and summed, both are the same matrix.)
    A = speck_amd.HostCSR(2, 3, [0, 3, 4], [2, 0, 2, 1], np.array([1., 2., 3., 4.]))
    B = speck_amd.HostCSR(2, 2, [5, 7, 7], [9, 9, 9, 9, 9, 1, 1], np.arange(7.))           # a view: its entries start at 5
    ro, ci, vb, info, _, _ = numpy_bmat([(0, 1, B), (0, 0, A)], 1, 2)
    assert ro.tolist() == [0, 5, 6] and ci.tolist() == [2, 0, 2, 4, 4, 1] and vb.view(np.float64).tolist() == [1, 2, 3, 5, 6, 4]
    assert info == dict(blocks=2, rows_out=2, cols_out=5, nnz_out=6, pieces=4, rows_empty=0, max_row_entries=5)
    W = sp.hstack([sp.csr_matrix((A.data, A.col_ids, A.row_offsets), shape=(2, 3)),
                   sp.csr_matrix((B.data[5:], B.col_ids[5:], B.row_offsets - 5), shape=(2, 2))]).tocsr()
    W.sum_duplicates()
    assert W.nnz == 4 and W.indices.tolist() == [0, 2, 4, 1]                        # scipy: sorted, the two pairs summed
    G = sp.csr_matrix((vb.view(np.float64), ci, ro), shape=(2, 5))
    G.sum_duplicates()
    assert np.array_equal(G.indptr, W.indptr) and np.array_equal(G.indices, W.indices) and np.array_equal(G.data, W.data)


# ---------------------------------------------------------------------------------------------------- the layout
def _dcsr(rows, cols, nnz, ptr=4096):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.row_offsets, m.col_ids, m.data = ptr, ptr + 1024, ptr + 2048
    return m


def _params(cells, block_rows, block_cols, row_sizes=None, col_sizes=None, n_blocks=None, null_blocks=False):
    """(speck_bmat_params, what it points to); cells: (block_row, block_col, DCsr or None)"""
    arr = (_lib.CBmatBlock * max(len(cells), 1))()
    for k, (g, q, m) in enumerate(cells):
        arr[k].block_row, arr[k].block_col = g, q
        if m is not None:
            arr[k].M = ctypes.pointer(m)
    p = _lib.CBmatParams()
    p.block_rows, p.block_cols, p.n_blocks = block_rows, block_cols, len(cells) if n_blocks is None else n_blocks
    p.blocks = None if null_blocks else arr
    rs = None if row_sizes is None else (ctypes.c_uint64 * max(len(row_sizes), 1))(*row_sizes)
    cs = None if col_sizes is None else (ctypes.c_uint64 * max(len(col_sizes), 1))(*col_sizes)
    p.row_sizes, p.col_sizes = rs, cs
    return p, (arr, rs, cs, cells)


def _layout(p, arrays=True):
    out = _lib.CBmatLayoutOut(7, 7, 7, 7)
    ro = (ctypes.c_uint64 * (p.block_rows + 1))(*([7] * (p.block_rows + 1)))
    co = (ctypes.c_uint64 * (p.block_cols + 1))(*([7] * (p.block_cols + 1)))
    if arrays:
        out.row_origins, out.col_origins = ro, co
    rc = _lib.load().speck_bmat_layout(ctypes.byref(p), ctypes.byref(out))
    return rc, (out.rows, out.cols, out.nnz, out.pieces), list(ro), list(co)


def test_layout_is_scipys_shape_and_the_running_sums():
    rng = np.random.default_rng(5)
    h, w = rng.integers(0, 50, size=6), rng.integers(0, 40, size=5)
    present = rng.random((6, 5)) < 0.5
    present[2, :], present[:, 3] = False, False                                    # a line of either kind without a block
    nnz = rng.integers(0, 9, size=(6, 5))
    cells = [(g, q, _dcsr(int(h[g]), int(w[q]), int(nnz[g, q]) if h[g] and w[q] else 0)) for g in range(6) for q in range(5) if present[g, q]]
    order = rng.permutation(len(cells))
    p, keep = _params([cells[k] for k in order], 6, 5, row_sizes=h.tolist(), col_sizes=w.tolist())
    rc, shape, ro, co = _layout(p)
    W = sp.bmat([[sp.csr_matrix((int(h[g]), int(w[q]))) for q in range(5)] for g in range(6)])
    assert rc == OK and shape[:2] == W.shape
    assert ro == np.concatenate([[0], np.cumsum(h)]).tolist() and co == np.concatenate([[0], np.cumsum(w)]).tolist()
    assert shape[2] == sum(m.nnz for _, _, m in cells) and shape[3] == sum(int(h[g]) * int(present[g].sum()) for g in range(6))
    assert _layout(p, arrays=False)[:2] == (OK, shape)                             # the arrays may be NULL
    # without sizes: from the blocks, where every line has one
    full = [(g, q, _dcsr(int(h[g]), int(w[q]), 0)) for g in range(6) for q in range(5) if (g + q) % 2 == 0]
    p, keep = _params(full, 6, 5)
    assert _layout(p)[1:] == ((int(h.sum()), int(w.sum()), 0, sum(int(h[g]) * len([1 for q in range(5) if (g + q) % 2 == 0]) for g in range(6))),
                              np.concatenate([[0], np.cumsum(h)]).tolist(), np.concatenate([[0], np.cumsum(w)]).tolist())
    # no block at all: both size arrays give the shape
    p, keep = _params([], 3, 2, row_sizes=[4, 0, 5], col_sizes=[6, 1])
    assert _layout(p) == (OK, (9, 7, 0, 0), [0, 4, 4, 9], [0, 6, 7])


def _refusals():
    """name -> (params, status): every refusal the host can decide"""
    A, B, big = _dcsr(4, 6, 3), _dcsr(5, 6, 2), (1 << 27) + 1
    hollow = {}
    for field in ("row_offsets", "col_ids", "data"):
        m = _dcsr(4, 6, 3)
        setattr(m, field, None)
        hollow[field] = m
    r = {
        "n_blocks > 0 with NULL blocks": (_params([(0, 0, A)], 1, 1, null_blocks=True), ERR_INVALID),
        "NULL M": (_params([(0, 0, A), (1, 0, None)], 2, 1), ERR_INVALID),
        "a cell below the grid": (_params([(0, 0, A), (2, 0, B)], 2, 1), ERR_INVALID),
        "a cell beside the grid": (_params([(0, 0, A), (0, 1, A)], 1, 1), ERR_INVALID),
        "a cell named twice": (_params([(0, 0, A), (1, 0, B), (0, 0, A)], 2, 1), ERR_INVALID),
        "a block row with neither a block nor a size": (_params([(0, 0, A), (2, 0, B)], 3, 1), ERR_INVALID),
        "a block column with neither a block nor a size": (_params([(0, 0, A), (0, 2, A)], 1, 3, row_sizes=[4]), ERR_INVALID),
        "a block that disagrees with its row's size": (_params([(0, 0, A)], 1, 1, row_sizes=[5]), ERR_INVALID),
        "a block that disagrees with its column's size": (_params([(0, 0, A)], 1, 1, col_sizes=[5]), ERR_INVALID),
        "two blocks of one block row that differ in rows": (_params([(0, 0, A), (0, 1, B)], 1, 2), ERR_INVALID),
        "two blocks of one block column that differ in cols": (_params([(0, 0, A), (1, 0, _dcsr(4, 7, 0))], 2, 1), ERR_INVALID),
        "entries but no row": (_params([(0, 0, _dcsr(0, 6, 3))], 1, 1), ERR_INVALID),
        "entries but no column": (_params([(0, 0, _dcsr(4, 0, 3))], 1, 1), ERR_INVALID),
        "more blocks than SPECK_BMAT_MAX_BLOCKS": (_params([(0, 0, A)], 1, 1, n_blocks=65537), ERR_DIM_LIMIT),
        "a block above 2^27 rows": (_params([(0, 0, _dcsr(big, 6, 3))], 1, 1), ERR_DIM_LIMIT),
        "a block above 2^27 columns": (_params([(0, 0, _dcsr(4, big, 3))], 1, 1), ERR_DIM_LIMIT),
        "rows of C above 2^27": (_params([(0, 0, _dcsr(1 << 26, 6, 0)), (1, 0, _dcsr(1 << 26, 6, 0)), (2, 0, _dcsr(1, 6, 0))], 3, 1), ERR_DIM_LIMIT),
        "cols of C above 2^27": (_params([(0, 0, A)], 1, 2, col_sizes=[6, 1 << 27]), ERR_DIM_LIMIT),
        "a size above 2^27": (_params([], 1, 1, row_sizes=[1 << 40], col_sizes=[3]), ERR_DIM_LIMIT),
        "2^32 pieces": (_params([(0, q, _dcsr(1 << 27, 1, 0)) for q in range(32)], 1, 32), ERR_DIM_LIMIT),
        "a block of 2^32 entries": (_params([(0, 0, _dcsr(4, 6, 1 << 32))], 1, 1), ERR_NNZ_OVERFLOW),
        "2^32 entries in two blocks": (_params([(0, 0, _dcsr(4, 6, 1 << 31)), (1, 0, _dcsr(4, 6, 1 << 31))], 2, 1), ERR_NNZ_OVERFLOW),
    }
    for field, m in hollow.items():
        r[f"nnz > 0 and a NULL {field}"] = (_params([(0, 0, A), (1, 0, m)], 2, 1), ERR_INVALID)
    return r


def test_layout_refuses_what_the_host_can_decide_and_writes_nothing():
    assert _lib.load().speck_bmat_layout(None, ctypes.byref(_lib.CBmatLayoutOut())) == ERR_INVALID
    p, keep = _params([(0, 0, _dcsr(4, 6, 3))], 1, 1)
    assert _lib.load().speck_bmat_layout(ctypes.byref(p), None) == ERR_INVALID
    for name, ((p, keep), status) in _refusals().items():
        rc, shape, ro, co = _layout(p)
        assert rc == status, name
        assert shape == (7, 7, 7, 7) and set(ro) == {7} and set(co) == {7}, name
    # one piece and one entry less than the limits pass
    p, keep = _params([(0, q, _dcsr(1 << 27, 1, 0)) for q in range(31)] + [(1, 0, _dcsr(0, 1, 0))], 2, 31)
    assert _layout(p)[:2] == (OK, (1 << 27, 31, 0, 31 << 27))
    p, keep = _params([(0, 0, _dcsr(4, 6, 1 << 31)), (1, 0, _dcsr(4, 6, (1 << 31) - 1))], 2, 1)
    assert _layout(p)[:2] == (OK, (8, 6, (1 << 32) - 1, 8))


def test_python_layout_and_return_offsets_agree_with_the_c_call():
    mats = [speck_amd.dCSR.from_device(r, c, n, 4096, 8192, 12288) for r, c, n in ((4, 6, 3), (0, 3, 0), (5, 0, 0), (9, 9, 11))]
    lay = speck_amd.bmat_layout([[mats[i] if i == j else None for j in range(4)] for i in range(4)])
    p, keep = _params([(i, i, m._c) for i, m in enumerate(mats)], 4, 4)
    rc, shape, ro, co = _layout(p)
    assert rc == OK and (lay.rows, lay.cols, lay.nnz, lay.pieces) == shape == (18, 18, 14, 18)
    assert list(lay.row_origins) == ro == [0, 4, 4, 9, 18] and list(lay.col_origins) == co == [0, 6, 9, 9, 18]
    lay = speck_amd.bmat_layout([[mats[0], None], [None, None]], row_sizes=[4, 2], col_sizes=[6, 1])
    assert (lay.rows, lay.cols, lay.nnz, lay.pieces, lay.row_origins, lay.col_origins) == (6, 7, 3, 4, (0, 4, 6), (0, 6, 7))
    assert repr(lay) == "BmatLayout(rows=6, cols=7, nnz=3, pieces=4)"


# ---------------------------------------------------------------------------------------------------- declarations
def test_header_library_and_table_agree():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P = ctypes.POINTER
    for name in ("speck_bmat_f64", "speck_bmat_f32"):
        assert name in declared and hasattr(lib, name) and name in _lib.declared_symbols(), name
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == [ctypes.c_void_p, P(_lib.CBmatParams), P(_lib.DCsr), P(_lib.CBmatInfo)]
        assert _kinds(header, name) == ["speck_config*", "constspeck_bmat_params*", "speck_dcsr*", "speck_bmat_info*"]
    name = "speck_bmat_layout"
    assert name in declared and hasattr(lib, name) and name in _lib.declared_symbols()
    assert _lib._SIGS[name] == (ctypes.c_int, [P(_lib.CBmatParams), P(_lib.CBmatLayoutOut)])
    assert _kinds(header, name) == ["constspeck_bmat_params*", "speck_bmat_layout_out*"]


def test_structs_hold_exactly_the_listed_fields():
    header = _header()
    P = ctypes.POINTER
    fields = _struct_fields(header, "speck_bmat_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CBmatInfo._fields_] == INFO_FIELDS
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CBmatInfo._fields_)
    assert ctypes.sizeof(_lib.CBmatInfo) == 8 * len(INFO_FIELDS)
    assert _struct_fields(header, "speck_bmat_block") == [("block_row", "uint32_t"), ("block_col", "uint32_t"), ("M", "const speck_dcsr *")]
    assert _lib.CBmatBlock._fields_ == [("block_row", ctypes.c_uint32), ("block_col", ctypes.c_uint32), ("M", P(_lib.DCsr))]
    assert ctypes.sizeof(_lib.CBmatBlock) == 16 and _lib.CBmatBlock.M.offset == 8
    assert _struct_fields(header, "speck_bmat_params") == [
        ("block_rows", "uint32_t"), ("block_cols", "uint32_t"), ("n_blocks", "uint32_t"), ("blocks", "const speck_bmat_block *"),
        ("row_sizes", "const uint64_t *"), ("col_sizes", "const uint64_t *")]
    assert _lib.CBmatParams._fields_ == [("block_rows", ctypes.c_uint32), ("block_cols", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32),
                                         ("blocks", P(_lib.CBmatBlock)), ("row_sizes", P(ctypes.c_uint64)), ("col_sizes", P(ctypes.c_uint64))]
    assert ctypes.sizeof(_lib.CBmatParams) == 40 and _lib.CBmatParams.blocks.offset == 16
    assert _struct_fields(header, "speck_bmat_layout_out") == [("rows", "uint64_t"), ("cols", "uint64_t"), ("nnz", "uint64_t"), ("pieces", "uint64_t"),
                                                              ("row_origins", "uint64_t *"), ("col_origins", "uint64_t *")]
    assert [f for f, _ in _lib.CBmatLayoutOut._fields_] == ["rows", "cols", "nnz", "pieces", "row_origins", "col_origins"]
    assert ctypes.sizeof(_lib.CBmatLayoutOut) == 48
    assert int(re.search(r"#define SPECK_BMAT_TILE_ENTRIES (\d+)", header).group(1)) == speck_amd.BMAT_TILE_ENTRIES == 4096
    assert int(re.search(r"#define SPECK_BMAT_MAX_BLOCKS (\d+)", header).group(1)) == speck_amd.BMAT_MAX_BLOCKS == 65536
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "bmat.hip")).read()
    assert "kTile = SPECK_BMAT_TILE_ENTRIES" in source


def test_the_header_names_what_is_not_built():
    block = re.search(r"/\* ---- assembly from blocks.*?---- \*/", _header(), re.S).group(0)
    not_built = re.sub(r"\s*\*\s+", " ", block[block.index("Not built:"):])
    for what in NOT_BUILT:
        assert what in not_built, what
    assert "OF ITS OWN BLOCK" in block                                             # the per-block id check
    # the two sentences the earlier blocks keep, word for word
    assert "hstack / vstack" in re.search(r"/\* ---- sub-matrix by index.*?---- \*/", _header(), re.S).group(0)
    assert "blocked or batched graphs" in _header()


def test_info_class_wraps_its_c_struct():
    values = dict(zip(INFO_FIELDS, range(1, 8)))
    c = _lib.CBmatInfo()
    for field, v in values.items():
        setattr(c, field, v)
    cls = speck_amd.BmatInfo
    assert cls is speck_amd.api.BmatInfo and cls.__name__ == "BmatInfo" and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values and all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == "BmatInfo(blocks=1, rows_out=2, cols_out=3, nnz_out=4, pieces=5, rows_empty=6, max_row_entries=7)"


def test_caller_that_includes_bmat_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_bmat.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["BMat.h"]
    out = str(tmp_path / "caller_bmat")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_values_move_as_integers_and_atomics_run_on_the_statistics_only():
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "bmat.hip")).read()
    code = re.sub(r"//[^\n]*", "", source)
    assert not re.findall(r"atomic\w+\(", code)                                    # (the two counters: offset_stats_kernel, scan.hpp)
    assert not re.search(r"\b(float|double)\b", code)                              # u32 / u64 stand for the two value types


# ---------------------------------------------------------------------------------------------------- argument checks
def test_bmat_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    kc = np.zeros(1024, dtype=np.uint64)
    pc = kc.ctypes.data
    ref = ctypes.byref
    for fn in (L.speck_bmat_f64, L.speck_bmat_f32):
        def call(p, out=True, C=None):
            C = _mat(9, 9, 9, pc) if C is None else C
            before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
            info = _lib.CBmatInfo(*([7] * 7))
            rc = fn(None, ref(p) if p is not None else None, ref(C) if out else None, ref(info))
            assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before       # the struct keeps its sentinel
            assert [getattr(info, f) for f in INFO_FIELDS] == [7] * 7                        # ... and so does *info
            return rc

        good, keep = _params([(0, 0, _dcsr(4, 6, 3))], 1, 1)
        assert call(None) == ERR_INVALID                                            # NULL params
        assert call(good, out=False) == ERR_INVALID                                 # NULL C
        for name, ((p, keep2), status) in _refusals().items():
            assert call(p) == status, name
        # C sharing a buffer with any block -- the first, the last
        A, B = _dcsr(4, 6, 3), _dcsr(5, 6, 2, ptr=65536)
        p, keep2 = _params([(0, 0, A), (1, 0, B)], 2, 1)
        for M in (A, B):
            for field in ("row_offsets", "col_ids", "data"):
                C = _mat(9, 9, 9, pc)
                setattr(C, field, getattr(M, field))
                assert call(p, C=C) == ERR_INVALID, field
    assert not kc.any()


def test_without_a_gpu_it_fails_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    kc = np.zeros(1024, dtype=np.uint64)
    A, B = _dcsr(4, 6, 3), _dcsr(5, 6, 2, ptr=65536)
    sound = [_params([(1, 0, B), (0, 0, A)], 2, 1), _params([(0, 0, A), (1, 1, B)], 2, 2), _params([(0, 0, A)], 2, 2, row_sizes=[4, 1], col_sizes=[6, 0]),
             _params([], 2, 1, row_sizes=[3, 0], col_sizes=[5]), _params([], 0, 0, row_sizes=[], col_sizes=[]), _params([(0, 0, _dcsr(0, 0, 0))], 1, 1)]
    for fn in (L.speck_bmat_f64, L.speck_bmat_f32):
        for p, keep in sound:
            for C in (_lib.DCsr(), _mat(9, 9, 9, kc.ctypes.data)):
                before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
                info = _lib.CBmatInfo(*([7] * 7))
                assert fn(None, ctypes.byref(p), ctypes.byref(C), ctypes.byref(info)) == no_device
                assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before
                assert [getattr(info, f) for f in INFO_FIELDS] == [0] * 7           # the arguments have passed: *info is zero
    dA = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    for call in (lambda: speck_amd.vstack([dA, dA], None), lambda: speck_amd.hstack([dA, dA], None), lambda: speck_amd.block_diag([dA, dA], None),
                 lambda: speck_amd.bmat([[dA, None], [None, dA]], None)):
        with pytest.raises(speck_amd.SpeckError) as e:
            call()
        assert e.value.status == no_device
    assert not kc.any()


# ---------------------------------------------------------------------------------------------------- the Python wrappers
def test_python_refuses_wrong_grids_before_it_asks_for_an_address():
    A = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    B = speck_amd.dCSR.from_device(5, 6, 2, 4096, 8192, 12288)
    F = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288, dtype=np.float32)
    tensor = Block((4, 6), dtype="float64")                                        # (asked for its address, it raises)
    with pytest.raises(ValueError, match="bmat: blocks is ragged"):
        speck_amd.bmat([[A, None], [B]], None)
    with pytest.raises(ValueError, match="bmat: blocks must be a list of lists"):
        speck_amd.bmat([A, B], None)
    for foreign in (tensor, "a string", 1.5, np.zeros((4, 6))):
        with pytest.raises(ValueError, match=r"bmat: the cell \(1, 0\) must be a dCSR or None"):
            speck_amd.bmat([[A], [foreign]], None)
        for fn, who in ((speck_amd.vstack, "vstack"), (speck_amd.hstack, "hstack"), (speck_amd.block_diag, "block_diag")):
            with pytest.raises(ValueError, match=f"{who}: mats must be a list of dCSR"):
                fn([A, foreign], None)
    with pytest.raises(TypeError, match="bmat: the blocks hold .*float32.*float64.*mixed value type are not converted"):
        speck_amd.bmat([[A], [F]], None)
    for fn in (speck_amd.vstack, speck_amd.hstack, speck_amd.block_diag):
        with pytest.raises(TypeError, match="mixed value type"):
            fn([A, F], None)
    with pytest.raises(ValueError, match="bmat: block row 1 has neither a block nor a size"):
        speck_amd.bmat([[A, None], [None, None]], None, col_sizes=[6, 2])
    with pytest.raises(ValueError, match="bmat: block column 1 has neither a block nor a size"):
        speck_amd.bmat([[A, None], [None, None]], None, row_sizes=[4, 2])
    with pytest.raises(ValueError, match="bmat: row_sizes must hold 2 non-negative integers"):
        speck_amd.bmat([[A, None], [None, None]], None, row_sizes=[4], col_sizes=[6, 2])
    with pytest.raises(ValueError, match="bmat: col_sizes must hold 2 non-negative integers"):
        speck_amd.bmat([[A, None], [None, None]], None, row_sizes=[4, 2], col_sizes=[6, -1])
    for fn, who in ((speck_amd.vstack, "vstack"), (speck_amd.hstack, "hstack"), (speck_amd.block_diag, "block_diag")):
        with pytest.raises(ValueError, match=f"{who}: matOut is one of the blocks"):
            fn([B, A], None, matOut=A)
    with pytest.raises(ValueError, match="bmat: matOut is one of the blocks"):
        speck_amd.bmat([[A, None], [None, B]], None, matOut=B)
    with pytest.raises(ValueError, match="vstack: mats is empty"):
        speck_amd.vstack([], None)
    # what only the C call decides comes back as its status: blocks of one block row that differ in rows
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.hstack([A, B], None)
    assert e.value.status == ERR_INVALID
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.bmat_layout([[A, B]])
    assert e.value.status == ERR_INVALID
