"""speck_extract_* on the GPU (speck_amd/csrc/extract.hip).  The expectation is the numpy statement of the contract
(tests/test_extract_host.py, numpy_extract, which that file compares with scipy), compared byte for byte.  The value of an
entry of A is its position -- as an integer at even positions, in the payload of a NaN at odd ones --, so the order of the
result is visible and a value that went through arithmetic would lose its bits.  Device arrays the library must not touch,
or must fill exactly, live in frames of a payload byte whose padding must survive.  T = 4096 gathered ("gross") entries per
tile of the marking and placing passes, a thread holds 4 consecutive ones; LDS holds the rows of a tile up to 4096 of them."""
import ctypes as C_
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib
from test_extract_host import DROP32, INFO_FIELDS, bits, numpy_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NNZ_OVERFLOW = 0, 1, 5
DEV = "cuda:0"
T = sa.EXTRACT_TILE_ENTRIES
PER = 4                                   # entries a thread holds: one word of keep bytes
LDS_ROWS = 4096                           # rows of a tile that LDS holds; a tile more rows touch reads them from global memory
PAYLOAD = 0xC3
PAD = 64                                  # payload bytes on either side of a frame
COMBOS = [(np.float64, 8), (np.float64, 4), (np.float32, 8), (np.float32, 4)]
COMBO_IDS = ["f64-i64", "f64-u32", "f32-i64", "f32-u32"]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def dev_ids(a, iw, shift=0):
    """the ids on the device, 8 bytes (int64) or 4 bytes (uint32 bits in an int32 tensor) wide, one at least (an empty tensor
    has no address); shift: the array starts that many ids behind an aligned address"""
    a = np.asarray(a, dtype=np.int64)
    h = a if iw == 8 else (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    t = torch.from_numpy(np.concatenate([np.zeros(shift, h.dtype), h, np.zeros(1 if len(h) == 0 else 0, h.dtype)])).to(DEV)
    return t[shift:]


def pos_values(n, vdtype):
    """the position of every entry: the number at even positions, a NaN with the position for a payload at odd ones"""
    pos = np.arange(n, dtype=np.uint64)
    if vdtype == np.float64:
        b = np.where(pos % 2 == 0, pos.astype(np.float64).view(np.uint64), np.uint64(0x7FF8000000000000) | pos)
        return b.view(np.float64)
    assert n <= 1 << 22
    b = np.where(pos % 2 == 0, pos.astype(np.float32).view(np.uint32), np.uint32(0x7FC00000) | pos.astype(np.uint32))
    return b.astype(np.uint32).view(np.float32)


def host_csr(lens, cols, vdtype=np.float64, seed=1, col=None):
    """rows of the given lengths; column ids at random (unsorted, duplicates among them) unless given"""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    ci = np.random.default_rng(seed).integers(0, max(cols, 1), size=n) if col is None else np.asarray(col)
    return sa.HostCSR(len(lens), cols, ro, ci.astype(np.uint32), pos_values(n, vdtype))


def random_map(cols, out_cols, seed, drop=0.3):
    """not injective, not monotone, about `drop` of the columns dropped"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, max(out_cols, 1), size=cols)
    m[rng.random(cols) < drop] = -1
    return m


def want_of(H, p, cmap, out_cols, iw):
    m = None if cmap is None else (np.asarray(cmap, dtype=np.int64) & DROP32 if iw == 4 else np.asarray(cmap, dtype=np.int64))
    return numpy_extract(H.row_offsets, H.col_ids, H.data, p, m, H.cols, out_cols, index_bytes=iw)


def call(cfg, dA, p, cmap, out_cols, iw, C=None, shift=0, n_rows=None, index_ptr=None, map_ptr=None):
    """(status, C, ExtractInfo); p / cmap: numpy arrays or None; index_ptr / map_ptr: device addresses instead"""
    prm = _lib.CExtractParams()
    keep = [dev_ids(p, iw, shift) if p is not None else None, dev_ids(cmap, iw, shift) if cmap is not None else None]
    prm.n_rows = (len(p) if p is not None else dA.rows) if n_rows is None else n_rows
    prm.out_cols, prm.index_bytes = out_cols, iw
    prm.d_row_index = index_ptr if index_ptr is not None else keep[0].data_ptr() if p is not None else None
    prm.d_col_map = map_ptr if map_ptr is not None else keep[1].data_ptr() if cmap is not None else None
    C = sa.dCSR(dA.dtype) if C is None else C
    info = _lib.CExtractInfo(*([7] * 7))
    fn = _lib.load().speck_extract_f32 if dA.dtype == np.float32 else _lib.load().speck_extract_f64
    rc = fn(cfg._h if cfg is not None else None, C_.byref(dA._c), C_.byref(prm), C_.byref(C._c), C_.byref(info))
    torch.cuda.synchronize()
    del keep
    return rc, C, sa.ExtractInfo(info)


def check(C, info, want, out_cols):
    ro, ci, vb, winfo = want
    assert (C.rows, C.cols, C.nnz) == (len(ro) - 1, out_cols, len(ci))
    assert C._c.data and C._c.col_ids and C._c.row_offsets                          # (buffers of one entry where nnz is 0)
    H = C.to_host()
    assert np.array_equal(H.row_offsets, ro), "row_offsets"
    assert np.array_equal(H.col_ids, ci), "col_ids"
    assert np.array_equal(bits(H.data), vb), "values"
    assert vars(info) == winfo


def run_case(cfg, H, p, cmap, out_cols, iw, shift=0, cfg_none=False, dA=None):
    dA = sa.dCSR.from_host(H) if dA is None else dA
    rc, C, info = call(None if cfg_none else cfg, dA, p, cmap, out_cols, iw, shift=shift)
    assert rc == OK
    check(C, info, want_of(H, p, cmap, out_cols, iw), out_cols)
    return C, info


def frame(nbytes):
    """(tensor, address): nbytes of the payload between two pads of it"""
    t = torch.full((nbytes + 2 * PAD,), PAYLOAD, dtype=torch.uint8, device=DEV)
    return t, t.data_ptr() + PAD


def frame_bytes(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def untouched(*frames):
    return all(bool((frame_bytes(t) == PAYLOAD).all()) for t in frames)


def framed(t, nbytes, dtype):
    """the nbytes of a frame as `dtype`, after checking that both pads still hold the payload"""
    b = frame_bytes(t)
    assert (b[:PAD] == PAYLOAD).all() and (b[PAD + nbytes:] == PAYLOAD).all(), "a pad of the frame"
    return b[PAD:PAD + nbytes].copy().view(dtype)


def framed_c(rows, cols, nnz, vdtype):
    """a C whose three arrays are frames of the payload: what a call reuses when rows and nnz match (non-owning)"""
    vs = np.dtype(vdtype).itemsize
    fd, fc, fr = frame(max(nnz, 1) * vs), frame(max(nnz, 1) * 4), frame((rows + 1) * 4)
    C = sa.dCSR.from_device(rows, cols, nnz, fr[1], fc[1], fd[1], dtype=vdtype, keep=(fd, fc, fr))
    return C, (fd[0], fc[0], fr[0])


def struct_of(C):
    return (C._c.rows, C._c.cols, C._c.nnz, C._c.data, C._c.col_ids, C._c.row_offsets)


# ---------------------------------------------------------------------------------------------------- 1: types, alignment, views
@functools.lru_cache(maxsize=None)
def mixed_case(vdtype):
    """short rows, empty rows, rows at both sides of a tile and a hub of 2 T + 5; an index with repeats; a map that drops"""
    rng = np.random.default_rng(7)
    lens = np.concatenate([rng.integers(0, 9, size=700), [2 * T + 5, 0, 0, T - 1, 1, T], rng.integers(0, 40, size=300)])
    H = host_csr(lens, 5000, vdtype, seed=8)
    p = rng.integers(0, H.rows, size=1500)
    p[[3, 700, 1499]] = 700                                                         # the hub three times
    return H, p, random_map(5000, 333, seed=9)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cfg_none", [False, True], ids=["cfg", "no-cfg"])
def test_value_and_index_types(cfg, cfg_none, vdtype, iw):
    H, p, cmap = mixed_case(vdtype)
    run_case(cfg, H, p, cmap, 333, iw, cfg_none=cfg_none)
    run_case(cfg, H, p, None, 5000, iw, cfg_none=cfg_none)                          # no map: nothing is marked
    run_case(cfg, H, None, cmap, 333, iw, cfg_none=cfg_none)                        # no index: every row


@pytest.mark.parametrize("iw", [8, 4])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_index_and_map_that_start_off_an_aligned_address(cfg, shift, iw):
    H, p, cmap = mixed_case(np.float64)
    run_case(cfg, H, p, cmap, 333, iw, shift=shift)


def test_same_bytes_from_run_to_run(cfg):
    H, p, cmap = mixed_case(np.float64)
    dA = sa.dCSR.from_host(H)
    for _ in range(3):
        run_case(cfg, H, p, cmap, 333, 8, dA=dA)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_a_view_gives_what_its_copy_gives(cfg, vdtype, iw):
    H, _, cmap = mixed_case(vdtype)
    dA = sa.dCSR.from_host(H)
    r0, r1 = int(np.nonzero(H.row_offsets % 2 == 1)[0][0]), H.rows - 2               # an odd first offset
    V = dA.row_view(r0, r1)
    assert int(H.row_offsets[r0]) % 2 == 1 and 0 < r0 < 50
    rng = np.random.default_rng(12)
    p = rng.integers(0, r1 - r0, size=900)
    p[:2] = [0, r1 - r0 - 1]
    view_h = sa.HostCSR(r1 - r0, H.cols, H.row_offsets[r0:r1 + 1], H.col_ids, H.data)
    want = want_of(view_h, p, cmap, 333, iw)
    rc, C, info = call(cfg, V, p, cmap, 333, iw)
    assert rc == OK
    check(C, info, want, 333)
    rc, C2, info2 = call(cfg, V.copy(), p, cmap, 333, iw)
    assert rc == OK
    check(C2, info2, want, 333)
    rc, C3, info3 = call(cfg, V, None, None, H.cols, iw)                            # identity on the view: its copy, offsets rebased
    assert rc == OK
    G, W = C3.to_host(), V.copy().to_host()
    assert np.array_equal(G.row_offsets, W.row_offsets) and np.array_equal(G.col_ids, W.col_ids) and np.array_equal(bits(G.data), bits(W.data))


# ---------------------------------------------------------------------------------------------------- 2: gross-tile edges
def edge_cases():
    """name -> (row lengths of A, index or None)"""
    c = {}
    for g in (T - 1, T, T + 1):
        c[f"one row of {g}"] = ([g], None)
        c[f"rows that end at {g}"] = ([1000, 7, g - 1000], [0, 2])
        c[f"two tiles that end at {T + g}"] = ([T - 3, 3 + g], None)
    c["rows that start and end inside one thread's four"] = ([1, 2, 1, 3, 1, 1, 1, 2, 4, 4, 5, 1, 1, 1, 1, 7], None)
    c["one row of three tiles"] = ([3, 2 * T + 5, 2], None)
    c["the row of three tiles three times in a row"] = ([3, 2 * T + 5, 2], [0, 1, 1, 1, 2])
    c["empty rows in front of a tile edge"] = ([0, T - 1, 0, 0, 3, 0], None)
    c["empty rows on a tile edge"] = ([0, T, 0, 0, 3, 0], None)
    c["empty rows behind a tile edge"] = ([T + 1, 0, 0, 3, 0], None)
    c["empty rows on two edges, a row that ends on the second"] = ([0, T - 2, 0, 0, 2, 0, 0, T, 0, 5, 0], None)
    c["a first and a last row that are empty"] = ([0, 5, 0], None)
    c["only empty rows"] = ([0, 0, 0], None)
    c["an empty row many times"] = ([5, 0], [1] * 70)
    c[f"{T} rows of 1"] = ([1] * T, None)
    c[f"{T + 1} rows of 1"] = ([1] * (T + 1), None)
    for g in (0, 1, 3, 4, 5):
        c[f"gross {g}"] = ([0, g, 0], None)
    # more rows than LDS holds touch one tile
    c["5000 empty rows between two entries"] = ([2] + [0] * 5000 + [3] + [1] * 100, None)
    c[f"{T + 1} rows of 1 between empty rows"] = ([1, 0] * (T + 1), None)
    c[f"exactly {LDS_ROWS} and {LDS_ROWS + 1} rows in a tile"] = ([1] + [0] * (LDS_ROWS - 2) + [T - 1] + [1] + [0] * (LDS_ROWS - 1) + [T - 1, 9], None)
    return c


EDGE_CASES = edge_cases()


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_gross_tile_edges(cfg, name, vdtype, iw):
    lens, p = EDGE_CASES[name]
    H = host_csr(lens, 600, vdtype, seed=len(lens))
    dA = sa.dCSR.from_host(H)
    _, info = run_case(cfg, H, p, random_map(600, 900, seed=2), 900, iw, dA=dA)
    assert info.gross == int(np.asarray(lens)[np.arange(len(lens)) if p is None else p].sum())
    run_case(cfg, H, p, None, 600, iw, dA=dA)


# ---------------------------------------------------------------------------------------------------- 3: drops by position
def positional(n_entries, lens=None):
    """a matrix whose entry at position e has the column id e: map[e] decides about position e"""
    return host_csr([n_entries] if lens is None else lens, n_entries, col=np.arange(n_entries))


def keep_map(keep):
    """kept positions get a new id (descending, so the map is not monotone), the others are dropped"""
    keep = np.asarray(keep, dtype=bool)
    return np.where(keep, len(keep) - 1 - np.arange(len(keep)), -1)


DROPS = {
    "alternating inside a word": lambda e: e % 2 == 0,
    "the other half of every word": lambda e: e % 2 == 1,
    "0110 1001": lambda e: np.isin(e % 8, [1, 2, 4, 7]),
    "a whole word dropped": lambda e: e // PER != 5,
    "every second word dropped": lambda e: (e // PER) % 2 == 0,
    "a whole tile dropped": lambda e: e // T != 1,
    "only the first tile kept": lambda e: e < T,
    "the only kept entry in the middle tile": lambda e: e == T + T // 2 + 1,
    "the last entry alone": lambda e: e == 2 * T + 4,
    "everything kept": lambda e: e >= 0,
}


@pytest.mark.parametrize("iw", [8, 4])
@pytest.mark.parametrize("name", list(DROPS))
def test_drops_placed_by_position(cfg, name, iw):
    n = 2 * T + 5
    keep = DROPS[name](np.arange(n))
    for lens in ([n], [3, 1, T - 4, 0, T + 1, 4]):                                  # one row of three tiles; rows around the edges
        H = positional(n, lens)
        C, info = run_case(cfg, H, None, keep_map(keep), n, iw)
        assert info.nnz_out == int(keep.sum()) and info.dropped == n - info.nnz_out and info.cols_kept == info.nnz_out


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_everything_dropped(cfg, vdtype, iw):
    H = host_csr([3, 2 * T + 5, 0, 2], 600, vdtype)
    C, info = run_case(cfg, H, [1, 0, 3, 1], np.full(600, -1), 4, iw)
    assert C.nnz == 0 and info.nnz_out == 0 and info.rows_empty == 4 and info.cols_kept == 0 and info.max_row_entries == 0
    assert C._c.data and C._c.col_ids                                               # one-entry buffers of its own


# ---------------------------------------------------------------------------------------------------- 4: maps and index lists
@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_identity_is_the_copy(cfg, vdtype, iw):
    H, _, _ = mixed_case(vdtype)
    dA = sa.dCSR.from_host(H)
    rc, C, info = call(cfg, dA, None, None, H.cols, iw)
    assert rc == OK
    G, W = C.to_host(), dA.copy().to_host()
    assert np.array_equal(G.row_offsets, W.row_offsets) and np.array_equal(G.col_ids, W.col_ids) and np.array_equal(bits(G.data), bits(W.data))
    assert vars(info) == dict(rows_out=H.rows, rows_empty=int((np.diff(H.row_offsets.astype(np.int64)) == 0).sum()), gross=H.nnz,
                              nnz_out=H.nnz, dropped=0, cols_kept=H.cols, max_row_entries=2 * T + 5)


@pytest.mark.parametrize("iw", [8, 4])
def test_maps(cfg, iw):
    H, p, _ = mixed_case(np.float64)
    dA = sa.dCSR.from_host(H)
    cols = H.cols
    run_case(cfg, H, p, cols - 1 - np.arange(cols), cols, iw, dA=dA)                # reverse
    two_to_one = np.arange(cols) // 2                                               # columns 2 j and 2 j + 1 become j: duplicates stay,
    C, info = run_case(cfg, H, p, two_to_one, cols // 2, iw, dA=dA)                 #   in input order
    assert info.dropped == 0
    run_case(cfg, H, p, random_map(cols, 17, seed=3), 17, iw, dA=dA)                # out_cols far below cols
    run_case(cfg, H, p, np.arange(cols) * 3 + 1, 3 * cols + 5, iw, dA=dA)           # ... and above
    run_case(cfg, H, p, np.arange(cols) + ((1 << 27) - cols), 1 << 27, iw, dA=dA)   # the largest id there is
    run_case(cfg, H, None, np.arange(cols), cols, iw, dA=dA)                        # an identity that is spelled out


@pytest.mark.parametrize("iw", [8, 4])
def test_index_lists(cfg, iw):
    H, _, cmap = mixed_case(np.float64)
    dA = sa.dCSR.from_host(H)
    rows = H.rows
    run_case(cfg, H, np.arange(rows)[::-1], cmap, 333, iw, dA=dA)                   # reversed
    run_case(cfg, H, np.repeat(np.arange(rows), 2), cmap, 333, iw, dA=dA)           # every row twice
    run_case(cfg, H, np.tile(np.arange(rows), 2), None, H.cols, iw, dA=dA)          # the matrix twice
    _, info = run_case(cfg, H, np.full(37, 700), None, H.cols, iw, dA=dA)           # the hub 37 times
    assert info.gross == 37 * (2 * T + 5)
    C, info = run_case(cfg, H, np.zeros(0, dtype=np.int64), cmap, 333, iw, dA=dA)   # no row at all
    assert (C.rows, C.cols, C.nnz) == (0, 333, 0)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_a_permutation_and_its_inverse_give_the_matrix_back(cfg, vdtype, iw):
    H, _, _ = mixed_case(vdtype)
    dA = sa.dCSR.from_host(H)
    rng = np.random.default_rng(31)
    rp, cp = rng.permutation(H.rows), rng.permutation(H.cols)
    rc, B, _ = call(cfg, dA, rp, cp, H.cols, iw)
    assert rc == OK
    rc, back, info = call(cfg, B, np.argsort(rp), np.argsort(cp), H.cols, iw)
    assert rc == OK and info.dropped == 0
    G = back.to_host()
    assert np.array_equal(G.row_offsets, H.row_offsets) and np.array_equal(G.col_ids, H.col_ids) and np.array_equal(bits(G.data), bits(H.data))


# ---------------------------------------------------------------------------------------------------- 5: compositions
def scipy_graph(n, per_row, seed):
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=per_row / n, format="csr", random_state=rng, dtype=np.float64)
    S.data = rng.integers(1, 9, size=S.nnz).astype(np.float64)
    S.sort_indices()
    return S


def to_device(S):
    return sa.dCSR.from_host(sa.HostCSR(S.shape[0], S.shape[1], S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.copy()))


def same_as_scipy(C, W):
    W = W.tocsr()
    W.sort_indices()
    G = C.to_host()
    return (C.rows, C.cols) == W.shape and np.array_equal(G.row_offsets, W.indptr) and np.array_equal(G.col_ids, W.indices) and \
        np.array_equal(G.data, W.data)


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_induced_subgraph_against_scipy_and_into_the_multiply(cfg, index_dtype):
    from oracle import pyoracle as po
    S = scipy_graph(2000, 12, seed=41)
    dA = to_device(S)
    nodes = np.random.default_rng(42).permutation(2000)[:700]
    C, info = sa.induced_subgraph(dA, torch.from_numpy(nodes).to(DEV).to(index_dtype), cfg)
    W = S[nodes][:, nodes]
    assert same_as_scipy(C, W) and info.rows_out == 700 and info.cols_kept == 700 and info.nnz_out == W.nnz
    raw, _ = sa.induced_subgraph(dA, torch.from_numpy(nodes).to(DEV).to(index_dtype), cfg, canonical=False)
    assert raw.nnz == W.nnz and not same_as_scipy(raw, W)                           # the rows keep A's order until they are sorted
    out = sa.dCSR()
    sa.MultiplyspECK(C, C, out, cfg, sa.Timings())                                  # speck_multiply_f64 takes the canonical result
    G = C.to_host()
    R, _ = po.spgemm(po.HostCSR(700, 700, G.row_offsets, G.col_ids, G.data), po.HostCSR(700, 700, G.row_offsets, G.col_ids, G.data))
    P = out.to_host()
    assert np.array_equal(P.row_offsets, R.row_offsets) and np.array_equal(P.col_ids, R.col_ids) and np.array_equal(P.data, R.data)


def test_permute_select_columns_and_gather_rows_against_scipy(cfg):
    S = scipy_graph(1500, 9, seed=43)
    dA = to_device(S)
    rng = np.random.default_rng(44)
    perm = rng.permutation(1500)
    perm_t = torch.from_numpy(perm).to(DEV)
    C, info = sa.permute(dA, perm_t, perm_t, cfg)
    assert info.dropped == 0 and not same_as_scipy(C, S[perm][:, perm])
    sa.sort_rows(C, cfg)
    assert same_as_scipy(C, S[perm][:, perm])
    assert same_as_scipy(sa.permute(dA, row_perm=perm_t, config=cfg)[0], S[perm])
    assert same_as_scipy(sa.permute(dA, col_perm=perm_t, config=cfg, canonical=True)[0], S[:, perm])
    cols = rng.permutation(1500)[:400]
    assert same_as_scipy(sa.select_columns(dA, torch.from_numpy(cols).to(DEV), cfg, canonical=True)[0], S[:, cols])
    rows = rng.integers(0, 1500, size=2222)                                         # with replacement
    assert same_as_scipy(sa.gather_rows(dA, torch.from_numpy(rows).to(DEV).to(torch.int32), cfg)[0], S[rows])
    # an aggregation: a map that is not injective, then the duplicates summed, is A P
    agg = rng.integers(0, 50, size=1500)
    C, _ = sa.extract(dA, col_map=torch.from_numpy(agg).to(DEV), out_cols=50, config=cfg, sum_duplicates=True)
    assert same_as_scipy(C, S @ sp.csr_matrix((np.ones(1500), (np.arange(1500), agg)), shape=(1500, 50)))


# ---------------------------------------------------------------------------------------------------- 6: refusals
def refusal_case(vdtype, iw):
    rng = np.random.default_rng(51)
    lens = np.concatenate([rng.integers(1, 9, size=400), [2 * T + 5], rng.integers(1, 9, size=99)])
    H = host_csr(lens, 800, vdtype, seed=52)
    p = rng.integers(0, 500, size=700)
    cmap = random_map(800, 300, seed=53)
    return H, p, cmap, want_of(H, p, cmap, 300, iw)


def device_matrix(H, ro=None, col=None, nnz=None):
    """A from torch tensors (the upload would not take hostile offsets or ids)"""
    ro_t = torch.from_numpy(np.asarray(H.row_offsets if ro is None else ro, dtype=np.uint32).view(np.int32)).to(DEV)
    col_t = torch.from_numpy(np.asarray(H.col_ids if col is None else col, dtype=np.uint32).view(np.int32)).to(DEV)
    val_t = torch.from_numpy(H.data).to(DEV)
    return sa.dCSR.from_device(H.rows, H.cols, H.nnz if nnz is None else nnz, ro_t.data_ptr(), col_t.data_ptr(), val_t.data_ptr(),
                               dtype=H.data.dtype, keep=(ro_t, col_t, val_t))


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_hostile_input_is_refused_with_nothing_written(cfg, vdtype, iw):
    H, p, cmap, want = refusal_case(vdtype, iw)
    n, nnz_out = len(p), len(want[1])
    dA = device_matrix(H)
    C, frames = framed_c(n, 300, nnz_out, vdtype)                                   # rows and nnz match: every buffer would be reused
    before = struct_of(C)

    def refused(A, p2, m2, out_cols=300, what=None, **kw):
        rc, _, info = call(cfg, A, p2, m2, out_cols, iw, C=C, **kw)
        assert rc == ERR_INVALID, what
        assert struct_of(C) == before and list(vars(info).values()) == [0] * 7, what
        assert untouched(*frames), what

    # a row index that is rows, -1 or 2^32 + 3 (four bytes wide: rows and 2^32 - 1), first, middle, last
    for bad in [H.rows, (1 << 32) - 1] + ([-1, (1 << 32) + 3, -(1 << 63)] if iw == 8 else []):
        for at in (0, n // 2, n - 1):
            p2 = p.copy()
            p2[at] = bad
            refused(dA, p2, cmap, what=("index", bad, at))
    # a map value that is out_cols (referenced or not: every entry is checked), or anything above
    for bad in [300, 301, (1 << 32) - 2] + ([(1 << 32) + 3, (1 << 62)] if iw == 8 else []):
        for at in (0, 399, 799):
            m2 = cmap.copy()
            m2[at] = bad
            refused(dA, p, m2, what=("map", bad, at))
    # an id >= cols in a gathered row is found before it indexes the map -- with a map and without one
    ids_case(cfg, H, p, cmap, iw, vdtype)
    # offsets: a descent, an offset beyond the entries, a last offset short of nnz -- in rows nobody gathers, too
    unused = int(np.setdiff1d(np.arange(1, H.rows - 1), p)[0])
    used = int(p[(p > 0) & (p < H.rows - 1)][0])
    for what, change in (("a descent in a row nobody gathers", lambda ro: ro.__setitem__(unused, ro[unused + 1] + 1)),
                         ("a descent in a gathered row", lambda ro: ro.__setitem__(used, ro[used + 1] + 1)),
                         ("an offset beyond the entries", lambda ro: ro.__setitem__(slice(401, None), H.nnz + 1)),
                         ("an offset near 2^32", lambda ro: ro.__setitem__(slice(401, None), 0xFFFFFFF0)),
                         ("a last offset short of nnz", lambda ro: ro.__setitem__(H.rows, H.nnz - 1))):
        ro = H.row_offsets.copy()
        change(ro)
        refused(device_matrix(H, ro=ro), p, cmap, what=what)
    refused(device_matrix(H, nnz=H.nnz - 1), p, cmap, what="the declared nnz is what the rows hold")
    # ... and the clean call fills exactly the three arrays
    rc, _, info = call(cfg, dA, p, cmap, 300, iw, C=C)
    assert rc == OK and struct_of(C) == before and vars(info) == want[3]
    vs = np.dtype(vdtype).itemsize
    assert np.array_equal(framed(frames[2], (n + 1) * 4, np.uint32), want[0])
    assert np.array_equal(framed(frames[1], nnz_out * 4, np.uint32), want[1])
    assert np.array_equal(framed(frames[0], nnz_out * vs, want[2].dtype), want[2])


def ids_case(cfg, H, p, cmap, iw, vdtype):
    """an id >= cols: refused where its row is gathered -- with a map and without --, never read where it is not"""
    unused = int(np.setdiff1d(np.arange(H.rows), p)[0])
    hub = 400
    p_hub = np.append(p, hub)
    for row, at_in_row in ((int(p[0]), 0), (hub, T + 7), (hub, 2 * T + 4), (int(p[-1]), -1)):
        a, b = int(H.row_offsets[row]), int(H.row_offsets[row + 1])
        at = a + at_in_row if at_in_row >= 0 else b - 1
        for bad in (H.cols, 0xFFFFFFFF):
            col = H.col_ids.copy()
            col[at] = bad
            A = device_matrix(H, col=col)
            for m2, out_cols in ((cmap, 300), (None, H.cols)):
                want = want_of(H, p_hub, m2, out_cols, iw)
                C, frames = framed_c(len(p_hub), out_cols, len(want[1]), vdtype)
                before = struct_of(C)
                rc, _, info = call(cfg, A, p_hub, m2, out_cols, iw, C=C)
                assert rc == ERR_INVALID and struct_of(C) == before and untouched(*frames), (row, at, bad)
                assert list(vars(info).values()) == [0] * 7
    # the same kind of id in a row that is NOT gathered: served
    col = H.col_ids.copy()
    col[int(H.row_offsets[unused])] = H.cols
    A = device_matrix(H, col=col)
    for m2, out_cols in ((cmap, 300), (None, H.cols)):
        rc, C, info = call(cfg, A, p, m2, out_cols, iw)
        assert rc == OK
        check(C, info, want_of(H, p, m2, out_cols, iw), out_cols)
    rc, _, _ = call(cfg, A, None, cmap, 300, iw)                                    # ... and refused once every row is
    assert rc == ERR_INVALID


@pytest.mark.parametrize("iw", [8, 4])
def test_an_index_or_a_map_inside_a_matrix_is_refused(cfg, iw):
    H, p, cmap, want = refusal_case(np.float64, iw)
    dA = sa.dCSR.from_host(H)
    C, frames = framed_c(len(p), 300, len(want[1]), np.float64)
    before = struct_of(C)
    V = dA.row_view(5, H.rows - 1)                                                  # its entries start at an offset only the device knows
    base = int(H.row_offsets[5])
    good_i, good_m = dev_ids(p, iw), dev_ids(cmap, iw)
    for A, inside in ((dA, dA._c.col_ids), (dA, dA._c.data + 8), (dA, dA._c.row_offsets + 4),
                      (V, dA._c.col_ids + 4 * base), (V, dA._c.col_ids + 4 * (base + V.nnz) - 1), (V, dA._c.data + 8 * base + 16),
                      (dA, C._c.data + 16), (dA, C._c.col_ids), (dA, C._c.row_offsets + 4 * len(p))):
        for kw in (dict(index_ptr=inside, map_ptr=good_m.data_ptr()), dict(index_ptr=good_i.data_ptr(), map_ptr=inside)):
            rc, _, info = call(cfg, A, p % A.rows, cmap, 300, iw, C=C, **kw)
            assert rc == ERR_INVALID and struct_of(C) == before and untouched(*frames), (inside, kw)
    rc, _, _ = call(cfg, dA, p, cmap, 300, iw, C=dA)                                # C sharing its buffers with A
    assert rc == ERR_INVALID
    assert np.array_equal(dA.to_host().col_ids, H.col_ids) and np.array_equal(bits(dA.to_host().data), bits(H.data))


def test_gathered_entries_beyond_32_bits_are_refused_before_anything_is_allocated(cfg):
    # one row of 65536 entries gathered 65536 times: 2^32 gathered entries exactly -- a 32-bit sum would wrap to 0 and
    # "succeed" with an empty result.  Only the check pass ever runs.  (One time less fits, and would take about 50 GB.)
    n = 1 << 16
    H = host_csr([3, n, 2], 1000)
    dA = sa.dCSR.from_host(H)
    for cmap, out_cols in ((None, 1000), (random_map(1000, 50, seed=1), 50)):
        C = sa.dCSR()
        rc, _, info = call(cfg, dA, np.full(n, 1), cmap, out_cols, 8, C=C)
        assert rc == ERR_NNZ_OVERFLOW
        assert struct_of(C) == (0, 0, 0, None, None, None) and list(vars(info).values()) == [0] * 7
    C, frames = framed_c(n, 1000, 5, np.float64)
    before = struct_of(C)
    rc, _, _ = call(cfg, dA, np.full(n, 1), None, 1000, 4, C=C)
    assert rc == ERR_NNZ_OVERFLOW and struct_of(C) == before and untouched(*frames)
    _, info = run_case(cfg, H, np.zeros(n, dtype=np.int64), None, 1000, 8, dA=dA)   # the row of 3 entries as often: served
    assert info.gross == 3 * n


# ---------------------------------------------------------------------------------------------------- 7: ownership, stream, guards
def test_c_keeps_the_buffers_whose_size_stays(cfg):
    H, p, cmap = mixed_case(np.float64)
    dA = sa.dCSR.from_host(H)
    C, info = run_case(cfg, H, p, cmap, 333, 8, dA=dA)
    p0 = struct_of(C)[3:]

    def again(p2, m2, out_cols):
        rc, _, info2 = call(cfg, dA, p2, m2, out_cols, 8, C=C)
        assert rc == OK
        check(C, info2, want_of(H, p2, m2, out_cols, 8), out_cols)
        return struct_of(C)[3:], info2

    p1, info1 = again(p, np.where(cmap >= 0, (cmap + 1) % 333, -1), 333)            # same rows, same kept columns, other ids:
    assert info1.nnz_out == info.nnz_out and p1 == p0                               #   same nnz -- all three stay
    p2, info2 = again(p, None, H.cols)                                              # another nnz: data and col_ids are new
    assert info2.nnz_out != info.nnz_out and p2[2] == p0[2] and p2[0] != p0[0] and p2[1] != p0[1]
    p3, _ = again(np.append(p, 3), None, H.cols)                                    # another n_rows: row_offsets is new
    assert p3[2] != p2[2]
    p4, _ = again(p[:10], cmap, 333)                                                # everything differs
    assert p4[0] != p3[0] and p4[1] != p3[1] and p4[2] != p3[2]


def test_an_index_made_on_the_callers_stream_needs_no_synchronise(cfg):
    H, _, cmap = mixed_case(np.float64)
    dA = sa.dCSR.from_host(H)
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    cmap_t = torch.from_numpy(cmap).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big = torch.randint(0, 1 << 40, (1 << 23,), device=DEV, generator=g)
        big = torch.sort(big).values                                                # work in front of the index on the stream
        rows_t = (torch.randint(0, 1 << 40, (3000,), device=DEV, generator=g) + big[:1] * 0) % H.rows
        C, info = sa.extract(dA, rows=rows_t, col_map=cmap_t, out_cols=333, config=cfg)   # no synchronise in between
    torch.cuda.synchronize()
    cfg.set_stream(None)
    check(C, info, want_of(H, rows_t.cpu().numpy(), cmap, 333, 8), 333)


def test_guard_zones_stay_clean(cfg):
    cfg.set_option("guard_bytes", 4096)
    try:
        H, p, cmap = mixed_case(np.float64)
        dA = sa.dCSR.from_host(H)
        C, _ = run_case(cfg, H, p, cmap, 333, 8, dA=dA)
        C2, _ = run_case(cfg, H, p, None, H.cols, 4, dA=dA)
        lens, _ = EDGE_CASES["5000 empty rows between two entries"]
        run_case(cfg, host_csr(lens, 600), None, random_map(600, 900, seed=2), 900, 8)
        del C, C2
    finally:
        cfg.set_option("guard_bytes", 0)


def test_the_caller_that_includes_extract_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_extract.cpp")
    out = str(tmp_path / "caller_extract")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "extract caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
