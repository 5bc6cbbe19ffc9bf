"""speck_bmat_* on the GPU (speck_amd/csrc/bmat.hip).  The expectation is the numpy statement of the contract
(tests/test_bmat_host.py, numpy_bmat, which that file compares with scipy), compared byte for byte.  The value of an entry is
its position in its own block behind a per-block offset (test_gpu_extract.pos_values: the number at even positions, a NaN
with the position for a payload at odd ones), so an entry from the wrong place or the wrong block, or one that went
through arithmetic, shows.  Device arrays the library must not touch, or must fill exactly, lie in frames of a payload
byte whose padding must survive.  T = 4096 output entries per tile, a thread holds 4 consecutive ones; LDS holds the units
of a tile -- pieces, or whole blocks where every block row of the tile holds one block -- up to 4096 of them."""
import ctypes as C_
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
import test_bmat_host as HOST
import test_gpu_extract as EX
import test_gpu_high_offsets as HO
from speck_amd import _lib
from test_bmat_host import INFO_FIELDS, numpy_bmat
from test_extract_host import bits
from test_gpu_extract import cfg  # noqa: F401  (the fixture)
from test_gpu_high_offsets import stores  # noqa: F401  (the fixture: the backing stores of that file, one value type at a time)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID = 0, 1
DEV = "cuda:0"
T = sa.BMAT_TILE_ENTRIES
LDS_UNITS = 4096
TAG = 12289                               # block k's positions start at k * TAG
VDTYPES = [np.float64, np.float32]
VIDS = ["f64", "f32"]


# ---------------------------------------------------------------------------------------------------- helpers
def block(lens, cols, vdtype, tag, seed=None, col=None):
    """rows of the given lengths; ids at random (unsorted, duplicates among them) unless given; the value of entry e is
    position tag * TAG + e"""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert n == 0 or cols > 0
    ci = np.random.default_rng(tag if seed is None else seed).integers(0, max(cols, 1), size=n) if col is None else np.asarray(col)
    return sa.HostCSR(len(lens), cols, ro, ci.astype(np.uint32), EX.pos_values(tag * TAG + n, vdtype)[tag * TAG:])


def split(total, parts, seed):
    """`parts` row lengths that sum to `total`"""
    cuts = np.sort(np.random.default_rng(seed).integers(0, total + 1, size=parts - 1))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def up(H):
    return sa.dCSR.from_host(H)


def call(cfg, cells, block_rows, block_cols, vdtype, row_sizes=None, col_sizes=None, C=None):
    """(status, C, BmatInfo); cells: (block_row, block_col, dCSR) in the order the C ABI gets them"""
    p, keep = HOST._params([(g, q, d._c) for g, q, d in cells], block_rows, block_cols, row_sizes, col_sizes)
    C = sa.dCSR(vdtype) if C is None else C
    info = _lib.CBmatInfo(*([7] * 7))
    fn = _lib.load().speck_bmat_f32 if np.dtype(vdtype) == np.float32 else _lib.load().speck_bmat_f64
    rc = fn(cfg._h if cfg is not None else None, C_.byref(p), C_.byref(C._c), C_.byref(info))
    torch.cuda.synchronize()
    del keep
    return rc, C, sa.BmatInfo(info)


def check(C, info, want):
    ro, ci, vb, winfo = want[:4]
    assert (C.rows, C.cols, C.nnz) == (len(ro) - 1, winfo["cols_out"], len(ci))
    assert C._c.data and C._c.col_ids and C._c.row_offsets                          # (buffers of one entry where nnz is 0)
    H = C.to_host()
    assert np.array_equal(H.row_offsets, ro), ("row_offsets", np.nonzero(H.row_offsets != ro)[0][:8])
    assert np.array_equal(H.col_ids, ci), ("col_ids", np.nonzero(H.col_ids != ci)[0][:8])
    assert np.array_equal(bits(H.data), vb), ("values", np.nonzero(bits(H.data) != vb)[0][:8])
    if info is not None:
        assert vars(info) == winfo


def run(cfg, cells, block_rows, block_cols, vdtype, row_sizes=None, col_sizes=None, devs=None, shuffle=None):
    """cells: (block_row, block_col, HostCSR); devs: their device matrices where they exist already (views, shared ones)"""
    devs = [up(H) for _, _, H in cells] if devs is None else devs
    placed = [(g, q, d) for (g, q, _), d in zip(cells, devs)]
    if shuffle is not None:
        placed = [placed[k] for k in np.random.default_rng(shuffle).permutation(len(placed))]
    want = numpy_bmat(cells, block_rows, block_cols, row_sizes, col_sizes, vdtype)
    rc, C, info = call(cfg, placed, block_rows, block_cols, vdtype, row_sizes, col_sizes)
    assert rc == OK
    check(C, info, want)
    return C, info, want


def vcells(mats):
    return [(g, 0, H) for g, H in enumerate(mats)], len(mats), 1


def hcells(mats):
    return [(0, q, H) for q, H in enumerate(mats)], 1, len(mats)


def dcells(mats):
    return [(i, i, H) for i, H in enumerate(mats)], len(mats), len(mats)


# ---------------------------------------------------------------------------------------------------- 1: vstack, the seam
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("seam", [1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 2])
def test_vstack_with_the_seam_at(cfg, seam, vdtype):
    A = block(split(seam, 3, seam) if seam > 5 else [0, seam, 0], 700, vdtype, 1)
    B = block(split(T + 3, 5, 2), 700, vdtype, 2)
    _, info, want = run(cfg, *vcells([A, B]), vdtype)
    assert want[0][A.rows] == seam and info.pieces == A.rows + B.rows and info.nnz_out == seam + T + 3
    run(cfg, *vcells([B, A]), vdtype)                                               # ... and the short block last


# ---------------------------------------------------------------------------------------------------- 2: hstack, the pieces
def hstack_cases(vdtype):
    """name -> three blocks over 5 rows"""
    def three(l0, l1, l2, cols=(300, 200, 100)):
        return [block(l, c, vdtype, k + 1) for k, (l, c) in enumerate(zip((l0, l1, l2), cols))]
    c = {}
    for g in (T - 1, T, T + 1):
        c[f"a piece seam at {g}"] = three([g, 1, 0, 2, 5], [3, 0, 7, 1, 1], [2, 2, 2, 0, 9])
        c[f"a piece seam at {g} behind two pieces"] = three([1000, 1, 0, 2, 5], [g - 1007, 0, 7, 1, 1], [7, 2, 2, 0, 9])
    c["a hub of 2 T + 7 fed from two blocks"] = three([3, 1, 5, 0, 2], [1, 2, 2 * T + 7, 0, 4], [0, 4, 6, 1, 1])
    c["the hub piece first and last in its row"] = three([2 * T + 7, 1, 0, 0, 2], [1, 2, 0, 0, 4], [0, 4, 6, 1, 2 * T + 7])
    c["the middle piece empty in some rows"] = three([3, 1, 5, 0, 2], [0, 2, 0, 0, 4], [1, 4, 6, 1, 1])
    c["a middle block without an entry"] = three([3, 1, T, 0, 2], [0, 0, 0, 0, 0], [1, 4, 6, 1, 1])
    c["a block of 0 columns"] = three([3, 1, T, 0, 2], [0, 0, 0, 0, 0], [1, 4, 6, 1, 1], cols=(300, 0, 100))
    c["a first block of 0 columns, a last without an entry"] = three([0] * 5, [3, 1, 5, 0, 2], [0] * 5, cols=(0, 200, 100))
    c["no entry at all"] = three([0] * 5, [0] * 5, [0] * 5)
    c["pieces inside one thread's four"] = three([1, 2, 1, 0, 1], [1, 1, 1, 1, 1], [2, 0, 1, 3, 1])
    return c


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("name", list(hstack_cases(np.float64)))
def test_hstack_of_three_blocks_over_five_rows(cfg, name, vdtype):
    mats = hstack_cases(vdtype)[name]
    C, info, want = run(cfg, *hcells(mats), vdtype)
    assert info.pieces == 15 and info.cols_out == sum(H.cols for H in mats)
    if name == "no entry at all":
        assert (C.nnz, info.rows_empty, info.max_row_entries) == (0, 5, 0)


# ---------------------------------------------------------------------------------------------------- 3: units per tile
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("units", [LDS_UNITS, LDS_UNITS + 1, 9000])
def test_pieces_that_touch_one_tile(cfg, units, vdtype):
    """hstack of 3 blocks: piece 0 holds the tile's first entry, piece units - 1 its last one, every piece between is empty"""
    rows = (units - 1) // 3 + 36
    lens = [np.zeros(rows, dtype=np.int64) for _ in range(3)]
    lens[0][0] = 1
    lens[(units - 1) % 3][(units - 1) // 3] += T + 10
    lens[2][rows - 1] = 5
    lens[1][rows - 20] = 3
    mats = [block(l, 50 + k, vdtype, k + 1) for k, l in enumerate(lens)]
    _, info, want = run(cfg, *hcells(mats), vdtype)
    G = np.concatenate([[0], np.cumsum(np.stack(lens, axis=1).reshape(-1))])
    first, last = np.searchsorted(G[1:], 0, side="right"), np.searchsorted(G[1:], T - 1, side="right")
    assert last - first + 1 == units and info.pieces == 3 * rows                    # the premise: what the first tile touches


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("units", [LDS_UNITS, LDS_UNITS + 1, 6000])
def test_blocks_that_touch_one_tile(cfg, units, vdtype):
    """vstack and block_diag: the units are the blocks.  One block without an entry stands in units - 2 cells between the
    block of the tile's first and the block of its last entry"""
    X, E, Y = block([1], 9, vdtype, 1), block([0], 9, vdtype, 2), block([2, T + 10, 3], 9, vdtype, 3)
    dX, dE, dY = up(X), up(E), up(Y)
    mats, devs = [X] + [E] * (units - 2) + [Y, X], [dX] + [dE] * (units - 2) + [dY, dX]
    run(cfg, *vcells(mats), vdtype, devs=devs)
    _, info, _ = run(cfg, *dcells(mats), vdtype, devs=devs)
    assert info.cols_out == 9 * (units + 1)


# ---------------------------------------------------------------------------------------------------- 4: many small blocks
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_block_diag_of_300_small_blocks_in_shuffled_order(cfg, vdtype):
    rng = np.random.default_rng(11)
    mats = []
    for k in range(300):
        rows, cols = int(rng.integers(0, 8)), int(rng.integers(0, 6))
        if k in (0, 17, 299):
            rows = 0                                                                # 0 x k
        if k in (1, 18, 298):
            cols = 0                                                                # k x 0
        lens = rng.integers(0, 7, size=rows) if cols else np.zeros(rows, dtype=np.int64)   # more entries than columns: duplicates
        mats.append(block(lens, cols, vdtype, k))
    C, info, want = run(cfg, *dcells(mats), vdtype, shuffle=3)
    assert info.blocks == 300 and info.pieces == C.rows == sum(H.rows for H in mats)
    # the wrapper and its origins
    devs = [up(H) for H in mats]
    C2, info2, ro, co = sa.block_diag(devs, cfg, return_info=True, return_offsets=True)
    check(C2, info2, want)
    assert list(ro) == want[4].tolist() and list(co) == want[5].tolist()


# ---------------------------------------------------------------------------------------------------- 5: grids
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_grids(cfg, vdtype):
    A, B = block(split(T + 9, 40, 1), 33, vdtype, 1), block(split(300, 25, 2), 61, vdtype, 2)
    run(cfg, [(0, 0, A), (1, 1, B)], 2, 2, vdtype)                                  # [[A, None], [None, B]]
    H, Bt, Bm = block(split(2 * T, 40, 3), 40, vdtype, 3), block(split(500, 40, 4), 25, vdtype, 4), block(split(T - 1, 25, 5), 40, vdtype, 5)
    run(cfg, [(1, 0, Bm), (0, 1, Bt), (0, 0, H)], 2, 2, vdtype)                     # [[H, Bt], [B, None]], named in another order
    run(cfg, [(0, 0, A), (2, 0, A)], 3, 1, vdtype, row_sizes=[40, 7, 40])           # an empty block row given by row_sizes
    run(cfg, [(0, 0, A), (3, 0, A)], 5, 1, vdtype, row_sizes=[40, 7, 2, 40, 3])     # two neighbours, and a last one
    run(cfg, [(0, 0, A), (0, 2, block([0] * 40, 61, vdtype, 7))], 1, 3, vdtype, col_sizes=[33, 5, 61])   # an empty block column given by col_sizes
    run(cfg, [(0, 2, A)], 1, 3, vdtype, col_sizes=[4, 0, 33])                       # an empty block column in front
    run(cfg, [(1, 1, A)], 3, 3, vdtype, row_sizes=[2, 40, 3], col_sizes=[4, 33, 9])
    C, info, _ = run(cfg, [], 3, 2, vdtype, row_sizes=[4, 0, 5], col_sizes=[6, 1])  # n_blocks == 0
    assert (C.rows, C.cols, C.nnz, info.rows_empty) == (9, 7, 0, 9)
    C, info, _ = run(cfg, [], 2, 2, vdtype, row_sizes=[0, 0], col_sizes=[6, 1])     # ... without a row
    assert (C.rows, C.cols, C.nnz) == (0, 7, 0)
    # the wrappers
    dA, dB = up(A), up(B)
    C, info = sa.bmat([[dA, None], [None, dB]], cfg, return_info=True)
    check(C, info, numpy_bmat([(0, 0, A), (1, 1, B)], 2, 2, vdtype=vdtype))
    check(sa.bmat([[None, None], [None, None]], cfg, row_sizes=[1, 2], col_sizes=[3, 4], dtype=vdtype), None,
          numpy_bmat([], 2, 2, [1, 2], [3, 4], vdtype))
    check(sa.hstack([dA, dA], cfg), None, numpy_bmat(hcells([A, A])[0], 1, 2, vdtype=vdtype))
    check(sa.vstack([dB, dB, dB], None), None, numpy_bmat(vcells([B, B, B])[0], 3, 1, vdtype=vdtype))


# ---------------------------------------------------------------------------------------------------- 6: views and reuse
@functools.lru_cache(maxsize=None)
def big(vdtype):
    rng = np.random.default_rng(21)
    lens = np.concatenate([rng.integers(0, 9, size=300), [2 * T + 5, 0, 0, T - 1, 1, T], rng.integers(0, 40, size=200)])
    return block(lens, 900, vdtype, 5)


def view_of(H, dA, r0, r1):
    return sa.HostCSR(r1 - r0, H.cols, H.row_offsets[r0:r1 + 1], H.col_ids, H.data), dA.row_view(r0, r1)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_views_and_one_matrix_in_several_cells(cfg, vdtype):
    H = big(vdtype)
    dA = up(H)
    run(cfg, [(0, 0, H), (1, 1, H), (0, 1, H)], 2, 2, vdtype, devs=[dA, dA, dA])    # the same matrix in three cells
    other = block(split(77, 30, 6), 40, vdtype, 6)
    for rem in (1, 2, 3):                                                           # a view whose base is rem modulo 4
        r0 = int(np.nonzero((H.row_offsets[:250] % 4 == rem) & (np.arange(250) > 0))[0][0])
        Hv, dv = view_of(H, dA, r0, r0 + 30)
        assert int(Hv.row_offsets[0]) % 4 == rem
        run(cfg, *vcells([Hv, H]), vdtype, devs=[dv, dA])
        run(cfg, *hcells([other, Hv, other]), vdtype, devs=[up(other), dv, up(other)])
    # a single block is its copy
    Hv, dv = view_of(H, dA, 7, H.rows - 3)
    for Hs, ds in ((H, dA), (Hv, dv)):
        C, _, _ = run(cfg, [(0, 0, Hs)], 1, 1, vdtype, devs=[ds])
        G, W = C.to_host(), ds.copy().to_host()
        assert np.array_equal(G.row_offsets, W.row_offsets) and np.array_equal(G.col_ids, W.col_ids) and np.array_equal(bits(G.data), bits(W.data))
    # vstack of the k row-range views of a matrix is the matrix
    cuts = [0, 1, 130, 301, 302, 303, 400, H.rows]
    views = [view_of(H, dA, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    C, info, want = run(cfg, *vcells([v[0] for v in views]), vdtype, devs=[v[1] for v in views])
    assert np.array_equal(want[0], H.row_offsets) and np.array_equal(want[1], H.col_ids) and np.array_equal(want[2], bits(H.data))
    assert info.max_row_entries == 2 * T + 5


# ---------------------------------------------------------------------------------------------------- 7: offsets past 2^31
@pytest.mark.parametrize("vdtype, where", [(np.float32, "straddle"), (np.float32, "top"), (np.float64, "straddle")],
                         ids=["f32-straddle", "f32-top", "f64-straddle"])
def test_a_block_that_is_a_view_with_high_offsets(cfg, stores, vdtype, where):  # noqa: F811
    """the view of tests/test_gpu_high_offsets.py (its offsets cross 2^31, or end at 0xFFFFFFFF) between two small blocks, and
    beside one: numpy on the host copy, and the bytes its low twin gives"""
    store = stores.get(vdtype)
    H = HO.view_matrix(vdtype)
    hi, lo = HO.place_with_twin(store, where, H)
    above, below = block(split(T + 1, 9, 1), H.cols, vdtype, 1), block(split(37, 5, 2), H.cols, vdtype, 2)
    beside = block(split(2 * T, H.rows, 3), 77, vdtype, 3)
    d_above, d_below, d_beside = up(above), up(below), up(beside)
    for (cells, br, bc), others in ((vcells([above, H, below]), (d_above, d_below)), (hcells([beside, H]), (d_beside,))):
        want = numpy_bmat(cells, br, bc, vdtype=vdtype)
        seen = []
        for p in (hi, lo):
            devs = [others[0], p.d, others[1]] if len(others) == 2 else [others[0], p.d]
            rc, C, info = call(cfg, [(g, q, d) for (g, q, _), d in zip(cells, devs)], br, bc, vdtype)
            assert rc == OK
            check(C, info, want)
            G = C.to_host()
            seen.append(G.row_offsets.tobytes() + G.col_ids.tobytes() + G.data.tobytes())
            p.check_intact()
        assert seen[0] == seen[1]


# ---------------------------------------------------------------------------------------------------- 8: round trips
def scipy_graph(rows, cols, per_row, seed):
    rng = np.random.default_rng(seed)
    S = sp.random(rows, cols, density=per_row / cols, format="csr", random_state=rng, dtype=np.float64)
    S.data = rng.integers(1, 9, size=S.nnz).astype(np.float64)
    S.sort_indices()
    return S


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_a_2x2_split_by_extract_put_back_gives_the_matrix(cfg, vdtype):
    H = big(vdtype)
    dA = up(H)
    r, c = 311, 400
    rows = [torch.arange(0, r, device=DEV), torch.arange(r, H.rows, device=DEV)]
    maps = [torch.where(torch.arange(H.cols, device=DEV) < c, torch.arange(H.cols, device=DEV), -1),
            torch.where(torch.arange(H.cols, device=DEV) >= c, torch.arange(H.cols, device=DEV) - c, -1)]
    parts = [[sa.extract(dA, rows=rows[i], col_map=maps[j], out_cols=(c, H.cols - c)[j], config=cfg)[0] for j in range(2)] for i in range(2)]
    C = sa.bmat(parts, cfg)
    G = C.to_host()
    # (the entries of a row come back grouped by block column: A's rows hold their ids in random order, so compare sorted
    #  by (column block, position) -- which for a matrix whose rows are split at column c is a stable partition of each row)
    ro = H.row_offsets.astype(np.int64)
    row_of = np.repeat(np.arange(H.rows), np.diff(ro))
    order = np.lexsort((np.arange(H.nnz), H.col_ids >= c, row_of))
    assert np.array_equal(G.row_offsets, H.row_offsets) and np.array_equal(G.col_ids, H.col_ids[order])
    assert np.array_equal(bits(G.data), bits(H.data)[order])
    # a canonical matrix comes back byte for byte
    S = scipy_graph(600, 500, 7, seed=31)
    dS = EX.to_device(S)
    maps = [torch.where(torch.arange(500, device=DEV) < 123, torch.arange(500, device=DEV), -1),
            torch.where(torch.arange(500, device=DEV) >= 123, torch.arange(500, device=DEV) - 123, -1)]
    rows = [torch.arange(0, 250, device=DEV), torch.arange(250, 600, device=DEV)]
    parts = [[sa.extract(dS, rows=rows[i], col_map=maps[j], out_cols=(123, 377)[j], config=cfg)[0] for j in range(2)] for i in range(2)]
    assert EX.same_as_scipy(sa.bmat(parts, cfg), S)


def test_one_multiply_on_the_block_diagonal_is_the_two_products(cfg):
    A, B = scipy_graph(700, 700, 6, seed=41), scipy_graph(450, 450, 9, seed=42)
    dA, dB = EX.to_device(A), EX.to_device(B)
    M = sa.block_diag([dA, dB], cfg)
    assert EX.same_as_scipy(M, sp.block_diag([A, B]))
    MM, AA, BB = sa.dCSR(), sa.dCSR(), sa.dCSR()
    sa.MultiplyspECK(M, M, MM, cfg, sa.Timings())
    sa.MultiplyspECK(dA, dA, AA, cfg, sa.Timings())
    sa.MultiplyspECK(dB, dB, BB, cfg, sa.Timings())
    W = sa.block_diag([AA, BB], cfg).to_host()
    G = MM.to_host()
    assert np.array_equal(G.row_offsets, W.row_offsets) and np.array_equal(G.col_ids, W.col_ids)
    assert np.array_equal(G.data, W.data)                                          # integers: the sums are exact


# ---------------------------------------------------------------------------------------------------- 9: hostile input
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("shape", ["vstack", "hstack"])
def test_hostile_blocks_are_refused_with_nothing_written(cfg, shape, vdtype):
    """three blocks into a C whose buffers would all be reused.  Refusals of clamped values: nothing here may fault"""
    if shape == "vstack":
        mats = [block(split(n, 30, k), 50, vdtype, k) for k, n in ((1, T + 5), (2, 300), (3, 2 * T + 1))]
        cells, br, bc = vcells(mats)
    else:
        mats = [block(split(n, 30, k), c, vdtype, k) for k, n, c in ((1, T + 5, 50), (2, 300, 40), (3, 2 * T + 1, 60))]
        cells, br, bc = hcells(mats)
    want = numpy_bmat(cells, br, bc, vdtype=vdtype)
    good = [EX.device_matrix(H) for H in mats]
    C, frames = EX.framed_c(len(want[0]) - 1, want[3]["cols_out"], len(want[1]), vdtype)
    before = EX.struct_of(C)

    def refused(k, what, **change):
        devs = list(good)
        devs[k] = EX.device_matrix(mats[k], **change)
        rc, _, info = call(cfg, [(g, q, d) for (g, q, _), d in zip(cells, devs)], br, bc, vdtype, C=C)
        assert rc == ERR_INVALID, (k, what)
        assert EX.struct_of(C) == before and list(vars(info).values()) == [0] * 7, (k, what)
        assert EX.untouched(*frames), (k, what)

    for k in (0, 2, 1):
        H = mats[k]
        r = next(i for i in range(10, 29) if H.row_offsets[i + 1] > H.row_offsets[i])
        ro = H.row_offsets.copy()
        ro[r] = ro[r + 1] + 1
        refused(k, "offsets that descend", ro=ro)
        ro = H.row_offsets.copy()
        ro[-1] -= 1
        refused(k, "a last offset that does not span nnz", ro=ro)
        refused(k, "a declared nnz that the offsets do not span", nnz=H.nnz - 1)
        ro = H.row_offsets.copy()
        ro[15] = 0xFFFFFFF0
        refused(k, "a far-off offset in the middle", ro=ro)
        ro = H.row_offsets.copy()
        ro[15:] = 0xFFFFFFF0
        refused(k, "far-off offsets from the middle on", ro=ro)
        for at in (0, H.nnz - 1, H.nnz // 2):
            for bad in (H.cols, 0xFFFFFFFF):                                        # in an hstack H.cols is below cols(C)
                col = H.col_ids.copy()
                col[at] = bad
                refused(k, ("an id", bad, "at", at), col=col)
    for d, H in zip(good, mats):                                                    # the blocks are as they were
        G = d.to_host()
        assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes() and G.data.tobytes() == H.data.tobytes()
    # ... and the clean call fills exactly the three arrays
    rc, _, info = call(cfg, [(g, q, d) for (g, q, _), d in zip(cells, good)], br, bc, vdtype, C=C)
    assert rc == OK and EX.struct_of(C) == before and vars(info) == want[3]
    vs = np.dtype(vdtype).itemsize
    assert np.array_equal(EX.framed(frames[2], len(want[0]) * 4, np.uint32), want[0])
    assert np.array_equal(EX.framed(frames[1], len(want[1]) * 4, np.uint32), want[1])
    assert np.array_equal(EX.framed(frames[0], len(want[1]) * vs, want[2].dtype), want[2])
    rc, _, _ = call(cfg, [(g, q, d) for (g, q, _), d in zip(cells, good)], br, bc, vdtype, C=good[1])   # C sharing buffers with a block
    assert rc == ERR_INVALID


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_a_c_whose_buffers_start_off_16_bytes(cfg, shift):
    """reused buffers that are not aligned: the 16-byte stores must not be taken"""
    mats = [block(split(n, 30, k), 50, np.float32, k) for k, n in ((1, T + 5), (2, 300))]
    cells, br, bc = vcells(mats)
    want = numpy_bmat(cells, br, bc, vdtype=np.float32)
    n = len(want[1])
    fd, fc, fr = EX.frame(n * 4 + 16), EX.frame(n * 4 + 16), EX.frame(len(want[0]) * 4)
    C = sa.dCSR.from_device(len(want[0]) - 1, 50, n, fr[1], fc[1] + 4 * shift, fd[1] + 4 * shift, dtype=np.float32, keep=(fd, fc, fr))
    rc, _, info = call(cfg, [(g, q, up(H)) for g, q, H in cells], br, bc, np.float32, C=C)
    assert rc == OK and vars(info) == want[3]
    assert np.array_equal(EX.framed(fc[0], n * 4 + 16, np.uint32)[shift:shift + n], want[1])
    assert np.array_equal(EX.framed(fd[0], n * 4 + 16, np.uint32)[shift:shift + n], want[2])
    pay = np.uint32(EX.PAYLOAD * 0x01010101)
    for f in (fc, fd):
        got = EX.framed(f[0], n * 4 + 16, np.uint32)
        assert (got[:shift] == pay).all() and (got[shift + n:] == pay).all()


# ---------------------------------------------------------------------------------------------------- 10: ownership
def test_c_keeps_the_buffers_whose_size_stays(cfg):
    vdtype = np.float64
    A, B, D = block(split(500, 40, 1), 33, vdtype, 1), block(split(300, 25, 2), 33, vdtype, 2), block(split(300, 25, 3), 33, vdtype, 3)
    E = block(split(301, 25, 4), 33, vdtype, 4)
    C, _, _ = run(cfg, *vcells([A, B]), vdtype)
    p0 = EX.struct_of(C)[3:]

    def again(mats):
        cells, br, bc = vcells(mats)
        rc, _, info = call(cfg, [(g, q, up(H)) for g, q, H in cells], br, bc, vdtype, C=C)
        assert rc == OK
        check(C, info, numpy_bmat(cells, br, bc, vdtype=vdtype))
        return EX.struct_of(C)[3:]

    p1 = again([A, D])                                                              # equal rows, equal nnz: all three stay
    assert p1 == p0
    p2 = again([A, E])                                                              # equal rows, another nnz: row_offsets stays
    assert p2[2] == p0[2] and p2[0] != p0[0] and p2[1] != p0[1]
    p3 = again([E, A, block([1], 33, vdtype, 5)])                                   # another row count: everything is new
    assert p3[0] != p2[0] and p3[1] != p2[1] and p3[2] != p2[2]
    F = block(np.concatenate([split(501, 40, 1), split(301, 25, 6), [0]]), 33, vdtype, 6)
    p4 = again([F])                                                                 # equal nnz, equal rows from one block: all stay
    assert p4 == p3


# ---------------------------------------------------------------------------------------------------- 11: stream, guards, cfg
def test_blocks_made_on_the_callers_stream_need_no_synchronise(cfg):
    H = big(np.float64)
    dA = up(H)
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big_t = torch.sort(torch.randint(0, 1 << 40, (1 << 23,), device=DEV, generator=g)).values     # work in front on the stream
        rows_t = (torch.randint(0, 1 << 40, (700,), device=DEV, generator=g) + big_t[:1] * 0) % H.rows
        P, _ = sa.extract(dA, rows=rows_t, config=cfg)                              # a block produced on the stream
        C, info = sa.vstack([P, dA, P], cfg, return_info=True)                      # no synchronise in between
    torch.cuda.synchronize()
    cfg.set_stream(None)
    Hp = P.to_host()
    check(C, info, numpy_bmat(vcells([Hp, H, Hp])[0], 3, 1, vdtype=np.float64))
    assert np.array_equal(Hp.col_ids, EX.want_of(H, rows_t.cpu().numpy(), None, H.cols, 8)[1])


def test_guard_zones_stay_clean(cfg):
    cfg.set_option("guard_bytes", 4096)
    try:
        for vdtype in VDTYPES:
            H = big(vdtype)
            run(cfg, [(0, 0, H), (1, 1, H), (0, 1, H)], 2, 2, vdtype)
            run(cfg, *hcells(hstack_cases(vdtype)["a hub of 2 T + 7 fed from two blocks"]), vdtype)
            run(cfg, [], 3, 2, vdtype, row_sizes=[4, 0, 5], col_sizes=[6, 1])
    finally:
        cfg.set_option("guard_bytes", 0)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_without_a_config(vdtype):
    H = big(vdtype)
    cells = [(0, 0, H), (1, 1, H), (0, 1, H)]
    rc, C, info = call(None, [(g, q, up(M)) for g, q, M in cells], 2, 2, vdtype)
    assert rc == OK
    check(C, info, numpy_bmat(cells, 2, 2, vdtype=vdtype))
    check(sa.block_diag([up(H), up(H)], None), None, numpy_bmat(dcells([H, H])[0], 2, 2, vdtype=vdtype))


def test_same_bytes_from_run_to_run(cfg):
    mats = hstack_cases(np.float64)["a hub of 2 T + 7 fed from two blocks"]
    devs = [up(H) for H in mats]
    for _ in range(3):
        run(cfg, *hcells(mats), np.float64, devs=devs)


def test_the_caller_that_includes_bmat_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_bmat.cpp")
    out = str(tmp_path / "caller_bmat")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "bmat caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
