"""speck_sample_* on the GPU (speck_amd/csrc/sample.hip).  The expectation is the numpy statement of the contract
(tests/test_sample_host.py, numpy_sample, which that file compares with a brute-force count of smaller keys), compared byte
for byte: row_offsets, col_ids, the values' bits and every field of info.  Column ids are random, unsorted and repeat, and
the values carry their position in the low mantissa bits (NaNs with payloads, -0.0, infinities and subnormals among them):
an entry that comes from another place shows.  The class limits come from speck_amd.SAMPLE_GROUP_MAX / SAMPLE_LDS_MAX: a
group of 8 / 16 / 32 / 64 lanes ranks cut rows of up to GROUP_MAX / 8, / 4, / 2, GROUP_MAX entries, a workgroup with the
keys in LDS rows of up to LDS_MAX, the long-row kernel the rest; the debug options sample_group_max / sample_lds_max lower
them, so one row can be sent through every class."""
import ctypes as C_
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import speck_amd as sa
from speck_amd import _lib
from test_gpu_topk import device_matrix, frame, framed, framed_c, host_csr, struct_of, untouched
from test_sample_host import INFO_FIELDS, WITH, WITHOUT, bits, numpy_sample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NNZ_OVERFLOW = 0, 1, 5
DEV = "cuda:0"
G, LDS, TILE = sa.SAMPLE_GROUP_MAX, sa.SAMPLE_LDS_MAX, sa.SAMPLE_TILE_ENTRIES
VDTYPES = [np.float64, np.float32]
VIDS = ["f64", "f32"]
ITYPES = [torch.int64, torch.int32]
IIDS = ["int64", "uint32"]
MODES = [WITHOUT, WITH]
MIDS = ["without", "with"]
# (sample_group_max, sample_lds_max): the classes a cut row can be sent through
CLASSES = {"group": (G, LDS), "lds": (0, LDS), "long": (0, 0)}
GROUP_TRIP = 2048 * 32                    # rows of the narrowest group one launch takes before its workgroups stride
ROW_TRIP = 2048                           # ... rows of the LDS class; the long class strides after 1024
IDS_TRIP = 1024 * TILE                    # gross entries the id check takes before its workgroups stride


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def index_tensor(rows, itype):
    """the index list on the device, one element at least (a tensor without elements has no address)"""
    rows = np.asarray(rows, dtype=np.int64)
    t = torch.from_numpy(rows if len(rows) else np.zeros(1, dtype=np.int64)).to(DEV)
    return t if itype is torch.int64 else t.to(torch.int32)


def call(cfg, dA, k, seed, rows=None, mode=WITHOUT, row_base=0, C=None, itype=torch.int64, index=None, n_rows=None, index_bytes=None):
    """(status, C, SampleInfo).  rows: a list of indices (uploaded as itype), None for every row; index: a tensor as it is"""
    prm = _lib.CSampleParams()
    prm.k, prm.seed, prm.row_base, prm.mode = k, seed, row_base, mode
    if rows is not None:
        index, n_rows = index_tensor(rows, itype), len(rows)
    prm.n_rows = dA.rows if index is None and n_rows is None else n_rows
    prm.d_row_index = index.data_ptr() if index is not None else None
    prm.index_bytes = index_bytes if index_bytes is not None else 8 if index is None else index.element_size()
    C = sa.dCSR(dA.dtype) if C is None else C
    info = _lib.CSampleInfo(*([7] * 6))
    fn = _lib.load().speck_sample_f32 if dA.dtype == np.float32 else _lib.load().speck_sample_f64
    torch.cuda.synchronize()
    rc = fn(cfg._h if cfg is not None else None, C_.byref(dA._c), C_.byref(prm), C_.byref(C._c), C_.byref(info))
    torch.cuda.synchronize()
    return rc, C, sa.SampleInfo(info)


def check(C, info, want, cols):
    ro, ci, vb, winfo = want[:4]
    assert (C.rows, C.cols, C.nnz) == (len(ro) - 1, cols, len(ci))
    assert C._c.data and C._c.col_ids and C._c.row_offsets                          # (buffers of one entry where nnz is 0)
    H = C.to_host()
    assert np.array_equal(H.row_offsets, ro), "row_offsets"
    assert np.array_equal(H.col_ids, ci), "col_ids"
    assert np.array_equal(bits(H.data), vb), "values"
    assert vars(info) == winfo


def want_of(H, k, seed, rows=None, mode=WITHOUT, row_base=0):
    return numpy_sample(H.row_offsets, H.col_ids, H.data, k, seed, rows, mode, row_base)


def run_case(cfg, H, k, seed, rows=None, mode=WITHOUT, dA=None, itype=torch.int64):
    dA = sa.dCSR.from_host(H) if dA is None else dA
    rc, C, info = call(cfg, dA, k, seed, rows, mode, itype=itype)
    assert rc == OK
    check(C, info, want_of(H, k, seed, rows, mode), H.cols)
    return C, info


def set_classes(cfg, name):
    cfg.set_option("sample_group_max", CLASSES[name][0])
    cfg.set_option("sample_lds_max", CLASSES[name][1])


def same_matrix(P, Q):
    P, Q = P.to_host(), Q.to_host()
    return np.array_equal(P.row_offsets, Q.row_offsets) and np.array_equal(P.col_ids, Q.col_ids) and np.array_equal(bits(P.data), bits(Q.data))


# ---------------------------------------------------------------------------------------------------- 1: lengths around k, class edges
EDGES = [G // 8, G // 8 + 1, G // 4, G // 4 + 1, G // 2, G // 2 + 1, G, G + 1, LDS, LDS + 1]


@functools.lru_cache(maxsize=None)
def edge_matrix(vdtype):
    """both sides of every group width and of both class limits, the lengths around every k below, a hub of 70001 entries
    (several trips of the long-row loops) in the middle of a few hundred short and empty rows"""
    rng = np.random.default_rng(11)
    around = [0, 1, 2, 3, 30, 31, 32, 33, 254, 255, 256, 257, 258, 4999, 5000, 5001]
    lens = rng.integers(0, 12, size=150).tolist()
    for e in EDGES + around:
        lens += [e] + rng.integers(0, 12, size=2).tolist()
    lens += [70001] + rng.integers(0, 12, size=150).tolist()
    return host_csr(lens, 100000, vdtype, seed=12)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("k", [0, 1, 2, 31, 32, 255, 256, 257, 5000, 1 << 32])
def test_lengths_around_k_and_every_class_switch(cfg, k, vdtype):
    H = edge_matrix(vdtype)
    assert G == 256 and LDS == 4096                        # (the lengths above are written out for these limits)
    lens = np.diff(H.row_offsets.astype(np.int64))
    for x in (k - 1, k, k + 1):
        assert k >= 5002 or x < 0 or x in lens
    dA = sa.dCSR.from_host(H)
    C, info = run_case(cfg, H, k, seed=k + 5, dA=dA)
    assert info.rows_cut == int((lens > k).sum()) and info.max_row_entries == min(k, 70001) and info.gross == H.nnz
    if k == 0:
        assert C.nnz == 0 and info.rows_empty == H.rows
    if k == 1 << 32:                                       # C is A, bit for bit
        assert same_matrix(C, dA)
        for more in ((1 << 32) - 1, 1 << 40, (1 << 64) - 1, 70001):
            C, info = run_case(cfg, H, more, seed=3, dA=dA)
            assert same_matrix(C, dA) and info.rows_cut == 0
        _, info = run_case(cfg, H, 70000, seed=3, dA=dA)   # one row is cut by one entry
        assert info.rows_cut == 1 and info.nnz_out == H.nnz - 1


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_empty_rows_only_and_no_rows(cfg, vdtype):
    H = host_csr([0] * 700, 50, vdtype)
    for mode in MODES:
        for k in (0, 3, 1 << 40):
            C, info = run_case(cfg, H, k, 9, mode=mode)
            assert C.nnz == 0 and vars(info) == dict(rows_out=700, rows_empty=700, rows_cut=0, gross=0, nnz_out=0, max_row_entries=0)
        C, info = run_case(cfg, H, 3, 9, rows=[5, 5, 699, 0], mode=mode)      # a list naming only empty rows
        assert C.rows == 4 and C.nnz == 0 and info.rows_empty == 4
    H0 = host_csr([], 50, vdtype)
    for c in (cfg, None):
        for mode in MODES:
            rc, C, info = call(c, device_matrix(H0), 3, 1, mode=mode)
            assert rc == OK and (C.rows, C.cols, C.nnz) == (0, 50, 0) and list(vars(info).values()) == [0] * 6
            assert C.to_host().row_offsets.tolist() == [0]


def test_lists_longer_than_a_launchs_first_trip(cfg):
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "sample.hip")).read()       # (the grids the constants above restate)
    assert "kGroupGrid = 2048, kLdsGrid = 2048, kLongGrid = 1024" in source and "kIdsGrid = 1024" in source
    H = host_csr([9] * (GROUP_TRIP + 500), 64, np.float64, seed=13)                   # the narrowest group: 32 rows per workgroup
    _, info = run_case(cfg, H, 3, 1)
    assert info.rows_cut == GROUP_TRIP + 500
    H = host_csr([9, 0, 2, 11] * (ROW_TRIP // 2 + 50), 64, np.float32, seed=14)
    dA = sa.dCSR.from_host(H)
    for name in ("lds", "long"):                                                    # one row per workgroup
        set_classes(cfg, name)
        _, info = run_case(cfg, H, 3, 2, dA=dA)
        assert info.rows_cut == ROW_TRIP + 100


# ---------------------------------------------------------------------------------------------------- 2: every class, the same bytes
@functools.lru_cache(maxsize=None)
def class_matrix(vdtype):
    lens = np.concatenate([np.arange(1, 301), [LDS + 7, 2 * LDS + 5, 9000]])
    return host_csr(np.random.default_rng(21).permutation(lens), 20000, vdtype, seed=22)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_every_class_gives_the_same_bytes(cfg, vdtype):
    H = class_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    for k in (5, 40):
        want = want_of(H, k, 77)
        for gmax, lmax in ((G, LDS), (0, LDS), (0, 0), (G, 0), (G // 8, 200), (100, 1000), (G // 2 + 1, G), (G + 50, LDS + 50)):
            cfg.set_option("sample_group_max", gmax)                                    # (beyond the defines: clamped)
            cfg.set_option("sample_lds_max", lmax)
            for _ in range(2):                                                          # ... and from run to run
                rc, C, info = call(cfg, dA, k, 77)
                assert rc == OK
                check(C, info, want, H.cols)


@pytest.mark.parametrize("cls", list(CLASSES))
def test_the_hub_through_every_class_of_long_rows(cfg, cls):
    H = edge_matrix(np.float64)
    set_classes(cfg, cls)
    for k in (1, 300, 69999):
        run_case(cfg, H, k, seed=k)


# ---------------------------------------------------------------------------------------------------- 3: row lists
@functools.lru_cache(maxsize=None)
def list_matrix(vdtype):
    """short rows, empty rows, one row of every class, and two entries 6000 empty rows apart (a tile of the id check and of
    the draw that more rows touch than LDS holds ends of)"""
    rng = np.random.default_rng(31)
    lens = np.concatenate([rng.integers(0, 40, size=300), [G - 3, LDS - 5, LDS + 900], [5], np.zeros(6000, dtype=np.int64), [7, 0, 0, 2]])
    return host_csr(lens, 3000, vdtype, seed=32)


@pytest.mark.parametrize("mode", MODES, ids=MIDS)
@pytest.mark.parametrize("itype", ITYPES, ids=IIDS)
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_row_lists(cfg, vdtype, itype, mode):
    H = list_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    rng = np.random.default_rng(33)
    k = 6
    run_case(cfg, H, k, 5, None, mode, dA=dA)                                       # NULL: every row
    everything = np.arange(H.rows)
    run_case(cfg, H, k, 5, everything[::-1].copy(), mode, dA=dA, itype=itype)       # reversed
    C, info = run_case(cfg, H, k, 5, everything, mode, dA=dA, itype=itype)          # the identity is the NULL list
    rc, C0, _ = call(cfg, dA, k, 5, None, mode)
    assert rc == OK and same_matrix(C, C0)
    cut = int(np.nonzero(np.diff(H.row_offsets.astype(np.int64))[:300] > k)[0][0])   # a short row that is cut
    picks = np.concatenate([rng.integers(0, H.rows, size=500), [300, 301, 302, 302, 301, 300, cut, cut, cut, H.rows - 1]])
    C, info = run_case(cfg, H, k, 5, picks, mode, dA=dA, itype=itype)               # repeats: the same row twice, the same sample twice
    P = C.to_host()
    ro = P.row_offsets.astype(np.int64)
    for a, b in ((500, 505), (501, 504), (506, 507), (507, 508)):
        assert picks[a] == picks[b] and ro[a + 1] - ro[a] == ro[b + 1] - ro[b] > 0
        assert np.array_equal(P.col_ids[ro[a]:ro[a + 1]], P.col_ids[ro[b]:ro[b + 1]])
        assert np.array_equal(bits(P.data[ro[a]:ro[a + 1]]), bits(P.data[ro[b]:ro[b + 1]]))
    C, info = run_case(cfg, H, k, 5, np.zeros(0, dtype=np.int64), mode, dA=dA, itype=itype)   # an empty list
    assert (C.rows, C.cols, C.nnz) == (0, H.cols, 0) and list(vars(info).values()) == [0] * 6
    empties = np.nonzero(np.diff(H.row_offsets.astype(np.int64)) == 0)[0]
    C, info = run_case(cfg, H, k, 5, empties[::7], mode, dA=dA, itype=itype)        # only empty rows
    assert C.nnz == 0 and info.rows_empty == len(empties[::7]) and info.gross == 0


@pytest.mark.parametrize("mode", MODES, ids=MIDS)
def test_a_hub_named_many_times_is_many_tiles(cfg, mode):
    # more gross entries than the id check's grid takes in one trip; the expectation of one row, repeated
    H = edge_matrix(np.float64)
    hub = int(np.argmax(np.diff(H.row_offsets.astype(np.int64))))
    times = IDS_TRIP // 70001 + 3
    assert times * 70001 > IDS_TRIP + 2 * TILE
    ro, ci, vb, _, _ = want_of(H, 4, 21, [hub], mode)
    dA = sa.dCSR.from_host(H)
    rc, C, info = call(cfg, dA, 4, 21, [hub] * times, mode)
    assert rc == OK
    want = (np.arange(times + 1, dtype=np.uint32) * 4, np.tile(ci, times), np.tile(vb, times),
            dict(rows_out=times, rows_empty=0, rows_cut=times, gross=times * 70001, nnz_out=4 * times, max_row_entries=4))
    check(C, info, want, H.cols)
    # ... and a bad id at the hub's last place is found in every one of them
    col = H.col_ids.copy()
    col[int(H.row_offsets[hub + 1]) - 1] = H.cols
    before = struct_of(C)
    rc, _, info = call(cfg, device_matrix(H, col=col), 4, 21, [hub] * times, mode, C=C)
    assert rc == ERR_INVALID and struct_of(C) == before and list(vars(info).values()) == [0] * 6


# ---------------------------------------------------------------------------------------------------- 4: views, value types, seeds
@pytest.mark.parametrize("mode", MODES, ids=MIDS)
@pytest.mark.parametrize("cfg_none", [False, True], ids=["cfg", "no-cfg"])
def test_a_view_with_its_row_base_gives_the_rows_of_the_whole(cfg, cfg_none, mode):
    H = class_matrix(np.float64)
    dA = sa.dCSR.from_host(H)
    r0, r1 = int(np.nonzero(H.row_offsets % 2 == 1)[0][0]), H.rows - 3                # an odd first offset
    assert 0 < r0 < 50 and int(H.row_offsets[r0]) % 2 == 1
    V = dA.row_view(r0, r1)
    c = None if cfg_none else cfg
    k, seed = 6, 40
    rc, whole, winfo = call(c, dA, k, seed, mode=mode)
    assert rc == OK
    check(whole, winfo, want_of(H, k, seed, mode=mode), H.cols)
    view_h = sa.HostCSR(r1 - r0, H.cols, H.row_offsets[r0:r1 + 1], H.col_ids, H.data)
    rc, C, info = call(c, V, k, seed, mode=mode, row_base=r0)
    assert rc == OK
    check(C, info, want_of(view_h, k, seed, mode=mode, row_base=r0), H.cols)
    W, P = whole.to_host(), C.to_host()
    a, b = int(W.row_offsets[r0]), int(W.row_offsets[r1])
    assert np.array_equal(P.col_ids, W.col_ids[a:b]) and np.array_equal(bits(P.data), bits(W.data[a:b]))
    assert np.array_equal(P.row_offsets.astype(np.int64), W.row_offsets[r0:r1 + 1].astype(np.int64) - a)
    # the same view with row_base = 0 is another sample (rows are cut: the row keys differ), and still the statement's
    rc, C0, info0 = call(c, V, k, seed, mode=mode, row_base=0)
    assert rc == OK and info0.rows_cut > 0
    check(C0, info0, want_of(view_h, k, seed, mode=mode, row_base=0), H.cols)
    assert not same_matrix(C0, C)
    # a list into the view, a row_base beyond 2^32
    picks = np.random.default_rng(41).integers(0, r1 - r0, size=200)
    rc, C1, info1 = call(c, V, k, seed, picks, mode, row_base=(1 << 62))
    assert rc == OK
    check(C1, info1, want_of(view_h, k, seed, picks, mode, row_base=(1 << 62)), H.cols)


@pytest.mark.parametrize("mode", MODES, ids=MIDS)
def test_f32_and_f64_give_the_same_structure(cfg, mode):
    H64, H32 = class_matrix(np.float64), class_matrix(np.float32)
    assert np.array_equal(H64.row_offsets, H32.row_offsets) and np.array_equal(H64.col_ids, H32.col_ids)
    special = lambda v: (int(np.isnan(v).sum()), int((np.signbit(v) & (v == 0)).sum()), int(((v != 0) & (np.abs(v) < np.finfo(v.dtype).tiny)).sum()))
    assert min(special(H64.data)) > 0 and min(special(H32.data)) > 0                  # NaNs, -0.0 and subnormals go in
    picks = np.random.default_rng(42).integers(0, H64.rows, size=400)
    for rows in (None, picks):
        C64, _ = run_case(cfg, H64, 9, 1234, rows, mode)
        C32, _ = run_case(cfg, H32, 9, 1234, rows, mode)
        P, Q = C64.to_host(), C32.to_host()
        assert np.array_equal(P.row_offsets, Q.row_offsets) and np.array_equal(P.col_ids, Q.col_ids)
        assert min(special(P.data)) > 0 and min(special(Q.data)) > 0                  # ... and come out, bit for bit (run_case)


@pytest.mark.parametrize("mode", MODES, ids=MIDS)
def test_one_seed_one_sample_two_seeds_two(cfg, mode):
    H = class_matrix(np.float32)
    dA = sa.dCSR.from_host(H)
    C1, _ = run_case(cfg, H, 7, 99, mode=mode, dA=dA)
    C2, _ = run_case(cfg, H, 7, 99, mode=mode, dA=dA)
    assert same_matrix(C1, C2)
    for seed in (100, 0, (1 << 64) - 1):
        C3, _ = run_case(cfg, H, 7, seed, mode=mode, dA=dA)
        assert not same_matrix(C1, C3)


# ---------------------------------------------------------------------------------------------------- 5: with replacement
@pytest.mark.parametrize("itype", ITYPES, ids=IIDS)
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_draws_with_replacement(cfg, vdtype, itype):
    H = edge_matrix(vdtype)
    lens = np.diff(H.row_offsets.astype(np.int64))
    dA = sa.dCSR.from_host(H)
    ones = np.nonzero(lens == 1)[0]
    assert len(ones) > 3
    for k in (1, 5, 300):                                                           # k = 1; k > len for most rows; a tile per few rows
        C, info = run_case(cfg, H, k, 8, mode=WITH, dA=dA)
        assert info.nnz_out == k * int((lens > 0).sum()) and info.rows_empty == int((lens == 0).sum()) and info.max_row_entries == k
        assert info.rows_cut == int((lens > k).sum())
        P = C.to_host()
        r = int(ones[0])                                                            # a row of one entry: k copies
        a = int(P.row_offsets[r])
        assert (P.col_ids[a:a + k] == H.col_ids[H.row_offsets[r]]).all()
    hub = int(np.argmax(lens))
    picks = np.concatenate([[hub, int(ones[1]), hub], np.random.default_rng(51).integers(0, H.rows, size=100)])
    C, info = run_case(cfg, H, 5000, 8, picks, WITH, dA=dA, itype=itype)            # many tiles of one row; two draws of the hub agree
    P = C.to_host()
    assert np.array_equal(P.col_ids[:5000], P.col_ids[10000:15000]) and len(np.unique(P.col_ids[:5000])) > 4000
    run_case(cfg, H, 0, 8, picks, WITH, dA=dA, itype=itype)                         # k = 0: empty rows


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_an_output_of_2_32_entries_is_refused_before_anything_is_written(cfg, vdtype):
    H = list_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    row = int(np.nonzero(np.diff(H.row_offsets.astype(np.int64)) > 0)[0][0])
    C, frames = framed_c(1 << 20, H.cols, 77, vdtype)                               # (its rows match: the offsets would be reused)
    before = struct_of(C)
    rows = np.full(1 << 20, row)
    for k in (4096, 1 << 32, (1 << 64) - 1):                                        # 2^20 * 4096 = 2^32
        rc, _, info = call(cfg, dA, k, 1, rows, WITH, C=C)
        assert rc == ERR_NNZ_OVERFLOW and struct_of(C) == before and list(vars(info).values()) == [0] * 6
        assert untouched(*frames)
    rc, C1, info = call(cfg, dA, 4095, 1, rows[:2048], WITH)                        # ... and one draw fewer per row is served
    assert rc == OK and info.nnz_out == 2048 * 4095
    # without replacement: the gathered rows may not hold 2^32 entries either (as the extraction)
    hub = int(np.argmax(np.diff(H.row_offsets.astype(np.int64))))
    rc, _, info = call(cfg, dA, 2, 1, np.full(1 << 20, hub), WITHOUT, C=C)
    assert (1 << 20) * (LDS + 900) >= 1 << 32 and rc == ERR_NNZ_OVERFLOW and struct_of(C) == before and untouched(*frames)


# ---------------------------------------------------------------------------------------------------- 6: refusals on the device
@pytest.mark.parametrize("mode", MODES, ids=MIDS)
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_hostile_input_is_refused_with_nothing_written(cfg, vdtype, mode):
    rng = np.random.default_rng(61)
    lens = np.concatenate([rng.integers(1, 9, size=400), [2 * LDS + 5], rng.integers(1, 9, size=99)])
    H = host_csr(lens, 800, vdtype, seed=62)
    hub, k, seed = 400, 5, 17
    picks = np.concatenate([rng.permutation(np.arange(0, 500, 2)), [hub, 3]])         # the even rows and row 3: row 7 is not gathered
    want = want_of(H, k, seed, picks, mode)
    nnz_out = len(want[1])
    C, frames = framed_c(len(picks), 800, nnz_out, vdtype)                          # rows and nnz match: every buffer would be reused
    before = struct_of(C)
    good = sa.dCSR.from_host(H)

    def refused(A, what, rows=picks, itype=torch.int64, **kw):
        rc, _, info = call(cfg, A, k, seed, rows, mode, C=C, itype=itype, **kw)
        assert rc == ERR_INVALID, what
        assert struct_of(C) == before and list(vars(info).values()) == [0] * 6, what
        assert untouched(*frames), what

    for bad_index in (-1, (1 << 32) + 3, H.rows, 1 << 62):
        for at in (0, len(picks) - 1):
            rows = picks.copy()
            rows[at] = bad_index
            refused(good, ("index", bad_index, at), rows=rows)
    for bad_index in (H.rows, -1):                                                   # (as uint32: 2^32 - 1)
        rows = picks.copy()
        rows[100] = bad_index
        refused(good, ("index", bad_index, "uint32"), rows=rows, itype=torch.int32)
    for what, change in (("an offset that descends", lambda ro: ro.__setitem__(17, ro[18] + 1)),      # (a row nobody gathers: all rows are checked)
                         ("a descent in front of the long row", lambda ro: ro.__setitem__(hub, ro[hub + 1] + 1)),
                         ("an offset past nnz", lambda ro: ro.__setitem__(slice(401, None), H.nnz + 1)),
                         ("an offset near 2^32", lambda ro: ro.__setitem__(slice(401, None), 0xFFFFFFF0)),
                         ("a last offset short of nnz", lambda ro: ro.__setitem__(H.rows, H.nnz - 1))):
        ro = H.row_offsets.copy()
        change(ro)
        refused(device_matrix(H, ro=ro), what)
    refused(device_matrix(H, nnz=H.nnz - 1), "the declared nnz is what the rows hold")
    # an id = cols in a gathered row: at its first place, at its last, and at a place the sample did not take
    taken = set(want[4].tolist())
    a, b = int(H.row_offsets[hub]), int(H.row_offsets[hub + 1])
    skipped = next(p for p in range(a + 1, b - 1) if p not in taken)
    short = int(picks[5])
    for at in (a, b - 1, skipped, int(H.row_offsets[short]), int(H.row_offsets[short + 1]) - 1):
        for bad in (H.cols, 0xFFFFFFFF):
            col = H.col_ids.copy()
            col[at] = bad
            refused(device_matrix(H, col=col), ("id", at, bad))
    # ... the same bad id in a row nobody gathers is served: its ids are never read
    col = H.col_ids.copy()
    col[int(H.row_offsets[7])] = H.cols
    rc, _, info = call(cfg, device_matrix(H, col=col), k, seed, picks, mode, C=C)
    assert rc == OK and struct_of(C) == before and vars(info) == want[3]
    vs = np.dtype(vdtype).itemsize
    assert np.array_equal(framed(frames[2], (len(picks) + 1) * 4, np.uint32), want[0])   # the clean call fills exactly the three arrays
    assert np.array_equal(framed(frames[1], nnz_out * 4, np.uint32), want[1])
    assert np.array_equal(framed(frames[0], nnz_out * vs, want[2].dtype), want[2])
    # the arguments the host refuses, with a device behind them
    dA = device_matrix(H)
    for kw in (dict(mode=2), dict(index_bytes=2), dict(row_base=(1 << 62) + 1), dict(n_rows=H.rows + 1), dict(n_rows=0)):
        rc, _, info = call(cfg, dA, k, seed, None, kw.pop("mode", mode), C=C, **kw)
        assert rc == ERR_INVALID and struct_of(C) == before, kw
    rc, _, _ = call(cfg, dA, k, seed, None, mode, C=dA)                             # C sharing its buffers with A
    assert rc == ERR_INVALID
    # the index inside A's entries or C's buffers: refused before a word of it is read
    keep = dA._keep
    filled = [t.clone() for t in frames]                                            # (the clean call's result lies in the frames now)
    for inside in (keep[1], keep[2], frames[1]):                                    # A's col_ids and data, C's col_ids
        rc, _, _ = call(cfg, dA, k, seed, None, mode, C=C, index=inside.view(torch.int32)[32:], n_rows=2, index_bytes=4)
        assert rc == ERR_INVALID and struct_of(C) == before and all(torch.equal(t, f) for t, f in zip(frames, filled))


def test_the_index_inside_a_views_entries_is_found_on_the_device(cfg):
    # the host knows where a view's buffers start, not where its entries lie: the check pass compares the spans
    H = class_matrix(np.float64)
    dA = device_matrix(H)
    r0, r1 = 280, 300
    a, nnz = int(H.row_offsets[r0]), int(H.row_offsets[r1]) - int(H.row_offsets[r0])
    assert a > nnz + 8                                                              # (the host's span of col_ids ends in front of the view's entries)
    V = sa.dCSR.from_device(r1 - r0, H.cols, nnz, dA._c.row_offsets + 4 * r0, dA._c.col_ids, dA._c.data, dtype=np.float64, keep=dA)
    ids = dA._keep[1]
    C, frames = framed_c(3, H.cols, 5, np.float64)
    before = struct_of(C)
    rc, _, _ = call(cfg, V, 2, 1, index=ids[a + 1:], n_rows=3, index_bytes=4, C=C)  # inside the view's ids
    assert rc == ERR_INVALID and struct_of(C) == before and untouched(*frames)


# ---------------------------------------------------------------------------------------------------- 7: ownership, guards, stream
def test_c_keeps_the_buffers_whose_size_stays(cfg):
    H = class_matrix(np.float64)
    dA = sa.dCSR.from_host(H)
    C, info = run_case(cfg, H, 6, 1, dA=dA)
    p0 = struct_of(C)[3:]
    rc, _, info1 = call(cfg, dA, 6, 2, C=C)                                           # same rows, same nnz: all three stay
    assert rc == OK and info1.nnz_out == info.nnz_out and struct_of(C)[3:] == p0
    check(C, info1, want_of(H, 6, 2), H.cols)
    rc, _, info2 = call(cfg, dA, 9, 2, C=C)                                           # another nnz: data and col_ids are new
    p2 = struct_of(C)[3:]
    assert rc == OK and info2.nnz_out != info.nnz_out and p2[2] == p0[2] and p2[0] != p0[0] and p2[1] != p0[1]
    check(C, info2, want_of(H, 9, 2), H.cols)
    rc, _, info3 = call(cfg, dA, 9, 2, [5, 4, 3], WITH, C=C)                          # another number of rows: row_offsets is new
    assert rc == OK and struct_of(C)[5] != p2[2] and C.rows == 3
    check(C, info3, want_of(H, 9, 2, [5, 4, 3], WITH), H.cols)


def test_guard_zones_stay_clean(cfg):
    cfg.set_option("guard_bytes", 4096)
    try:
        H = edge_matrix(np.float64)
        dA = sa.dCSR.from_host(H)
        picks = np.random.default_rng(71).integers(0, H.rows, size=300)
        C, _ = run_case(cfg, H, 3, 1, dA=dA)
        set_classes(cfg, "long")
        C2, _ = run_case(cfg, H, 40, 2, picks, dA=dA)
        C3, _ = run_case(cfg, H, 40, 2, picks, WITH, dA=dA)
        del C, C2, C3
    finally:
        cfg.set_option("guard_bytes", 0)


@pytest.mark.parametrize("replace", [False, True], ids=MIDS)
def test_the_wrapper_its_positions_and_the_callers_stream(cfg, replace):
    H = class_matrix(np.float64)
    mode = WITH if replace else WITHOUT
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    dA = device_matrix(H)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big = torch.sort(torch.rand(1 << 23, device=DEV)).values                      # work in front of the indices on the stream
        picks_t = torch.randint(0, H.rows, (500,), device=DEV) + (big[:1] * 0).long()
        C, info, pos = sa.sample_neighbors(dA, 8, 5, rows=picks_t, replace=replace, return_pos=True, cfg=cfg)   # no synchronise in between
    torch.cuda.synchronize()
    cfg.set_stream(None)
    picks = picks_t.cpu().numpy()
    want = want_of(H, 8, 5, picks, mode)
    check(C, info, want, H.cols)
    assert pos.dtype == torch.int64 and pos.is_cuda and np.array_equal(pos.cpu().numpy(), want[4])
    P = C.to_host()
    at = pos.cpu().numpy()
    assert np.array_equal(H.col_ids[at], P.col_ids) and np.array_equal(bits(H.data[at]), bits(P.data))   # the edge ids
    # int32 indices, no list, no config; a float matrix; a view's positions count from the start of its buffers
    for rows in (None, picks_t.to(torch.int32)):
        C1, info1 = sa.sample_neighbors(dA, 8, 5, rows=rows, replace=replace)
        check(C1, info1, want_of(H, 8, 5, None if rows is None else picks, mode), H.cols)
    H32 = class_matrix(np.float32)
    C2, info2, pos2 = sa.sample_neighbors(sa.dCSR.from_host(H32), 8, 5, rows=picks_t, replace=replace, return_pos=True, cfg=cfg)
    check(C2, info2, want_of(H32, 8, 5, picks, mode), H.cols)
    assert torch.equal(pos2, pos)
    for view in (sa.dCSR.from_host(H).row_view(40, 250),
                 sa.dCSR.from_device(210, H.cols, int(H.row_offsets[250]) - int(H.row_offsets[40]), dA._c.row_offsets + 160, dA._c.col_ids,
                                     dA._c.data, keep=dA)):                          # (the second without host offsets)
        view_h = sa.HostCSR(210, H.cols, H.row_offsets[40:251], H.col_ids, H.data)
        C3, info3, pos3 = sa.sample_neighbors(view, 8, 5, replace=replace, row_base=40, return_pos=True, cfg=cfg)
        want3 = want_of(view_h, 8, 5, None, mode, row_base=40)
        check(C3, info3, want3, H.cols)
        assert np.array_equal(pos3.cpu().numpy(), want3[4])
    C4, info4, pos4 = sa.sample_neighbors(dA, 8, 5, rows=picks_t[:0], replace=replace, return_pos=True, cfg=cfg)   # an empty list
    assert (C4.rows, C4.nnz, len(pos4)) == (0, 0, 0)


def test_the_sample_feeds_the_pipeline(cfg):
    # sample_neighbors -> induced_subgraph: the sampled frontier's adjacency; a canonical A gives canonical rows
    import scipy.sparse as sp
    rng = np.random.default_rng(81)
    S = sp.random(1500, 1500, density=20 / 1500, format="csr", random_state=rng, dtype=np.float64)
    S.sort_indices()
    dA = sa.dCSR.from_host(sa.HostCSR(1500, 1500, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.copy()))
    seeds = torch.from_numpy(rng.permutation(1500)[:64]).to(DEV)
    C, info = sa.sample_neighbors(dA, 5, 2026, rows=seeds, cfg=cfg)
    check(C, info, numpy_sample(S.indptr, S.indices, S.data, 5, 2026, seeds.cpu().numpy()), 1500)
    Hc = C.to_host()
    assert all(np.all(np.diff(Hc.col_ids[a:b].astype(np.int64)) > 0) for a, b in zip(Hc.row_offsets[:-1], Hc.row_offsets[1:]))
    out = sa.dCSR()
    sa.MultiplyspECK(C, dA, out, cfg, sa.Timings())                                   # speck_multiply_f64 takes it as it is
    assert out.rows == 64 and out.nnz > 0
    nodes = torch.unique(torch.cat([seeds, torch.from_numpy(Hc.col_ids.astype(np.int64)).to(DEV)]))
    sub, sub_info = sa.induced_subgraph(dA, nodes, config=cfg)
    assert sub.rows == sub.cols == len(nodes) and sub_info.nnz_out > 0


def test_the_caller_that_includes_sample_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_sample.cpp")
    out = str(tmp_path / "caller_sample")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "sample caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
