"""speck_from_coo_* and speck_to_coo on the GPU (speck_amd/csrc/coo.hip).  The expectation is numpy in this file, compared
byte for byte: with p = np.argsort(row, kind="stable") the result holds col[p] and val[p], and its offsets are the running
sum of np.bincount(row).  The value of an entry is its input position -- as an integer at even positions, in the payload of
a NaN at odd ones --, so the order of the result is visible and a value that went through arithmetic would lose its bits.
Device arrays the library must not touch, or must fill exactly, live in frames of a payload byte whose padding must
survive.  TILE = 2048 entries per tile of the check pass, a thread holds 8 consecutive ids; the sort walks tiles of 2048
entries in 1024 slices of whole tiles."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID = 0, 1
DEV = "cuda:0"
TILE = sa.COO_TILE_ENTRIES
PER = 8                                   # ids a thread of the check pass holds
SLICES = sa.TRANSPOSE_BLOCKS
PAYLOAD = 0xC3
PAD = 64                                  # payload bytes on either side of a frame
INFO_FIELDS = ["entries", "rows_empty", "max_row_entries", "sorted_input", "sort_passes"]
COMBOS = [(np.float64, 8), (np.float64, 4), (np.float32, 8), (np.float32, 4)]
COMBO_IDS = ["f64-i64", "f64-u32", "f32-i64", "f32-u32"]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def passes_for(rows):
    """ceil(log2(rows) / 8)"""
    return ((rows - 1).bit_length() + 7) // 8 if rows > 1 else 0


def dev_ids(a, iw, shift=0):
    """the ids on the device, 8 bytes (int64) or 4 bytes (uint32 bits in an int32 tensor) wide; shift: the array starts that
    many ids behind an aligned address"""
    a = np.asarray(a, dtype=np.int64)
    h = a if iw == 8 else (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    t = torch.from_numpy(np.concatenate([np.zeros(shift, h.dtype), h])).to(DEV)
    return t[shift:]


def pos_values(n, vdtype):
    """the input position of every entry: the number at even positions, a NaN with the position for a payload at odd ones"""
    pos = np.arange(n, dtype=np.uint64)
    if vdtype == np.float64:
        b = np.where(pos % 2 == 0, pos.astype(np.float64).view(np.uint64), np.uint64(0x7FF8000000000000) | pos)
        return b.view(np.float64)
    assert n <= 1 << 22
    b = np.where(pos % 2 == 0, pos.astype(np.float32).view(np.uint32), np.uint32(0x7FC00000) | pos.astype(np.uint32))
    return b.astype(np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def expect(row, col, val, rows):
    row = np.asarray(row, dtype=np.int64)
    p = np.argsort(row, kind="stable")
    ro = np.zeros(rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(np.bincount(row, minlength=rows))
    return ro, np.asarray(col)[p].astype(np.uint32), bits(val)[p]


def call(cfg, row_t, col_t, val_t, rows, cols, vdtype, iw, C=None, nnz=None):
    coo = _lib.CDcoo()
    coo.rows, coo.cols, coo.index_bytes = rows, cols, iw
    coo.nnz = int(row_t.numel()) if nnz is None else nnz
    coo.row_ids = row_t.data_ptr() if row_t is not None and row_t.numel() else None
    coo.col_ids = col_t.data_ptr() if col_t is not None and col_t.numel() else None
    coo.data = val_t.data_ptr() if val_t is not None and val_t.numel() else None
    C = sa.dCSR(vdtype) if C is None else C
    info = _lib.CFromCooInfo(7, 7, 7, 7, 7)
    fn = _lib.load().speck_from_coo_f32 if vdtype == np.float32 else _lib.load().speck_from_coo_f64
    rc = fn(cfg._h if cfg is not None else None, C_.byref(coo), C_.byref(C._c), C_.byref(info))
    return rc, C, sa.FromCooInfo(info)


def check(C, info, row, col, val, rows, cols, want=None):
    """C and info against numpy; `want`: an expectation computed before (ro, col, value bits)"""
    ro, ci, vb = expect(row, col, val, rows) if want is None else want
    H = C.to_host()
    assert (C.rows, C.cols, C.nnz) == (rows, cols, len(ci))
    assert np.array_equal(H.row_offsets, ro), "row_offsets"
    assert np.array_equal(H.col_ids, ci), "col_ids"
    assert np.array_equal(bits(H.data), vb), "values"
    lens = np.diff(ro.astype(np.int64))
    in_order = bool((np.diff(np.asarray(row, dtype=np.int64)) >= 0).all())
    assert vars(info) == dict(entries=len(ci), rows_empty=int((lens == 0).sum()), max_row_entries=int(lens.max()) if rows else 0,
                              sorted_input=int(in_order), sort_passes=0 if in_order else passes_for(rows))


def run_case(cfg, row, col, rows, cols, vdtype, iw, shift=0, cfg_none=False):
    val = pos_values(len(row), vdtype)
    rc, C, info = call(None if cfg_none else cfg, dev_ids(row, iw, shift), dev_ids(col, iw, shift), torch.from_numpy(val).to(DEV),
                       rows, cols, vdtype, iw)
    assert rc == OK
    check(C, info, row, col, val, rows, cols)
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


# ---------------------------------------------------------------------------------------------------- 1: stability, sort tiles
ENTRY_COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, SLICES * TILE - 1, SLICES * TILE, SLICES * TILE + 1]
PATTERNS = ["random", "one_row", "alternating", "first_last"]


def pattern_rows(pattern, n, seed):
    rng = np.random.default_rng(seed)
    if pattern == "random":
        return rng.integers(0, 300, size=n)
    if pattern == "one_row":
        return np.full(n, 7, dtype=np.int64)
    if pattern == "alternating":
        return np.where(np.arange(n) % 2 == 0, 5, 2).astype(np.int64)
    return rng.choice(np.array([0, 299]), size=n)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ENTRY_COUNTS)
def test_rows_keep_their_input_order(cfg, n, pattern, vdtype, iw):
    row = pattern_rows(pattern, n, seed=n % 1000 + 1)
    col = np.random.default_rng(n % 1000 + 2).integers(0, 1000, size=n)
    run_case(cfg, row, col, 300, 1000, vdtype, iw)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("n", [5, 65, TILE + 1, 3 * TILE + 3])
@pytest.mark.parametrize("shift", [1, 3])
def test_id_arrays_that_start_off_16_bytes(cfg, shift, n, vdtype, iw):
    rng = np.random.default_rng(n + shift)
    run_case(cfg, rng.integers(0, 300, size=n), rng.integers(0, 1000, size=n), 300, 1000, vdtype, iw, shift=shift)
    run_case(cfg, np.sort(rng.integers(0, 300, size=n)), rng.integers(0, 1000, size=n), 300, 1000, vdtype, iw, shift=shift)


def test_same_bytes_from_run_to_run_and_without_a_config(cfg):
    n = 5 * TILE + 17
    rng = np.random.default_rng(11)
    row, col = rng.integers(0, 300, size=n), rng.integers(0, 1000, size=n)
    for _ in range(3):
        run_case(cfg, row, col, 300, 1000, np.float64, 8)
    run_case(cfg, row, col, 300, 1000, np.float32, 4, cfg_none=True)


# ---------------------------------------------------------------------------------------------------- 2: pass counts
PASS_ROWS = [1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 1 << 27]


@functools.lru_cache(maxsize=1)
def pass_case(rows):
    """about 5000 entries in random rows that include row 0 and row rows - 1, and their expectation per value type"""
    rng = np.random.default_rng(rows % 9973)
    row = rng.integers(0, rows, size=5000)
    row[1234], row[77] = 0, rows - 1
    col = rng.integers(0, 4096, size=5000)
    want = {vd: expect(row, col, pos_values(5000, vd), rows) for vd in (np.float64, np.float32)}
    return row, col, want


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("rows", PASS_ROWS)
def test_sort_passes_follow_the_row_count(cfg, rows, vdtype, iw):
    row, col, want = pass_case(rows)
    val = pos_values(5000, vdtype)
    rc, C, info = call(cfg, dev_ids(row, iw), dev_ids(col, iw), torch.from_numpy(val).to(DEV), rows, 4096, vdtype, iw)
    assert rc == OK
    assert info.sort_passes == (passes_for(rows) if rows > 1 else 0) and info.sorted_input == (1 if rows == 1 else 0)
    check(C, info, row, col, val, rows, 4096, want=want[vdtype])


# ---------------------------------------------------------------------------------------------------- 3: sorted detection
# where a descent row[i] < row[i - 1] is placed: i
DESCENTS = {"inside a 16-byte load": PER * 5 + 1, "between two loads of a thread": PER * 5 + 4, "between lanes": PER * 6,
            "between waves": PER * 64, "across the tile edge": TILE, "at the last pair": 2 * TILE}


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_sorted_input_is_detected_and_one_descent_anywhere_is_not(cfg, vdtype, iw):
    n = 2 * TILE + 1
    row = np.arange(n, dtype=np.int64)                          # strictly ascending: rows = n, an entry each
    col = np.random.default_rng(5).integers(0, 1000, size=n)
    val = pos_values(n, vdtype)
    rc, C, info = call(cfg, dev_ids(row, iw), dev_ids(col, iw), torch.from_numpy(val).to(DEV), n, 1000, vdtype, iw)
    assert rc == OK and info.sorted_input == 1 and info.sort_passes == 0
    base = expect(row, col, val, n)
    check(C, info, row, col, val, n, 1000, want=base)
    for where, i in DESCENTS.items():
        # the triplets i - 1 and i change places: one descent, at i, and the same matrix
        p = np.arange(n)
        p[i - 1], p[i] = i, i - 1
        r2, c2, v2 = row[p], col[p], val[p]
        assert (np.diff(r2) < 0).sum() == 1 and r2[i] < r2[i - 1]
        rc, C, info = call(cfg, dev_ids(r2, iw), dev_ids(c2, iw), torch.from_numpy(v2).to(DEV), n, 1000, vdtype, iw)
        assert rc == OK and info.sorted_input == 0 and info.sort_passes == passes_for(n), where
        check(C, info, r2, c2, v2, n, 1000, want=base)


def test_equal_neighbours_are_in_order(cfg):
    n = 2 * TILE + 1
    row = np.arange(n, dtype=np.int64) // 3
    _, info = run_case(cfg, row, np.arange(n) % 1000, int(row[-1]) + 1, 1000, np.float64, 8)
    assert info.sorted_input == 1


# ---------------------------------------------------------------------------------------------------- 4: hostile ids
@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_one_bad_id_anywhere_is_refused_with_nothing_written(cfg, vdtype, iw):
    n, rows, cols = 2 * TILE + 1, 300, 1000
    rng = np.random.default_rng(3)
    row, col = rng.integers(0, rows, size=n), rng.integers(0, cols, size=n)
    val_t = torch.from_numpy(pos_values(n, vdtype)).to(DEV)
    C, frames = framed_c(rows, cols, n, vdtype)                 # rows and nnz match: every buffer would be reused
    before = struct_of(C)
    wide_only = [-1, (1 << 32) + 3, -(1 << 63)] if iw == 8 else []
    for which, limit in (("row", rows), ("col", cols)):
        for bad in [limit, (1 << 32) - 1] + wide_only:
            for at in (0, n // 2, TILE - 1, TILE, n - 1):
                r2, c2 = row.copy(), col.copy()
                (r2 if which == "row" else c2)[at] = bad
                rc, _, info = call(cfg, dev_ids(r2, iw), dev_ids(c2, iw), val_t, rows, cols, vdtype, iw, C=C)
                assert rc == ERR_INVALID, (which, bad, at)
                assert struct_of(C) == before and list(vars(info).values()) == [0] * 5, (which, bad, at)
                assert untouched(*frames), (which, bad, at)
    # ... and the clean list fills exactly the three arrays
    rc, _, info = call(cfg, dev_ids(row, iw), dev_ids(col, iw), val_t, rows, cols, vdtype, iw, C=C)
    assert rc == OK and struct_of(C) == before
    ro, ci, vb = expect(row, col, pos_values(n, vdtype), rows)
    vs = np.dtype(vdtype).itemsize
    assert np.array_equal(framed(frames[2], (rows + 1) * 4, np.uint32), ro)
    assert np.array_equal(framed(frames[1], n * 4, np.uint32), ci)
    assert np.array_equal(framed(frames[0], n * vs, vb.dtype), vb)


# ---------------------------------------------------------------------------------------------------- 5: ownership, ones, empty
def test_c_keeps_the_buffers_whose_size_stays(cfg):
    rng = np.random.default_rng(8)
    n = 1000
    C, _ = run_case(cfg, rng.integers(0, 300, size=n), rng.integers(0, 50, size=n), 300, 50, np.float64, 8)
    p0 = struct_of(C)[3:]
    val = pos_values(n, np.float64)

    def again(rows, count):
        row, col = rng.integers(0, rows, size=count), rng.integers(0, 50, size=count)
        v = pos_values(count, np.float64)
        rc, _, info = call(cfg, dev_ids(row, 8), dev_ids(col, 8), torch.from_numpy(v).to(DEV), rows, 50, np.float64, 8, C=C)
        assert rc == OK
        check(C, info, row, col, v, rows, 50)
        return struct_of(C)[3:]

    assert val.size == n and again(300, n) == p0                                    # same rows, same nnz: all three stay
    p1 = again(300, n + 5)                                                          # another nnz: data and col_ids are new
    assert p1[2] == p0[2] and p1[0] != p0[0] and p1[1] != p0[1]
    p2 = again(301, n + 5)                                                          # other rows: row_offsets is new
    assert p2[:2] == p1[:2] and p2[2] != p1[2]
    p3 = again(17, 3)                                                               # everything differs
    assert p3[0] != p2[0] and p3[1] != p2[1] and p3[2] != p2[2]


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
def test_no_values_gives_ones(cfg, vdtype, iw):
    n = TILE + 9
    rng = np.random.default_rng(4)
    for row in (rng.integers(0, 300, size=n), np.sort(rng.integers(0, 300, size=n))):
        col = rng.integers(0, 1000, size=n)
        rc, C, info = call(cfg, dev_ids(row, iw), dev_ids(col, iw), None, 300, 1000, vdtype, iw)
        assert rc == OK
        check(C, info, row, col, np.ones(n, dtype=vdtype), 300, 1000)


@pytest.mark.parametrize("vdtype, iw", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("rows", [0, 5])
def test_no_entries(cfg, rows, vdtype, iw):
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    rc, C, info = call(cfg, empty, empty, None, rows, 9, vdtype, iw)
    assert rc == OK and (C.rows, C.cols, C.nnz) == (rows, 9, 0)
    assert np.array_equal(C.to_host().row_offsets, np.zeros(rows + 1, dtype=np.uint32))
    assert vars(info) == dict(entries=0, rows_empty=rows, max_row_entries=0, sorted_input=1, sort_passes=0)


# ---------------------------------------------------------------------------------------------------- 6: to_coo
def host_csr(lens, cols, vdtype=np.float64, seed=1):
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    rng = np.random.default_rng(seed)
    return sa.HostCSR(len(lens), cols, ro, rng.integers(0, cols, size=n).astype(np.uint32), pos_values(n, vdtype))


# empty rows at the front, in the middle (more than a wave's 64 rows of them) and at the end; rows at both sides of the
# 16-entry switch and of the wave's 64 lanes; hub rows
LENS = [0, 0, 0, 5, 2, 16, 17, 15] + [0] * 70 + [3001, 64, 65, 63, 1, 0, 2] + [1] * 130 + [700, 0, 0]


def run_to_coo(cfg, dA, iw, row_base, with_cols=True):
    n = dA.nnz
    fr, fc = frame(max(n, 1) * iw), frame(max(n, 1) * iw)
    rc = _lib.load().speck_to_coo(cfg._h if cfg is not None else None, C_.byref(dA._c), iw, row_base, fr[1], fc[1] if with_cols else None)
    return rc, fr[0], fc[0]


@pytest.mark.parametrize("iw", [8, 4])
@pytest.mark.parametrize("kind", ["owner", "view"])
def test_to_coo_expands_the_rows(cfg, kind, iw):
    H = host_csr(LENS, 1000)
    dA = sa.dCSR.from_host(H)
    r0, r1, row_base = (0, H.rows, 0) if kind == "owner" else (5, H.rows - 1, 1000003)
    A = dA if kind == "owner" else dA.row_view(r0, r1)
    lo, hi = int(H.row_offsets[r0]), int(H.row_offsets[r1])
    assert kind == "owner" or (lo % 2 == 1 and r0 % 2 == 1)                         # an odd base in both senses
    dt = np.int64 if iw == 8 else np.uint32
    want_row = (np.repeat(np.arange(r0, r1), np.diff(H.row_offsets[r0:r1 + 1].astype(np.int64))) - r0 + row_base).astype(dt)
    for with_cols in (True, False):
        rc, fr, fc = run_to_coo(cfg, A, iw, row_base, with_cols)
        assert rc == OK
        assert np.array_equal(framed(fr, (hi - lo) * iw, dt), want_row)
        if with_cols:
            assert np.array_equal(framed(fc, (hi - lo) * iw, dt), H.col_ids[lo:hi].astype(dt))
        else:
            assert untouched(fc)
    # the Python wrapper: torch tensors
    row_t, col_t = sa.to_coo(A, cfg, index_dtype=torch.int64 if iw == 8 else torch.int32, row_base=row_base)
    assert row_t.dtype == (torch.int64 if iw == 8 else torch.int32) and np.array_equal(row_t.cpu().numpy().astype(np.int64), want_row.astype(np.int64))
    assert np.array_equal(col_t.cpu().numpy().astype(np.int64), H.col_ids[lo:hi].astype(np.int64))
    assert sa.to_coo(A, None, cols=False)[1] is None


@pytest.mark.parametrize("rows", [0, 5])
def test_to_coo_of_a_matrix_without_entries(cfg, rows):
    dA = sa.dCSR.from_host(host_csr([0] * rows, 9))
    rc, fr, fc = run_to_coo(cfg, dA, 8, 3)
    assert rc == OK and untouched(fr, fc)
    row_t, col_t = sa.to_coo(dA, cfg)
    assert row_t.shape == (0,) and col_t.shape == (0,) and row_t.dtype == torch.int64
    C, info = sa.from_coo(row_t, col_t, None, (rows, 9), cfg)
    assert (C.rows, C.cols, C.nnz) == (rows, 9, 0) and info.sorted_input == 1


def test_to_coo_refuses_what_does_not_fit_four_bytes(cfg):
    H = host_csr(LENS, 1000)
    dA = sa.dCSR.from_host(H)
    rc, fr, fc = run_to_coo(cfg, dA, 4, (1 << 32) - H.rows + 1)
    assert rc == ERR_INVALID and untouched(fr, fc)
    rc, fr, fc = run_to_coo(cfg, dA, 4, (1 << 32) - H.rows)                         # the last row is 2^32 - 1
    assert rc == OK
    want = (np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64))) + (1 << 32) - H.rows).astype(np.uint32)
    assert np.array_equal(framed(fr, H.nnz * 4, np.uint32), want)
    rc, fr, fc = run_to_coo(cfg, dA, 8, (1 << 40) + 1)                              # ... and eight bytes hold it
    assert rc == OK and framed(fr, H.nnz * 8, np.int64)[-1] == (1 << 40) + H.rows - 2


@pytest.mark.parametrize("iw", [8, 4])
def test_to_coo_refuses_hostile_offsets_and_ids(cfg, iw):
    H = host_csr(LENS, 1000)
    n = H.nnz
    col_t = torch.from_numpy(H.col_ids.view(np.int32)).to(DEV)
    val_t = torch.from_numpy(H.data).to(DEV)

    def attempt(ro, col=col_t, nnz=n, with_cols=True):
        ro_t = torch.from_numpy(np.asarray(ro, dtype=np.uint32).view(np.int32)).to(DEV)
        A = sa.dCSR.from_device(H.rows, H.cols, nnz, ro_t.data_ptr(), col.data_ptr(), val_t.data_ptr(), keep=(ro_t, col, val_t))
        rc, fr, fc = run_to_coo(cfg, A, iw, 0, with_cols)
        return rc, untouched(fr, fc)

    assert attempt(H.row_offsets)[0] == OK
    hub = LENS.index(3001)
    for what, change in (("a descent", lambda ro: ro.__setitem__(hub, ro[hub + 1] + 1)),
                         ("an offset beyond the entries", lambda ro: ro.__setitem__(hub + 1, n + 1)),
                         ("an offset near 2^32", lambda ro: ro.__setitem__(slice(hub + 1, None), 0xFFFFFFF0)),
                         ("a last offset short of nnz", lambda ro: ro.__setitem__(H.rows, n - 1))):
        ro = H.row_offsets.copy()
        change(ro)
        assert attempt(ro) == (ERR_INVALID, True), what
    ro = H.row_offsets.copy()
    ro[0] = 7                                                                       # a first offset above the second, in a view
    assert attempt(ro, nnz=n - 7) == (ERR_INVALID, True)                            # whose n - 7 entries end where the buffers do
    assert attempt(H.row_offsets, nnz=n - 1) == (ERR_INVALID, True)                 # the declared nnz is what the rows hold
    for at in (0, int(H.row_offsets[hub]) + 2999, n - 1):                           # a short row's id, a hub row's, the last
        bad = H.col_ids.copy()
        bad[at] = H.cols
        bad_t = torch.from_numpy(bad.view(np.int32)).to(DEV)
        assert attempt(H.row_offsets, col=bad_t) == (ERR_INVALID, True), at
        assert attempt(H.row_offsets, col=bad_t, with_cols=False)[0] == OK          # nobody asked for the columns


def test_to_coo_refuses_outputs_inside_the_matrix(cfg):
    H = host_csr(LENS, 1000)
    dA = sa.dCSR.from_host(H)
    V = dA.row_view(5, H.rows - 1)                                                  # its entries start at an offset only the device knows
    base = int(H.row_offsets[5])
    spare, ptr = frame(V.nnz * 8)
    L = _lib.load()
    before = dA.to_host()
    for inside in (dA._c.col_ids + 4 * base, dA._c.col_ids + 4 * (base + V.nnz) - 1, dA._c.data + 8 * base + 16):
        assert L.speck_to_coo(cfg._h, C_.byref(V._c), 8, 0, inside, ptr) == ERR_INVALID
        assert L.speck_to_coo(cfg._h, C_.byref(V._c), 8, 0, ptr, inside) == ERR_INVALID
    after = dA.to_host()
    assert untouched(spare) and np.array_equal(before.col_ids, after.col_ids) and np.array_equal(bits(before.data), bits(after.data))


# ---------------------------------------------------------------------------------------------------- 7: round trips
@pytest.mark.parametrize("vdtype", [np.float64, np.float32])
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_there_and_back_is_a_copy(cfg, index_dtype, vdtype):
    H = host_csr(LENS, 1000, vdtype)
    dA = sa.dCSR.from_host(H)
    row, col = sa.to_coo(dA, cfg, index_dtype=index_dtype)
    C, info = sa.from_coo(row, col, dA._c.data, (H.rows, H.cols), cfg, dtype=vdtype, nnz=H.nnz)
    assert info.sorted_input == 1 and info.sort_passes == 0
    G, W = C.to_host(), dA.copy().to_host()
    assert np.array_equal(G.row_offsets, W.row_offsets) and np.array_equal(G.col_ids, W.col_ids) and np.array_equal(bits(G.data), bits(W.data))
    assert np.array_equal(bits(G.data), bits(H.data))


def test_a_shuffled_list_with_duplicates_becomes_a_matrix_the_multiply_takes(cfg):
    from oracle import pyoracle as po
    n, E = 500, 6000
    rng = np.random.default_rng(21)
    r, c = rng.integers(0, n, size=E), rng.integers(0, n, size=E)
    r[:500], c[:500] = r[500:1000], c[500:1000]                                     # every one of these pairs twice at least
    v = rng.integers(1, 9, size=E).astype(np.float64)
    p = rng.permutation(E)
    r, c, v = r[p], c[p], v[p]
    C, info = sa.from_coo(torch.from_numpy(r).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(v).to(DEV), (n, n), cfg,
                          sum_duplicates=True)
    assert info.sorted_input == 0 and info.entries == E
    S = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    S.sort_indices()
    G = C.to_host()
    assert C.nnz == S.nnz < E
    assert np.array_equal(G.row_offsets, S.indptr.astype(np.uint32)) and np.array_equal(G.col_ids, S.indices.astype(np.uint32))
    assert np.array_equal(G.data, S.data)
    out = sa.dCSR()
    sa.MultiplyspECK(C, C, out, cfg, sa.Timings())
    Hh = po.HostCSR(n, n, G.row_offsets, G.col_ids, G.data)
    R, _ = po.spgemm(Hh, Hh)
    P = out.to_host()
    assert np.array_equal(P.row_offsets, R.row_offsets) and np.array_equal(P.col_ids, R.col_ids) and np.array_equal(P.data, R.data)


@pytest.mark.parametrize("E", [TILE + 1, TILE + 2])        # E odd: the column ids start 8 bytes off a 16-byte address
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_from_edge_index(cfg, index_dtype, E):
    rng = np.random.default_rng(E)
    ei = np.stack([rng.integers(0, 300, size=E), rng.integers(0, 200, size=E)])
    t = torch.from_numpy(ei).to(DEV).to(index_dtype)
    C, info = sa.from_edge_index(t, None, (300, 200), cfg, dtype=np.float32)
    check(C, info, ei[0], ei[1], np.ones(E, dtype=np.float32), 300, 200)
    w = pos_values(E, np.float64)
    wide = torch.zeros((2, E + 5), dtype=index_dtype, device=DEV)                   # rows E + 5 apart
    wide[:, :E] = t
    C, info = sa.from_edge_index(wide[:, :E], torch.from_numpy(w).to(DEV), (300, 200), cfg)
    check(C, info, ei[0], ei[1], w, 300, 200)
    with pytest.raises(ValueError, match="from_edge_index: edge_index"):
        sa.from_edge_index(t.t().contiguous().t(), None, (300, 200), cfg)           # E x 2 in memory
    with pytest.raises(sa.SpeckError) as e:
        sa.from_edge_index(t, None, (300, int(ei[1].max())), cfg)
    assert e.value.status == ERR_INVALID


# ---------------------------------------------------------------------------------------------------- 8: stream, guards, caller
def test_ids_made_on_the_callers_stream_need_no_synchronise(cfg):
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    n = 3 * TILE + 5
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    with torch.cuda.stream(s):
        big = torch.randint(0, 1 << 40, (1 << 23,), device=DEV, generator=g)
        big = torch.sort(big).values                                                # work in front of the ids on the stream
        ids = torch.randint(0, 1 << 40, (2, n), device=DEV, generator=g) + big[:1] * 0
        row_t, col_t = ids[0] % 300, (ids[1] >> 3) % 1000
        val_t = torch.arange(n, device=DEV, dtype=torch.float64) * 0.5
        C, info = sa.from_coo(row_t, col_t, val_t, (300, 1000), cfg)                # no synchronise in between
    torch.cuda.synchronize()
    cfg.set_stream(None)
    check(C, info, row_t.cpu().numpy(), col_t.cpu().numpy(), val_t.cpu().numpy(), 300, 1000)


def test_guard_zones_stay_clean(cfg):
    cfg.set_option("guard_bytes", 4096)
    try:
        n = 2 * TILE + 3
        rng = np.random.default_rng(2)
        for row in (rng.integers(0, 300, size=n), np.sort(rng.integers(0, 300, size=n))):
            C, _ = run_case(cfg, row, rng.integers(0, 1000, size=n), 300, 1000, np.float64, 8)
        H = C.to_host()
        rc, fr, fc = run_to_coo(cfg, C, 8, 0)
        assert rc == OK
        assert np.array_equal(framed(fr, n * 8, np.int64), np.repeat(np.arange(300), np.diff(H.row_offsets.astype(np.int64))))
        del C
    finally:
        cfg.set_option("guard_bytes", 0)


def test_the_caller_that_includes_fromcoo_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_from_coo.cpp")
    out = str(tmp_path / "caller_from_coo")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "from_coo caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
