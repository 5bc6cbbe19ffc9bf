"""speck_topk_* on the GPU (speck_amd/csrc/topk.hip).  The expectation is the numpy statement of the contract
(tests/test_topk_host.py, numpy_topk, which that file compares with a brute-force count of beaters), compared byte for byte:
row_offsets, col_ids, the values' bits and every field of info.  Column ids are random, unsorted and repeat, and the values
that are not ties carry their position in the low mantissa bits: an entry that lands in another place shows.  The class
limits come from speck_amd.TOPK_GROUP_MAX / TOPK_LDS_MAX: a group of 8 / 16 / 32 / 64 lanes ranks rows of up to GROUP_MAX / 8,
/ 4, / 2, GROUP_MAX entries, a workgroup with the keys in LDS rows of up to LDS_MAX, the long-row kernel the rest; the debug
options topk_group_max / topk_lds_max lower them, so one row can be sent through every class."""
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
from test_topk_host import INFO_FIELDS, MODES, bits, numpy_topk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID = 0, 1
DEV = "cuda:0"
G, LDS = sa.TOPK_GROUP_MAX, sa.TOPK_LDS_MAX
PAYLOAD = 0xC3
PAD = 64                                  # payload bytes on either side of a frame
VDTYPES = [np.float64, np.float32]
VIDS = ["f64", "f32"]
# (topk_group_max, topk_lds_max): the classes a row of more than k entries can be sent through
CLASSES = {"group": (G, LDS), "lds": (0, LDS), "long": (0, 0)}
GROUP_TRIP = 2048 * 32                    # rows of the narrowest group one launch takes before its workgroups stride
ROW_TRIP = 2048                           # ... rows of the LDS class; the long class strides after 1024


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def utype(vdtype):
    return np.uint64 if np.dtype(vdtype).itemsize == 8 else np.uint32


def nan_bits(pos, vdtype, negative=None):
    """quiet NaNs whose payload is the position"""
    pos = np.asarray(pos, dtype=np.uint64)
    if np.dtype(vdtype).itemsize == 8:
        b = np.uint64(0x7FF8000000000000) | (pos & np.uint64(0xFFFFFFFF))
        sign = np.uint64(1 << 63)
    else:
        b = (np.uint64(0x7FC00000) | (pos & np.uint64(0x3FFFFF))).astype(np.uint32)
        sign = np.uint32(1 << 31)
    return b if negative is None else np.where(negative, b | sign, b)


def mixed_values(n, vdtype, seed):
    """distinct magnitudes over seven decades with the position in the low mantissa bits (both signs); a quarter of the
    entries from a pool of seven values (heavy ties, -0.0 and 0.0 among them); NaNs with payloads, infinities, subnormals"""
    rng = np.random.default_rng(seed)
    u = utype(vdtype)
    low = 16 if u is np.uint64 else 10
    mag = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)).astype(vdtype)
    pos = np.arange(n, dtype=np.uint64)
    b = (bits(mag) & ~u((1 << low) - 1)) | (pos & np.uint64((1 << low) - 1)).astype(u)
    kind = rng.random(n)
    pool = np.array([1.0, -1.0, 3.0, -3.0, 0.0, -0.0, 2.5], dtype=vdtype)
    b = np.where(kind < 0.25, bits(pool[rng.integers(0, len(pool), size=n)]), b)
    b = np.where((kind >= 0.25) & (kind < 0.30), nan_bits(pos, vdtype, rng.random(n) < 0.5), b)
    b = np.where((kind >= 0.30) & (kind < 0.33), bits(np.where(rng.random(n) < 0.5, np.inf, -np.inf).astype(vdtype)), b)
    sub = ((pos & np.uint64((1 << low) - 1)) + np.uint64(1)).astype(u) | np.where(rng.random(n) < 0.5, u(1) << u(8 * u().itemsize - 1), u(0))
    b = np.where((kind >= 0.33) & (kind < 0.38), sub, b)
    return np.ascontiguousarray(b.astype(u)).view(vdtype)


def host_csr(lens, cols=5000, vdtype=np.float64, seed=1, values=None):
    """rows of the given lengths; column ids at random (unsorted, duplicates among them)"""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    ci = np.random.default_rng(seed).integers(0, max(cols, 1), size=n)
    val = mixed_values(n, vdtype, seed + 1) if values is None else np.ascontiguousarray(values, dtype=vdtype)
    assert len(val) == n
    return sa.HostCSR(len(lens), cols, ro, ci.astype(np.uint32), val)


def rows_csr(rows, vdtype, cols=5000, seed=3):
    """a matrix from a list of value arrays, a row each"""
    return host_csr([len(r) for r in rows], cols, vdtype, seed, values=np.concatenate([np.asarray(r, dtype=vdtype) for r in rows]))


def call(cfg, dA, k, mode, C=None, reserved=0):
    """(status, C, TopKInfo)"""
    prm = _lib.CTopKParams()
    prm.k, prm.mode, prm.reserved = k, mode, reserved
    C = sa.dCSR(dA.dtype) if C is None else C
    info = _lib.CTopKInfo(*([7] * 8))
    fn = _lib.load().speck_topk_f32 if dA.dtype == np.float32 else _lib.load().speck_topk_f64
    rc = fn(cfg._h if cfg is not None else None, C_.byref(dA._c), C_.byref(prm), C_.byref(C._c), C_.byref(info))
    torch.cuda.synchronize()
    return rc, C, sa.TopKInfo(info)


def check(C, info, want, cols):
    ro, ci, vb, winfo = want
    assert (C.rows, C.cols, C.nnz) == (len(ro) - 1, cols, len(ci))
    assert C._c.data and C._c.col_ids and C._c.row_offsets                          # (buffers of one entry where nnz is 0)
    H = C.to_host()
    assert np.array_equal(H.row_offsets, ro), "row_offsets"
    assert np.array_equal(H.col_ids, ci), "col_ids"
    assert np.array_equal(bits(H.data), vb), "values"
    assert vars(info) == winfo


def want_of(H, k, mode):
    return numpy_topk(H.row_offsets, H.col_ids, H.data, k, mode)


def run_case(cfg, H, k, mode, dA=None):
    dA = sa.dCSR.from_host(H) if dA is None else dA
    rc, C, info = call(cfg, dA, k, mode)
    assert rc == OK
    check(C, info, want_of(H, k, mode), H.cols)
    return C, info


def set_classes(cfg, name):
    cfg.set_option("topk_group_max", CLASSES[name][0])
    cfg.set_option("topk_lds_max", CLASSES[name][1])


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


def device_matrix(H, ro=None, col=None, nnz=None, framed_pads=False):
    """A from torch tensors (the upload would not take hostile offsets or ids), one element at least each"""
    def dev(a):
        a = np.ascontiguousarray(a)
        a = a if len(a) else np.zeros(1, dtype=a.dtype)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)
    ro_t = dev(np.asarray(H.row_offsets if ro is None else ro, dtype=np.uint32))
    col_t = dev(np.asarray(H.col_ids if col is None else col, dtype=np.uint32))
    val_t = dev(H.data)
    return sa.dCSR.from_device(H.rows, H.cols, H.nnz if nnz is None else nnz, ro_t.data_ptr(), col_t.data_ptr(), val_t.data_ptr(),
                               dtype=H.data.dtype, keep=(ro_t, col_t, val_t))


# ---------------------------------------------------------------------------------------------------- 1: lengths around k
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_lengths_around_k(cfg, k, vdtype):
    lens = [k - 1, k, k + 1, 0, k + 1, k, 0, 0, k - 1, k + 1] * 7 + [0]
    H = host_csr(lens, 300, vdtype, seed=k)
    dA = sa.dCSR.from_host(H)
    for mode in MODES.values():
        C, info = run_case(cfg, H, k, mode, dA=dA)
        assert info.rows_cut == 21 and info.max_row_entries == k and info.dropped == 21


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_k_zero_and_k_beyond_every_row(cfg, vdtype):
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(0, 30, size=400), [G + 1, 0, LDS + 1, 3]])
    H = host_csr(lens, 900, vdtype, seed=6)
    dA = sa.dCSR.from_host(H)
    for mode in MODES.values():
        C, info = run_case(cfg, H, 0, mode, dA=dA)
        assert C.nnz == 0 and info.nnz_out == 0 and info.dropped == H.nnz and info.rows_cut == int((lens > 0).sum())
        assert info.max_row_entries == 0 and info.ties_cut == 0 and info.nan_kept == 0
        for k in (LDS + 1, LDS + 2, (1 << 32) - 1, 1 << 32, 1 << 40, (1 << 64) - 1):      # C is A, bit for bit
            C, info = run_case(cfg, H, k, mode, dA=dA)
            G_ = C.to_host()
            assert np.array_equal(G_.row_offsets, H.row_offsets) and np.array_equal(G_.col_ids, H.col_ids) and np.array_equal(bits(G_.data), bits(H.data))
            assert info.rows_cut == 0 and info.dropped == 0 and info.ties_cut == 0 and info.max_row_entries == LDS + 1
            assert info.nan_kept == int(np.isnan(H.data).sum()) > 0
    _, info = run_case(cfg, H, LDS, MODES["abs"], dA=dA)                              # one row is cut by one entry
    assert info.rows_cut == 1 and info.dropped == 1


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_empty_rows_only_and_no_rows(cfg, vdtype):
    H = host_csr([0] * 700, 50, vdtype)
    for k in (0, 3, 1 << 40):
        C, info = run_case(cfg, H, k, MODES["largest"])
        assert C.nnz == 0 and vars(info) == dict(rows=700, rows_cut=0, entries_in=0, nnz_out=0, dropped=0, max_row_entries=0, ties_cut=0, nan_kept=0)
    H0 = host_csr([], 50, vdtype)
    for c in (cfg, None):
        rc, C, info = call(c, device_matrix(H0), 3, MODES["abs"])
        assert rc == OK and (C.rows, C.cols, C.nnz) == (0, 50, 0) and list(vars(info).values()) == [0] * 8
        assert C.to_host().row_offsets.tolist() == [0]


# ---------------------------------------------------------------------------------------------------- 2: class edges
@functools.lru_cache(maxsize=None)
def edge_matrix(vdtype):
    """every lane-group width's last and first length, the two class limits and the lengths beyond them, long rows that take
    several trips of a workgroup, short and empty rows between them: all classes in one matrix"""
    edges = [G // 8, G // 8 + 1, G // 4, G // 4 + 1, G // 2, G // 2 + 1, G, G + 1, LDS, LDS + 1, 2 * LDS + 5, 70001]
    rng = np.random.default_rng(11)
    lens = []
    for e in edges:
        lens += [e] + rng.integers(0, 12, size=5).tolist()
    return host_csr(lens, 100000, vdtype, seed=12), edges


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("k", [3, G // 8, G // 4 + 1, G, LDS])
def test_class_edges(cfg, k, vdtype):
    H, edges = edge_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    for mode in MODES.values():
        _, info = run_case(cfg, H, k, mode, dA=dA)
        short = int((np.diff(H.row_offsets.astype(np.int64)) < 12).sum()) if k < 12 else 0   # (the rows between the edges hold < 12 entries)
        assert sum(e > k for e in edges) <= info.rows_cut <= sum(e > k for e in edges) + short and info.max_row_entries == k


def test_lists_longer_than_a_launchs_first_trip(cfg):
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "topk.hip")).read()         # (the grids the two constants above restate)
    assert "kGroupGrid = 2048, kLdsGrid = 2048, kLongGrid = 1024" in source and GROUP_TRIP == 2048 * 32 and ROW_TRIP == 2048
    H = host_csr([9] * (GROUP_TRIP + 500), 64, np.float64, seed=13)                   # the narrowest group: 32 rows per workgroup
    _, info = run_case(cfg, H, 3, MODES["largest"])
    assert info.rows_cut == GROUP_TRIP + 500
    H = host_csr([9, 0, 2, 11] * (ROW_TRIP // 2 + 50), 64, np.float32, seed=14)
    dA = sa.dCSR.from_host(H)
    for name in ("lds", "long"):                                                    # one row per workgroup
        set_classes(cfg, name)
        _, info = run_case(cfg, H, 3, MODES["abs"], dA=dA)
        assert info.rows_cut == ROW_TRIP + 100


# ---------------------------------------------------------------------------------------------------- 3: every class, the same bytes
@functools.lru_cache(maxsize=None)
def class_matrix(vdtype):
    lens = np.concatenate([np.arange(1, 301), [LDS + 7, 2 * LDS + 5, 9000]])
    return host_csr(np.random.default_rng(21).permutation(lens), 20000, vdtype, seed=22)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("by", list(MODES))
def test_every_class_gives_the_same_bytes(cfg, by, vdtype):
    H = class_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    for k in (5, 40):
        want = want_of(H, k, MODES[by])
        for gmax, lmax in ((G, LDS), (0, LDS), (0, 0), (G, 0), (G // 8, 200), (100, 1000), (G // 2 + 1, G), (G + 50, LDS + 50)):
            cfg.set_option("topk_group_max", gmax)                                      # (beyond the defines: clamped)
            cfg.set_option("topk_lds_max", lmax)
            for _ in range(2):                                                          # ... and from run to run
                rc, C, info = call(cfg, dA, k, MODES[by])
                assert rc == OK
                check(C, info, want, H.cols)


# ---------------------------------------------------------------------------------------------------- 4: ties and the cut
def tie_rows(k, vdtype, n=200):
    rng = np.random.default_rng(31)
    f = np.dtype(vdtype).type
    desc = (n - np.arange(n)).astype(vdtype)                                         # n distinct values, descending
    rows = {}
    rows["all equal"] = np.full(n, 2.5)
    same = desc.copy()
    same[k] = same[k - 1]                                                            # the k-th and the (k+1)-th key are equal
    rows["the k-th and the next are equal"] = rng.permutation(same)
    ulp = desc.copy()
    ulp[k] = np.nextafter(ulp[k - 1], f(-np.inf))                                    # ... one ulp apart
    rows["the k-th and the next one ulp apart"] = rng.permutation(ulp)
    zeros = -np.arange(1, n + 1).astype(vdtype)
    zeros[rng.permutation(n)[:k + 4]] = np.where(np.arange(k + 4) % 2 == 0, -0.0, 0.0)   # k + 4 zeros of both signs above negatives
    rows["-0.0 against +0.0"] = zeros
    threes = np.where(rng.random(n) < 0.5, 1.0, 2.0)
    threes[rng.permutation(n)[:k + 3]] = np.where(np.arange(k + 3) % 2 == 0, -3.0, 3.0)
    rows["-3 against 3"] = threes
    above = rng.random(n) * 0.5                                                      # exactly k keys above the bin of the k-th: t == 0
    above[rng.permutation(n)[:k]] = 1024.0 + np.arange(k)
    rows["exactly k keys above the rest"] = above
    whole = rng.random(n) * 0.5
    at = rng.permutation(n)[:k]
    whole[at[:k - 3]] = 1024.0 + np.arange(k - 3)
    whole[at[k - 3:]] = 5.0                                                          # the three equals are all taken: t is the whole bin
    rows["t is the whole bin"] = whole
    part = whole.copy()
    part[rng.permutation(np.setdiff1d(np.arange(n), at))[:2]] = 5.0                  # ... three of five
    rows["t is a part of the bin"] = part
    long_n = 3000                                                                    # ties whose kept members lie in different chunks of the walk
    chunks = np.arange(long_n) * 0.0001
    chunks[rng.permutation(np.setdiff1d(np.arange(long_n), [100, 1100, 2100, 2900]))[:k - 2]] = 9.0 + np.arange(k - 2)
    chunks[[100, 1100, 2100, 2900]] = 5.0
    rows["ties across the chunks of a long row"] = chunks
    trip_n = 2 * LDS + 808                                                           # ... in different trips of the long-row kernel's walk
    at = [100, LDS + 900, 2 * LDS + 300, 2 * LDS + 700]                              #     (it takes 4 x 1024 entries a trip: three trips)
    trips = np.arange(trip_n) * 0.0001
    trips[rng.permutation(np.setdiff1d(np.arange(trip_n), at))[:k - 2]] = 9.0 + np.arange(k - 2)
    trips[at] = 5.0
    rows["ties across the trips of a long row's walk"] = trips
    return rows


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_ties_and_the_cut(cfg, cls, vdtype):
    k = 7
    rows = tie_rows(k, vdtype)
    set_classes(cfg, cls)
    H = rows_csr(list(rows.values()), vdtype)
    dA = sa.dCSR.from_host(H)
    for mode in MODES.values():
        run_case(cfg, H, k, mode, dA=dA)
    for name, by, ties in (("all equal", "largest", 1), ("the k-th and the next are equal", "largest", 1), ("the k-th and the next one ulp apart", "largest", 0),
                           ("-0.0 against +0.0", "largest", 1), ("-3 against 3", "abs", 1), ("exactly k keys above the rest", "abs", 0),
                           ("t is the whole bin", "largest", 0), ("t is a part of the bin", "largest", 1), ("ties across the chunks of a long row", "abs", 1),
                           ("ties across the trips of a long row's walk", "abs", 1)):
        H1 = rows_csr([rows[name]], vdtype, seed=len(name))
        C, info = run_case(cfg, H1, k, MODES[by])
        assert info.ties_cut == ties and info.nnz_out == k, name
        if name == "all equal":                                                      # the first k positions
            assert np.array_equal(C.to_host().col_ids, H1.col_ids[:k])


# ---------------------------------------------------------------------------------------------------- 5: radix digits, special values
def digit_rows(k, vdtype):
    """rows of 200 entries: a group's row by default, an LDS row and a long row through the options"""
    rng = np.random.default_rng(41)
    u = utype(vdtype)
    size = u().itemsize
    digits = np.array([0, 0, 0] + list(range(1, 197)) + [255], dtype=u)              # bin 0 three times, bin 255 once
    rows = []
    for byte in range(size):                                                         # keys that differ in one byte only
        if byte == size - 1:
            base = u(0x0000123456789ABC) if size == 8 else u(0x00012345)             # (the exponent never fills: no NaN, no inf)
        else:
            base = bits(np.array([1.5], dtype=vdtype))[0] & ~(u(0xFF) << u(8 * byte))
        rows.append((base | (rng.permutation(digits) << u(8 * byte))).view(vdtype))
    n = 200
    rows.append(rng.permutation(np.arange(-100, 100)).astype(vdtype) / 8)            # both sides of the sign flip, a zero
    sub = (rng.permutation(n).astype(u) + u(1)) | np.where(rng.random(n) < 0.5, u(1) << u(8 * size - 1), u(0))
    rows.append(sub.view(vdtype))                                                    # subnormals of both signs
    inf = rng.standard_normal(n).astype(vdtype)
    m = min(k + 5, n)
    inf[rng.permutation(n)[:m]] = np.where(np.arange(m) % 2 == 0, np.inf, -np.inf)
    rows.append(inf)
    for nans in (k + 3, k, max(k - 2, 0)):                                           # more NaNs than k, exactly k, fewer
        v = bits((rng.standard_normal(n) * 100).astype(vdtype)).copy()
        at = rng.permutation(n)[:nans]
        v[at] = nan_bits(at, vdtype, at % 2 == 1)
        rows.append(v.view(vdtype))
    return rows


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_radix_digits_and_special_values(cfg, cls, vdtype):
    set_classes(cfg, cls)
    for k in (1, 100, 198):                                                          # the k-th key in bin 255, in the middle, in bin 0
        rows = digit_rows(k, vdtype)
        H = rows_csr(rows, vdtype)
        dA = sa.dCSR.from_host(H)
        for by, mode in MODES.items():
            C, info = run_case(cfg, H, k, mode, dA=dA)
            kept_nans = int(np.isnan(C.to_host().data).sum())
            assert info.nan_kept == kept_nans == sum(min(k, int(np.isnan(r).sum())) for r in rows), (k, by)


@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_input_order_duplicate_ids_and_positions(cfg, vdtype):
    # unsorted rows whose ids repeat: nothing is merged, the kept entries are a subsequence of the row
    rng = np.random.default_rng(51)
    lens = rng.integers(0, 400, size=300)
    H = host_csr(lens, 7, vdtype, seed=52)                                           # seven columns: every id many times in a row
    for mode in MODES.values():
        C, info = run_case(cfg, H, 9, mode)
        assert info.nnz_out == int(np.minimum(lens, 9).sum())


# ---------------------------------------------------------------------------------------------------- 6: views, stream, ownership
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
@pytest.mark.parametrize("cfg_none", [False, True], ids=["cfg", "no-cfg"])
def test_a_view_gives_the_rows_of_the_whole(cfg, cfg_none, vdtype):
    H = class_matrix(vdtype)
    dA = sa.dCSR.from_host(H)
    r0, r1 = int(np.nonzero(H.row_offsets % 2 == 1)[0][0]), H.rows - 3                # an odd first offset
    assert 0 < r0 < 50 and int(H.row_offsets[r0]) % 2 == 1
    V = dA.row_view(r0, r1)
    c = None if cfg_none else cfg
    for by, mode in MODES.items():
        rc, whole, winfo = call(c, dA, 6, mode)
        assert rc == OK
        check(whole, winfo, want_of(H, 6, mode), H.cols)
        view_h = sa.HostCSR(r1 - r0, H.cols, H.row_offsets[r0:r1 + 1], H.col_ids, H.data)
        want = want_of(view_h, 6, mode)
        rc, C, info = call(c, V, 6, mode)
        assert rc == OK
        check(C, info, want, H.cols)
        W, P = whole.to_host(), C.to_host()
        a, b = int(W.row_offsets[r0]), int(W.row_offsets[r1])
        assert np.array_equal(P.col_ids, W.col_ids[a:b]) and np.array_equal(bits(P.data), bits(W.data[a:b]))
        assert np.array_equal(P.row_offsets.astype(np.int64), W.row_offsets[r0:r1 + 1].astype(np.int64) - a)


def test_the_callers_stream_and_the_python_wrapper(cfg):
    H = class_matrix(np.float64)
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    val_t = torch.from_numpy(H.data).to(DEV)
    ro_t = torch.from_numpy(H.row_offsets.view(np.int32)).to(DEV)
    col_t = torch.from_numpy(H.col_ids.view(np.int32)).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big = torch.sort(torch.rand(1 << 23, device=DEV)).values                      # work in front of the values on the stream
        val2 = val_t + big[:1] * 0                                                    # (what it holds is read back below)
        dA = sa.dCSR.from_device(H.rows, H.cols, H.nnz, ro_t.data_ptr(), col_t.data_ptr(), val2.data_ptr(), keep=(ro_t, col_t, val2))
        C, info = sa.topk(dA, 5, by="abs", cfg=cfg, return_info=True)                 # no synchronise in between
    torch.cuda.synchronize()
    cfg.set_stream(None)
    H2 = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, val2.cpu().numpy())
    check(C, info, want_of(H2, 5, MODES["abs"]), H.cols)
    out = sa.topk(dA, 5, by="smallest", cfg=cfg, out=C)                               # out= takes the result, no info
    assert out is C
    rc, C2, info2 = call(cfg, dA, 5, MODES["smallest"])
    check(out, info2, want_of(H2, 5, MODES["smallest"]), H.cols)
    assert isinstance(sa.topk(dA, 2, cfg=None), sa.dCSR)


def test_c_keeps_the_buffers_whose_size_stays(cfg):
    H = class_matrix(np.float64)
    dA = sa.dCSR.from_host(H)
    C, info = run_case(cfg, H, 6, MODES["largest"], dA=dA)
    p0 = struct_of(C)[3:]
    rc, _, info1 = call(cfg, dA, 6, MODES["abs"], C=C)                                # same rows, same nnz: all three stay
    assert rc == OK and info1.nnz_out == info.nnz_out and struct_of(C)[3:] == p0
    check(C, info1, want_of(H, 6, MODES["abs"]), H.cols)
    rc, _, info2 = call(cfg, dA, 9, MODES["abs"], C=C)                                # another nnz: data and col_ids are new
    p2 = struct_of(C)[3:]
    assert rc == OK and info2.nnz_out != info.nnz_out and p2[2] == p0[2] and p2[0] != p0[0] and p2[1] != p0[1]
    check(C, info2, want_of(H, 9, MODES["abs"]), H.cols)
    V = dA.row_view(0, 100)                                                         # another number of rows: row_offsets is new
    rc, _, info3 = call(cfg, V, 9, MODES["abs"], C=C)
    assert rc == OK and struct_of(C)[5] != p2[2] and C.rows == 100


def test_guard_zones_stay_clean(cfg):
    cfg.set_option("guard_bytes", 4096)
    try:
        H, _ = edge_matrix(np.float64)
        dA = sa.dCSR.from_host(H)
        C, _ = run_case(cfg, H, 3, MODES["abs"], dA=dA)
        set_classes(cfg, "long")
        C2, _ = run_case(cfg, H, 40, MODES["smallest"], dA=dA)
        del C, C2
    finally:
        cfg.set_option("guard_bytes", 0)


# ---------------------------------------------------------------------------------------------------- 7: refusals on the device
@pytest.mark.parametrize("vdtype", VDTYPES, ids=VIDS)
def test_hostile_input_is_refused_with_nothing_written(cfg, vdtype):
    rng = np.random.default_rng(61)
    lens = np.concatenate([rng.integers(1, 9, size=400), [2 * LDS + 5], rng.integers(1, 9, size=99)])
    H = host_csr(lens, 800, vdtype, seed=62)
    k, mode = 5, MODES["abs"]
    want = want_of(H, k, mode)
    nnz_out = len(want[1])
    C, frames = framed_c(H.rows, 800, nnz_out, vdtype)                               # rows and nnz match: every buffer would be reused
    before = struct_of(C)

    def refused(A, what, k=k):
        rc, _, info = call(cfg, A, k, mode, C=C)
        assert rc == ERR_INVALID, what
        assert struct_of(C) == before and list(vars(info).values()) == [0] * 8, what
        assert untouched(*frames), what

    hub = 400
    for what, change in (("an offset that descends", lambda ro: ro.__setitem__(17, ro[18] + 1)),
                         ("a descent in front of the long row", lambda ro: ro.__setitem__(hub, ro[hub + 1] + 1)),
                         ("an offset past nnz", lambda ro: ro.__setitem__(slice(401, None), H.nnz + 1)),
                         ("an offset near 2^32", lambda ro: ro.__setitem__(slice(401, None), 0xFFFFFFF0)),
                         ("a last offset short of nnz", lambda ro: ro.__setitem__(H.rows, H.nnz - 1))):
        ro = H.row_offsets.copy()
        change(ro)
        refused(device_matrix(H, ro=ro), what)
    refused(device_matrix(H, nnz=H.nnz - 1), "the declared nnz is what the rows hold")
    short = int(np.nonzero(lens <= k)[0][3])                                         # a row that is kept whole: only the check reads its ids
    for row, at_in_row in ((short, 0), (hub, 0), (hub, LDS + 7), (hub, 2 * LDS + 4), (H.rows - 1, -1)):
        a, b = int(H.row_offsets[row]), int(H.row_offsets[row + 1])
        at = a + at_in_row if at_in_row >= 0 else b - 1
        for bad in (H.cols, 0xFFFFFFFF):
            col = H.col_ids.copy()
            col[at] = bad
            refused(device_matrix(H, col=col), (row, at, bad))
            refused(device_matrix(H, col=col), (row, at, bad, "k = 0"), k=0)          # C must be a sound matrix whatever is kept
    # ... and the clean call fills exactly the three arrays
    rc, _, info = call(cfg, device_matrix(H), k, mode, C=C)
    assert rc == OK and struct_of(C) == before and vars(info) == want[3]
    vs = np.dtype(vdtype).itemsize
    assert np.array_equal(framed(frames[2], (H.rows + 1) * 4, np.uint32), want[0])
    assert np.array_equal(framed(frames[1], nnz_out * 4, np.uint32), want[1])
    assert np.array_equal(framed(frames[0], nnz_out * vs, want[2].dtype), want[2])
    # the arguments the host refuses, with a device behind them
    dA = device_matrix(H)
    for kw in (dict(mode=3), dict(mode=mode, reserved=1)):
        rc, _, info = call(cfg, dA, k, kw["mode"], C=C, reserved=kw.get("reserved", 0))
        assert rc == ERR_INVALID and struct_of(C) == before
    rc, _, _ = call(cfg, dA, k, mode, C=dA)                                          # C sharing its buffers with A
    assert rc == ERR_INVALID


# ---------------------------------------------------------------------------------------------------- 8: compositions
def scipy_graph(n, per_row, seed):
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=per_row / n, format="csr", random_state=rng, dtype=np.float64)
    S.data = rng.integers(1, 9, size=S.nnz).astype(np.float64) * np.where(rng.random(S.nnz) < 0.3, -1.0, 1.0)
    S.sort_indices()
    return S


def to_device(S):
    return sa.dCSR.from_host(sa.HostCSR(S.shape[0], S.shape[1], S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data.copy()))


def test_the_multiply_accepts_the_result_and_normalize_rows_follows(cfg):
    from oracle import pyoracle as po
    S = scipy_graph(1500, 20, seed=71)
    dA = to_device(S)
    C, info = sa.topk(dA, 6, by="abs", cfg=cfg, return_info=True)
    Hc = C.to_host()
    check(C, info, numpy_topk(S.indptr, S.indices, S.data, 6, MODES["abs"]), 1500)
    assert all(np.all(np.diff(Hc.col_ids[a:b].astype(np.int64)) > 0) for a, b in zip(Hc.row_offsets[:-1], Hc.row_offsets[1:]))   # canonical stays canonical
    out = sa.dCSR()
    sa.MultiplyspECK(C, dA, out, cfg, sa.Timings())                                   # speck_multiply_f64 takes it as it is
    R, _ = po.spgemm(po.HostCSR(1500, 1500, Hc.row_offsets, Hc.col_ids, Hc.data),
                     po.HostCSR(1500, 1500, S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data))
    P = out.to_host()
    assert np.array_equal(P.row_offsets, R.row_offsets) and np.array_equal(P.col_ids, R.col_ids) and np.array_equal(P.data, R.data)
    # the pruning of an MCL step: topk(by="abs"), then rows that sum to 1
    N, _ = sa.normalize_rows(C, cfg)
    Hn = N.to_host()
    ro = Hn.row_offsets.astype(np.int64)
    sums = np.add.reduceat(np.abs(Hn.data), ro[:-1][np.diff(ro) > 0])
    # (the values are small integers: a row's norm is exact; six quotients rounded once each, |q| <= 1, and five roundings
    #  of the sum here: 6 * 2^-53 at the most)
    assert np.array_equal(Hn.col_ids, Hc.col_ids) and np.allclose(sums, 1.0, rtol=0, atol=6 * 2.0 ** -53)


def test_the_caller_that_includes_topk_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_topk.cpp")
    out = str(tmp_path / "caller_topk")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "topk caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
