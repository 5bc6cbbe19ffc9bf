"""speck_topk_* without a GPU: the declarations, the exports, the ctypes mirrors and the Python info class, a C++ caller that
includes TopK.h only, the contract as numpy (numpy_topk: what tests/test_gpu_topk.py compares the device with, byte for
byte) against a brute-force count of beaters, the argument checks that come before anything touches a device, the Python
wrapper's refusals, and the loud failure where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 0, 1, 2, 5
INFO_FIELDS = ["rows", "rows_cut", "entries_in", "nnz_out", "dropped", "max_row_entries", "ties_cut", "nan_kept"]
LARGEST, SMALLEST, ABS = 0, 1, 2
MODES = {"largest": LARGEST, "smallest": SMALLEST, "abs": ABS}


# ---------------------------------------------------------------------------------------------------- the contract
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def keys_of(val, mode):
    """(key, isnan): the key of every value, widened to double -- v, -v or |v|; 0 where the value is a NaN; -0.0 as +0.0"""
    v = np.asarray(val).astype(np.float64)
    isnan = np.isnan(v)
    key = v if mode == LARGEST else -v if mode == SMALLEST else np.abs(v)
    return np.where(isnan, 0.0, key) + 0.0, isnan


def numpy_topk(ro, col, val, k, mode):
    """The k best entries of every row as the header states it: (row_offsets, col_ids, the values' bits, info).  ro may be a
    view's absolute offsets.  Per row: order = np.lexsort((pos, -key, ~isnan)); kept = np.sort(order[:k]) -- here for all
    rows at once, the row as the first sort key."""
    ro = np.asarray(ro, dtype=np.int64)
    k = min(int(k), 1 << 32)                              # (a row holds fewer than 2^32 entries: such a k cuts none)
    rows, base = len(ro) - 1, int(ro[0]) if len(ro) else 0
    lens = np.diff(ro)
    n = int(lens.sum())
    key, isnan = keys_of(np.asarray(val)[base:base + n], mode)
    start = np.repeat(ro[:-1] - base, lens)
    row = np.repeat(np.arange(rows), lens)
    pos = np.arange(n, dtype=np.int64) - start
    order = np.lexsort((pos, -key, ~isnan, row))
    rank = np.arange(n, dtype=np.int64) - start          # (the sorted entries of a row take the row's places)
    kept = np.sort(order[rank < k])
    new_lens = np.minimum(lens, k)
    new_ro = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.uint32)
    # the rows in which the strongest dropped entry has the key of the weakest kept one
    first_dropped = np.nonzero(rank == k)[0] if k >= 1 else np.zeros(0, dtype=np.int64)
    a, b = order[first_dropped], order[first_dropped - 1]
    ties = int(((isnan[a] == isnan[b]) & (key[a] == key[b])).sum())
    info = dict(rows=rows, rows_cut=int((lens > k).sum()), entries_in=n, nnz_out=len(kept), dropped=n - len(kept),
                max_row_entries=int(new_lens.max()) if rows else 0, ties_cut=ties, nan_kept=int(isnan[kept].sum()))
    return new_ro, np.asarray(col)[base:base + n][kept].astype(np.uint32), bits(np.asarray(val)[base:base + n])[kept], info


def brute_topk(ro, val, k, mode):
    """entry by entry: kept iff fewer than k entries of its row beat it.  (kept positions, rows in which the tie rule decided)"""
    kept, ties = [], 0
    for r in range(len(ro) - 1):
        a, b = int(ro[r]), int(ro[r + 1])
        key, isnan = keys_of(val[a:b], mode)
        rank = [(2, 0.0) if isnan[p] else (1, float(key[p])) for p in range(b - a)]      # a NaN above every number
        row_kept = []
        for p in range(b - a):
            beaters = sum(1 for q in range(b - a) if rank[q] > rank[p] or (rank[q] == rank[p] and q < p))
            if beaters < k:
                row_kept.append(p)
        kept_keys = {rank[p] for p in row_kept}
        ties += any(rank[p] in kept_keys for p in range(b - a) if p not in row_kept)
        kept += [a + p for p in row_kept]
    return np.asarray(kept, dtype=np.int64), ties


SPECIALS = {"nan": [np.nan, -np.nan], "zero": [0.0, -0.0], "inf": [np.inf, -np.inf]}


@pytest.mark.parametrize("special", list(SPECIALS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("vdtype", [np.float64, np.float32])
def test_numpy_statement_is_the_count_of_beaters(vdtype, mode, special):
    rng = np.random.default_rng(len(mode) * 7 + len(special))
    lens = np.concatenate([np.arange(41), rng.integers(0, 41, size=60)])
    ro = np.concatenate([[0], np.cumsum(lens)])
    n = int(ro[-1])
    pool = np.array([-3.0, -1.0, 1.0, 1.0, 2.0, 3.0, 3.0] + SPECIALS[special] * 2)       # few values: heavy ties
    val = pool[rng.integers(0, len(pool), size=n)].astype(vdtype)
    col = rng.integers(0, 50, size=n).astype(np.uint32)
    for k in (0, 1, 2, 5, 13, 40, 41, 1 << 40, (1 << 64) - 1):
        new_ro, ci, vb, info = numpy_topk(ro, col, val, k, MODES[mode])
        kept, ties = brute_topk(ro, val, k, MODES[mode])
        assert np.array_equal(ci, col[kept]) and np.array_equal(vb, bits(val)[kept]), k
        new_lens = np.minimum(lens, min(k, 41))
        assert np.array_equal(np.diff(new_ro.astype(np.int64)), new_lens)
        assert info == dict(rows=len(lens), rows_cut=int((lens > k).sum()), entries_in=n, nnz_out=len(kept), dropped=n - len(kept),
                            max_row_entries=int(new_lens.max()), ties_cut=ties, nan_kept=int(np.isnan(val[kept]).sum())), k


def test_numpy_statement_on_a_view_and_by_hand():
    # a view with an odd first offset; row 0: 1 -5 3 3, row 1: empty, row 2: nan -0.0 0.0 -7
    ro = np.array([3, 7, 7, 11], dtype=np.uint32)
    col = np.arange(11, dtype=np.uint32)[::-1].copy()
    val = np.array([9, 9, 9, 1, -5, 3, 3, np.nan, -0.0, 0.0, -7])
    got = numpy_topk(ro, col, val, 2, LARGEST)
    assert got[0].tolist() == [0, 2, 2, 4] and got[1].tolist() == [5, 4, 3, 2]          # 3 3 | nan -0.0 (before its equal 0.0)
    assert got[3] == dict(rows=3, rows_cut=2, entries_in=8, nnz_out=4, dropped=4, max_row_entries=2, ties_cut=1, nan_kept=1)
    got = numpy_topk(ro, col, val, 2, ABS)
    assert got[1].tolist() == [6, 5, 3, 0] and got[3]["ties_cut"] == 1                  # -5 and the first 3 | nan -7
    got = numpy_topk(ro, col, val, 1, SMALLEST)
    assert got[1].tolist() == [6, 3] and got[3]["nan_kept"] == 1 and got[3]["ties_cut"] == 0
    assert np.array_equal(got[2], bits(val)[[4, 7]])


# ---------------------------------------------------------------------------------------------------- declarations
def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _kinds(header, name):
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"((?:const )?\w+)\s*(.*)$", decl, re.S).groups()
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_header_library_and_table_agree():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P = ctypes.POINTER
    for name in ("speck_topk_f64", "speck_topk_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == [ctypes.c_void_p, P(_lib.DCsr), P(_lib.CTopKParams), P(_lib.DCsr), P(_lib.CTopKInfo)]
        assert _kinds(header, name) == ["speck_config*", "constspeck_dcsr*", "constspeck_topk_params*", "speck_dcsr*", "speck_topk_info*"]


def test_structs_hold_exactly_the_listed_fields():
    header = _header()
    fields = _struct_fields(header, "speck_topk_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CTopKInfo._fields_] == INFO_FIELDS
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CTopKInfo._fields_)
    assert ctypes.sizeof(_lib.CTopKInfo) == 8 * len(INFO_FIELDS)
    assert [getattr(_lib.CTopKInfo, f).offset for f in INFO_FIELDS] == [8 * i for i in range(len(INFO_FIELDS))]
    fields = _struct_fields(header, "speck_topk_params")
    want = [("k", "uint64_t"), ("mode", "uint32_t"), ("reserved", "uint32_t")]
    assert fields == want
    mirror = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    assert _lib.CTopKParams._fields_ == [(n, mirror[t]) for n, t in want]
    assert ctypes.sizeof(_lib.CTopKParams) == 16
    assert [getattr(_lib.CTopKParams, f).offset for f, _ in want] == [0, 8, 12]


def test_defines_are_the_python_constants_and_what_the_kernels_use():
    header = _header()
    assert int(re.search(r"#define SPECK_TOPK_GROUP_MAX (\d+)", header).group(1)) == speck_amd.TOPK_GROUP_MAX
    assert int(re.search(r"#define SPECK_TOPK_LDS_MAX (\d+)", header).group(1)) == speck_amd.TOPK_LDS_MAX
    assert speck_amd.TOPK_GROUP_MAX % 8 == 0 and speck_amd.TOPK_GROUP_MAX < speck_amd.TOPK_LDS_MAX
    enum = re.search(r"enum \{ SPECK_TOPK_LARGEST = (\d), SPECK_TOPK_SMALLEST = (\d), SPECK_TOPK_LARGEST_ABS = (\d) \};", header).groups()
    assert tuple(int(x) for x in enum) == (speck_amd.TOPK_LARGEST, speck_amd.TOPK_SMALLEST, speck_amd.TOPK_LARGEST_ABS) == (0, 1, 2)
    assert speck_amd.TOPK_MODES == MODES
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "topk.hip")).read()
    assert "kGroupMax = SPECK_TOPK_GROUP_MAX, kLdsMax = SPECK_TOPK_LDS_MAX" in source
    scratch = open(os.path.join(ROOT, "speck_amd", "csrc", "topk.hpp")).read()
    assert "group_max = SPECK_TOPK_GROUP_MAX" in scratch and "lds_max = SPECK_TOPK_LDS_MAX" in scratch
    options = open(os.path.join(ROOT, "speck_amd", "csrc", "pipeline.hip")).read()
    for name, define in (("topk_group_max", "SPECK_TOPK_GROUP_MAX"), ("topk_lds_max", "SPECK_TOPK_LDS_MAX")):
        assert re.search(r'n == "%s"\) c->topk\.\w+ = \(u32\)std::min<int64_t>\(std::max<int64_t>\(value, 0\), %s\);' % (name, define), options)
    assert options.count("c->topk.release();") == 2


def test_the_header_names_what_is_not_built():
    block = re.search(r"/\* ---- per-row top-k.*?---- \*/", _header(), re.S).group(0)
    not_built = re.sub(r"\s*\*\s+", " ", block[block.index("Not built:"):])
    for what in ("per-row k from a device array", "threshold or cumulative-mass cut fused in", "threshold key returned as a vector",
                 "top-k per column", "in-place", "hub row split over several workgroups", "top-k fused behind speck_sddmm_"):
        assert what in not_built, what
    flat = re.sub(r"\s*\*\s+", " ", block)
    assert "np.lexsort((pos, -key, ~isnan))" in flat and "NaN ranks ABOVE every number" in flat
    assert "no floating-point atomic and no floating-point arithmetic at all" in flat


def test_info_class_wraps_its_c_struct():
    values = dict(zip(INFO_FIELDS, range(1, 9)))
    c = _lib.CTopKInfo()
    for field, v in values.items():
        setattr(c, field, v)
    cls = speck_amd.TopKInfo
    assert cls is speck_amd.api.TopKInfo and cls.__name__ == "TopKInfo" and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values and all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == "TopKInfo(rows=1, rows_cut=2, entries_in=3, nnz_out=4, dropped=5, max_row_entries=6, ties_cut=7, nan_kept=8)"


def test_caller_that_includes_topk_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_topk.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["TopK.h"]
    out = str(tmp_path / "caller_topk")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_atomics_run_on_integer_counts_only():
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "topk.hip")).read()
    code = re.sub(r"//[^\n]*", "", source)
    targets = re.findall(r"atomic\w+\(\s*&?\s*([^,]+),", code)
    # (nan_kept goes through row_tiles.hpp -- wave_counter_to_lds, lds_counter_to_status --, nnz_out through scan.hpp)
    assert targets and set(targets) <= {"st->max_row", "st->cnt[c]", "st->ties_cut", "s_hist[d0]", "s_hist[digit]"}, targets
    for word in ("float", "double"):                                                # declared u32 / unsigned long long, every one
        assert not re.search(r"%s\s+(s_hist|s_nan|s_ties)\b" % word, code)
    status = re.search(r"struct TopkStatus \{(.*?)\};", code, re.S).group(1)
    assert "float" not in status and "double" not in status
    # no floating-point arithmetic: values are read as bits, the keys are unsigned integers
    assert not re.search(r"\bfabs|\bisnan|\bfmax|\bfmin", code)


# ---------------------------------------------------------------------------------------------------- argument checks
def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _a(rows, cols, nnz, pa):
    A = _mat(rows, cols, nnz, pa)
    A.row_offsets, A.col_ids, A.data = pa, pa + 1024, pa + 2048
    return A


def _params(k, mode=LARGEST, reserved=0):
    p = _lib.CTopKParams()
    p.k, p.mode, p.reserved = k, mode, reserved
    return p


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_topk_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    ka, kc = (np.zeros(1024, dtype=np.uint64) for _ in range(2))
    pa, pc = ka.ctypes.data, kc.ctypes.data
    ref = ctypes.byref
    for fn in (L.speck_topk_f64, L.speck_topk_f32):
        def call(A, p, out=True, C=None):
            C = _mat(9, 9, 9, pc) if C is None else C
            before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
            info = _lib.CTopKInfo(*([7] * 8))
            rc = fn(None, ref(A) if A is not None else None, ref(p) if p is not None else None, ref(C) if out else None, ref(info))
            assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before       # the struct keeps its sentinel
            assert [getattr(info, f) for f in INFO_FIELDS] == [7] * 8                        # ... and so does *info
            return rc

        A = _a(4, 6, 3, pa)
        good = _params(2)
        assert call(None, good) == ERR_INVALID                                      # NULL A
        assert call(A, None) == ERR_INVALID                                         # NULL params
        assert call(A, good, out=False) == ERR_INVALID                              # NULL C
        for mode in (3, 4, 0xFFFFFFFF):
            assert call(A, _params(2, mode=mode)) == ERR_INVALID
        for reserved in (1, 0x80000000):
            assert call(A, _params(2, reserved=reserved)) == ERR_INVALID
        big = (1 << 27) + 1
        assert call(_a(big, 6, 3, pa), good) == ERR_DIM_LIMIT
        assert call(_a(4, big, 3, pa), good) == ERR_DIM_LIMIT
        assert call(_a(big, 6, 3, pa), _params(2, mode=3)) == ERR_INVALID           # the mode is asked first
        assert call(_a(4, 6, 1 << 32, pa), good) == ERR_NNZ_OVERFLOW
        assert call(_a(4, 6, 1 << 40, pa), _params(0)) == ERR_NNZ_OVERFLOW
        for field in ("row_offsets", "col_ids", "data"):                            # NULL buffers with a count
            hollow = _a(4, 6, 3, pa)
            setattr(hollow, field, None)
            assert call(hollow, good) == ERR_INVALID, field
        assert call(_a(0, 6, 3, pa), good) == ERR_INVALID                           # entries, but no row
        assert call(_a(4, 0, 3, pa), good) == ERR_INVALID                           # entries, but no column
        for field in ("row_offsets", "col_ids", "data"):                            # C sharing a buffer with A
            C = _mat(9, 9, 9, pc)
            setattr(C, field, getattr(A, field))
            assert call(A, good, C=C) == ERR_INVALID, field
    assert not ka.any() and not kc.any()


def test_without_a_gpu_it_fails_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    ka, kc = (np.zeros(1024, dtype=np.uint64) for _ in range(2))
    pa = ka.ctypes.data
    for fn in (L.speck_topk_f64, L.speck_topk_f32):
        for A, p in ((_a(4, 6, 3, pa), _params(2)), (_a(4, 6, 3, pa), _params(0, mode=ABS)), (_mat(0, 0, 0, None), _params(1 << 40)),
                     (_a(4, 6, 0, pa), _params(1, mode=SMALLEST))):
            for C in (_lib.DCsr(), _mat(9, 9, 9, kc.ctypes.data)):
                before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
                info = _lib.CTopKInfo(*([7] * 8))
                assert fn(None, ctypes.byref(A), ctypes.byref(p), ctypes.byref(C), ctypes.byref(info)) == no_device
                assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before
                assert [getattr(info, f) for f in INFO_FIELDS] == [0] * 8           # the arguments have passed: *info is zero
    dA = speck_amd.dCSR.from_device(4, 6, 3, pa, pa + 1024, pa + 2048)
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.topk(dA, 2, by="abs")
    assert e.value.status == no_device
    assert not ka.any() and not kc.any()


def test_python_refuses_a_wrong_k_or_mode_before_the_library_is_asked():
    A = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    for by in ("Largest", "magnitude", None, 2):
        with pytest.raises(ValueError, match="topk: by must be one of"):
            speck_amd.topk(A, 2, by=by)
    for k in (-1, 1.5, "3", None, True, 1 << 64):
        with pytest.raises(ValueError, match="topk: k must be an integer"):
            speck_amd.topk(A, k)
