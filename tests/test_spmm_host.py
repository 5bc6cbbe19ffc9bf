"""speck_spmm_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes SpMM.h only,
the argument checks that come before anything touches a device -- the arithmetic of the two spans with padded rows among
them -- the Python wrapper's refusals, and the loud failure where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 1, 2, 5


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def test_header_library_and_table_agree_on_spmm():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_spmm_f64", "speck_spmm_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(_lib.DCsr), ctypes.c_void_p, ctypes.c_uint64,
                        ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(_lib.CSpmmInfo)]
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        kinds = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]
        assert kinds == ["speck_config*", "double", "constspeck_dcsr*", "constdouble*", "uint64_t", "uint32_t", "double",
                         "double*", "uint64_t", "speck_spmm_info*"]


def test_info_struct_and_the_limit_match_the_header():
    header = _header()
    body = re.search(r"typedef struct speck_spmm_info \{(.*?)\} speck_spmm_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSpmmInfo._fields_] == ["rows_empty", "rows_split", "tiles", "entries",
                                                                                 "terms"]
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CSpmmInfo._fields_)
    assert ctypes.sizeof(_lib.CSpmmInfo) == 40
    # (the first four are speck_spmv_info, field for field)
    assert _lib.CSpmmInfo._fields_[:4] == _lib.CSpmvInfo._fields_
    limit = int(re.search(r"#define\s+SPECK_SPMM_MAX_RHS\s+(\d+)", header).group(1))
    assert speck_amd.SPMM_MAX_RHS == limit == 1024
    block = int(re.search(r"#define\s+SPECK_SPMM_COLUMN_BLOCK\s+(\d+)", header).group(1))
    assert speck_amd.SPMM_COLUMN_BLOCK == block and block % 2 == 0          # (a 16-byte gather takes two columns)


def test_caller_that_includes_spmm_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_spmm.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["SpMM.h"]
    out = str(tmp_path / "caller_spmm")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


ROWS, COLS, K, LDX, LDY = 4, 6, 3, 5, 4
X_SPAN = 8 * ((COLS - 1) * LDX + K)        # bytes from d_X to the end of X(cols - 1, k - 1): 28 doubles
Y_SPAN = 8 * ((ROWS - 1) * LDY + K)        # ... and of Y: 15 doubles


def test_spmm_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    pa, px = ka.ctypes.data, kb.ctypes.data + 1024
    py = px + X_SPAN + 64
    ref = ctypes.byref
    nan = float("nan")

    for fn in (L.speck_spmm_f64, L.speck_spmm_f32):
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)

        def call(A, x=px, y=py, alpha=1.0, beta=0.0, k=K, ldx=LDX, ldy=LDY):
            return fn(None, alpha, ref(A) if A is not None else None, x, ldx, k, beta, y, ldy, ref(info))

        A = _mat(ROWS, COLS, 3, pa)
        assert call(None) == ERR_INVALID                                            # NULL A
        hollow = _mat(ROWS, COLS, 3, pa)
        hollow.row_offsets = None
        assert call(hollow) == ERR_INVALID                                          # NULL row_offsets
        assert call(A, y=None) == ERR_INVALID                                       # NULL Y with rows > 0
        assert call(A, x=None) == ERR_INVALID                                       # NULL X with nnz > 0
        for field in ("data", "col_ids"):                                           # NULL data / col_ids with nnz > 0
            hollow = _mat(ROWS, COLS, 3, pa)
            setattr(hollow, field, None)
            assert call(hollow) == ERR_INVALID, field
        assert call(A, alpha=nan) == ERR_INVALID                                    # NaN coefficients
        assert call(A, beta=nan) == ERR_INVALID
        assert call(A, alpha=nan, beta=nan) == ERR_INVALID
        for field in ("data", "col_ids", "row_offsets"):                            # a block is one of A's buffers
            for vec in (px, py):
                alias = _mat(ROWS, COLS, 3, pa)
                setattr(alias, field, vec)
                assert call(alias) == ERR_INVALID, field
        # the spans [px, px + X_SPAN) and [y, y + Y_SPAN), padding inside included: every way the two can share a byte
        for y in (px, px + 8, px + X_SPAN - 8, px - 8, px - Y_SPAN + 8, px + 8 * K, px + 8 * LDX):
            assert call(A, y=y) == ERR_INVALID, y - px
        # (with ld == k the last pair would be spmv-like disjoint ranges; here Y would sit in X's padding and rows)
        # the same two blocks one element closer than touching, counted with ld > k
        assert call(A, y=px + X_SPAN - 8) == ERR_INVALID and call(A, y=px - Y_SPAN + 8) == ERR_INVALID
        # two column slices of one tensor of 7 columns: they share no element, and interleave
        assert call(A, x=px, y=px + 8 * 3, k=3, ldx=7, ldy=7) == ERR_INVALID
        assert call(A, ldx=K - 1) == ERR_INVALID                                    # rows of X closer than k
        assert call(A, ldy=K - 1) == ERR_INVALID
        assert call(A, k=1, ldx=0) == ERR_INVALID
        assert call(A, k=speck_amd.SPMM_MAX_RHS + 1, ldx=2000, ldy=2000) == ERR_DIM_LIMIT
        assert call(A, ldx=(1 << 32) + 1) == ERR_DIM_LIMIT                          # (the spans would leave 64 bits)
        assert call(A, ldy=(1 << 32) + 1) == ERR_DIM_LIMIT
        assert call(_mat((1 << 27) + 1, COLS, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, COLS, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert call(_mat(ROWS, 0, 3, pa)) == ERR_INVALID                            # entries, but no column: every id is >= cols
        assert call(_mat(0, COLS, 3, pa)) == ERR_INVALID                            # entries, but no row
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms) == (7, 7, 7, 7, 7)   # refused at the arguments
    assert not ka.any() and not kb.any()


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_spans_that_touch_but_do_not_overlap_pass_the_argument_checks():
    """Y right behind X's span and X right behind Y's span are two ranges without a common byte, also where the rows are
    padded: the call gets as far as the device; info is zero by then"""
    no_device = _no_device_status()
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    A = _mat(ROWS, COLS, 3, ka.ctypes.data)
    px = kb.ctypes.data + 1024
    for y in (px + X_SPAN, px - Y_SPAN):
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)
        assert L.speck_spmm_f64(None, 1.0, ctypes.byref(A), px, LDX, K, 0.0, y, LDY, ctypes.byref(info)) == no_device
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms) == (0, 0, 0, 0, 0)
    # k == 0 and rows == 0 pass the checks too (and would return SPECK_OK with nothing written)
    assert L.speck_spmm_f64(None, 1.0, ctypes.byref(A), px, 0, 0, 0.0, px, 0, None) == no_device
    none = _mat(0, COLS, 0, ka.ctypes.data)
    assert L.speck_spmm_f32(None, 1.0, ctypes.byref(none), px, LDX, K, 0.0, px, LDY, None) == no_device
    assert not ka.any() and not kb.any()


def test_spmm_without_a_gpu_fails_loudly():
    no_device = _no_device_status()
    k, kx, ky = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=dtype)
        for kwargs in ({}, {"alpha": 2.0}, {"beta": 0.5, "Y": ky.ctypes.data}, {"Y": ky.ctypes.data, "ldx": 5, "ldy": 4}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.spmm(A, kx.ctypes.data, None, k=3, **kwargs)
            assert e.value.status == no_device, kwargs


class Block:
    """what the wrapper asks of a tensor; a refused block is not asked for its address"""

    def __init__(self, shape, stride=None, dtype="float64"):
        self.shape, self.dtype = shape, dtype
        self._stride = stride if stride is not None else (shape[1], 1) if len(shape) == 2 else (1,)

    def data_ptr(self):
        raise AssertionError("a refused block is not asked for its address")

    def stride(self, d):
        return self._stride[d]


def test_python_refuses_a_missing_y_with_beta_and_wrong_blocks():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(ValueError, match="spmm: beta"):
        speck_amd.spmm(A, k.ctypes.data, None, beta=1.0, k=2)                       # nothing to read
    with pytest.raises(ValueError, match="spmm: X"):
        speck_amd.spmm(A, k.ctypes.data, None)                                      # an address without k
    for X in (Block((5, 3)),                                                        # not cols rows
              Block((6, 3), dtype="float32"),
              Block((6, 3), stride=(1, 6)),                                         # column-major
              Block((6, 3), stride=(2, 1)),                                         # rows closer than k
              Block((6, 3), stride=(6, 2)),                                         # every other column
              Block((6,)),                                                          # a vector
              Block((6, 3, 1), stride=(3, 1, 1)),
              "a string", 1.5, None):
        with pytest.raises(ValueError, match="spmm: X"):
            speck_amd.spmm(A, X, None)
    with pytest.raises(ValueError, match="spmm: X"):
        speck_amd.spmm(A, Block((6, 3)), None, k=4)                                 # k says otherwise
    with pytest.raises(ValueError, match="spmm: X"):
        speck_amd.spmm(A, Block((6, 3), stride=(5, 1)), None, ldx=4)                # ldx says otherwise
    for Y in (Block((6, 3)),                                                        # not rows rows
              Block((4, 2)),                                                        # not X's k
              Block((4, 3), dtype="float32"),
              Block((4, 3), stride=(1, 4)),
              Block((4, 3), stride=(2, 1)),
              Block((4,)),
              "a string", 2.5):
        with pytest.raises(ValueError, match="spmm: Y"):
            speck_amd.spmm(A, k.ctypes.data, None, Y=Y, k=3)
    with pytest.raises(ValueError, match="spmm: k"):
        speck_amd.spmm(A, k.ctypes.data, None, k=3, ldx=2)
    with pytest.raises(ValueError, match="spmm: k"):
        speck_amd.spmm(A, k.ctypes.data, None, Y=k.ctypes.data, k=3, ldy=2)
    assert not k.any()
