"""speck_spmv_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes SpMV.h only,
the argument checks that come before anything touches a device, and the loud failure where no device exists."""
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


def test_header_library_and_table_agree_on_spmv():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_spmv_f64", "speck_spmv_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(_lib.DCsr), ctypes.c_void_p, ctypes.c_double,
                        ctypes.c_void_p, ctypes.POINTER(_lib.CSpmvInfo)]
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        kinds = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]
        assert kinds == ["speck_config*", "double", "constspeck_dcsr*", "constdouble*", "double", "double*", "speck_spmv_info*"]


def test_info_struct_and_tile_size_match_the_header():
    header = _header()
    body = re.search(r"typedef struct speck_spmv_info \{(.*?)\} speck_spmv_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSpmvInfo._fields_] == ["rows_empty", "rows_split", "tiles", "entries"]
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CSpmvInfo._fields_)
    assert ctypes.sizeof(_lib.CSpmvInfo) == ctypes.sizeof(_lib.CReduceInfo) == 32     # "as speck_reduce_info"
    tile = int(re.search(r"#define\s+SPECK_SPMV_TILE_ENTRIES\s+(\d+)", header).group(1))
    assert speck_amd.SPMV_TILE_ENTRIES == tile == speck_amd.REDUCE_TILE_ENTRIES == 4096


def test_caller_that_includes_spmv_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_spmv.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["SpMV.h"]
    out = str(tmp_path / "caller_spmv")
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


def test_spmv_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    ka, kx, ky = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    pa, px, py = ka.ctypes.data, kx.ctypes.data, ky.ctypes.data
    ref = ctypes.byref
    nan = float("nan")

    for fn in (L.speck_spmv_f64, L.speck_spmv_f32):
        info = _lib.CSpmvInfo(7, 7, 7, 7)

        def call(A, x=px, y=py, alpha=1.0, beta=0.0):
            return fn(None, alpha, ref(A) if A is not None else None, x, beta, y, ref(info))

        A = _mat(4, 6, 3, pa)
        assert call(None) == ERR_INVALID                                            # NULL A
        hollow = _mat(4, 6, 3, pa)
        hollow.row_offsets = None
        assert call(hollow) == ERR_INVALID                                          # NULL row_offsets
        assert call(A, y=None) == ERR_INVALID                                       # NULL y with rows > 0
        assert call(A, x=None) == ERR_INVALID                                       # NULL x with nnz > 0
        for field in ("data", "col_ids"):                                           # NULL data / col_ids with nnz > 0
            hollow = _mat(4, 6, 3, pa)
            setattr(hollow, field, None)
            assert call(hollow) == ERR_INVALID, field
        assert call(A, alpha=nan) == ERR_INVALID                                    # NaN coefficients
        assert call(A, beta=nan) == ERR_INVALID
        assert call(A, alpha=nan, beta=nan) == ERR_INVALID
        for field in ("data", "col_ids", "row_offsets"):                            # a vector is one of A's buffers
            for vec in (px, py):
                alias = _mat(4, 6, 3, pa)
                setattr(alias, field, vec)
                assert call(alias) == ERR_INVALID, field
        # x is [px, px + 6 doubles), y is [y, y + 4 doubles): every way the two can share a byte
        for y in (px, px + 8, px + 40, px - 8, px - 24):
            assert call(A, y=y) == ERR_INVALID, y - px
        assert call(_mat((1 << 27) + 1, 6, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(4, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(4, 6, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert call(_mat(4, 0, 3, pa)) == ERR_INVALID                               # entries, but no column: every id is >= cols
        assert call(_mat(0, 6, 3, pa)) == ERR_INVALID                               # entries, but no row
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == (7, 7, 7, 7)   # refused at the arguments
    assert not ka.any() and not kx.any() and not ky.any()


def test_vectors_that_touch_but_do_not_overlap_pass_the_argument_checks():
    """y right behind x and x right behind y are two ranges without a common byte: the call gets as far as the device"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    L = _lib.load()
    ka, kx = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    A = _mat(4, 6, 3, ka.ctypes.data)
    px = kx.ctypes.data + 64
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    for y in (px + 48, px - 32):
        assert L.speck_spmv_f64(None, 1.0, ctypes.byref(A), px, 0.0, y, None) == e.value.status
    assert not ka.any() and not kx.any()


def test_spmv_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    k, kx, ky = (np.zeros(16, dtype=np.uint64) for _ in range(3))
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=dtype)
        for kwargs in ({}, {"alpha": 2.0}, {"beta": 0.5, "y": ky.ctypes.data}, {"y": ky.ctypes.data}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.spmv(A, kx.ctypes.data, None, **kwargs)
            assert e.value.status == no_device, kwargs


def test_python_refuses_a_missing_y_with_beta_and_wrong_vectors():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(ValueError):
        speck_amd.spmv(A, k.ctypes.data, None, beta=1.0)                            # nothing to read

    class Vec:
        def __init__(self, n, dtype="float64", contiguous=True):
            self.n, self.dtype, self.contiguous = n, dtype, contiguous

        def data_ptr(self):
            raise AssertionError("a refused vector is not asked for its address")

        def numel(self):
            return self.n

        def is_contiguous(self):
            return self.contiguous

    for x in (Vec(5), Vec(6, "float32"), Vec(6, contiguous=False)):
        with pytest.raises(ValueError, match="spmv: x"):
            speck_amd.spmv(A, x, None)
    for y in (Vec(6), Vec(4, "float32"), Vec(4, contiguous=False)):
        with pytest.raises(ValueError, match="spmv: y"):
            speck_amd.spmv(A, k.ctypes.data, None, y=y)
