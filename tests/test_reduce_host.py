"""speck_reduce_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes Reduce.h only,
the argument checks that come before anything touches a device, and the loud failure where no device exists."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 1, 2, 5
SENTINEL = struct.unpack("<d", struct.pack("<Q", 0x7FF8DEADBEEF1234))[0]  # a NaN with a payload


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def test_header_library_and_table_agree_on_reduce():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_reduce_f64", "speck_reduce_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.POINTER(_lib.DCsr), ctypes.c_int, ctypes.c_void_p,
                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_lib.CReduceInfo)]


def test_info_struct_ops_and_tile_sizes_match_the_header():
    header = _header()
    body = re.search(r"typedef struct speck_reduce_info \{(.*?)\} speck_reduce_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [f for f, _ in fields] == [f[0] for f in _lib.CReduceInfo._fields_] == ["rows_empty", "rows_split", "tiles", "entries"]
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CReduceInfo._fields_)
    assert ctypes.sizeof(_lib.CReduceInfo) == 32
    ops = {k: int(v) for k, v in re.findall(r"SPECK_REDUCE_(SUM|ABS_SUM|SQ_SUM|MAX|MIN|ABS_MAX)\s*=\s*(\d+)", header)}
    assert ops == {"SUM": speck_amd.REDUCE_SUM, "ABS_SUM": speck_amd.REDUCE_ABS_SUM, "SQ_SUM": speck_amd.REDUCE_SQ_SUM,
                   "MAX": speck_amd.REDUCE_MAX, "MIN": speck_amd.REDUCE_MIN, "ABS_MAX": speck_amd.REDUCE_ABS_MAX}
    assert sorted(ops.values()) == list(range(6))
    assert {k.upper(): v for k, v in speck_amd.REDUCE_OPS.items()} == ops
    macros = {k: int(v) for k, v in re.findall(r"#define\s+SPECK_REDUCE_(TILE_ENTRIES|THREAD_ENTRIES|WAVE_ENTRIES)\s+(\d+)", header)}
    assert speck_amd.REDUCE_TILE_ENTRIES == macros["TILE_ENTRIES"] == 4096
    assert speck_amd.REDUCE_THREAD_ENTRIES == macros["THREAD_ENTRIES"]
    assert speck_amd.REDUCE_WAVE_ENTRIES == macros["WAVE_ENTRIES"] == 64 * macros["THREAD_ENTRIES"]


def test_caller_that_includes_reduce_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_reduce.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Reduce.h"]
    out = str(tmp_path / "caller_reduce")
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


def test_reduce_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    k1, k2 = (np.zeros(16, dtype=np.uint64) for _ in range(2))
    out = k2.ctypes.data
    total = ctypes.c_double(SENTINEL)
    sentinel_bytes = bytes(total)
    ref = ctypes.byref

    def call(fn, A, op=0, rows=out, tot=True):
        rc = fn(None, ref(A) if A is not None else None, op, rows, ref(total) if tot else None, None)
        assert bytes(total) == sentinel_bytes  # a refused call leaves the host total alone
        return rc

    for fn in (L.speck_reduce_f64, L.speck_reduce_f32):
        A = _mat(4, 6, 3, k1.ctypes.data)
        assert call(fn, None) == ERR_INVALID                                        # NULL A
        hollow = _mat(4, 6, 3, k1.ctypes.data)
        hollow.row_offsets = None
        assert call(fn, hollow) == ERR_INVALID                                      # NULL row_offsets
        hollow = _mat(4, 6, 3, k1.ctypes.data)
        hollow.data = None
        assert call(fn, hollow) == ERR_INVALID                                      # NULL data with nnz > 0
        for op in (-1, 6, 1 << 30):                                                 # unknown ops
            assert call(fn, A, op=op) == ERR_INVALID
        assert call(fn, A, rows=None, tot=False) == ERR_INVALID                     # both outputs NULL
        for field in ("data", "col_ids", "row_offsets"):                            # the output is one of A's buffers
            alias = _mat(4, 6, 3, k1.ctypes.data)
            setattr(alias, field, out)
            assert call(fn, alias) == ERR_INVALID, field
        assert call(fn, _mat((1 << 27) + 1, 6, 3, k1.ctypes.data)) == ERR_DIM_LIMIT
        assert call(fn, _mat(4, 6, 1 << 32, k1.ctypes.data)) == ERR_NNZ_OVERFLOW
    assert not k1.any() and not k2.any()


def test_reduce_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    k = np.zeros(16, dtype=np.uint64)
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=dtype)
        for kwargs in ({"rows": False}, {"op": "abs_max", "rows": False}, {"op": speck_amd.REDUCE_MIN, "total": False, "out_ptr": 4096}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.reduce(A, None, **kwargs)
            assert e.value.status == no_device


def test_an_unknown_op_name_is_refused_in_python():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    for op in ("mean", "SUM", "", 6, -1):
        with pytest.raises(ValueError):
            speck_amd.reduce(A, None, op=op)
