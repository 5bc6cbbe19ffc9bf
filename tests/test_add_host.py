"""speck_add_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes Add.h only, the
argument checks that come before anything touches a device, and the loud failure where no device exists."""
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


def test_header_library_and_table_agree_on_add():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_add_f64", "speck_add_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(_lib.DCsr), ctypes.c_double, ctypes.POINTER(_lib.DCsr),
                        ctypes.POINTER(_lib.DCsr), ctypes.c_int, ctypes.POINTER(_lib.CAddInfo)]


def test_info_struct_mode_and_tile_sizes_match_the_header():
    header = _header()
    body = re.search(r"typedef struct speck_add_info \{(.*?)\} speck_add_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [f for f, _ in fields] == [f[0] for f in _lib.CAddInfo._fields_] == ["only_a", "only_b", "both", "nnz_out"]
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CAddInfo._fields_)
    assert ctypes.sizeof(_lib.CAddInfo) == 32
    m = re.search(r"SPECK_ADD_UNION\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == speck_amd.ADD_UNION == 0
    macros = {k: int(v) for k, v in
              re.findall(r"#define\s+SPECK_ADD_(TILE_ROWS_LONG|TILE_ROWS_SHORT|LONG_ROW_AVG|TILE_ENTRIES)\s+(\d+)", header)}
    assert speck_amd.ADD_TILE_ROWS == (macros["TILE_ROWS_LONG"], macros["TILE_ROWS_SHORT"])
    assert speck_amd.ADD_LONG_ROW_AVG == macros["LONG_ROW_AVG"]
    assert speck_amd.ADD_TILE_ENTRIES == macros["TILE_ENTRIES"]


def test_caller_that_includes_add_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_add.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Add.h"]
    out = str(tmp_path / "caller_add")
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


def test_add_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    k1, k2, k3 = (np.zeros(16, dtype=np.uint64) for _ in range(3))
    ref = ctypes.byref
    FNS = (L.speck_add_f64, L.speck_add_f32)

    def call(A, B, C, flags=0, fn=L.speck_add_f64, alpha=1.0, beta=1.0):
        return fn(None, alpha, ref(A) if A is not None else None, beta, ref(B) if B is not None else None,
                  ref(C) if C is not None else None, flags, None)

    A, B = _mat(4, 6, 3, k1.ctypes.data), _mat(4, 6, 3, k2.ctypes.data)
    C = _lib.DCsr()
    for fn in FNS:
        assert call(None, B, C, fn=fn) == ERR_INVALID and call(A, None, C, fn=fn) == ERR_INVALID    # NULLs
        assert call(A, B, None, fn=fn) == ERR_INVALID
        for flags in (1, 2, -1, 1 << 30):                                                          # flags != 0
            assert call(A, B, C, flags=flags, fn=fn) == ERR_INVALID
        assert call(A, _mat(3, 6, 3, k2.ctypes.data), C, fn=fn) == ERR_INVALID                      # shape mismatch
        assert call(A, _mat(4, 5, 3, k2.ctypes.data), C, fn=fn) == ERR_INVALID
        assert call(_mat(5, 6, 3, k1.ctypes.data), B, C, fn=fn) == ERR_INVALID
        for field in ("data", "col_ids", "row_offsets"):                                           # hollow operands
            hollow = _mat(4, 6, 3, k1.ctypes.data)
            setattr(hollow, field, None)
            assert call(hollow, B, C, fn=fn) == ERR_INVALID, field
            assert call(A, hollow, C, fn=fn) == ERR_INVALID, field
        for other in (A, B):                                                                       # the six aliasings
            for field in ("data", "col_ids", "row_offsets"):
                alias = _mat(4, 6, 3, k3.ctypes.data)
                setattr(alias, field, getattr(other, field))
                before = bytes(alias)
                assert call(A, B, alias, fn=fn) == ERR_INVALID
                assert bytes(alias) == before
        big = (1 << 27) + 1                                                                        # dimensions over 2^27
        assert call(_mat(big, 6, 3, k1.ctypes.data), _mat(big, 6, 3, k2.ctypes.data), C, fn=fn) == ERR_DIM_LIMIT
        assert call(_mat(4, big, 3, k1.ctypes.data), _mat(4, big, 3, k2.ctypes.data), C, fn=fn) == ERR_DIM_LIMIT
        for na, nb in ((1 << 31, 1 << 31), ((1 << 32) - 1, 1), (1, (1 << 32) - 1), (1 << 32, 0), (0, 1 << 32)):
            assert na + nb >= 1 << 32                                                              # nnz(A) + nnz(B) == 2^32
            assert call(_mat(4, 6, na, k1.ctypes.data), _mat(4, 6, nb, k2.ctypes.data), C, fn=fn) == ERR_NNZ_OVERFLOW
    assert bytes(C) == bytes(_lib.DCsr())                                                          # C never changed


def test_add_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    keep = [np.zeros(16, dtype=np.uint64) for _ in range(2)]
    A, B = (speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data) for k in keep)
    for kwargs in ({}, {"alpha": 2.0, "beta": -1.0}, {"alpha": 0.0}):
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.add(A, B, None, **kwargs)
        assert e.value.status == no_device
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.add(A, A, None)
    assert e.value.status == no_device


def test_add_of_mixed_value_types_is_refused_in_python():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    B = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=np.float32)
    assert A.dtype != B.dtype
    with pytest.raises(ValueError):
        speck_amd.add(A, B, None)
    with pytest.raises(ValueError):
        speck_amd.add(B, A, None)
    R = speck_amd.dCSR.from_device(4, 5, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(ValueError):
        speck_amd.symmetrize(R, None)
