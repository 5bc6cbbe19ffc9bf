"""speck_select_* without a GPU: the declaration, the export, the ctypes mirrors, a C++ caller that includes Select.h only,
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
ERR_INVALID, ERR_DIM_LIMIT = 1, 2
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
C_TYPES = {"uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _struct_fields(header, name):
    """[(field, C type)] of a struct of the header, in declaration order (one type, several names per line allowed)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+speck_dcsr\s*\*|[a-z0-9_]+)\s*(.*)", decl)
        ctype = re.sub(r"\s+", " ", m.group(1))
        out += [(n.strip(), ctype) for n in m.group(2).split(",")]
    return out


def test_header_library_and_table_agree_on_select():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_select_f64", "speck_select_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()


def test_structs_flags_and_tile_sizes_match_the_header():
    header = _header()
    # the two structs: field order and types as the header gives them, sizes as a C compiler lays them out
    fields = _struct_fields(header, "speck_select_params")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSelectParams._fields_]
    for (name, ctype), (_, mirror) in zip(fields, _lib.CSelectParams._fields_):
        assert mirror is (ctypes.POINTER(_lib.DCsr) if "speck_dcsr" in ctype else C_TYPES[ctype]), name
    assert ctypes.sizeof(_lib.CSelectParams) == 48
    fields = _struct_fields(header, "speck_select_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSelectInfo._fields_]
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CSelectInfo._fields_)
    assert ctypes.sizeof(_lib.CSelectInfo) == 32
    # the flags
    for name in ("BAND", "ABS", "PATTERN", "NOT_BAND", "NOT_ABS", "NOT_PATTERN"):
        m = re.search(r"SPECK_SELECT_%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(speck_amd, "SELECT_" + name), name
    assert [speck_amd.SELECT_NOT_BAND, speck_amd.SELECT_NOT_ABS, speck_amd.SELECT_NOT_PATTERN] == \
        [16 * b for b in (speck_amd.SELECT_BAND, speck_amd.SELECT_ABS, speck_amd.SELECT_PATTERN)]
    # the tile sizes of the marking pass are public constants, mirrored in the Python layer
    macros = {k: int(v) for k, v in re.findall(r"#define\s+SPECK_SELECT_(TILE_ROWS_LONG|TILE_ROWS_SHORT|LONG_ROW_AVG)\s+(\d+)", header)}
    assert speck_amd.SELECT_TILE_ROWS == (macros["TILE_ROWS_LONG"], macros["TILE_ROWS_SHORT"])
    assert speck_amd.SELECT_LONG_ROW_AVG == macros["LONG_ROW_AVG"]


def test_caller_that_includes_select_h_only_links(tmp_path):
    out = str(tmp_path / "caller_select")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "caller_select.cpp"),
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _params(flags=0, lo=INT64_MIN, hi=INT64_MAX, t=0.0, pattern=None, row_base=0):
    p = _lib.CSelectParams()
    p.flags, p.band_lo, p.band_hi, p.abs_threshold, p.row_base = flags, lo, hi, t, row_base
    if pattern is not None:
        p.pattern = ctypes.pointer(pattern)
    return p


def test_select_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    k1, k2, k3 = (np.zeros(16, dtype=np.uint64) for _ in range(3))
    ref = ctypes.byref
    BAND, ABS, PATTERN = speck_amd.SELECT_BAND, speck_amd.SELECT_ABS, speck_amd.SELECT_PATTERN
    NOT_BAND, NOT_ABS, NOT_PATTERN = speck_amd.SELECT_NOT_BAND, speck_amd.SELECT_NOT_ABS, speck_amd.SELECT_NOT_PATTERN

    def call(A, p, C, fn=L.speck_select_f64):
        return fn(None, ref(A) if A is not None else None, ref(p) if p is not None else None,
                  ref(C) if C is not None else None, None)

    A, M = _mat(4, 6, 3, k1.ctypes.data), _mat(4, 6, 3, k2.ctypes.data)
    C = _lib.DCsr()
    ok = _params(BAND, -1, 1)
    assert call(None, ok, C) == ERR_INVALID and call(A, None, C) == ERR_INVALID and call(A, ok, None) == ERR_INVALID
    for flags in (8, 128, 1 << 31, BAND | 256):                                                  # unknown flag
        assert call(A, _params(flags), C) == ERR_INVALID
    for flags in (NOT_BAND, NOT_ABS, NOT_PATTERN, BAND | NOT_ABS, ABS | NOT_PATTERN, BAND | ABS | NOT_PATTERN):
        assert call(A, _params(flags, pattern=M), C) == ERR_INVALID                              # NOT_x without x
    assert call(A, _params(BAND, 1, 0), C) == ERR_INVALID                                        # band_lo > band_hi
    assert call(A, _params(BAND | NOT_BAND, INT64_MAX, INT64_MIN), C) == ERR_INVALID
    for t in (float("nan"), -1.0, -float("inf"), -5e-324):                                       # threshold NaN / negative
        assert call(A, _params(ABS, t=t), C) == ERR_INVALID
        assert call(A, _params(ABS | NOT_ABS, t=t), C, fn=L.speck_select_f32) == ERR_INVALID
    assert call(A, _params(PATTERN), C) == ERR_INVALID                                           # PATTERN without a pattern
    assert call(A, _params(PATTERN, pattern=_mat(3, 6, 3, k2.ctypes.data)), C) == ERR_INVALID    # ... of another shape
    assert call(A, _params(PATTERN | NOT_PATTERN, pattern=_mat(4, 5, 3, k2.ctypes.data)), C) == ERR_INVALID
    hollow = _mat(4, 6, 3, k1.ctypes.data)
    hollow.data = None
    assert call(hollow, ok, C) == ERR_INVALID                                                    # entries without values
    hollow = _mat(4, 6, 3, k2.ctypes.data)
    hollow.col_ids = None
    assert call(A, _params(PATTERN, pattern=hollow), C) == ERR_INVALID                           # a pattern without columns
    for other, p in ((A, ok), (M, _params(PATTERN, pattern=M))):                                 # C shares a buffer
        for field in ("data", "col_ids", "row_offsets"):
            alias = _mat(4, 6, 3, k3.ctypes.data)
            setattr(alias, field, getattr(other, field))
            assert call(A, p, alias) == ERR_INVALID
            assert (alias.rows, alias.cols, alias.nnz, getattr(alias, field)) == (4, 6, 3, getattr(other, field))
    big = (1 << 27) + 1
    assert call(_mat(big, 6, 3, k1.ctypes.data), ok, C) == ERR_DIM_LIMIT                         # dimensions over 2^27
    assert call(_mat(4, big, 3, k1.ctypes.data), ok, C, fn=L.speck_select_f32) == ERR_DIM_LIMIT
    assert call(_mat(big, 6, 3, k1.ctypes.data), _params(PATTERN, pattern=_mat(big, 6, 3, k2.ctypes.data)), C) == ERR_DIM_LIMIT
    assert bytes(C) == bytes(_lib.DCsr())                                                        # C never changed


def test_python_layer_refuses_an_unknown_predicate_name():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(ValueError):
        speck_amd.select(A, None, band=(0, 0), negate=("bend",))
    with pytest.raises(speck_amd.SpeckError) as e:                     # NOT_ABS without ABS: the library's answer
        speck_amd.select(A, None, band=(0, 0), negate="abs")
    assert e.value.status == ERR_INVALID


def test_select_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    keep = [np.zeros(16, dtype=np.uint64) for _ in range(2)]
    A, M = (speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data) for k in keep)
    for kwargs in ({}, {"band": (None, -1)}, {"abs_gt": 0.0}, {"pattern": M, "negate": ("pattern",)}):
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.select(A, None, **kwargs)
        assert e.value.status == no_device
    for fn in (speck_amd.tril, speck_amd.triu):
        with pytest.raises(speck_amd.SpeckError) as e:
            fn(A, None, k=-1)
        assert e.value.status == no_device
