"""speck_tplan_* and speck_spmm_t_* without a GPU: the declarations, the exports, the ctypes mirrors and the four Python info
classes, a C++ caller that includes SpMMT.h only, the argument checks that come before anything touches a device, the
Python wrapper's refusals, and the loud failure where no device exists."""
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


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _kinds(header, name):
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]


def test_header_library_and_table_agree():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P = ctypes.POINTER
    sigs = {
        "speck_tplan_create": ([ctypes.c_void_p, P(_lib.DCsr), P(ctypes.c_void_p), P(_lib.CTplanInfo)],
                               ["speck_config*", "constspeck_dcsr*", "speck_tplan**", "speck_tplan_info*"]),
        "speck_tplan_destroy": ([ctypes.c_void_p], ["speck_tplan*"]),
    }
    for name in ("speck_spmm_t_f64", "speck_spmm_t_f32"):
        sigs[name] = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, P(_lib.DCsr), ctypes.c_void_p, ctypes.c_uint64,
                       ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, P(_lib.CSpmmTInfo)],
                      ["speck_config*", "constspeck_tplan*", "double", "constspeck_dcsr*", "constdouble*", "uint64_t", "uint32_t",
                       "double", "double*", "uint64_t", "speck_spmm_t_info*"])
    for name, (args, kinds) in sigs.items():
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == args, name
        assert _kinds(header, name) == kinds, name
    assert re.search(r"typedef struct speck_tplan speck_tplan;", header)          # opaque


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("cname, mirror, want", [
    ("speck_tplan_info", _lib.CTplanInfo, ["rows", "cols", "nnz", "cols_empty", "max_col_entries", "bytes"]),
    ("speck_spmm_t_info", _lib.CSpmmTInfo, ["cols_empty", "cols_split", "tiles", "entries", "terms"]),
])
def test_info_structs_hold_exactly_the_listed_fields(cname, mirror, want):
    fields = _struct_fields(_header(), cname)
    assert [f for f, _ in fields] == [f[0] for f in mirror._fields_] == want
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in mirror._fields_)
    assert ctypes.sizeof(mirror) == 8 * len(want)


# (class name, the C struct, its fields filled with distinct small integers, the repr of the wrapped struct)
INFO_CASES = [
    ("TplanInfo", "CTplanInfo", dict(rows=1, cols=2, nnz=3, cols_empty=4, max_col_entries=5, bytes=6),
     "TplanInfo(rows=1, cols=2, nnz=3, cols_empty=4, max_col_entries=5, bytes=6)"),
    ("SpmmTInfo", "CSpmmTInfo", dict(cols_empty=1, cols_split=2, tiles=3, entries=4, terms=5),
     "SpmmTInfo(cols_empty=1, cols_split=2, tiles=3, entries=4, terms=5)"),
]


@pytest.mark.parametrize("name, cname, values, text", INFO_CASES, ids=[c[0] for c in INFO_CASES])
def test_info_class_wraps_its_c_struct(name, cname, values, text):
    cstruct = getattr(_lib, cname)
    assert cstruct.__name__ == cname and issubclass(cstruct, ctypes.Structure)
    assert [f for f, _ in cstruct._fields_] == list(values)
    c = cstruct()
    for field, v in values.items():
        setattr(c, field, v)
    cls = getattr(speck_amd, name)
    assert cls is getattr(speck_amd.api, name) and cls.__name__ == name and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values
    assert all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == text


def test_caller_that_includes_spmmt_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_spmm_t.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["SpMMT.h"]
    out = str(tmp_path / "caller_spmm_t")
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


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_destroying_no_plan_is_ok():
    assert _lib.load().speck_tplan_destroy(None) == OK


def test_plan_creation_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    k = np.zeros(64, dtype=np.uint64)
    pa = k.ctypes.data
    ref = ctypes.byref

    def create(A, out=True):
        h = ctypes.c_void_p()
        info = _lib.CTplanInfo(7, 7, 7, 7, 7, 7)
        rc = L.speck_tplan_create(None, ref(A) if A is not None else None, ref(h) if out else None, ref(info))
        assert not h and [getattr(info, f) for f, _ in info._fields_] == [7] * 6      # *out and *info untouched
        return rc

    assert create(None) == ERR_INVALID                                              # NULL A
    assert create(_mat(4, 6, 3, pa), out=False) == ERR_INVALID                      # NULL out
    hollow = _mat(4, 6, 3, pa)
    hollow.row_offsets = None
    assert create(hollow) == ERR_INVALID                                            # NULL row_offsets with rows > 0
    hollow = _mat(4, 6, 3, pa)
    hollow.col_ids = None
    assert create(hollow) == ERR_INVALID                                            # NULL col_ids with nnz > 0
    assert create(_mat(0, 6, 3, pa)) == ERR_INVALID                                 # entries, but no row
    assert create(_mat(4, 0, 3, pa)) == ERR_INVALID                                 # entries, but no column
    assert create(_mat((1 << 27) + 1, 6, 3, pa)) == ERR_DIM_LIMIT
    assert create(_mat(4, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
    assert create(_mat(4, 6, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
    assert not k.any()


def test_plan_creation_without_a_gpu_fails_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    k = np.zeros(64, dtype=np.uint64)
    for A in (_mat(4, 6, 3, k.ctypes.data), _mat(0, 6, 0, None), _mat(4, 6, 0, k.ctypes.data)):
        valueless = _mat(A.rows, A.cols, A.nnz, A.row_offsets)
        valueless.data = None                                                       # (the values are not read)
        for M in (A, valueless):
            h = ctypes.c_void_p()
            assert L.speck_tplan_create(None, ctypes.byref(M), ctypes.byref(h), None) == no_device
            assert not h
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.transpose_plan(A)
    assert e.value.status == no_device
    with pytest.raises(speck_amd.SpeckError) as e:                                  # plan=None builds one first
        speck_amd.spmm_t(A, k.ctypes.data, None, k=3)
    assert e.value.status == no_device
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spmv_t(A, k.ctypes.data, None)
    assert e.value.status == no_device
    assert not k.any()


def test_spmm_t_refuses_a_null_plan_before_everything_else():
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    A = _mat(4, 6, 3, ka.ctypes.data)
    px = kb.ctypes.data
    py = px + 1024
    nan = float("nan")
    for fn in (L.speck_spmm_t_f64, L.speck_spmm_t_f32):
        info = _lib.CSpmmTInfo(7, 7, 7, 7, 7)
        for kwargs in (dict(), dict(alpha=nan), dict(k=2000), dict(ldx=1), dict(y=px), dict(k=0)):
            alpha, k, ldx, y = kwargs.get("alpha", 1.0), kwargs.get("k", 3), kwargs.get("ldx", 5), kwargs.get("y", py)
            assert fn(None, None, alpha, ctypes.byref(A), px, ldx, k, 0.0, y, 4, ctypes.byref(info)) == ERR_INVALID, kwargs
        assert fn(None, None, 1.0, None, px, 5, 3, 0.0, py, 4, None) == ERR_INVALID
        assert (info.cols_empty, info.cols_split, info.tiles, info.entries, info.terms) == (7, 7, 7, 7, 7)
    assert not ka.any() and not kb.any()


class Block:
    """what the wrapper asks of a tensor; a refused block is not asked for its address"""

    def __init__(self, shape, stride=None, dtype="float64"):
        self.shape, self.dtype = shape, dtype
        self._stride = stride if stride is not None else (shape[1], 1) if len(shape) == 2 else (1,)

    def data_ptr(self):
        raise AssertionError("a refused block is not asked for its address")

    def stride(self, d):
        return self._stride[d]


def test_python_refuses_wrong_blocks_and_wrong_plans_before_it_builds_a_plan():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    with pytest.raises(ValueError, match="spmm_t: beta"):
        speck_amd.spmm_t(A, k.ctypes.data, None, beta=1.0, k=2)                     # nothing to read
    with pytest.raises(ValueError, match="spmv_t: beta"):
        speck_amd.spmv_t(A, k.ctypes.data, None, beta=1.0)
    with pytest.raises(ValueError, match="spmm_t: X"):
        speck_amd.spmm_t(A, k.ctypes.data, None)                                    # an address without k
    for X in (Block((6, 3)),                                                        # cols rows: X has A.rows of them
              Block((4, 3), dtype="float32"),
              Block((4, 3), stride=(1, 4)),                                         # column-major
              Block((4, 3), stride=(2, 1)),                                         # rows closer than k
              Block((4,)),
              "a string", 1.5, None):
        with pytest.raises(ValueError, match="spmm_t: X"):
            speck_amd.spmm_t(A, X, None)
    for Y in (Block((4, 3)),                                                        # rows rows: Y has A.cols of them
              Block((6, 2)),                                                        # not X's k
              Block((6, 3), dtype="float32"),
              Block((6, 3), stride=(1, 6)),
              "a string", 2.5):
        with pytest.raises(ValueError, match="spmm_t: Y"):
            speck_amd.spmm_t(A, k.ctypes.data, None, Y=Y, k=3)
    with pytest.raises(ValueError, match="spmm_t: k"):
        speck_amd.spmm_t(A, k.ctypes.data, None, k=3, ldx=2)
    for plan in ("a string", 3, A):
        with pytest.raises(ValueError, match="spmm_t: plan"):
            speck_amd.spmm_t(A, k.ctypes.data, None, plan=plan, k=3)
    assert not k.any()
