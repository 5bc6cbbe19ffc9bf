"""speck_from_coo_* and speck_to_coo without a GPU: the declarations, the exports, the ctypes mirrors and the Python info
class, a C++ caller that includes FromCOO.h only, the argument checks that come before anything touches a device, the
Python wrappers' refusals, and the loud failure where no device exists."""
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
INFO_FIELDS = ["entries", "rows_empty", "max_row_entries", "sorted_input", "sort_passes"]


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
            for n in names.split(","):
                n = n.strip()
                fields.append((n.lstrip("* "), ctype + " *" if n.startswith("*") else ctype))
    return fields


def test_header_library_and_table_agree():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P = ctypes.POINTER
    sigs = {"speck_to_coo": ([ctypes.c_void_p, P(_lib.DCsr), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
                             ["speck_config*", "constspeck_dcsr*", "uint32_t", "uint64_t", "void*", "void*"])}
    for name in ("speck_from_coo_f64", "speck_from_coo_f32"):
        sigs[name] = ([ctypes.c_void_p, P(_lib.CDcoo), P(_lib.DCsr), P(_lib.CFromCooInfo)],
                      ["speck_config*", "constspeck_dcoo*", "speck_dcsr*", "speck_from_coo_info*"])
    for name, (args, kinds) in sigs.items():
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == args, name
        assert _kinds(header, name) == kinds, name


def test_structs_hold_exactly_the_listed_fields():
    header = _header()
    fields = _struct_fields(header, "speck_from_coo_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CFromCooInfo._fields_] == INFO_FIELDS
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CFromCooInfo._fields_)
    assert ctypes.sizeof(_lib.CFromCooInfo) == 8 * len(INFO_FIELDS)
    # speck_dcoo: the reference's COO<T> (rows, cols, nnz, data, row_ids, col_ids) and the width of the indices
    fields = _struct_fields(header, "speck_dcoo")
    want = [("rows", "uint64_t"), ("cols", "uint64_t"), ("nnz", "uint64_t"), ("data", "const void *"), ("row_ids", "const void *"),
            ("col_ids", "const void *"), ("index_bytes", "uint32_t")]
    assert fields == want
    mirror = {"uint64_t": ctypes.c_uint64, "const void *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}
    assert _lib.CDcoo._fields_ == [(n, mirror[t]) for n, t in want]
    assert ctypes.sizeof(_lib.CDcoo) == 56 and _lib.CDcoo.index_bytes.offset == 48
    assert int(re.search(r"#define SPECK_COO_TILE_ENTRIES (\d+)", header).group(1)) == speck_amd.COO_TILE_ENTRIES == 2048


def test_info_class_wraps_its_c_struct():
    values = dict(zip(INFO_FIELDS, range(1, 6)))
    c = _lib.CFromCooInfo()
    for field, v in values.items():
        setattr(c, field, v)
    cls = speck_amd.FromCooInfo
    assert cls is speck_amd.api.FromCooInfo and cls.__name__ == "FromCooInfo" and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values and all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == "FromCooInfo(entries=1, rows_empty=2, max_row_entries=3, sorted_input=4, sort_passes=5)"


def test_caller_that_includes_fromcoo_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_from_coo.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["FromCOO.h"]
    out = str(tmp_path / "caller_from_coo")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_there_is_one_radix_sort_in_the_tree():
    csrc = os.path.join(ROOT, "speck_amd", "csrc")
    defining = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".cpp"))
                and re.search(r"void radix_scatter_kernel\(", open(os.path.join(csrc, f)).read())]
    assert defining == ["extras.hip"]
    coo = open(os.path.join(csrc, "coo.hip")).read()
    assert '#include "radix_pairs.hpp"' in coo and len(re.findall(r"\bradix_sort_pairs\(", coo)) == 1
    assert not re.search(r"atomic\w*\((?![^;]*(rows_empty|max_row))", coo)          # counters only: nothing orders by an atomic


def _coo(rows, cols, nnz, buf, index_bytes=8):
    c = _lib.CDcoo()
    c.rows, c.cols, c.nnz, c.index_bytes = rows, cols, nnz, index_bytes
    c.data = c.row_ids = c.col_ids = buf
    return c


def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _same(m, rows, cols, nnz, buf):
    return (m.rows, m.cols, m.nnz, m.data, m.col_ids, m.row_offsets) == (rows, cols, nnz, buf, buf, buf)


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_from_coo_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    ka, kc = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    pa, pc = ka.ctypes.data, kc.ctypes.data
    ref = ctypes.byref
    for fn in (L.speck_from_coo_f64, L.speck_from_coo_f32):
        def call(coo, out=True, C=None):
            C = _mat(9, 9, 9, pc) if C is None else C
            before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
            info = _lib.CFromCooInfo(7, 7, 7, 7, 7)
            rc = fn(None, ref(coo) if coo is not None else None, ref(C) if out else None, ref(info))
            assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before       # the struct keeps its sentinel
            assert [getattr(info, f) for f in INFO_FIELDS] == [7] * 5                        # ... and so does *info
            return rc

        assert call(None) == ERR_INVALID                                            # NULL coo
        assert call(_coo(4, 6, 3, pa), out=False) == ERR_INVALID                    # NULL C
        for width in (0, 2, 16):
            assert call(_coo(4, 6, 3, pa, index_bytes=width)) == ERR_INVALID
        assert call(_coo((1 << 27) + 1, 6, 3, pa)) == ERR_DIM_LIMIT
        assert call(_coo(4, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
        assert call(_coo(4, 6, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        hollow = _coo(4, 6, 3, pa)
        hollow.row_ids = None
        assert call(hollow) == ERR_INVALID                                          # NULL row ids with nnz > 0
        hollow = _coo(4, 6, 3, pa)
        hollow.col_ids = None
        assert call(hollow) == ERR_INVALID
        assert call(_coo(0, 6, 3, pa)) == ERR_INVALID                               # entries, but no row
        assert call(_coo(4, 0, 3, pa)) == ERR_INVALID                               # entries, but no column
        # one of C's pointers inside an input array: its start, its middle, its last byte -- for each of the three
        for width in (4, 8):
            for field in ("data", "col_ids", "row_offsets"):
                for at in (0, 8, 3 * width - 1):
                    C = _mat(9, 9, 9, pc)
                    setattr(C, field, pa + at)
                    assert call(_coo(4, 6, 3, pa, index_bytes=width), C=C) == ERR_INVALID, (width, field, at)
    assert not ka.any() and not kc.any()


def test_to_coo_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    ka, ko = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    pa, po = ka.ctypes.data, ko.ctypes.data
    ref = ctypes.byref
    A = _mat(4, 6, 3, pa)
    A.row_offsets, A.col_ids, A.data = pa, pa + 64, pa + 128
    fn = L.speck_to_coo
    assert fn(None, None, 8, 0, po, po + 256) == ERR_INVALID                        # NULL A
    assert fn(None, ref(A), 8, 0, None, po + 256) == ERR_INVALID                    # NULL row output
    for width in (0, 2, 16):
        assert fn(None, ref(A), width, 0, po, po + 256) == ERR_INVALID
    big = _mat((1 << 27) + 1, 6, 3, pa)
    assert fn(None, ref(big), 8, 0, po, None) == ERR_DIM_LIMIT
    assert fn(None, ref(_mat(4, 6, 1 << 32, pa)), 8, 0, po, None) == ERR_NNZ_OVERFLOW
    hollow = _mat(4, 6, 3, pa)
    hollow.row_offsets = None
    assert fn(None, ref(hollow), 8, 0, po, None) == ERR_INVALID
    hollow = _mat(4, 6, 3, pa)
    hollow.col_ids = None
    assert fn(None, ref(hollow), 8, 0, po, po + 256) == ERR_INVALID                 # columns asked of a matrix without ids
    assert fn(None, ref(_mat(0, 6, 3, pa)), 8, 0, po, None) == ERR_INVALID          # entries, but no row
    # the last row index must fit the index type
    assert fn(None, ref(A), 4, (1 << 32) - 3, po, None) == ERR_INVALID              # 2^32 - 3 + 4 rows > 2^32
    assert fn(None, ref(A), 4, 1 << 40, po, None) == ERR_INVALID
    assert fn(None, ref(A), 8, (1 << 63) - 3, po, None) == ERR_INVALID
    assert fn(None, ref(A), 8, (1 << 64) - 1, po, None) == ERR_INVALID
    # aliasing: an output that is one of A's arrays or lies in its offsets, outputs that overlap
    for p in (A.row_offsets, A.col_ids, A.data, A.row_offsets + 4 * 4):
        assert fn(None, ref(A), 8, 0, p, None) == ERR_INVALID
        assert fn(None, ref(A), 8, 0, po, p) == ERR_INVALID
    assert fn(None, ref(A), 8, 0, po, po) == ERR_INVALID
    assert fn(None, ref(A), 8, 0, po, po + 23) == ERR_INVALID                       # 3 ids of 8 bytes: [po, po + 24)
    assert fn(None, ref(A), 4, 0, po + 11, po) == ERR_INVALID
    assert not ka.any() and not ko.any()


def test_without_a_gpu_both_fail_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    ka, kc, ko = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    for fn in (L.speck_from_coo_f64, L.speck_from_coo_f32):
        for coo in (_coo(4, 6, 3, ka.ctypes.data), _coo(4, 6, 3, ka.ctypes.data, index_bytes=4), _coo(0, 0, 0, None), _coo(5, 6, 0, None)):
            for C in (_lib.DCsr(), _mat(9, 9, 9, kc.ctypes.data)):
                before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
                assert fn(None, ctypes.byref(coo), ctypes.byref(C), None) == no_device
                assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before
    A = _mat(4, 6, 3, ka.ctypes.data)
    assert L.speck_to_coo(None, ctypes.byref(A), 8, 0, ko.ctypes.data, ko.ctypes.data + 256) == no_device
    assert L.speck_to_coo(None, ctypes.byref(_mat(0, 6, 0, None)), 4, 0, ko.ctypes.data, None) == no_device
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.from_coo(ka.ctypes.data, ka.ctypes.data + 64, None, (4, 6), None, nnz=3, index_bytes=8)
    assert e.value.status == no_device
    assert not ka.any() and not kc.any() and not ko.any()


class Block:
    """what the wrappers ask of a tensor; a refused block is not asked for its address"""

    def __init__(self, shape, stride=None, dtype="int64"):
        self.shape, self.dtype = shape, dtype
        self._stride = stride if stride is not None else (shape[1], 1) if len(shape) == 2 else (1,)

    def data_ptr(self):
        raise AssertionError("a refused block is not asked for its address")

    def stride(self, d):
        return self._stride[d]


def test_python_refuses_wrong_arrays_before_it_asks_for_an_address():
    ids, vals = Block((5,)), Block((5,), dtype="float64")
    for bad in (Block((5,), dtype="float64"), Block((5,), dtype="int16"), Block((5,), dtype="uint8"),   # wrong dtypes
                Block((5,), stride=(2,)),                                                                # not contiguous
                Block((5, 1)), "a string", 1.5, None):
        with pytest.raises(ValueError, match="from_coo: row"):
            speck_amd.from_coo(bad, ids, vals, (4, 6), None)
        with pytest.raises(ValueError, match="from_coo: col"):
            speck_amd.from_coo(ids, bad, vals, (4, 6), None)
    for bad in (Block((5,), dtype="int64"), Block((5,), dtype="float16"), Block((5,), dtype="float64", stride=(3,)), "a string"):
        with pytest.raises(ValueError, match="from_coo: val"):
            speck_amd.from_coo(ids, ids, bad, (4, 6), None)
    with pytest.raises(ValueError, match="from_coo: row holds 5 ids, col 4"):                            # lengths that differ
        speck_amd.from_coo(ids, Block((4,)), vals, (4, 6), None)
    with pytest.raises(ValueError, match="from_coo: val holds 6 values for 5 ids"):
        speck_amd.from_coo(ids, ids, Block((6,), dtype="float64"), (4, 6), None)
    with pytest.raises(ValueError, match="from_coo: row and col must hold ids of one width"):
        speck_amd.from_coo(ids, Block((5,), dtype="int32"), vals, (4, 6), None)
    with pytest.raises(ValueError, match="from_coo: val is float64, dtype asks for float32"):
        speck_amd.from_coo(ids, ids, vals, (4, 6), None, dtype=np.float32)
    with pytest.raises(ValueError, match="from_coo: dtype"):
        speck_amd.from_coo(ids, ids, None, (4, 6), None, dtype=np.float16)
    for shape in (((1 << 27) + 1, 6), (4, (1 << 27) + 1), (-1, 6), (4,), "ab", None):                    # a shape beyond the limits
        with pytest.raises(ValueError, match="from_coo: shape"):
            speck_amd.from_coo(ids, ids, vals, shape, None)
    with pytest.raises(ValueError, match="from_coo: row is an address"):                                 # an address without nnz
        speck_amd.from_coo(4096, 8192, None, (4, 6), None)
    with pytest.raises(ValueError, match="from_coo: row and col must hold ids of one width"):
        speck_amd.from_coo(4096, 8192, None, (4, 6), None, nnz=3, index_bytes=2)


def test_python_refuses_wrong_edge_lists_before_it_asks_for_an_address():
    vals = Block((5,), dtype="float64")
    for bad in (Block((2, 5), dtype="float32"), Block((3, 5)), Block((5, 2)), Block((10,)),
                Block((2, 5), stride=(1, 2)),                                                            # a transposed E x 2
                "a string", None):
        with pytest.raises(ValueError, match="from_edge_index: edge_index"):
            speck_amd.from_edge_index(bad, vals, (4, 6), None)
    good = Block((2, 5))
    with pytest.raises(ValueError, match="from_edge_index: shape"):
        speck_amd.from_edge_index(good, vals, ((1 << 27) + 1, 6), None)
    with pytest.raises(ValueError, match="from_edge_index: val"):
        speck_amd.from_edge_index(good, Block((5,), dtype="int64"), (4, 6), None)
