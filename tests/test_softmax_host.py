"""speck_softmax_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes Softmax.h
only, the argument checks that come before anything touches a device, the Python wrappers' refusals, and the loud
failure where no device exists."""
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
NORMALIZED, EXP, BACKWARD = 0, 1, 2


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.rsplit(None, 1) if "," not in decl else decl.split(None, 1)
            fields += [(n.strip().lstrip("*"), ctype.replace(" ", "") + ("*" if n.strip().startswith("*") else ""))
                       for n in names.split(",")]
    return fields


def test_header_library_and_table_agree_on_softmax():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_softmax_f64", "speck_softmax_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.POINTER(_lib.DCsr), ctypes.POINTER(_lib.CSoftmaxParams), ctypes.POINTER(_lib.DCsr),
                        ctypes.POINTER(_lib.CSoftmaxInfo)]
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        kinds = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]
        assert kinds == ["speck_config*", "constspeck_dcsr*", "constspeck_softmax_params*", "speck_dcsr*", "speck_softmax_info*"]


def test_structs_the_enum_and_the_define_match_the_header():
    header = _header()
    info = _struct_fields(header, "speck_softmax_info")
    assert [f for f, _ in info] == [f[0] for f in _lib.CSoftmaxInfo._fields_] == ["entries", "nonfinite", "rows_empty", "rows_split",
                                                                                  "tiles"]
    assert all(ctype == "uint64_t" for _, ctype in info) and all(m is ctypes.c_uint64 for _, m in _lib.CSoftmaxInfo._fields_)
    assert ctypes.sizeof(_lib.CSoftmaxInfo) == 40
    assert speck_amd.SoftmaxInfo._fields == tuple(f for f, _ in info)
    params = _struct_fields(header, "speck_softmax_params")
    assert params == [("mode", "uint32_t"), ("reserved", "uint32_t"), ("alpha", "double"), ("d_G", "constvoid*"),
                      ("d_row_max", "double*"), ("d_row_sum", "double*")]
    mirror = {"uint32_t": ctypes.c_uint32, "double": ctypes.c_double, "constvoid*": ctypes.c_void_p, "double*": ctypes.c_void_p}
    assert _lib.CSoftmaxParams._fields_ == [(f, mirror[t]) for f, t in params]
    assert ctypes.sizeof(_lib.CSoftmaxParams) == 40
    assert int(re.search(r"#define\s+SPECK_SOFTMAX_TILE_ENTRIES\s+(\d+)", header).group(1)) == speck_amd.SOFTMAX_TILE_ENTRIES == 4096
    assert speck_amd.SOFTMAX_TILE_ENTRIES == speck_amd.REDUCE_TILE_ENTRIES
    modes = re.search(r"enum \{ SPECK_SOFTMAX_NORMALIZED = (\d+), SPECK_SOFTMAX_EXP = (\d+), SPECK_SOFTMAX_BACKWARD = (\d+) \};", header)
    assert tuple(int(g) for g in modes.groups()) == (NORMALIZED, EXP, BACKWARD) == \
        (speck_amd.SOFTMAX_NORMALIZED, speck_amd.SOFTMAX_EXP, speck_amd.SOFTMAX_BACKWARD)
    assert speck_amd.SOFTMAX_MODES == {"normalized": NORMALIZED, "exp": EXP}


def test_caller_that_includes_softmax_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_softmax.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Softmax.h"]
    out = str(tmp_path / "caller_softmax")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data, m.col_ids, m.row_offsets = buf, buf + 4096, buf + 8192       # three arrays, far from each other
    return m


def _params(mode=NORMALIZED, alpha=1.0, g=None, row_max=None, row_sum=None, reserved=0):
    p = _lib.CSoftmaxParams()
    p.mode, p.reserved, p.alpha, p.d_G, p.d_row_max, p.d_row_sum = mode, reserved, alpha, g, row_max, row_sum
    return p


ROWS, COLS, NNZ = 4, 6, 3
SEVENS = (7, 7, 7, 7, 7)


def _fakes():
    """device pointers nobody will follow: A's arrays at pa, + 4096, + 8192; C's behind them; G and the vectors elsewhere"""
    ka = np.zeros(8192, dtype=np.uint64)
    pa = ka.ctypes.data
    return ka, pa, pa + 16384, pa + 32768, pa + 40960, pa + 49152


def _info_tuple(info):
    return (info.entries, info.nonfinite, info.rows_empty, info.rows_split, info.tiles)


def test_softmax_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    ka, pa, pc, pg, pm, ps = _fakes()
    ref = ctypes.byref
    nan, inf = float("nan"), float("inf")

    for fn in (L.speck_softmax_f64, L.speck_softmax_f32):
        info = _lib.CSoftmaxInfo(*SEVENS)

        def call(A, C=None, **kw):
            p = _params(**kw)
            return fn(None, ref(A) if A is not None else None, ref(p), ref(C) if C is not None else None, ref(info))

        A = _mat(ROWS, COLS, NNZ, pa)
        C = _mat(0, 0, 0, pc)
        assert call(None) == ERR_INVALID                                            # NULL A
        assert fn(None, ref(A), None, None, ref(info)) == ERR_INVALID               # NULL p
        assert call(A, mode=3) == ERR_INVALID                                       # unknown mode
        assert call(A, mode=0xFFFFFFFF) == ERR_INVALID
        assert call(A, reserved=1) == ERR_INVALID                                   # reserved != 0
        assert call(A, mode=BACKWARD, g=pg, reserved=0x80000000) == ERR_INVALID
        for alpha in (nan, inf, -inf):                                              # alpha NaN or infinite
            assert call(A, alpha=alpha) == ERR_INVALID
            assert call(A, mode=EXP, alpha=alpha) == ERR_INVALID
            assert call(A, mode=BACKWARD, g=pg, alpha=alpha) == ERR_INVALID
        assert call(A, mode=BACKWARD) == ERR_INVALID                                # BACKWARD without d_G, nnz > 0
        assert call(A, g=pg) == ERR_INVALID                                         # d_G in a forward mode
        assert call(A, mode=EXP, g=pg) == ERR_INVALID
        assert call(A, mode=BACKWARD, g=pg, row_max=pm) == ERR_INVALID              # d_row_max in BACKWARD
        # a pointer of the call is one of A's or C's three, or two of them are one
        for field in ("data", "col_ids", "row_offsets"):
            for X, out in ((A, None), (A, C), (C, C)):
                at = getattr(X, field)
                assert call(A, C=out, row_max=at) == ERR_INVALID, field
                assert call(A, C=out, row_sum=at) == ERR_INVALID, field
                assert call(A, C=out, mode=BACKWARD, g=at) == ERR_INVALID, field
                assert call(A, C=out, mode=BACKWARD, g=pg, row_sum=at) == ERR_INVALID, field
        assert call(A, row_max=pm, row_sum=pm) == ERR_INVALID                       # one array for both vectors
        assert call(A, mode=BACKWARD, g=pg, row_sum=pg) == ERR_INVALID              # d_G is d_row_sum
        for off in (8, 8 * (ROWS - 1)):                                             # the two ranges of rows doubles overlap
            assert call(A, row_max=pm, row_sum=pm + off) == ERR_INVALID, off
            assert call(A, row_max=pm + off, row_sum=pm) == ERR_INVALID, off
        shared = _mat(ROWS, COLS, NNZ, pc)
        shared.col_ids = A.col_ids
        assert call(A, C=shared) == ERR_INVALID                                     # C shares a buffer with A
        hollow = _mat(ROWS, COLS, NNZ, pa)
        hollow.row_offsets = None
        assert call(hollow) == ERR_INVALID                                          # NULL row_offsets with rows > 0
        hollow = _mat(ROWS, COLS, NNZ, pa)
        hollow.data = None
        assert call(hollow) == ERR_INVALID                                          # NULL data with nnz > 0
        assert call(hollow, C=C) == ERR_INVALID
        hollow = _mat(ROWS, COLS, NNZ, pa)
        hollow.col_ids = None
        assert call(hollow, C=C) == ERR_INVALID                                     # a new C copies the ids
        assert call(_mat(0, COLS, NNZ, pa)) == ERR_INVALID                          # entries, but no row
        assert call(_mat((1 << 27) + 1, COLS, NNZ, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, (1 << 27) + 1, NNZ, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, COLS, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert _info_tuple(info) == SEVENS                                          # refused at the arguments
    assert not ka.any()


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_calls_that_pass_the_argument_checks_get_as_far_as_the_device():
    """every mode, both vectors right behind each other, col_ids NULL in place, BACKWARD without d_G where nnz == 0,
    rows == 0, alpha negative or zero: all reach the no-device status; info is zero by then"""
    no_device = _no_device_status()
    L = _lib.load()
    ka, pa, pc, pg, pm, ps = _fakes()
    ref = ctypes.byref
    A = _mat(ROWS, COLS, NNZ, pa)
    C = _mat(0, 0, 0, pc)

    def call(A, C=None, fn=L.speck_softmax_f64, **kw):
        info = _lib.CSoftmaxInfo(*SEVENS)
        p = _params(**kw)
        rc = fn(None, ref(A), ref(p), ref(C) if C is not None else None, ref(info))
        assert _info_tuple(info) == (0, 0, 0, 0, 0)
        return rc

    assert call(A) == no_device
    assert call(A, C=C, mode=EXP, alpha=-2.0, fn=L.speck_softmax_f32) == no_device
    assert call(A, alpha=0.0) == no_device
    assert call(A, row_max=pm, row_sum=ps) == no_device
    assert call(A, row_max=pm, row_sum=pm + 8 * ROWS) == no_device                  # the ranges touch
    assert call(A, row_max=pm + 8 * ROWS, row_sum=pm) == no_device
    assert call(A, mode=BACKWARD, g=pg, row_sum=ps) == no_device
    assert call(A, C=C, mode=BACKWARD, g=pg, fn=L.speck_softmax_f32) == no_device
    hollow = _mat(ROWS, COLS, NNZ, pa)
    hollow.col_ids = None
    assert call(hollow) == no_device                                                # in place never reads col_ids
    assert call(hollow, mode=BACKWARD, g=pg) == no_device
    none = _mat(ROWS, COLS, 0, pa)
    assert call(none, mode=BACKWARD) == no_device                                   # nnz == 0: d_G may be NULL
    none.data = None
    assert call(none) == no_device
    empty = _mat(0, COLS, 0, pa)
    assert call(empty, fn=L.speck_softmax_f32) == no_device                         # rows == 0
    assert call(empty, C=C) == no_device
    assert not ka.any()


def test_softmax_without_a_gpu_fails_loudly():
    no_device = _no_device_status()
    k, kg = (np.zeros(64, dtype=np.uint64) for _ in range(2))
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data + 64, k.ctypes.data + 128, dtype=dtype)
        G = speck_amd.dCSR.from_device(4, 4, 2, kg.ctypes.data, kg.ctypes.data + 64, kg.ctypes.data + 128, dtype=dtype)
        for kwargs in ({}, {"alpha": 0.5}, {"mode": "exp"}, {"inplace": True}, {"row_sum": k.ctypes.data + 256}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.softmax(A, None, **kwargs)
            assert e.value.status == no_device, kwargs
        for kwargs in ({}, {"alpha": -1.0}, {"inplace": True}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.softmax_backward(A, G, None, **kwargs)
            assert e.value.status == no_device, kwargs
    assert not k.any() and not kg.any()


def test_python_refuses_modes_inplace_with_matout_a_wrong_g_and_a_row_max_in_backward():
    k = np.zeros(64, dtype=np.uint64)
    at = k.ctypes.data
    A = speck_amd.dCSR.from_device(4, 6, 2, at, at + 64, at + 128)
    for mode in ("log", "backward", 2, 3, -1, None, True):
        with pytest.raises(ValueError, match="softmax: unknown mode"):
            speck_amd.softmax(A, None, mode=mode)
    with pytest.raises(ValueError, match="softmax: inplace"):
        speck_amd.softmax(A, None, inplace=True, matOut=speck_amd.dCSR())
    with pytest.raises(ValueError, match="softmax_backward: inplace"):
        speck_amd.softmax_backward(A, A, None, inplace=True, matOut=speck_amd.dCSR())
    for G in (speck_amd.dCSR.from_device(5, 6, 2, at + 256, at + 320, at + 384),                    # other rows
              speck_amd.dCSR.from_device(4, 6, 3, at + 256, at + 320, at + 384)):                   # other nnz
        with pytest.raises(ValueError, match="softmax_backward: G has"):
            speck_amd.softmax_backward(A, G, None)
    with pytest.raises(ValueError, match="softmax_backward: G holds"):
        speck_amd.softmax_backward(A, speck_amd.dCSR.from_device(4, 6, 2, at + 256, at + 320, at + 384, dtype=np.float32), None)
    for G in (at + 256, None, "a string", np.zeros(2)):
        with pytest.raises(ValueError, match="softmax_backward: G must be a dCSR"):
            speck_amd.softmax_backward(A, G, None)
    G = speck_amd.dCSR.from_device(4, 6, 2, at + 256, at + 320, at + 384)
    with pytest.raises(ValueError, match="softmax_backward: row_max"):
        speck_amd.softmax_backward(A, G, None, row_max=at + 448)
    assert not k.any()
