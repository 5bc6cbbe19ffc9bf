"""speck_scale_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes Scale.h only,
the argument checks that come before anything touches a device, and the loud failure where no device exists."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 1, 2, 5
NONE, MUL, DIV = speck_amd.SCALE_NONE, speck_amd.SCALE_MUL, speck_amd.SCALE_DIV


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.rsplit(None, 1) if "," not in decl else decl.split(None, 1)
            fields += [(n.strip().lstrip("*"), ctype + ("*" if n.strip().startswith("*") else "")) for n in names.split(",")]
    return fields


def test_header_library_and_table_agree_on_scale():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_scale_f64", "speck_scale_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.POINTER(_lib.DCsr), ctypes.POINTER(_lib.CScaleParams), ctypes.POINTER(_lib.DCsr),
                        ctypes.POINTER(_lib.CScaleInfo)]


def test_structs_enums_and_the_tile_size_match_the_header():
    header = _header()
    info = _fields(header, "speck_scale_info")
    assert [f for f, _ in info] == [f[0] for f in _lib.CScaleInfo._fields_] == ["entries", "nonfinite", "tiles"]
    assert all(t == "uint64_t" for _, t in info) and all(m is ctypes.c_uint64 for _, m in _lib.CScaleInfo._fields_)
    assert ctypes.sizeof(_lib.CScaleInfo) == 24
    params = _fields(header, "speck_scale_params")
    assert params == [("map", "uint32_t"), ("row_mode", "uint32_t"), ("col_mode", "uint32_t"), ("alpha", "double"),
                      ("d_row", "const double*"), ("d_col", "const double*")]
    assert [f[0] for f in _lib.CScaleParams._fields_] == [f for f, _ in params]
    mirror = {"uint32_t": ctypes.c_uint32, "double": ctypes.c_double, "const double*": ctypes.c_void_p}
    assert [f[1] for f in _lib.CScaleParams._fields_] == [mirror[t] for _, t in params]
    # the C layout: three words, a hole, alpha on 8 bytes, two pointers
    assert ctypes.sizeof(_lib.CScaleParams) == 40
    assert [getattr(_lib.CScaleParams, f).offset for f, _ in params] == [0, 4, 8, 16, 24, 32]
    maps = {k: int(v) for k, v in re.findall(r"SPECK_MAP_(IDENTITY|ABS|SQUARE|ONE)\s*=\s*(\d+)", header)}
    assert maps == {"IDENTITY": speck_amd.MAP_IDENTITY, "ABS": speck_amd.MAP_ABS, "SQUARE": speck_amd.MAP_SQUARE,
                    "ONE": speck_amd.MAP_ONE} and sorted(maps.values()) == [0, 1, 2, 3]
    assert {k.upper(): v for k, v in speck_amd.SCALE_MAPS.items()} == maps
    modes = {k: int(v) for k, v in re.findall(r"SPECK_SCALE_(NONE|MUL|DIV)\s*=\s*(\d+)", header)}
    assert modes == {"NONE": NONE, "MUL": MUL, "DIV": DIV} == {"NONE": 0, "MUL": 1, "DIV": 2}
    tile = int(re.search(r"#define\s+SPECK_SCALE_TILE_ENTRIES\s+(\d+)", header).group(1))
    assert speck_amd.SCALE_TILE_ENTRIES == tile == 4096


def test_caller_that_includes_scale_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_scale.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Scale.h"]
    out = str(tmp_path / "caller_scale")
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


def _params(map=0, row_mode=NONE, col_mode=NONE, alpha=1.0, d_row=None, d_col=None):
    p = _lib.CScaleParams()
    p.map, p.row_mode, p.col_mode, p.alpha, p.d_row, p.d_col = map, row_mode, col_mode, alpha, d_row, d_col
    return p


def test_scale_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    rng = np.random.default_rng(3)
    bufs = [rng.integers(1, 1 << 62, size=16).astype(np.uint64) for _ in range(4)]
    before = [b.copy() for b in bufs]
    ka, kc, kl, kr = (b.ctypes.data for b in bufs)
    ref = ctypes.byref

    def call(fn, A, p, C=None):
        info = _lib.CScaleInfo(7, 7, 7)
        c_before = bytes(C) if C is not None else None
        rc = fn(None, ref(A) if A is not None else None, ref(p) if p is not None else None, ref(C) if C is not None else None,
                ref(info))
        assert C is None or bytes(C) == c_before        # a refused call leaves C's struct alone
        return rc

    for fn in (L.speck_scale_f64, L.speck_scale_f32):
        A = _mat(4, 6, 3, ka)
        good = _params(row_mode=DIV, d_row=kl)
        assert call(fn, None, good) == ERR_INVALID                                   # NULL A
        assert call(fn, A, None) == ERR_INVALID                                      # NULL p
        hollow = _mat(4, 6, 3, ka)
        hollow.row_offsets = None
        assert call(fn, hollow, good) == ERR_INVALID                                 # NULL row_offsets
        hollow = _mat(4, 6, 3, ka)
        hollow.data = None
        assert call(fn, hollow, good) == ERR_INVALID                                 # NULL data with nnz > 0
        hollow = _mat(4, 6, 3, ka)
        hollow.col_ids = None                                                        # NULL col_ids where they are read:
        assert call(fn, hollow, _params(col_mode=MUL, d_col=kr)) == ERR_INVALID      # ... a column vector
        assert call(fn, hollow, _params(), C=_lib.DCsr()) == ERR_INVALID             # ... a new C
        for m in (4, 17, 1 << 31):                                                   # unknown maps and modes
            assert call(fn, A, _params(map=m)) == ERR_INVALID
        for m in (3, 1 << 20):
            assert call(fn, A, _params(row_mode=m, d_row=kl)) == ERR_INVALID
            assert call(fn, A, _params(col_mode=m, d_col=kr)) == ERR_INVALID
        for mode in (MUL, DIV):                                                      # a mode without its vector
            assert call(fn, A, _params(row_mode=mode)) == ERR_INVALID
            assert call(fn, A, _params(col_mode=mode)) == ERR_INVALID
        assert call(fn, A, _params(d_row=kl)) == ERR_INVALID                         # a vector without a mode
        assert call(fn, A, _params(d_col=kr)) == ERR_INVALID
        assert call(fn, A, _params(alpha=math.nan)) == ERR_INVALID                   # alpha NaN
        assert call(fn, A, _params(alpha=-math.nan, row_mode=MUL, d_row=kl)) == ERR_INVALID
        for field in ("data", "col_ids", "row_offsets"):                             # a vector is one of A's buffers ...
            alias = _mat(4, 6, 3, ka)
            setattr(alias, field, kl)
            assert call(fn, alias, _params(row_mode=MUL, d_row=kl)) == ERR_INVALID, field
            assert call(fn, alias, _params(col_mode=DIV, d_col=kl)) == ERR_INVALID, field
            Cm = _mat(4, 6, 3, kc)                                                   # ... or one of C's
            setattr(Cm, field, kr)
            assert call(fn, A, _params(col_mode=MUL, d_col=kr), C=Cm) == ERR_INVALID, field
            assert call(fn, A, _params(row_mode=MUL, d_row=kr), C=Cm) == ERR_INVALID, field
            Cm = _mat(4, 6, 3, kc)                                                   # C shares a buffer with A
            setattr(Cm, field, ka)
            assert call(fn, A, _params(), C=Cm) == ERR_INVALID, field
        assert call(fn, _mat((1 << 27) + 1, 6, 3, ka), _params()) == ERR_DIM_LIMIT
        assert call(fn, _mat(4, (1 << 27) + 1, 3, ka), _params()) == ERR_DIM_LIMIT
        assert call(fn, _mat(4, 6, 1 << 32, ka), _params()) == ERR_NNZ_OVERFLOW
    for b, was in zip(bufs, before):
        assert b.tobytes() == was.tobytes()


def test_scale_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    k, v = np.zeros(16, dtype=np.uint64), np.ones(16)
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=dtype)
        for kwargs in ({"inplace": True}, {"alpha": 2.0, "map": "square"}, {"row": v.ctypes.data, "row_div": True, "inplace": True},
                       {"row": v.ctypes.data, "col": v.ctypes.data, "map": speck_amd.MAP_ONE}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.scale(A, None, **kwargs)
            assert e.value.status == no_device
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.pattern_ones(A, None)
        assert e.value.status == no_device
        with pytest.raises(speck_amd.SpeckError):          # (its buffer for the norms is the first thing to fail)
            speck_amd.normalize_rows(A, None)
    assert not k.any() and (v == 1.0).all()


def test_unknown_names_and_wrong_vectors_are_refused_in_python():
    import torch
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    for m in ("sqrt", "ABS", "", 4, -1):
        with pytest.raises(ValueError):
            speck_amd.scale(A, None, map=m)
    with pytest.raises(ValueError):
        speck_amd.normalize_rows(A, None, norm="sq_sum")
    with pytest.raises(ValueError):
        speck_amd.scale(A, None, inplace=True, matOut=speck_amd.dCSR())
    ok_row, ok_col = torch.ones(4, dtype=torch.float64), torch.ones(6, dtype=torch.float64)
    for kwargs in ({"row": torch.ones(4, dtype=torch.float32)},               # dtype
                   {"col": torch.ones(6, dtype=torch.int64)},
                   {"row": torch.ones(5, dtype=torch.float64)},               # length
                   {"col": torch.ones(4, dtype=torch.float64)},
                   {"row": ok_row, "col": torch.ones(7, dtype=torch.float64)},
                   {"row": torch.ones(8, dtype=torch.float64)[::2]},          # contiguity
                   {"col": torch.ones(6, 2, dtype=torch.float64)[:, 0]}):
        with pytest.raises(ValueError):
            speck_amd.scale(A, None, **kwargs)
    if not torch.cuda.is_available():   # (tensors that pass: the call goes on to the library, which finds no device)
        with pytest.raises(speck_amd.SpeckError):
            speck_amd.scale(A, None, row=ok_row, col=ok_col)
