"""speck_sddmm_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes SDDMM.h only,
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
AXPBY, HADAMARD = 0, 1


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


def test_header_library_and_table_agree_on_sddmm():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_sddmm_f64", "speck_sddmm_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [ctypes.c_void_p, ctypes.POINTER(_lib.DCsr), ctypes.POINTER(_lib.CSddmmParams), ctypes.POINTER(_lib.DCsr),
                        ctypes.POINTER(_lib.CSddmmInfo)]
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        kinds = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]
        assert kinds == ["speck_config*", "constspeck_dcsr*", "constspeck_sddmm_params*", "speck_dcsr*", "speck_sddmm_info*"]


def test_structs_and_the_defines_match_the_header():
    header = _header()
    info = _struct_fields(header, "speck_sddmm_info")
    assert [f for f, _ in info] == [f[0] for f in _lib.CSddmmInfo._fields_] == ["entries", "terms", "nonfinite", "tiles", "lanes"]
    assert all(ctype == "uint64_t" for _, ctype in info) and all(m is ctypes.c_uint64 for _, m in _lib.CSddmmInfo._fields_)
    assert ctypes.sizeof(_lib.CSddmmInfo) == 40
    assert speck_amd.SddmmInfo._fields == tuple(f for f, _ in info)
    params = _struct_fields(header, "speck_sddmm_params")
    assert params == [("mode", "uint32_t"), ("k", "uint32_t"), ("alpha", "double"), ("beta", "double"),
                      ("d_U", "constdouble*"), ("ldu", "uint64_t"), ("d_V", "constdouble*"), ("ldv", "uint64_t")]
    mirror = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "constdouble*": ctypes.c_void_p}
    assert _lib.CSddmmParams._fields_ == [(f, mirror[t]) for f, t in params]
    assert ctypes.sizeof(_lib.CSddmmParams) == 56
    assert int(re.search(r"#define\s+SPECK_SDDMM_MAX_K\s+(\d+)", header).group(1)) == speck_amd.SDDMM_MAX_K == 1024
    assert speck_amd.SDDMM_MAX_K == speck_amd.SPMM_MAX_RHS
    assert int(re.search(r"#define\s+SPECK_SDDMM_TILE_ENTRIES\s+(\d+)", header).group(1)) == speck_amd.SDDMM_TILE_ENTRIES == 4096
    modes = re.search(r"enum \{ SPECK_SDDMM_AXPBY = (\d+), SPECK_SDDMM_HADAMARD = (\d+) \};", header)
    assert (int(modes.group(1)), int(modes.group(2))) == (speck_amd.SDDMM_AXPBY, speck_amd.SDDMM_HADAMARD) == (AXPBY, HADAMARD)
    assert speck_amd.SDDMM_MODES == {"axpby": AXPBY, "hadamard": HADAMARD}


def test_lanes_formula_of_the_header():
    """L(k) = min(8, max(1, pow2ceil(ceil(k / 4)))), as the header writes it"""
    assert "L(k) = min(8, max(1, pow2ceil(ceil(k / 4))))" in re.sub(r"\s*\n \*\s*", " ", _header())
    for k in range(0, 1025):
        quarter = (k + 3) // 4
        want = min(8, max(1, 1 << max(quarter - 1, 0).bit_length()))
        assert speck_amd.sddmm_lanes(k) == want, k
    assert [speck_amd.sddmm_lanes(k) for k in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 1024)] == \
        [1, 1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8]


def test_caller_that_includes_sddmm_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_sddmm.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["SDDMM.h"]
    out = str(tmp_path / "caller_sddmm")
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


def _params(u, v, k, ldu, ldv, alpha=1.0, beta=0.0, mode=AXPBY):
    p = _lib.CSddmmParams()
    p.mode, p.k, p.alpha, p.beta, p.d_U, p.ldu, p.d_V, p.ldv = mode, k, alpha, beta, u, ldu, v, ldv
    return p


ROWS, COLS, K, LDU, LDV = 4, 6, 3, 4, 5
U_SPAN = 8 * ((ROWS - 1) * LDU + K)        # bytes from d_U to the end of U(rows - 1, k - 1): 15 doubles
V_SPAN = 8 * ((COLS - 1) * LDV + K)        # ... and of V: 28 doubles
SEVENS = (7, 7, 7, 7, 7)


def _fakes():
    """device pointers nobody will follow: A's arrays at pa, + 4096, + 8192; C's behind them; the blocks elsewhere"""
    ka = np.zeros(8192, dtype=np.uint64)
    pa = ka.ctypes.data
    return ka, pa, pa + 16384, pa + 32768, pa + 40960


def _info_tuple(info):
    return (info.entries, info.terms, info.nonfinite, info.tiles, info.lanes)


def test_sddmm_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    ka, pa, pc, pu, pv = _fakes()
    ref = ctypes.byref
    nan = float("nan")

    for fn in (L.speck_sddmm_f64, L.speck_sddmm_f32):
        info = _lib.CSddmmInfo(*SEVENS)

        def call(A, C=None, u=pu, v=pv, k=K, ldu=LDU, ldv=LDV, **kw):
            p = _params(u, v, k, ldu, ldv, **kw)
            return fn(None, ref(A) if A is not None else None, ref(p), ref(C) if C is not None else None, ref(info))

        A = _mat(ROWS, COLS, 3, pa)
        assert call(None) == ERR_INVALID                                            # NULL A
        assert fn(None, ref(A), None, None, ref(info)) == ERR_INVALID               # NULL p
        hollow = _mat(ROWS, COLS, 3, pa)
        hollow.row_offsets = None
        assert call(hollow) == ERR_INVALID                                          # NULL row_offsets with rows > 0
        hollow = _mat(ROWS, COLS, 3, pa)
        hollow.col_ids = None
        assert call(hollow) == ERR_INVALID                                          # NULL col_ids with nnz > 0 and k > 0
        assert call(A, u=None) == ERR_INVALID                                       # NULL blocks with nnz > 0 and k > 0
        assert call(A, v=None) == ERR_INVALID
        # NULL data with nnz > 0: served only out of place, AXPBY, beta == 0
        hollow = _mat(ROWS, COLS, 3, pa)
        hollow.data = None
        C = _mat(0, 0, 0, pc)
        assert call(hollow) == ERR_INVALID                                          # in place
        assert call(hollow, C=C, beta=1.0) == ERR_INVALID                           # beta reads it
        assert call(hollow, C=C, mode=HADAMARD) == ERR_INVALID                      # the product reads it
        assert call(A, mode=2) == ERR_INVALID                                       # unknown mode
        assert call(A, mode=0xFFFFFFFF) == ERR_INVALID
        assert call(A, alpha=nan) == ERR_INVALID                                    # NaN coefficients
        assert call(A, beta=nan) == ERR_INVALID
        assert call(A, mode=HADAMARD, beta=1.0) == ERR_INVALID                      # HADAMARD takes no beta
        assert call(A, ldu=K - 1) == ERR_INVALID                                    # rows of a block closer than k
        assert call(A, ldv=K - 1) == ERR_INVALID
        assert call(A, k=1, ldu=0) == ERR_INVALID
        assert call(_mat(ROWS, 0, 3, pa)) == ERR_INVALID                            # entries, but no column
        assert call(_mat(0, COLS, 3, pa)) == ERR_INVALID                            # entries, but no row
        # a block is one of A's or C's buffers
        for field in ("data", "col_ids", "row_offsets"):
            for which in ("u", "v"):
                assert call(A, **{which: getattr(A, field)}) == ERR_INVALID, (field, which)
                assert call(A, C=C, **{which: getattr(C, field)}) == ERR_INVALID, (field, which)
        # the span arithmetic with ld > k: [u, u + U_SPAN) holds A->data -- at its first byte, in its padding, at its last
        # double -- and V's likewise
        for off in (0, 8 * K, 8 * LDU, U_SPAN - 8):
            assert call(A, u=A.data - off) == ERR_INVALID, off
            assert call(A, C=C, u=C.col_ids - off) == ERR_INVALID, off
        for off in (0, 8 * K, 8 * LDV, V_SPAN - 8):
            assert call(A, v=A.row_offsets - off) == ERR_INVALID, off
            assert call(A, C=C, v=C.data - off) == ERR_INVALID, off
        # (counted with ld == k the span would be shorter: this one is inside only because the rows are padded)
        assert 8 * ROWS * K <= U_SPAN - 8 and call(A, u=A.data - (U_SPAN - 8), ldu=LDU) == ERR_INVALID
        shared = _mat(ROWS, COLS, 3, pc)
        shared.col_ids = A.col_ids
        assert call(A, C=shared) == ERR_INVALID                                     # C shares a buffer with A
        assert call(A, k=speck_amd.SDDMM_MAX_K + 1, ldu=2000, ldv=2000) == ERR_DIM_LIMIT
        assert call(A, ldu=(1 << 32) + 1) == ERR_DIM_LIMIT                          # (the spans would leave 64 bits)
        assert call(A, ldv=(1 << 32) + 1) == ERR_DIM_LIMIT
        assert call(_mat((1 << 27) + 1, COLS, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
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
    """a span that ENDS at A->data, a span that starts right behind a pointer, U == V, overlapping U and V, the one served
    form of a NULL data, k == 0 with NULL blocks, rows == 0: all reach the no-device status; info is zero by then"""
    no_device = _no_device_status()
    L = _lib.load()
    ka, pa, pc, pu, pv = _fakes()
    ref = ctypes.byref
    A = _mat(ROWS, COLS, 3, pa)
    C = _mat(0, 0, 0, pc)

    def call(A, C=None, u=pu, v=pv, k=K, ldu=LDU, ldv=LDV, fn=L.speck_sddmm_f64, **kw):
        info = _lib.CSddmmInfo(*SEVENS)
        p = _params(u, v, k, ldu, ldv, **kw)
        rc = fn(None, ref(A), ref(p), ref(C) if C is not None else None, ref(info))
        assert _info_tuple(info) == (0, 0, 0, 0, 0)
        return rc

    assert call(A) == no_device
    assert call(A, u=A.data - U_SPAN) == no_device                                  # the span ends exactly at A->data
    assert call(A, v=A.row_offsets - V_SPAN) == no_device
    assert call(A, C=C, u=C.data - U_SPAN, v=C.col_ids - V_SPAN) == no_device
    assert call(A, u=A.data + 8, v=A.col_ids + 8) == no_device                      # a pointer in front of the span
    assert call(A, u=pu, v=pu, ldu=LDV) == no_device                                # U == V (rows == cols is not asked)
    assert call(A, u=pu, v=pu + 8) == no_device                                     # overlapping U and V
    assert call(A, u=pu, v=pu + 8 * K, ldu=7, ldv=7) == no_device                   # two column slices of one tensor
    hollow = _mat(ROWS, COLS, 3, pa)
    hollow.data = None
    assert call(hollow, C=C) == no_device                                           # AXPBY, beta == 0, out of place
    assert call(A, u=None, v=None, k=0, ldu=0, ldv=0) == no_device                  # k == 0: the blocks may be NULL
    assert call(A, u=A.data, v=A.data, k=0, ldu=0, ldv=0) == no_device              # ... and span nothing
    assert call(A, mode=HADAMARD, fn=L.speck_sddmm_f32) == no_device
    none = _mat(0, COLS, 0, pa)
    assert call(none, fn=L.speck_sddmm_f32) == no_device                            # rows == 0
    assert call(none, C=C) == no_device
    assert not ka.any()


def test_sddmm_without_a_gpu_fails_loudly():
    no_device = _no_device_status()
    k, ku, kv = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data + 64, k.ctypes.data + 128, dtype=dtype)
        for kwargs in ({}, {"alpha": 2.0}, {"beta": 0.5}, {"mode": "hadamard"}, {"inplace": True}, {"ldu": 5, "ldv": 4}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.sddmm(A, ku.ctypes.data, kv.ctypes.data, None, k=3, **kwargs)
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


def test_python_refuses_wrong_blocks_modes_and_a_beta_with_hadamard():
    k = np.zeros(64, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data + 64, k.ctypes.data + 128)
    addr = k.ctypes.data + 256
    with pytest.raises(ValueError, match="sddmm: beta"):
        speck_amd.sddmm(A, addr, addr, None, beta=1.0, mode="hadamard", k=2)
    with pytest.raises(ValueError, match="sddmm: beta"):
        speck_amd.sddmm(A, addr, addr, None, beta=-0.5, mode=speck_amd.SDDMM_HADAMARD, k=2)
    for mode in ("softmax", 2, None):
        with pytest.raises(ValueError, match="sddmm: unknown mode"):
            speck_amd.sddmm(A, addr, addr, None, mode=mode, k=2)
    with pytest.raises(ValueError, match="sddmm: inplace"):
        speck_amd.sddmm(A, addr, addr, None, k=2, inplace=True, matOut=speck_amd.dCSR())
    with pytest.raises(ValueError, match="sddmm: U"):
        speck_amd.sddmm(A, addr, addr, None)                                        # an address without k
    for U in (Block((5, 3)),                                                        # not rows rows
              Block((4, 3), dtype="float32"),
              Block((4, 3), stride=(1, 4)),                                         # column-major
              Block((4, 3), stride=(2, 1)),                                         # rows closer than k
              Block((4, 3), stride=(6, 2)),                                         # every other column
              Block((4,)),                                                          # a vector
              Block((4, 3, 1), stride=(3, 1, 1)),
              "a string", 1.5, None):
        with pytest.raises(ValueError, match="sddmm: U"):
            speck_amd.sddmm(A, U, addr, None)
    with pytest.raises(ValueError, match="sddmm: U"):
        speck_amd.sddmm(A, Block((4, 3)), addr, None, k=4)                          # k says otherwise
    with pytest.raises(ValueError, match="sddmm: U"):
        speck_amd.sddmm(A, Block((4, 3), stride=(5, 1)), addr, None, ldu=4)         # ldu says otherwise
    for V in (Block((4, 3)),                                                        # not cols rows
              Block((6, 2)),                                                        # not U's k
              Block((6, 3), dtype="float32"),
              Block((6, 3), stride=(1, 6)),
              Block((6, 3), stride=(2, 1)),
              Block((6,)),
              "a string", 2.5, None):
        with pytest.raises(ValueError, match="sddmm: V"):
            speck_amd.sddmm(A, addr, V, None, k=3)
    with pytest.raises(ValueError, match="sddmm: k"):
        speck_amd.sddmm(A, addr, addr, None, k=3, ldu=2)
    with pytest.raises(ValueError, match="sddmm: k"):
        speck_amd.sddmm(A, addr, addr, None, k=3, ldv=2)
    assert not k.any()
