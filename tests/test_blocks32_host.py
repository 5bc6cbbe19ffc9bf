"""speck_spmm_*_b32, speck_spmm_t_*_b32 and speck_sddmm_*_b32 (float blocks) without a GPU: the declarations, the exports, the
ctypes mirrors, three C++ callers that include one header each, the argument checks that come before anything touches a
device -- the arithmetic of the spans in elements of FOUR bytes among them -- the Python wrappers' refusals around the
keyword `blocks`, and the loud failure where no device exists."""
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
P = ctypes.POINTER


def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


SPMM_ARGS = [ctypes.c_void_p, ctypes.c_double, P(_lib.DCsr), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double,
             ctypes.c_void_p, ctypes.c_uint64, P(_lib.CSpmmInfo)]
SPMM_KINDS = ["speck_config*", "double", "constspeck_dcsr*", "constfloat*", "uint64_t", "uint32_t", "double", "float*", "uint64_t",
              "speck_spmm_info*"]
SPMM_T_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, P(_lib.DCsr), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
               ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, P(_lib.CSpmmTInfo)]
SPMM_T_KINDS = ["speck_config*", "constspeck_tplan*", "double", "constspeck_dcsr*", "constfloat*", "uint64_t", "uint32_t", "double",
                "float*", "uint64_t", "speck_spmm_t_info*"]
SDDMM_ARGS = [ctypes.c_void_p, P(_lib.DCsr), P(_lib.CSddmmParamsB32), P(_lib.DCsr), P(_lib.CSddmmInfo)]
SDDMM_KINDS = ["speck_config*", "constspeck_dcsr*", "constspeck_sddmm_params_b32*", "speck_dcsr*", "speck_sddmm_info*"]
SIX = {"speck_spmm_f64_b32": (SPMM_ARGS, SPMM_KINDS), "speck_spmm_f32_b32": (SPMM_ARGS, SPMM_KINDS),
       "speck_spmm_t_f64_b32": (SPMM_T_ARGS, SPMM_T_KINDS), "speck_spmm_t_f32_b32": (SPMM_T_ARGS, SPMM_T_KINDS),
       "speck_sddmm_f64_b32": (SDDMM_ARGS, SDDMM_KINDS), "speck_sddmm_f32_b32": (SDDMM_ARGS, SDDMM_KINDS)}


def test_header_library_and_table_agree_on_the_six_names():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (args, kinds) in SIX.items():
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, table = _lib._SIGS[name]
        assert res is ctypes.c_int and table == args, name
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        assert [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")] == kinds, name


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1) if "*" not in decl else decl.rsplit("*", 1)
            if "*" in decl:
                ctype += "*"
            fields += [(n.strip(), ctype.replace(" ", "")) for n in names.split(",")]
    return fields


def test_params_b32_match_the_header_and_the_double_params_field_for_field():
    header = _header()
    b32, f64 = _struct_fields(header, "speck_sddmm_params_b32"), _struct_fields(header, "speck_sddmm_params")
    assert [n for n, _ in b32] == [n for n, _ in f64] == [f[0] for f in _lib.CSddmmParamsB32._fields_]
    assert [f[0] for f in _lib.CSddmmParamsB32._fields_] == [f[0] for f in _lib.CSddmmParams._fields_]
    kinds = dict(b32)
    assert kinds["d_U"] == kinds["d_V"] == "constfloat*" and dict(f64)["d_U"] == "constdouble*"
    assert [(n, t) for n, t in b32 if not n.startswith("d_")] == [(n, t) for n, t in f64 if not n.startswith("d_")]
    mirror = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "constfloat*": ctypes.c_void_p}
    assert [mirror[t] for _, t in b32] == [f[1] for f in _lib.CSddmmParamsB32._fields_]
    assert ctypes.sizeof(_lib.CSddmmParamsB32) == ctypes.sizeof(_lib.CSddmmParams) == 56
    block = int(re.search(r"#define\s+SPECK_SPMM_COLUMN_BLOCK_B32\s+(\d+)", header).group(1))
    assert speck_amd.SPMM_COLUMN_BLOCK_B32 == block and block % 4 == 0       # (a 16-byte gather takes four columns)


@pytest.mark.parametrize("caller,only", [("caller_spmm_b32", "SpMM.h"), ("caller_spmm_t_b32", "SpMMT.h"),
                                         ("caller_sddmm_b32", "SDDMM.h")])
def test_callers_that_include_one_header_only_link(tmp_path, caller, only):
    src = os.path.join(ROOT, "tests", "cpp", caller + ".cpp")
    text = open(src).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == [only]
    assert "double*" not in text and "dCSR<double> B" not in text             # (the float overloads are the ones called)
    out = str(tmp_path / caller)
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
X_SPAN = 4 * ((COLS - 1) * LDX + K)        # bytes from d_X to the end of X(cols - 1, k - 1): 28 floats
Y_SPAN = 4 * ((ROWS - 1) * LDY + K)        # ... and of Y: 15 floats


def _fake_plan(rows, cols, nnz):
    """what the argument checks read of a plan: the shape it was made from, its first three words (tplan.hpp); zeros behind"""
    words = np.zeros(16, dtype=np.uint64)
    words[:3] = rows, cols, nnz
    return words


def _span_checks(call, A, px, py, x_span, y_span):
    """call(A, x=, y=, k=, ldx=, ldy=) on fake pointers: the spans [px, px + x_span) and [y, y + y_span) in BYTES"""
    assert call(A, alpha=float("nan")) == ERR_INVALID
    assert call(A, beta=float("nan")) == ERR_INVALID
    # every way the two spans can share a byte: Y one ELEMENT OF FOUR BYTES inside X's span on both sides among them
    for y in (px, px + 4, px + x_span - 4, px - 4, px - y_span + 4, px + 4 * K, px + 4 * LDX):
        assert call(A, y=y) == ERR_INVALID, y - px
    # (one float closer than touching, counted with ld > k; that the spans END there -- they would be twice as long in
    #  doubles -- is test_spans_of_floats_that_touch_pass_the_argument_checks)
    assert call(A, y=px + x_span - 4) == ERR_INVALID and call(A, y=px - y_span + 4) == ERR_INVALID
    # two column slices of one tensor of 7 columns: they share no element, and interleave
    assert call(A, x=px, y=px + 4 * 3, k=3, ldx=7, ldy=7) == ERR_INVALID
    assert call(A, ldx=K - 1) == ERR_INVALID                                        # rows of X closer than k
    assert call(A, ldy=K - 1) == ERR_INVALID
    assert call(A, k=1, ldx=0) == ERR_INVALID
    assert call(A, k=1025, ldx=2000, ldy=2000) == ERR_DIM_LIMIT
    assert call(A, ldx=(1 << 32) + 1) == ERR_DIM_LIMIT
    assert call(A, ldy=(1 << 32) + 1) == ERR_DIM_LIMIT


def test_spmm_b32_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    pa, px = ka.ctypes.data, kb.ctypes.data + 1024
    py = px + X_SPAN + 64
    ref = ctypes.byref
    for fn in (L.speck_spmm_f64_b32, L.speck_spmm_f32_b32):
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)

        def call(A, x=px, y=py, alpha=1.0, beta=0.0, k=K, ldx=LDX, ldy=LDY):
            return fn(None, alpha, ref(A) if A is not None else None, x, ldx, k, beta, y, ldy, ref(info))

        A = _mat(ROWS, COLS, 3, pa)
        assert call(None) == ERR_INVALID
        assert call(A, y=None) == ERR_INVALID and call(A, x=None) == ERR_INVALID
        for field in ("data", "col_ids", "row_offsets"):                            # a block is one of A's buffers
            for vec in (px, py):
                alias = _mat(ROWS, COLS, 3, pa)
                setattr(alias, field, vec)
                assert call(alias) == ERR_INVALID, field
        _span_checks(call, A, px, py, X_SPAN, Y_SPAN)
        assert call(_mat((1 << 27) + 1, COLS, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(ROWS, COLS, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert call(_mat(ROWS, 0, 3, pa)) == ERR_INVALID and call(_mat(0, COLS, 3, pa)) == ERR_INVALID
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms) == (7, 7, 7, 7, 7)
    assert not ka.any() and not kb.any()


def test_spmm_t_b32_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    pa, px = ka.ctypes.data, kb.ctypes.data + 1024
    # X is rows x k here and Y cols x k: the spans change sides
    x_span, y_span = 4 * ((ROWS - 1) * LDX + K), 4 * ((COLS - 1) * LDY + K)
    py = px + x_span + 64
    plan = _fake_plan(ROWS, COLS, 3)
    ref = ctypes.byref
    for fn in (L.speck_spmm_t_f64_b32, L.speck_spmm_t_f32_b32):
        info = _lib.CSpmmTInfo(7, 7, 7, 7, 7)

        def call(A, x=px, y=py, alpha=1.0, beta=0.0, k=K, ldx=LDX, ldy=LDY, plan=plan.ctypes.data):
            return fn(None, plan, alpha, ref(A) if A is not None else None, x, ldx, k, beta, y, ldy, ref(info))

        A = _mat(ROWS, COLS, 3, pa)
        assert call(A, plan=None) == ERR_INVALID and call(None) == ERR_INVALID
        assert call(_mat(ROWS + 1, COLS, 3, pa)) == ERR_INVALID                     # the plan was made from another shape
        assert call(_mat(ROWS, COLS, 4, pa)) == ERR_INVALID
        assert call(A, y=None) == ERR_INVALID and call(A, x=None) == ERR_INVALID
        _span_checks(call, A, px, py, x_span, y_span)
        assert (info.cols_empty, info.cols_split, info.tiles, info.entries, info.terms) == (7, 7, 7, 7, 7)
    assert list(plan[:3]) == [ROWS, COLS, 3] and not plan[3:].any()
    assert not ka.any() and not kb.any()


def _params(u, v, k=K, ldu=LDX, ldv=LDY, mode=0, alpha=1.0, beta=0.0):
    p = _lib.CSddmmParamsB32()
    p.mode, p.k, p.alpha, p.beta, p.d_U, p.ldu, p.d_V, p.ldv = mode, k, alpha, beta, u, ldu, v, ldv
    return p


def test_sddmm_b32_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(512, dtype=np.uint64)
    pa, pu = ka.ctypes.data, kb.ctypes.data + 1024
    u_span, v_span = 4 * ((ROWS - 1) * LDX + K), 4 * ((COLS - 1) * LDY + K)   # U is rows x k with ldu = LDX, V cols x k with ldv = LDY
    pv = pu + 1024
    ref = ctypes.byref
    nan = float("nan")
    for fn in (L.speck_sddmm_f64_b32, L.speck_sddmm_f32_b32):
        info = _lib.CSddmmInfo(7, 7, 7, 7, 7)

        def call(A, C=None, **kw):
            p = _params(kw.pop("u", pu), kw.pop("v", pv), **kw)
            return fn(None, ref(A) if A is not None else None, ref(p), ref(C) if C is not None else None, ref(info))

        A = _mat(ROWS, COLS, 3, pa)
        assert call(None) == ERR_INVALID
        assert fn(None, ref(A), None, None, ref(info)) == ERR_INVALID
        assert call(A, mode=2) == ERR_INVALID and call(A, mode=1, beta=1.0) == ERR_INVALID
        assert call(A, alpha=nan) == ERR_INVALID and call(A, beta=nan) == ERR_INVALID
        assert call(A, u=None) == ERR_INVALID and call(A, v=None) == ERR_INVALID
        assert call(A, ldu=K - 1) == ERR_INVALID and call(A, ldv=K - 1) == ERR_INVALID
        assert call(A, k=1025, ldu=2000, ldv=2000) == ERR_DIM_LIMIT
        assert call(A, ldu=(1 << 32) + 1) == ERR_DIM_LIMIT and call(A, ldv=(1 << 32) + 1) == ERR_DIM_LIMIT
        # a span counted in elements of 4 bytes holds one of A's pointers: its first byte, its last ELEMENT, the padding inside
        for block, span in (("u", u_span), ("v", v_span)):
            for field in ("data", "col_ids", "row_offsets"):
                for inside in (0, span - 4, span - 1, 4 * K):
                    alias = _mat(ROWS, COLS, 3, pa)
                    setattr(alias, field, (pu if block == "u" else pv) + inside)
                    assert call(alias) == ERR_INVALID, (block, field, inside)
        # ... or one of C's
        C = _mat(0, 0, 0, None)
        C.data = pv + v_span - 4
        assert call(A, C=C) == ERR_INVALID
        assert (info.entries, info.terms, info.nonfinite, info.tiles, info.lanes) == (7, 7, 7, 7, 7)
    assert not ka.any() and not kb.any()


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_spans_of_floats_that_touch_pass_the_argument_checks():
    """Y right behind X's span of FLOATS (inside the span the same block would have in doubles) and X right behind Y's are
    served: the call gets as far as the device; info is zero by then.  A span of U that ENDS at A's pointer likewise."""
    no_device = _no_device_status()
    L = _lib.load()
    ka, kb = np.zeros(64, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    A = _mat(ROWS, COLS, 3, ka.ctypes.data)
    px = kb.ctypes.data + 1024
    for y in (px + X_SPAN, px - Y_SPAN):
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)
        assert L.speck_spmm_f64_b32(None, 1.0, ctypes.byref(A), px, LDX, K, 0.0, y, LDY, ctypes.byref(info)) == no_device
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms) == (0, 0, 0, 0, 0)
    plan = _fake_plan(ROWS, COLS, 3)
    x_span, y_span = 4 * ((ROWS - 1) * LDX + K), 4 * ((COLS - 1) * LDY + K)
    for y in (px + x_span, px - y_span):
        info = _lib.CSpmmTInfo(7, 7, 7, 7, 7)
        assert L.speck_spmm_t_f32_b32(None, plan.ctypes.data, 1.0, ctypes.byref(A), px, LDX, K, 0.0, y, LDY,
                                      ctypes.byref(info)) == no_device
        assert (info.cols_empty, info.cols_split, info.tiles, info.entries, info.terms) == (0, 0, 0, 0, 0)
    behind = _mat(ROWS, COLS, 3, ka.ctypes.data)
    behind.data = px + x_span                                                       # (U: rows x k with ldu = LDX)
    p = _params(px, px + 1024)
    info = _lib.CSddmmInfo(7, 7, 7, 7, 7)
    assert L.speck_sddmm_f64_b32(None, ctypes.byref(behind), ctypes.byref(p), None, ctypes.byref(info)) == no_device
    assert (info.entries, info.terms, info.nonfinite, info.tiles, info.lanes) == (0, 0, 0, 0, 0)
    # k == 0 passes the checks too
    assert L.speck_spmm_f32_b32(None, 1.0, ctypes.byref(A), px, 0, 0, 0.0, px, 0, None) == no_device
    assert not ka.any() and not kb.any()


def test_float_blocks_without_a_gpu_fail_loudly():
    no_device = _no_device_status()
    k, kx, ky = (np.zeros(64, dtype=np.uint64) for _ in range(3))
    for dtype in (np.float64, np.float32):
        A = speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data, dtype=dtype)
        for kwargs in ({}, {"beta": 0.5, "Y": ky.ctypes.data}, {"Y": ky.ctypes.data, "ldx": 5, "ldy": 4}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.spmm(A, kx.ctypes.data, None, k=3, blocks="float32", **kwargs)
            assert e.value.status == no_device, kwargs
        with pytest.raises(speck_amd.SpeckError) as e:                              # (plan=None builds one first)
            speck_amd.spmm_t(A, kx.ctypes.data, None, k=3, blocks="float32")
        assert e.value.status == no_device
        for kwargs in ({"inplace": True}, {}, {"mode": "hadamard"}):
            with pytest.raises(speck_amd.SpeckError) as e:
                speck_amd.sddmm(A, kx.ctypes.data, ky.ctypes.data, None, k=3, blocks="float32", **kwargs)
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


def test_python_refuses_blocks_of_the_other_type_and_never_converts():
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    at = k.ctypes.data
    f32, f64 = "float32", "float64"
    # blocks="float32" with a float64 Block; blocks="float64" and the default with a float32 one: the same wording
    for name in ("float64", "torch.float64"):
        with pytest.raises(ValueError, match=r"spmm: X must be float32, not (torch\.)?float64"):
            speck_amd.spmm(A, Block((6, 3), dtype=name), None, blocks=f32)
        with pytest.raises(ValueError, match="spmm: Y must be float32"):
            speck_amd.spmm(A, at, None, Y=Block((4, 3), dtype=name), k=3, blocks=f32)
        with pytest.raises(ValueError, match="spmm_t: X must be float32"):
            speck_amd.spmm_t(A, Block((4, 3), dtype=name), None, blocks=f32)
        with pytest.raises(ValueError, match="spmm_t: Y must be float32"):
            speck_amd.spmm_t(A, at, None, Y=Block((6, 3), dtype=name), k=3, blocks=f32)
        with pytest.raises(ValueError, match="sddmm: U must be float32"):
            speck_amd.sddmm(A, Block((4, 3), dtype=name), at, None, k=3, blocks=f32)
        with pytest.raises(ValueError, match="sddmm: V must be float32"):
            speck_amd.sddmm(A, at, Block((6, 3), dtype=name), None, k=3, blocks=f32)
    for name in ("float32", "torch.float32"):
        for kw in ({}, {"blocks": f64}):
            with pytest.raises(ValueError, match=r"spmm: X must be float64, not (torch\.)?float32"):
                speck_amd.spmm(A, Block((6, 3), dtype=name), None, **kw)
            with pytest.raises(ValueError, match="spmm_t: X must be float64"):
                speck_amd.spmm_t(A, Block((4, 3), dtype=name), None, **kw)
            with pytest.raises(ValueError, match="sddmm: V must be float64"):
                speck_amd.sddmm(A, at, Block((6, 3), dtype=name), None, k=3, **kw)
    # a half block is neither
    for blocks in (f32, f64):
        with pytest.raises(ValueError, match="spmm: X must be " + blocks):
            speck_amd.spmm(A, Block((6, 3), dtype="torch.float16"), None, blocks=blocks)
    # an unknown `blocks`
    for blocks in ("float16", "double", "f32", np.float32, None, 32):
        with pytest.raises(ValueError, match="spmm: blocks"):
            speck_amd.spmm(A, at, None, k=3, blocks=blocks)
        with pytest.raises(ValueError, match="spmm_t: blocks"):
            speck_amd.spmm_t(A, at, None, k=3, blocks=blocks)
        with pytest.raises(ValueError, match="sddmm: blocks"):
            speck_amd.sddmm(A, at, at, None, k=3, blocks=blocks)
    # what the float64 wrappers refuse of a block's layout, the float32 ones refuse
    for X in (Block((5, 3), dtype=f32), Block((6, 3), stride=(1, 6), dtype=f32),   # not cols rows; column-major
              Block((6, 3), stride=(2, 1), dtype=f32), Block((6,), dtype=f32), "a string", 1.5, None):
        with pytest.raises(ValueError, match="spmm: X"):
            speck_amd.spmm(A, X, None, blocks=f32)
    with pytest.raises(ValueError, match="row-major"):
        speck_amd.spmm_t(A, Block((4, 3), stride=(1, 4), dtype=f32), None, blocks=f32)
    with pytest.raises(ValueError, match="row-major"):
        speck_amd.sddmm(A, Block((4, 3), stride=(1, 4), dtype=f32), at, None, blocks=f32)
    # beta != 0 without a Y
    with pytest.raises(ValueError, match="spmm: beta"):
        speck_amd.spmm(A, at, None, beta=1.0, k=2, blocks=f32)
    with pytest.raises(ValueError, match="spmm_t: beta"):
        speck_amd.spmm_t(A, at, None, beta=1.0, k=2, blocks=f32)
    with pytest.raises(ValueError, match="spmm: k"):
        speck_amd.spmm(A, at, None, k=3, ldx=2, blocks=f32)
    assert not k.any()


def test_spmv_and_spmv_t_take_no_blocks_keyword():
    """float vectors for spmv are not built: the keyword does not exist there"""
    k = np.zeros(16, dtype=np.uint64)
    A = speck_amd.dCSR.from_device(4, 6, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data)
    for fn in (speck_amd.spmv, speck_amd.spmv_t):
        with pytest.raises(TypeError):
            fn(A, k.ctypes.data, None, blocks="float32")
