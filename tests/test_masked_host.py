"""speck_multiply_masked_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes
MultiplyMasked.h only, the argument checks that come before anything touches a device, and the loud failure where no
device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_table_agree_on_multiply_masked():
    header = open(os.path.join(ROOT, "include", "speck_c_api.h")).read()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_multiply_masked_f64", "speck_multiply_masked_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
    assert ctypes.sizeof(_lib.CMaskedInfo) == 56
    # the class limits are public constants, mirrored in the Python layer
    for macro, value in (("SPECK_MASK_GROUP_MAX", speck_amd.MASK_GROUP_MAX), ("SPECK_MASK_LDS_MAX", speck_amd.MASK_LDS_MAX)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, header)
        assert m and int(m.group(1)) == value
    assert re.search(r"SPECK_MASK_STRUCTURE\s*=\s*0", header) and re.search(r"SPECK_MASK_FULL_PATTERN\s*=\s*1", header)
    # the field order of the struct is the one the header gives
    body = re.search(r"typedef struct speck_masked_info \{(.*?)\} speck_masked_info;", header, re.S).group(1)
    fields = re.findall(r"uint64_t\s+([a-z_]+)", body)
    assert fields == [f[0] for f in _lib.CMaskedInfo._fields_]


def test_caller_that_includes_multiply_masked_h_only_links(tmp_path):
    out = str(tmp_path / "caller_masked")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "caller_masked.cpp"),
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def test_masked_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    # (device pointers nobody will follow: every call below has to stop at its arguments)
    k1, k2, k3, k4 = (np.zeros(16, dtype=np.uint64) for _ in range(4))
    ref = ctypes.byref

    def call(A, B, M, C, flags=0, fn=L.speck_multiply_masked_f64):
        return fn(None, ref(A) if A is not None else None, ref(B) if B is not None else None,
                  ref(M) if M is not None else None, ref(C) if C is not None else None, flags, None)

    A, B, M = _mat(4, 6, 3, k1.ctypes.data), _mat(6, 5, 3, k2.ctypes.data), _mat(4, 5, 3, k3.ctypes.data)
    C = _lib.DCsr()
    assert call(None, B, M, C) == 1 and call(A, None, M, C) == 1 and call(A, B, None, C) == 1   # no matrix
    assert call(A, B, M, None) == 1
    assert call(A, B, M, C, flags=2) == 1 and call(A, B, M, C, flags=-1) == 1                   # unknown flag
    assert call(A, B, _mat(3, 5, 3, k3.ctypes.data), C) == 1                                    # M.rows != A.rows
    assert call(A, B, _mat(4, 6, 3, k3.ctypes.data), C) == 1                                    # M.cols != B.cols
    assert call(A, _mat(7, 5, 3, k2.ctypes.data), M, C) == 1                                    # A.cols != B.rows
    big = (1 << 27) + 1
    assert call(_mat(big, 6, 3, k1.ctypes.data), B, _mat(big, 5, 3, k3.ctypes.data), C,
                fn=L.speck_multiply_masked_f32) == 2                                            # SPECK_ERR_DIM_LIMIT
    assert call(A, _mat(6, big, 3, k2.ctypes.data), _mat(4, big, 3, k3.ctypes.data), C) == 2
    hollow = _mat(4, 6, 3, k1.ctypes.data)
    hollow.col_ids = None
    assert call(hollow, B, M, C) == 1                                                           # entries without buffers
    no_values = _mat(4, 5, 3, k3.ctypes.data)
    no_values.data = None                                                                       # (fine for a mask ...)
    hollow = _mat(6, 5, 3, k2.ctypes.data)
    hollow.data = None                                                                          # (... not for B)
    assert call(A, hollow, no_values, C) == 1
    for other in (A, B, M):                                                                     # C shares a buffer
        alias = _mat(4, 5, 3, k4.ctypes.data)
        alias.col_ids = other.col_ids
        assert call(A, B, M, alias) == 1
        assert (alias.rows, alias.cols, alias.nnz, alias.col_ids) == (4, 5, 3, other.col_ids)


def test_masked_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    keep = [np.zeros(16, dtype=np.uint64) for _ in range(3)]
    A, B, M = (speck_amd.dCSR.from_device(4, 4, 2, k.ctypes.data, k.ctypes.data, k.ctypes.data) for k in keep)
    for full_pattern in (False, True):
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.multiply_masked(A, B, M, None, full_pattern=full_pattern)
        assert e.value.status == no_device
