"""speck_sort_rows_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes SortRows.h
only, and the loud failure where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_table_agree_on_sort_rows():
    header = open(os.path.join(ROOT, "include", "speck_c_api.h")).read()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("speck_sort_rows_f64", "speck_sort_rows_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
    assert ctypes.sizeof(_lib.CSortInfo) == 48
    # the class limits are public constants, mirrored in the Python layer
    for macro, value in (("SPECK_SORT_REG_MAX", speck_amd.SORT_REG_MAX), ("SPECK_SORT_LDS_MAX", speck_amd.SORT_LDS_MAX)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, header)
        assert m and int(m.group(1)) == value
    assert re.search(r"SPECK_SORT_KEEP_DUPLICATES\s*=\s*0", header) and re.search(r"SPECK_SORT_SUM_DUPLICATES\s*=\s*1", header)


def test_caller_that_includes_sort_rows_h_only_links(tmp_path):
    out = str(tmp_path / "caller_sort_rows")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "caller_sort_rows.cpp"),
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_sort_rows_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    m = _lib.DCsr()
    assert L.speck_sort_rows_f64(None, None, 0, None) == 1                 # no matrix
    assert L.speck_sort_rows_f64(None, ctypes.byref(m), 2, None) == 1      # unknown flag
    m.rows, m.cols = (1 << 27) + 1, 8
    assert L.speck_sort_rows_f32(None, ctypes.byref(m), 0, None) == 2      # SPECK_ERR_DIM_LIMIT
    m.rows, m.cols, m.nnz = 4, 8, 3                                        # entries without buffers
    assert L.speck_sort_rows_f64(None, ctypes.byref(m), 0, None) == 1


def test_sort_rows_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    # (device pointers nobody will follow: the call has to stop at the missing device)
    keep = np.zeros(16, dtype=np.uint64)
    d = speck_amd.dCSR.from_device(2, 4, 2, keep.ctypes.data, keep.ctypes.data, keep.ctypes.data)
    for sum_duplicates in (False, True):
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.sort_rows(d, None, sum_duplicates=sum_duplicates)
        assert e.value.status == no_device
