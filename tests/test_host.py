"""CPU-side checks of the product library: it loads, exports every symbol the header
declares, its generators and on-disk formats match the oracle / the reference's own code.
No compute entry point is called here (there is no GPU in the build container)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "speck_c_api.h")).read()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.declared_symbols())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in _lib.load().speck_version()


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.DCsr) == 48                   # 3 x u64 + 3 pointers
    assert ctypes.sizeof(_lib.CTimings) == 8 + 12 * 4       # 2 flags + 12 floats
    assert _lib.load().speck_status_string(2).decode().startswith("matrix dimension")


def test_missing_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(speck_amd.SpeckError):
        speck_amd.spECKConfig.initialize(0)


def test_uniform_generator_is_config1():
    g = json.load(open(os.path.join(G, "synth10k.json")))
    A = speck_amd.gen_matrix("uniform", 1.0, 42)
    O = po.gen_uniform(10000, 42)
    assert A.nnz == g["nnzA"]
    assert (A.row_offsets == O.row_offsets).all() and (A.col_ids == O.col_ids).all()
    assert (A.data == O.data).all()


@pytest.mark.parametrize("kind,scale", [("scircuit", 0.05), ("webbase", 0.01), ("mac_econ", 0.05),
                                        ("cant", 0.05), ("nlpkkt", 0.0005)])
def test_standins_are_valid_sorted_csr(kind, scale):
    A = speck_amd.gen_matrix(kind, scale, 7, signed=True)
    B = speck_amd.gen_matrix(kind, scale, 7, signed=True)
    assert (A.col_ids == B.col_ids).all() and (A.data == B.data).all()  # deterministic
    assert A.rows == A.cols and A.row_offsets[0] == 0 and A.row_offsets[-1] == len(A.col_ids)
    for r in range(A.rows):
        c = A.col_ids[A.row_offsets[r]:A.row_offsets[r + 1]].astype(np.int64)
        assert (np.diff(c) > 0).all() and (len(c) == 0 or c[-1] < A.cols)
    assert (np.abs(A.data) >= 0.5).all() and (np.abs(A.data) < 1.5).all() and (A.data < 0).any()


# the SuiteSparse originals are not available offline, so the stand-ins
# are fitted to their n, nnz(A), P and nnz(C) -- in particular to the compression P / nnz(C) that
# decides how much a hash SpGEMM accumulates
STANDIN_TARGETS = {
    "scircuit": dict(n=170998, nnzA=958936, P=8.68e6, nnzC=5.22e6),
    "webbase": dict(n=1000005, nnzA=3105536, P=69.5e6, nnzC=51.1e6),
    "mac_econ": dict(n=206500, nnzA=1273389, P=7.56e6, nnzC=6.70e6),
    "cant": dict(n=62451, nnzA=4007383, P=269.5e6, nnzC=17.4e6),
}


@pytest.mark.parametrize("kind", sorted(STANDIN_TARGETS))
def test_standins_match_the_suitesparse_figures_within_5_percent(kind):
    want = STANDIN_TARGETS[kind]
    A = speck_amd.gen_matrix(kind, 1.0, 1, signed=True)     # bench.py's seed
    H = po.HostCSR(A.rows, A.cols, A.row_offsets, A.col_ids, A.data)
    P = po.analysis(H, H)["sum_products"]
    _, nnzc = po.symbolic(H, H)
    assert A.rows == want["n"]
    assert abs(A.nnz / want["nnzA"] - 1) < 0.05
    assert abs(P / want["P"] - 1) < 0.05
    assert abs(nnzc / want["nnzC"] - 1) < 0.05
    assert abs((P / nnzc) / (want["P"] / want["nnzC"]) - 1) < 0.05


def test_corrupt_hicsr_is_rejected_not_thrown(tmp_path):
    A = speck_amd.gen_matrix("mac_econ", 0.002, 3, signed=True)
    good = str(tmp_path / "g.hicsr")
    speck_amd.store_hicsr(A, good)
    raw = bytearray(open(good, "rb").read())
    cases = {}
    b = bytearray(raw); b[72:80] = (1 << 60).to_bytes(8, "little"); cases["huge_nnz"] = b      # num_non_zeroes
    cases["truncated"] = raw[:len(raw) - 8]
    b = bytearray(raw); b[-4:] = (7).to_bytes(4, "little"); cases["bad_last_offset"] = b
    b = bytearray(raw); off = 96 + A.nnz * 8; b[off:off + 4] = (0xFFFFFFF0).to_bytes(4, "little"); cases["col_oob"] = b
    for name, data in cases.items():
        path = str(tmp_path / (name + ".hicsr"))
        open(path, "wb").write(bytes(data))
        with pytest.raises(speck_amd.SpeckError):
            speck_amd.load_hicsr(path)


def test_mtx_reader_matches_reference_loader():
    meta = json.load(open(os.path.join(G, "formats.json")))
    for name, m in meta.items():
        A = speck_amd.load_mtx(os.path.join(G, "formats", name))
        assert (A.rows, A.cols, A.nnz) == (m["rows"], m["cols"], m["nnz"]), name
        assert list(A.row_offsets) == m["row_offsets"], name
        assert list(A.col_ids) == m["col_ids"], name
        assert list(A.data) == m["data"], name


def test_hicsr_reads_reference_bytes_and_roundtrips(tmp_path):
    meta = json.load(open(os.path.join(G, "formats.json")))
    for name, m in meta.items():
        ref_file = os.path.join(G, "formats", m["hicsr"])
        A = speck_amd.load_hicsr(ref_file)
        assert list(A.row_offsets) == m["row_offsets"] and list(A.col_ids) == m["col_ids"]
        assert list(A.data) == m["data"]
        out = tmp_path / (name + ".hicsr")
        speck_amd.store_hicsr(A, out)
        ours, theirs = open(out, "rb").read(), open(ref_file, "rb").read()
        assert len(ours) == len(theirs) == 96 + 12 * m["nnz"] + 4 * (m["rows"] + 1)
        # identical except the struct padding the reference leaves uninitialised
        # (7 bytes after the magic, 7 bytes after State::transpose)
        keep = [i for i in range(len(ours)) if not (9 <= i < 16 or 89 <= i < 96)]
        assert bytes(ours[i] for i in keep) == bytes(theirs[i] for i in keep), name


def test_cache_rule_of_the_data_loader(tmp_path):
    src = os.path.join(G, "formats", "general_real.mtx")
    dst = tmp_path / "m.mtx"
    dst.write_text(open(src).read())
    A = speck_amd.load_matrix(dst)
    assert os.path.exists(str(dst) + "d_.hicsr")          # DataLoader.cpp:9-26 file name
    dst.unlink()
    B = speck_amd.load_matrix(dst)                          # served from the cache
    assert (A.col_ids == B.col_ids).all() and (A.data == B.data).all()


def test_reference_binary_reads_our_hicsr(tmp_path):
    """The reference's loadCSR reads what store_hicsr writes.  Where oracle/_ref is not built (reference tree absent)
    the reference's dump of the same file, committed under tests/golden/formats by make_golden.py, stands in for the
    live run -- provided our writer still produces that file byte for byte."""
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_formats")
    A = speck_amd.gen_matrix("mac_econ", 0.002, 3, signed=True)
    path = tmp_path / "x.hicsr"
    speck_amd.store_hicsr(A, path)
    if os.path.exists(ref):
        dump = subprocess.check_output([ref, "dump", str(path)]).decode().split("\n")
    else:
        assert open(path, "rb").read() == open(os.path.join(G, "formats", "mac_econ_ours.hicsr"), "rb").read()
        dump = open(os.path.join(G, "formats", "mac_econ_ours.dump")).read().split("\n")
    assert [int(x) for x in dump[0].split()] == [A.rows, A.cols, A.nnz]
    assert [int(x) for x in dump[1].split()] == list(A.row_offsets)
    assert [int(x) for x in dump[2].split()] == list(A.col_ids)
    assert [float(x) for x in dump[3].split()] == list(A.data)


def test_gather_layout_cpp_unit(tmp_path):
    """Displacement arithmetic of the row-sharded gatherv (speck_amd/csrc/comm_layout.hpp), plain C++."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "t_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "speck_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "test_gather_layout.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert "gather layout ok" in out


def _tril_mirror(A):
    """What the loader makes of `symmetric` + lower triangle: L + L^T without the doubled diagonal."""
    import scipy.sparse as sp
    S = sp.csr_matrix((A.data, A.col_ids, A.row_offsets.astype(np.int64)), shape=(A.rows, A.cols))
    L = sp.tril(S, format="csr")
    M = (L + sp.tril(S, k=-1, format="csr").T).tocsr()
    M.sort_indices()
    return M


def test_mtx_symmetric_roundtrip_and_throughput(tmp_path):
    """A SuiteSparse-style `symmetric` file (lower triangle only) of the nlpkkt stand-in: written by
    speck_store_mtx, read by the parallel two-pass reader; mirrored exactly (reference source/COO.cpp:153-159),
    values bit-identical, and fast enough for the 230 M-entry original (>= 50 M entries/s is asserted on hosts
    with >= 16 cores; this container has 8: >= 10 M entries/s)."""
    import time
    A = speck_amd.gen_matrix("nlpkkt", 0.05, 3, signed=True)
    path = tmp_path / "nlpkkt_like.mtx"
    speck_amd.store_mtx(A, path, symmetric_lower=True)
    L = _lib.load()
    dt = 1e9
    for _ in range(3):   # the reader itself (the numpy copies of load_mtx are the harness'), best of three
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        assert L.speck_load_mtx(str(path).encode(), ctypes.byref(h)) == 0
        dt = min(dt, time.perf_counter() - t0)
        L.speck_host_csr_free(h)
    B = speck_amd.load_mtx(path)
    M = _tril_mirror(A)
    assert B.rows == A.rows and B.cols == A.cols and B.nnz == M.nnz
    assert (B.row_offsets == M.indptr).all() and (B.col_ids == M.indices).all()
    assert (B.data == M.data).all()
    rate = B.nnz / dt
    cores = len(os.sched_getaffinity(0))
    print(f"load_mtx: {B.nnz} entries in {dt:.3f} s = {rate / 1e6:.1f} M entries/s on {cores} cores")
    assert rate >= (50e6 if cores >= 16 else 15e6), rate
    # general round trip, values exact
    path2 = tmp_path / "general.mtx"
    speck_amd.store_mtx(A, path2)
    C = speck_amd.load_mtx(path2)
    assert (C.row_offsets == A.row_offsets).all() and (C.col_ids == A.col_ids).all() and (C.data == A.data).all()


def test_mtx_symmetric_file_with_both_triangles_yields_duplicates(tmp_path):
    """A `symmetric` banner over a file that lists (i, j) AND (j, i): the reference mirrors without
    deduplication (source/COO.cpp:153-159), so every off-diagonal entry appears twice in its row -- kept (file
    order), for the multiply to reject (SPECK_ERR_UNSORTED, tests/test_gpu_driver.py)."""
    p = tmp_path / "both.mtx"
    p.write_text("%%MatrixMarket matrix coordinate real symmetric\n% both triangles\n3 3 5\n"
                 "1 1 1.0\n2 1 2.0\n1 2 3.0\n3 3 4.0\n3 2 5.0\n")
    m = speck_amd.load_mtx(p)
    assert m.rows == 3 and m.nnz == 8
    assert list(m.row_offsets) == [0, 3, 6, 8]
    assert list(m.col_ids) == [0, 1, 1, 0, 0, 2, 1, 2]
    # (row 0: (1,1); (2,1) mirrored -> (0,1) 2.0; (1,2) -> (0,1) 3.0 -- file order among equal columns)
    assert list(m.data) == [1.0, 2.0, 3.0, 2.0, 3.0, 5.0, 5.0, 4.0]


def test_mtx_malformed_files_are_io_errors(tmp_path):
    for body in ("%%MatrixMarket matrix coordinate real general\n2 2 1\n3 1 1.0\n",      # row out of range
                 "%%MatrixMarket matrix coordinate real general\n2 2 1\n1 1 abc\n",      # bad value
                 "%%MatrixMarket matrix coordinate real general\n2 2 1\n0 1 1.0\n",      # 0-based index
                 "%%MatrixMarket matrix array real general\n2 2\n1.0\n",                 # not coordinate
                 "%%MatrixMarket matrix coordinate real skew-symmetric\n2 2 1\n2 1 1.0\n"):
        p = tmp_path / "bad.mtx"
        p.write_text(body)
        with pytest.raises(speck_amd.SpeckError) as e:
            speck_amd.load_mtx(p)
        assert e.value.status == 7


def _build_decl_only_caller(out):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-std=c++17", "-DSPECK_DECLARATIONS_ONLY", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                           os.path.join(root, "tests", "cpp", "caller_decl_only.cpp"),
                           "-L", os.path.join(root, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(root, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_caller_that_sees_declarations_only_links(tmp_path):
    """The library exports spECK::MultiplyspECK<float|double, 4, 1024, DYN, STATIC> (reference
    source/GPU/Multiply.cu:1130-1131): a translation unit compiled with plain g++ against DECLARATIONS only
    (SPECK_DECLARATIONS_ONLY) links; spECKConfig's public streams / events compile as hipStream_t / hipEvent_t."""
    _build_decl_only_caller(str(tmp_path / "caller"))
    syms = subprocess.check_output(["nm", "-DC", _lib.LIB_PATH]).decode()
    for t in ("float", "double"):
        assert f"void spECK::MultiplyspECK<{t}, 4, 1024, 163840, 65536>" in syms
