"""speck_extract_* without a GPU: the declarations, the exports, the ctypes mirrors and the Python info class, a C++ caller
that includes Extract.h only, the contract as numpy (numpy_extract: what tests/test_gpu_extract.py compares the device
with) against scipy, the argument checks that come before anything touches a device, the Python wrappers' refusals, and the
loud failure where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 0, 1, 2, 5
INFO_FIELDS = ["rows_out", "rows_empty", "gross", "nnz_out", "dropped", "cols_kept", "max_row_entries"]
DROP32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the contract
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def numpy_extract(ro, col, val, p, cmap, n_cols, out_cols, index_bytes=8):
    """C = A(p, cmap) as the header states it: (row_offsets, col_ids, the values' bits, info).  ro may be a view's absolute
    offsets; p None: every row; cmap None: identity.  index_bytes 4: the map holds uint32, 0xFFFFFFFF drops."""
    ro = np.asarray(ro, dtype=np.int64)
    p = np.arange(len(ro) - 1, dtype=np.int64) if p is None else np.asarray(p, dtype=np.int64)
    glen = ro[p + 1] - ro[p]
    G = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
    gross = int(G[-1])
    src = np.repeat(ro[p] - G[:-1], glen) + np.arange(gross, dtype=np.int64)
    ids = np.asarray(col)[src].astype(np.int64)
    if cmap is None:
        m, keep, cols_kept = ids, np.ones(gross, dtype=bool), n_cols
    else:
        cmap = np.asarray(cmap, dtype=np.int64)
        dropped = cmap == DROP32 if index_bytes == 4 else cmap < 0
        m = cmap[ids]
        keep = ~dropped[ids]
        cols_kept = int((~dropped).sum())
    row_of = np.repeat(np.arange(len(p)), glen)
    new_ro = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=len(p)))]).astype(np.uint32)
    lens = np.diff(new_ro.astype(np.int64))
    nnz = int(keep.sum())
    info = dict(rows_out=len(p), rows_empty=int((lens == 0).sum()), gross=gross, nnz_out=nnz, dropped=gross - nnz,
                cols_kept=cols_kept, max_row_entries=int(lens.max()) if len(p) else 0)
    return new_ro, m[keep].astype(np.uint32), bits(val)[src][keep], info


def _random_csr(rows, cols, per_row, seed, sort=True):
    rng = np.random.default_rng(seed)
    S = sp.random(rows, cols, density=per_row / cols, format="csr", random_state=rng, dtype=np.float64)
    S.data = rng.integers(1, 100, size=S.nnz).astype(np.float64)
    if sort:
        S.sort_indices()
    return S


def _as_scipy(ro, ci, vb, shape):
    return sp.csr_matrix((vb.view(np.float64), ci.astype(np.int64), ro.astype(np.int64)), shape=shape)


def _inverse(ids, n):
    cmap = np.full(n, -1, dtype=np.int64)
    cmap[ids] = np.arange(len(ids))
    return cmap


def test_numpy_statement_is_scipys_submatrix():
    S = _random_csr(300, 200, 8, seed=1)
    rng = np.random.default_rng(2)
    p = rng.integers(0, 300, size=450)                              # any order, repeats
    q = np.sort(rng.choice(200, size=70, replace=False))            # monotone on what it keeps: the rows stay ascending
    ro, ci, vb, info = numpy_extract(S.indptr, S.indices, S.data, p, _inverse(q, 200), 200, 70)
    W = S[p][:, q]
    W.sort_indices()
    assert np.array_equal(ro, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(vb.view(np.float64), W.data)
    assert info["rows_out"] == 450 and info["nnz_out"] == W.nnz and info["cols_kept"] == 70
    assert info["gross"] == int(np.diff(S.indptr)[p].sum()) and info["dropped"] == info["gross"] - W.nnz
    # the same with uint32 values
    cmap32 = _inverse(q, 200) & DROP32
    got = numpy_extract(S.indptr, S.indices, S.data, p, cmap32, 200, 70, index_bytes=4)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], (ro, ci, vb))) and got[3] == info


def test_numpy_statement_is_scipys_symmetric_permutation():
    S = _random_csr(257, 257, 6, seed=3)
    perm = np.random.default_rng(4).permutation(257)
    ro, ci, vb, info = numpy_extract(S.indptr, S.indices, S.data, perm, _inverse(perm, 257), 257, 257)
    G = _as_scipy(ro, ci, vb, (257, 257))
    G.sort_indices()                                              # sort both sides
    W = S[perm][:, perm]
    W.sort_indices()
    assert np.array_equal(G.indptr, W.indptr) and np.array_equal(G.indices, W.indices) and np.array_equal(G.data, W.data)
    assert info["dropped"] == 0 and info["cols_kept"] == 257 and info["nnz_out"] == S.nnz


def test_a_map_that_is_not_injective_then_summed_is_the_aggregation_product():
    S = _random_csr(120, 90, 7, seed=5)
    agg = np.random.default_rng(6).integers(0, 11, size=90)         # column j belongs to aggregate agg[j]
    ro, ci, vb, info = numpy_extract(S.indptr, S.indices, S.data, None, agg, 90, 11)
    assert info["nnz_out"] == S.nnz and info["dropped"] == 0        # duplicates stay ...
    G = _as_scipy(ro, ci, vb, (120, 11))
    G.sum_duplicates()                                              # ... until they are summed
    P = sp.csr_matrix((np.ones(90), (np.arange(90), agg)), shape=(90, 11))
    W = (S @ P).tocsr()
    W.sort_indices()
    assert np.array_equal(G.indptr, W.indptr) and np.array_equal(G.indices, W.indices) and np.array_equal(G.data, W.data)


def test_numpy_statement_on_a_view_and_in_input_order():
    # rows that are not sorted, a view with an odd first offset, a duplicate inside a row: the order of the input stays
    ro = np.array([3, 5, 5, 9], dtype=np.uint32)
    col = np.array([9, 9, 9, 4, 1, 7, 2, 7, 0], dtype=np.uint32)
    val = np.arange(9, dtype=np.float64)
    got_ro, got_ci, got_vb, info = numpy_extract(ro, col, val, [2, 0, 1, 2], [5, 6, -1, 3, 4, 2, 1, 0], 8, 7)
    assert got_ro.tolist() == [0, 3, 5, 5, 8] and got_ci.tolist() == [0, 0, 5, 4, 6, 0, 0, 5]
    assert got_vb.view(np.float64).tolist() == [5, 7, 8, 3, 4, 5, 7, 8]
    assert info == dict(rows_out=4, rows_empty=1, gross=10, nnz_out=8, dropped=2, cols_kept=7, max_row_entries=3)


# ---------------------------------------------------------------------------------------------------- declarations
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
    for name in ("speck_extract_f64", "speck_extract_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == [ctypes.c_void_p, P(_lib.DCsr), P(_lib.CExtractParams), P(_lib.DCsr), P(_lib.CExtractInfo)]
        assert _kinds(header, name) == ["speck_config*", "constspeck_dcsr*", "constspeck_extract_params*", "speck_dcsr*", "speck_extract_info*"]


def test_structs_hold_exactly_the_listed_fields():
    header = _header()
    fields = _struct_fields(header, "speck_extract_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CExtractInfo._fields_] == INFO_FIELDS
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CExtractInfo._fields_)
    assert ctypes.sizeof(_lib.CExtractInfo) == 8 * len(INFO_FIELDS)
    fields = _struct_fields(header, "speck_extract_params")
    want = [("n_rows", "uint64_t"), ("out_cols", "uint64_t"), ("d_row_index", "const void *"), ("d_col_map", "const void *"),
            ("index_bytes", "uint32_t")]
    assert fields == want
    mirror = {"uint64_t": ctypes.c_uint64, "const void *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}
    assert _lib.CExtractParams._fields_ == [(n, mirror[t]) for n, t in want]
    assert ctypes.sizeof(_lib.CExtractParams) == 40 and _lib.CExtractParams.index_bytes.offset == 32
    assert int(re.search(r"#define SPECK_EXTRACT_TILE_ENTRIES (\d+)", header).group(1)) == speck_amd.EXTRACT_TILE_ENTRIES == 4096
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "extract.hip")).read()
    assert "kTile = SPECK_EXTRACT_TILE_ENTRIES" in source


def test_the_header_names_what_is_not_built():
    block = re.search(r"/\* ---- sub-matrix by index.*?---- \*/", _header(), re.S).group(0)
    not_built = re.sub(r"\s*\*\s+", " ", block[block.index("Not built:"):])
    for what in ("inverse map from a node list", "fused sort or sum of duplicates", "in-place extraction", "scatter into a matrix",
                 "hstack / vstack", "per-row top-k", "plan that is reused across calls"):
        assert what in not_built, what
    assert "NEVER READ" in block                                    # the ids of rows that are not gathered


def test_info_class_wraps_its_c_struct():
    values = dict(zip(INFO_FIELDS, range(1, 8)))
    c = _lib.CExtractInfo()
    for field, v in values.items():
        setattr(c, field, v)
    cls = speck_amd.ExtractInfo
    assert cls is speck_amd.api.ExtractInfo and cls.__name__ == "ExtractInfo" and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values and all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == ("ExtractInfo(rows_out=1, rows_empty=2, gross=3, nnz_out=4, dropped=5, cols_kept=6, max_row_entries=7)")


def test_caller_that_includes_extract_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_extract.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Extract.h"]
    out = str(tmp_path / "caller_extract")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_atomics_run_on_integer_counts_only():
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "extract.hip")).read()
    code = re.sub(r"//[^\n]*", "", source)
    targets = re.findall(r"atomic\w+\(\s*&?\s*([^,]+),", code)
    # (the counters of the status block go through row_tiles.hpp -- wave_counter_to_lds, lds_counter_to_status -- and scan.hpp)
    assert targets and set(targets) <= {"cnt[cur]", "cnt[k_first]", "row_cnt[r0 + i]"}, targets


# ---------------------------------------------------------------------------------------------------- argument checks
def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _a(rows, cols, nnz, pa):
    A = _mat(rows, cols, nnz, pa)
    A.row_offsets, A.col_ids, A.data = pa, pa + 1024, pa + 2048
    return A


def _params(n_rows, out_cols, index, cmap, index_bytes=8):
    p = _lib.CExtractParams()
    p.n_rows, p.out_cols, p.d_row_index, p.d_col_map, p.index_bytes = n_rows, out_cols, index, cmap, index_bytes
    return p


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_extract_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    ka, kc, ki = (np.zeros(1024, dtype=np.uint64) for _ in range(3))
    pa, pc, pi = ka.ctypes.data, kc.ctypes.data, ki.ctypes.data
    ref = ctypes.byref
    for fn in (L.speck_extract_f64, L.speck_extract_f32):
        def call(A, p, out=True, C=None):
            C = _mat(9, 9, 9, pc) if C is None else C
            before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
            info = _lib.CExtractInfo(*([7] * 7))
            rc = fn(None, ref(A) if A is not None else None, ref(p) if p is not None else None, ref(C) if out else None, ref(info))
            assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before       # the struct keeps its sentinel
            assert [getattr(info, f) for f in INFO_FIELDS] == [7] * 7                        # ... and so does *info
            return rc

        A = _a(4, 6, 3, pa)
        good = _params(5, 3, pi, pi + 512)
        assert call(None, good) == ERR_INVALID                                      # NULL A
        assert call(A, None) == ERR_INVALID                                         # NULL params
        assert call(A, good, out=False) == ERR_INVALID                              # NULL C
        for width in (0, 2, 16):
            assert call(A, _params(5, 3, pi, pi + 512, index_bytes=width)) == ERR_INVALID
        assert call(A, _params(5, 3, None, pi + 512)) == ERR_INVALID                # NULL index with n_rows != rows
        assert call(A, _params(3, 3, None, pi + 512)) == ERR_INVALID
        assert call(A, _params(5, 3, pi, None)) == ERR_INVALID                      # NULL map with out_cols != cols
        assert call(A, _params(5, 7, pi, None)) == ERR_INVALID
        big = (1 << 27) + 1
        assert call(_a(big, 6, 3, pa), good) == ERR_DIM_LIMIT
        assert call(_a(4, big, 3, pa), good) == ERR_DIM_LIMIT
        assert call(A, _params(big, 3, pi, pi + 512)) == ERR_DIM_LIMIT
        assert call(A, _params(5, big, pi, pi + 512)) == ERR_DIM_LIMIT
        assert call(_a(big, 6, 3, pa), _params(5, 3, pi, pi + 512, index_bytes=3)) == ERR_INVALID   # the width is asked first
        assert call(_a(4, 6, 1 << 32, pa), good) == ERR_NNZ_OVERFLOW
        for field in ("row_offsets", "col_ids", "data"):                            # NULL buffers with a count
            hollow = _a(4, 6, 3, pa)
            setattr(hollow, field, None)
            assert call(hollow, good) == ERR_INVALID, field
        assert call(_a(0, 6, 3, pa), _params(0, 3, pi, pi + 512)) == ERR_INVALID    # entries, but no row
        assert call(_a(4, 0, 3, pa), _params(5, 3, pi, pi + 512)) == ERR_INVALID    # entries, but no column
        # C sharing a buffer with A
        for field in ("row_offsets", "col_ids", "data"):
            C = _mat(9, 9, 9, pc)
            setattr(C, field, getattr(A, field))
            assert call(A, good, C=C) == ERR_INVALID, field
        # the index (5 ids of `width` bytes) or the map (6 of them) inside one of A's or C's arrays: its start, its middle,
        # its last byte -- and ending right in front of it is fine as far as these checks go
        C = _mat(9, 9, 9, pc)
        C.row_offsets, C.col_ids, C.data = pc, pc + 1024, pc + 2048
        for width in (4, 8):
            spans = [(A.row_offsets, 5 * 4), (A.col_ids, 3 * 4), (A.data, 3 * (8 if fn is L.speck_extract_f64 else 4)),
                     (C.row_offsets, 10 * 4), (C.col_ids, 9 * 4), (C.data, 9 * (8 if fn is L.speck_extract_f64 else 4))]
            for start, length in spans:
                for at in (0, length // 2, length - 1):
                    assert call(A, _params(5, 3, start + at, pi + 512, index_bytes=width), C=C) == ERR_INVALID, (width, start, at)
                    assert call(A, _params(5, 3, pi, start + at, index_bytes=width), C=C) == ERR_INVALID, (width, start, at)
                assert call(A, _params(5, 3, start - 5 * width + 1, pi + 512, index_bytes=width), C=C) == ERR_INVALID   # its last byte inside
    assert not ka.any() and not kc.any() and not ki.any()


def test_without_a_gpu_it_fails_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    ka, kc, ki = (np.zeros(1024, dtype=np.uint64) for _ in range(3))
    pa, pi = ka.ctypes.data, ki.ctypes.data
    for fn in (L.speck_extract_f64, L.speck_extract_f32):
        for A, p in ((_a(4, 6, 3, pa), _params(5, 3, pi, pi + 512)), (_a(4, 6, 3, pa), _params(4, 6, None, None, index_bytes=4)),
                     (_mat(0, 0, 0, None), _params(0, 0, None, None)), (_a(4, 6, 0, pa), _params(0, 2, pi, pi + 512))):
            for C in (_lib.DCsr(), _mat(9, 9, 9, kc.ctypes.data)):
                before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
                info = _lib.CExtractInfo(*([7] * 7))
                assert fn(None, ctypes.byref(A), ctypes.byref(p), ctypes.byref(C), ctypes.byref(info)) == no_device
                assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before
                assert [getattr(info, f) for f in INFO_FIELDS] == [0] * 7           # the arguments have passed: *info is zero
    dA = speck_amd.dCSR.from_device(4, 6, 3, pa, pa + 1024, pa + 2048)
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.extract(dA, rows=pi, col_map=pi + 512, out_cols=3, n_rows=5, index_bytes=8)
    assert e.value.status == no_device
    assert not ka.any() and not kc.any() and not ki.any()


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
    A = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    ids, cmap = Block((5,)), Block((6,))
    for bad in (Block((5,), dtype="float64"), Block((5,), dtype="int16"), Block((5,), stride=(2,)), Block((5, 1)), "a string", 1.5):
        with pytest.raises(ValueError, match="extract: rows"):
            speck_amd.extract(A, rows=bad, col_map=cmap, out_cols=3)
        with pytest.raises(ValueError, match="extract: col_map"):
            speck_amd.extract(A, rows=ids, col_map=bad, out_cols=3)
    with pytest.raises(ValueError, match="extract: col_map holds 5 entries for 6 columns"):
        speck_amd.extract(A, rows=ids, col_map=Block((5,)), out_cols=3)
    with pytest.raises(ValueError, match="extract: out_cols is required"):
        speck_amd.extract(A, rows=ids, col_map=cmap)
    with pytest.raises(ValueError, match="extract: rows and col_map must hold ids of one width"):
        speck_amd.extract(A, rows=ids, col_map=Block((6,), dtype="int32"), out_cols=3)
    with pytest.raises(ValueError, match="extract: rows is an address: pass n_rows and index_bytes"):
        speck_amd.extract(A, rows=4096)
    with pytest.raises(ValueError, match="extract: col_map is an address: pass index_bytes"):
        speck_amd.extract(A, col_map=4096, out_cols=3)
    with pytest.raises(ValueError, match="extract: index_bytes must be 4 or 8"):
        speck_amd.extract(A, rows=4096, n_rows=5, index_bytes=2)
    with pytest.raises(ValueError, match="extract: .* beyond the limit"):
        speck_amd.extract(A, rows=ids, col_map=cmap, out_cols=(1 << 27) + 1)
    for fn, who in ((speck_amd.select_columns, "select_columns"), (speck_amd.induced_subgraph, "induced_subgraph")):
        for bad in (Block((5,), dtype="float32"), Block((5, 2)), "a string", None):
            with pytest.raises(ValueError, match=who):
                fn(A, bad)
    with pytest.raises(ValueError, match="gather_rows: rows"):
        speck_amd.gather_rows(A, Block((5,), dtype="float32"))
    with pytest.raises(ValueError, match="permute"):
        speck_amd.permute(A, row_perm=Block((3,)))                                  # 3 ids for 4 rows


def test_python_wrappers_build_their_maps_with_one_scatter():
    import torch
    A = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    cmap, k = speck_amd.api._inverse_map(torch.tensor([4, 0, 5]), 6, "select_columns", "cols")
    assert k == 3 and cmap.tolist() == [1, -1, -1, -1, 0, 2] and cmap.dtype == torch.int64
    cmap, k = speck_amd.api._inverse_map(torch.tensor([4, 0, 5], dtype=torch.int32), 6, "select_columns", "cols")
    assert cmap.dtype == torch.int32 and cmap.numpy().view(np.uint32).tolist() == [1, DROP32, DROP32, DROP32, 0, 2]
    with pytest.raises(ValueError, match="select_columns: cols holds an id more than once"):
        speck_amd.select_columns(A, torch.tensor([4, 0, 4]))
    with pytest.raises(ValueError, match=r"induced_subgraph: nodes holds an id outside \[0, 6\)"):
        speck_amd.induced_subgraph(A, torch.tensor([4, 6]))
    with pytest.raises(ValueError, match="induced_subgraph: nodes holds an id outside"):
        speck_amd.induced_subgraph(A, torch.tensor([-1, 2]))
    with pytest.raises(ValueError, match="permute: col_perm holds 3 ids for 6 columns"):
        speck_amd.permute(A, col_perm=torch.tensor([4, 0, 5]))
