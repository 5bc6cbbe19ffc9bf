"""speck_spmv_sr_* / speck_spmm_sr_* without a GPU: the declaration, the export, the ctypes mirror, a C++ caller that includes
Semiring.h only, the argument checks that come before anything touches a device, what the Python wrappers refuse, and the
numpy restatement of the products and of the two loops of speck_amd/graph.py -- the expectation of tests/test_gpu_semiring.py
-- against scipy.sparse.csgraph."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 1, 2, 5
NAMES = ["min_plus", "max_plus", "min_times", "max_times", "min_second", "max_second"]
VEC = ("speck_spmv_sr_f64", "speck_spmv_sr_f32")
BLK = ("speck_spmm_sr_f64", "speck_spmm_sr_f32")


# ---------------------------------------------------------------------------------------------------- the restatement
def restate(ro, col, data, X, semiring, Z=None):
    """(Y, changed) of one call, in numpy: ro absolute offsets of the rows (ro[0] may be a view's base), col and data the
    arrays they index, X (cols x k) and Z (rows x k) float64; semiring a name of NAMES.  data is not read with *_second."""
    ro = np.asarray(ro, dtype=np.int64)
    X = np.asarray(X, dtype=np.float64)
    mono, mul = semiring.split("_")
    comb, ident = (np.minimum, np.inf) if mono == "min" else (np.maximum, -np.inf)
    lo, hi = int(ro[0]), int(ro[-1])
    xs = X[np.asarray(col[lo:hi], dtype=np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        if mul == "second":
            t = xs
        else:
            a = np.asarray(data[lo:hi]).astype(np.float64)[:, None]
            t = a + xs if mul == "plus" else a * xs
        S = np.full((len(ro) - 1, X.shape[1]), ident)
        nonempty = np.nonzero(ro[1:] > ro[:-1])[0]
        if len(nonempty):
            S[nonempty] = comb.reduceat(t, ro[:-1][nonempty] - lo, axis=0)
        if Z is None:
            return S, 0
        Z = np.asarray(Z, dtype=np.float64)
        Y = comb(Z, S)
    return Y, int((~((Y == Z) | (np.isnan(Y) & np.isnan(Z)))).sum())


def sssp_case():
    """a directed random graph, n = 2000: (A with A(u, v) the weight of u -> v, its transpose in CSR, the five sources)"""
    A = sp.random(2000, 2000, density=0.0015, format="csr", random_state=5)
    A.data = np.floor(A.data * 99.0) + 1.0                        # integer weights 1 .. 99
    return A, A.T.tocsr(), [0, 400, 800, 1200, 1600]


def cc_case():
    """a symmetrised random graph, n = 3000: its pattern with ones"""
    S = sp.random(3000, 3000, density=0.0004, format="csr", random_state=9)
    return ((S + S.T) != 0).astype(np.float64).tocsr()


def sssp_numpy(At, sources, max_iters=None):
    """speck_amd.sssp with restate in place of spmm_sr"""
    n = At.shape[0]
    D = np.full((n, len(sources)), np.inf)
    D[np.asarray(sources), np.arange(len(sources))] = 0.0
    iterations, converged = 0, False
    while iterations < (n if max_iters is None else max_iters):
        D, changed = restate(At.indptr, At.indices, At.data, D, "min_plus", Z=D)
        iterations += 1
        if changed == 0:
            converged = True
            break
    return D, iterations, converged


def cc_numpy(S):
    """speck_amd.connected_components with restate in place of spmv_sr"""
    n = S.shape[0]
    lab = np.arange(n, dtype=np.float64)[:, None]
    iterations = 0
    while iterations < n:
        lab, changed = restate(S.indptr, S.indices, None, lab, "min_second", Z=lab)
        iterations += 1
        if changed == 0:
            break
    return lab[:, 0].astype(np.int64), iterations


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_the_restatement_on_a_matrix_small_enough_to_read():
    # A = [1 2 .; . . .; 5 . 7], x = [0 10 1]
    ro, col, a = [0, 2, 2, 4], [0, 1, 0, 2], np.array([1.0, 2.0, 5.0, 7.0])
    x = np.array([[0.0], [10.0], [1.0]])
    want = {"min_plus": [1, np.inf, 5], "max_plus": [12, -np.inf, 8], "min_times": [0, np.inf, 0], "max_times": [20, -np.inf, 7],
            "min_second": [0, np.inf, 0], "max_second": [10, -np.inf, 1]}
    for name in NAMES:
        Y, changed = restate(ro, col, a, x, name)
        assert Y[:, 0].tolist() == want[name] and changed == 0, name
    Y, changed = restate(ro, col, a, x, "min_plus", Z=x)
    assert Y[:, 0].tolist() == [0, 10, 1] and changed == 0
    Y, changed = restate(ro, col, a, x, "max_plus", Z=x)
    assert Y[:, 0].tolist() == [12, 10, 8] and changed == 2
    # a NaN is propagated and equals itself; inf + -inf is one; -0.0 equals +0.0
    z = np.array([[np.nan], [-0.0], [3.0]])
    Y, changed = restate([0, 1, 2, 3], [0, 1, 2], np.array([1.0, 0.0, -np.inf]), np.array([[5.0], [0.0], [np.inf]]), "min_plus", Z=z)
    assert np.isnan(Y[0, 0]) and Y[1, 0] == 0.0 and np.isnan(Y[2, 0]) and changed == 1
    # a view: rows 1 .. 2 of the matrix, offsets absolute
    Y, _ = restate(ro[1:], col, a, x, "min_plus")
    assert Y[:, 0].tolist() == [np.inf, 5]


def test_the_numpy_loops_agree_with_scipy():
    A, At, sources = sssp_case()
    D, iterations, converged = sssp_numpy(At, sources)
    assert converged and iterations == 20 and int(np.isinf(D).sum()) == 625
    assert np.array_equal(D, csgraph.dijkstra(A, directed=True, indices=sources).T)
    S = cc_case()
    labels, iterations = cc_numpy(S)
    n_comp, ref = csgraph.connected_components(S, directed=False)
    assert n_comp == 291 and iterations == 16 and len(set(labels.tolist())) == 291
    assert same_partition(labels, ref)
    assert all(labels[i] == min(np.nonzero(ref == ref[i])[0]) for i in range(0, 3000, 97))   # the smallest id of the component
    # a negative cycle never settles; a path of n vertices needs n steps, the last one to see that nothing moves
    cyc = sp.csr_matrix((np.array([1.0, 1.0, -3.0]), (np.array([1, 2, 0]), np.array([0, 1, 2]))), shape=(3, 3))
    assert sssp_numpy(cyc, [0], max_iters=10)[1:] == (10, False)
    path = sp.csr_matrix((np.ones(299), (np.arange(1, 300), np.arange(299))), shape=(300, 300))
    D, iterations, converged = sssp_numpy(path, [0])
    assert (iterations, converged) == (300, True) and np.array_equal(D[:, 0], np.arange(300.0))


# ---------------------------------------------------------------------------------------------------- the interface
def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _kinds(header, name):
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]


def test_header_library_and_table_agree_on_the_semiring_products():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P, V = ctypes.POINTER, ctypes.c_void_p
    for name in VEC + BLK:
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        if name in VEC:
            assert args == [V, ctypes.c_int, P(_lib.DCsr), V, V, V, P(_lib.CSemiringInfo)]
            assert _kinds(header, name) == ["speck_config*", "int", "constspeck_dcsr*", "constdouble*", "constdouble*", "double*",
                                            "speck_semiring_info*"]
        else:
            assert args == [V, ctypes.c_int, P(_lib.DCsr), V, ctypes.c_uint64, ctypes.c_uint32, V, ctypes.c_uint64, V, ctypes.c_uint64,
                            P(_lib.CSemiringInfo)]
            assert _kinds(header, name) == ["speck_config*", "int", "constspeck_dcsr*", "constdouble*", "uint64_t", "uint32_t",
                                            "constdouble*", "uint64_t", "double*", "uint64_t", "speck_semiring_info*"]


def test_enum_and_info_struct_match_the_header():
    header = _header()
    for number, name in enumerate(NAMES):
        assert int(re.search(r"SPECK_SR_%s\s*=\s*(\d+)" % name.upper(), header).group(1)) == number
        assert speck_amd.SEMIRINGS[name] == number == getattr(speck_amd, "SR_" + name.upper())
    assert list(speck_amd.SEMIRINGS) == NAMES
    body = re.search(r"typedef struct speck_semiring_info \{(.*?)\} speck_semiring_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = ["rows_empty", "rows_split", "tiles", "entries", "terms", "changed"]
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSemiringInfo._fields_] == want == list(speck_amd.SemiringInfo._fields)
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CSemiringInfo._fields_)
    assert ctypes.sizeof(_lib.CSemiringInfo) == 48


def test_caller_that_includes_semiring_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_semiring.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Semiring.h"]
    out = str(tmp_path / "caller_semiring")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_the_not_built_lists_no_longer_name_a_semiring():
    header = _header()
    assert "a semiring other" not in header
    assert "argmin" in header and "frontier mask" in header


# ---------------------------------------------------------------------------------------------------- the arguments
def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _buffers():
    """device pointers nobody will follow: every call that uses them has to stop at its arguments"""
    keep = [np.zeros(256, dtype=np.uint64) for _ in range(4)]
    return keep, [k.ctypes.data for k in keep]


def test_vector_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    keep, (pa, px, py, pz) = _buffers()
    ref = ctypes.byref
    for fn in (L.speck_spmv_sr_f64, L.speck_spmv_sr_f32):
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)

        def call(A, sr=0, x=px, z=None, y=py):
            return fn(None, sr, ref(A) if A is not None else None, x, z, y, ref(info))

        A = _mat(4, 6, 3, pa)
        assert call(None) == ERR_INVALID                                            # NULL A
        for sr in (-1, 6, 1 << 20):                                                 # an unknown semiring
            assert call(A, sr=sr) == ERR_INVALID, sr
        hollow = _mat(4, 6, 3, pa)
        hollow.row_offsets = None
        assert call(hollow) == ERR_INVALID                                          # NULL row_offsets
        assert call(A, y=None) == ERR_INVALID                                       # NULL y with rows > 0
        assert call(A, x=None) == ERR_INVALID                                       # NULL x with nnz > 0
        hollow = _mat(4, 6, 3, pa)
        hollow.col_ids = None
        for sr in range(6):
            assert call(hollow, sr=sr) == ERR_INVALID, sr                           # NULL col_ids with nnz > 0
        hollow = _mat(4, 6, 3, pa)
        hollow.data = None
        for sr in range(4):
            assert call(hollow, sr=sr) == ERR_INVALID, sr                           # NULL data: refused where it is read
        for field in ("data", "col_ids", "row_offsets"):                            # a vector is one of A's buffers
            for which in ("x", "z", "y"):
                alias = _mat(4, 6, 3, pa)
                setattr(alias, field, {"x": px, "z": pz, "y": py}[which])
                assert call(alias, z=pz) == ERR_INVALID, (field, which)
        # x is [px, px + 6 doubles), y is [y, y + 4 doubles): every way the two can share a byte
        for y in (px, px + 8, px + 40, px - 8, px - 24):
            assert call(A, y=y) == ERR_INVALID, y - px
            assert call(A, y=y, z=y) == ERR_INVALID, y - px
        # z is [z, z + 4 doubles): it may be y, and may not overlap it otherwise
        for z in (py + 8, py + 24, py - 8, py - 24):
            assert call(A, z=z) == ERR_INVALID, z - py
        assert call(_mat((1 << 27) + 1, 6, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(4, (1 << 27) + 1, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(4, 6, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert call(_mat(4, 0, 3, pa)) == ERR_INVALID                               # entries, but no column
        assert call(_mat(0, 6, 3, pa)) == ERR_INVALID                               # entries, but no row
        assert tuple(getattr(info, f) for f, _ in info._fields_) == (7,) * 6        # refused at the arguments
    assert not any(k.any() for k in keep)


def test_block_arguments_are_checked_before_anything_runs():
    L = _lib.load()
    keep, (pa, px, py, pz) = _buffers()
    ref = ctypes.byref
    for fn in (L.speck_spmm_sr_f64, L.speck_spmm_sr_f32):
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)

        def call(A, sr=0, x=px, ldx=5, k=3, z=None, ldz=0, y=py, ldy=4):
            return fn(None, sr, ref(A) if A is not None else None, x, ldx, k, z, ldz, y, ldy, ref(info))

        A = _mat(4, 6, 3, pa)
        assert call(None) == ERR_INVALID
        for sr in (-1, 6):
            assert call(A, sr=sr) == ERR_INVALID, sr
        assert call(A, ldx=2) == ERR_INVALID                                        # ld < k
        assert call(A, ldy=2) == ERR_INVALID
        assert call(A, z=pz, ldz=2) == ERR_INVALID
        assert call(A, k=1025, ldx=2000, ldy=2000) == ERR_DIM_LIMIT                 # k > SPECK_SPMM_MAX_RHS
        assert call(A, ldx=(1 << 32) + 1) == ERR_DIM_LIMIT
        assert call(A, ldy=(1 << 32) + 1) == ERR_DIM_LIMIT
        assert call(A, z=pz, ldz=(1 << 32) + 1) == ERR_DIM_LIMIT
        assert call(A, y=None) == ERR_INVALID
        assert call(A, x=None) == ERR_INVALID
        hollow = _mat(4, 6, 3, pa)
        hollow.data = None
        assert call(hollow, sr=2) == ERR_INVALID
        for which in ("x", "z", "y"):
            alias = _mat(4, 6, 3, pa)
            alias.col_ids = {"x": px, "z": pz, "y": py}[which]
            assert call(alias, z=pz, ldz=3) == ERR_INVALID, which
        # X spans [px, px + 5 * 5 + 3 doubles), Y [y, y + 3 * 4 + 3 doubles): two column slices of one tensor interleave
        for y in (px, px + 8 * 3, px + 8 * 27, px - 8 * 14, px - 8):
            assert call(A, y=y) == ERR_INVALID, y - px
        # Z is Y only with Y's leading dimension; any other overlap of the two spans is refused
        assert call(A, z=py, ldz=5) == ERR_INVALID
        for z in (py + 8, py + 8 * 14, py - 8 * 14, py - 8):
            assert call(A, z=z, ldz=4) == ERR_INVALID, z - py
        assert call(_mat((1 << 27) + 1, 6, 3, pa)) == ERR_DIM_LIMIT
        assert call(_mat(4, 6, 1 << 32, pa)) == ERR_NNZ_OVERFLOW
        assert call(_mat(0, 6, 3, pa)) == ERR_INVALID
        assert tuple(getattr(info, f) for f, _ in info._fields_) == (7,) * 6
    assert not any(k.any() for k in keep)


def test_what_is_allowed_gets_as_far_as_the_device():
    """z == x, z overlapping x, z == y (blocks: with y's ld), second without data, spans that touch: the arguments pass,
    and without a GPU the call ends where it asks for one"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    no_device = e.value.status
    L = _lib.load()
    keep, (pa, px, py, pz) = _buffers()
    ref = ctypes.byref
    A = _mat(6, 6, 3, pa)                                                           # square: z may be x
    nodata = _mat(6, 6, 3, pa)
    nodata.data = None
    for fn in (L.speck_spmv_sr_f64, L.speck_spmv_sr_f32):
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)
        assert fn(None, 0, ref(A), px, px, py, ref(info)) == no_device              # z == x
        assert tuple(getattr(info, f) for f, _ in info._fields_) == (0,) * 6        # the arguments have passed
        assert fn(None, 0, ref(A), px, px + 16, py, None) == no_device              # z overlaps x
        assert fn(None, 1, ref(A), px, py, py, None) == no_device                   # z == y: in place
        assert fn(None, 0, ref(A), px, None, px + 48, None) == no_device            # y right behind x
        assert fn(None, 0, ref(A), px, pz, pz + 48, None) == no_device              # y right behind z
        for sr in (4, 5):
            assert fn(None, sr, ref(nodata), px, None, py, None) == no_device       # second: data is not needed
    for fn in (L.speck_spmm_sr_f64, L.speck_spmm_sr_f32):
        assert fn(None, 0, ref(A), px, 4, 3, px, 4, py, 5, None) == no_device       # Z == X
        assert fn(None, 0, ref(A), px, 4, 3, px + 8, 3, py, 5, None) == no_device   # Z overlaps X
        assert fn(None, 3, ref(A), px, 4, 3, py, 5, py, 5, None) == no_device       # Z == Y with the same ld
        assert fn(None, 0, ref(A), px, 4, 3, None, 0, px + 8 * 23, 5, None) == no_device   # Y right behind X's span
        assert fn(None, 5, ref(nodata), px, 4, 3, None, 0, py, 5, None) == no_device
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)
        assert fn(None, 0, ref(A), px, 4, 0, None, 0, py, 5, ref(info)) == no_device       # (k == 0 asks for a device too)
    assert not any(k.any() for k in keep)


def test_python_refuses_unknown_semirings_and_wrong_vectors():
    k = np.zeros(64, dtype=np.uint64)
    p = k.ctypes.data
    A = speck_amd.dCSR.from_device(4, 6, 2, p, p, p)
    for bad in ("plus_min", "min", 6, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="unknown semiring"):
            speck_amd.spmv_sr(A, p, None, semiring=bad)
        with pytest.raises(ValueError, match="unknown semiring"):
            speck_amd.spmm_sr(A, p, None, semiring=bad, k=2)

    class Vec:
        def __init__(self, n, dtype="float64", contiguous=True):
            self.n, self.dtype, self.contiguous = n, dtype, contiguous

        def data_ptr(self):
            raise AssertionError("a refused vector is not asked for its address")

        def numel(self):
            return self.n

        def is_contiguous(self):
            return self.contiguous

    for x in (Vec(5), Vec(6, "float32"), Vec(6, contiguous=False)):
        with pytest.raises(ValueError, match="spmv_sr: x"):
            speck_amd.spmv_sr(A, x, None)
    for name in ("y", "z"):
        for v in (Vec(6), Vec(4, "float32"), Vec(4, "int64"), Vec(4, contiguous=False)):
            with pytest.raises(ValueError, match="spmv_sr: " + name):
                speck_amd.spmv_sr(A, p, None, **{name: v})

    class Blk:
        def __init__(self, shape, strides=None, dtype="torch.float64"):
            self.shape, self.dtype = shape, dtype
            self._s = strides if strides is not None else (shape[1], 1)

        def data_ptr(self):
            raise AssertionError("a refused block is not asked for its address")

        def stride(self, i):
            return self._s[i]

    for X in (Blk((5, 3)), Blk((6, 3), dtype="torch.float32"), Blk((6, 3), strides=(1, 6)), Blk((6, 3), strides=(2, 1))):
        with pytest.raises(ValueError, match="spmm_sr: X"):
            speck_amd.spmm_sr(A, X, None)
    for name in ("Y", "Z"):
        for B in (Blk((6, 3)), Blk((4, 2)), Blk((4, 3), dtype="torch.float32"), Blk((4, 3), strides=(1, 4))):
            with pytest.raises(ValueError, match="spmm_sr: " + name):
                speck_amd.spmm_sr(A, p, None, k=3, **{name: B})
    with pytest.raises(ValueError, match="spmm_sr"):
        speck_amd.spmm_sr(A, p, None, k=3, ldx=2)
    with pytest.raises(ValueError, match="spmm_sr"):
        speck_amd.spmm_sr(A, p, None, k=3, Z=p, ldz=2)
    with pytest.raises(ValueError, match="spmm_sr: X is a device address"):
        speck_amd.spmm_sr(A, p, None)


def test_the_graph_loops_refuse_what_they_cannot_run():
    k = np.zeros(16, dtype=np.uint64)
    p = k.ctypes.data
    wide = speck_amd.dCSR.from_device(4, 6, 2, p, p, p)
    with pytest.raises(ValueError, match="square"):
        speck_amd.sssp(wide, [0], None)
    with pytest.raises(ValueError, match="square"):
        speck_amd.connected_components(wide, None)
    A = speck_amd.dCSR.from_device(4, 4, 2, p, p, p)
    for sources in ([], [4], [-1]):
        with pytest.raises(ValueError, match="sources"):
            speck_amd.sssp(A, sources, None)
