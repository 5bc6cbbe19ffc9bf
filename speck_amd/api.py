"""Host-side mirror of the reference's interface for the SpGEMM path, over the C ABI.

Names, argument meaning and error behaviour follow the reference:
  MultiplyspECK(A, B, matOut, config, timings)  -- include/Multiply.h:15-16
  dCSR / convert()                              -- include/dCSR.h, source/dCSR.cpp
  spECKConfig.initialize / cleanup              -- include/spECKConfig.h:15-43
  Timings (+=, /=)                              -- include/Timings.h:4-49
  CSR (host)                                    -- include/CSR.h:57-65
All compute goes through libspeck_amd.so; nothing here has a CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CStats, CTimings, DCsr, NUM_NUM_BINS, NUM_SYM_BINS

SYM_CLASS_NAMES = ["g16", "wave256", "wave1k", "block4k", "block16k", "block32k", "bitmap256k", "bitmap1m",
                   "numeric_first", "global_hash", "g8", "wave128", "r32", "r64"]
NUM_CLASS_NAMES = ["direct", "g16", "wave128", "wave512", "block2k", "block8k", "dense4k", "dense16k", "global",
                   "wave256", "nfcopy", "g8", "r32", "r64"]


class SpeckError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = _lib.load().speck_status_string(status).decode()
        super().__init__(f"{where}: {msg} (status {status})" if where else f"{msg} (status {status})")


def _check(status, where=""):
    if status != 0:
        raise SpeckError(status, where)


def lib_path():
    return _lib.LIB_PATH


class HostCSR:
    """Host CSR<T> (reference include/CSR.h): u32 row_offsets[rows+1], u32 col_ids, T data."""

    def __init__(self, rows, cols, row_offsets, col_ids, data):
        self.rows = int(rows)
        self.cols = int(cols)
        self.row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint32)
        self.col_ids = np.ascontiguousarray(col_ids, dtype=np.uint32)
        self.data = np.ascontiguousarray(data)
        if self.row_offsets.shape != (self.rows + 1,):
            raise ValueError("row_offsets must have rows+1 entries")

    @property
    def nnz(self):
        return int(self.row_offsets[-1]) - int(self.row_offsets[0])

    @staticmethod
    def _from_handle(h):
        L = _lib.load()
        r, c, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(L.speck_host_csr_dims(h, C.byref(r), C.byref(c), C.byref(n)))
        ro = np.empty(r.value + 1, dtype=np.uint32)
        ci = np.empty(n.value, dtype=np.uint32)
        da = np.empty(n.value, dtype=np.float64)
        _check(L.speck_host_csr_copy(h, ro.ctypes.data, ci.ctypes.data, da.ctypes.data))
        L.speck_host_csr_free(h)
        return HostCSR(r.value, c.value, ro, ci, da)

    def _to_handle(self):
        L = _lib.load()
        h = C.c_void_p()
        d = np.ascontiguousarray(self.data, dtype=np.float64)
        _check(L.speck_host_csr_from_arrays(self.rows, self.cols, self.nnz, self.row_offsets.ctypes.data,
                                            self.col_ids.ctypes.data, d.ctypes.data, C.byref(h)))
        return h


def gen_matrix(kind, scale=1.0, seed=42, signed=False):
    """Synthetic stand-ins of SURVEY.md 8d: uniform|scircuit|webbase|mac_econ|cant|nlpkkt."""
    h = C.c_void_p()
    _check(_lib.load().speck_gen_matrix(kind.encode(), float(scale), int(seed), int(bool(signed)),
                                        C.byref(h)), f"gen_matrix({kind})")
    return HostCSR._from_handle(h)


def load_mtx(path):
    h = C.c_void_p()
    _check(_lib.load().speck_load_mtx(str(path).encode(), C.byref(h)), f"load_mtx({path})")
    return HostCSR._from_handle(h)


def store_mtx(mat, path, symmetric_lower=False):
    """MatrixMarket coordinate real; symmetric_lower: only the lower triangle, banner `symmetric`."""
    h = mat._to_handle()
    try:
        _check(_lib.load().speck_store_mtx(h, str(path).encode(), int(bool(symmetric_lower))), f"store_mtx({path})")
    finally:
        _lib.load().speck_host_csr_free(h)


def load_hicsr(path):
    h = C.c_void_p()
    _check(_lib.load().speck_load_hicsr(str(path).encode(), C.byref(h)), f"load_hicsr({path})")
    return HostCSR._from_handle(h)


def store_hicsr(mat, path):
    h = mat._to_handle()
    try:
        _check(_lib.load().speck_store_hicsr(h, str(path).encode()), f"store_hicsr({path})")
    finally:
        _lib.load().speck_host_csr_free(h)


def load_matrix(path, write_cache=True):
    """DataLoader rule (source/DataLoader.cpp:24-58): '<path>d_.hicsr' cache, else .mtx."""
    h = C.c_void_p()
    _check(_lib.load().speck_load_matrix(str(path).encode(), int(write_cache), C.byref(h)),
           f"load_matrix({path})")
    return HostCSR._from_handle(h)


class Timings:
    """reference include/Timings.h:4-49 (milliseconds)."""
    FIELDS = ("init", "countProducts", "loadBalanceCounting", "globalMapsCounting", "spGEMMCounting",
              "allocC", "loadBalanceNumeric", "globalMapsNumeric", "spGEMMNumeric", "sorting",
              "cleanup", "complete")

    def __init__(self, measureAll=False, measureCompleteTime=False):
        self.measureAll = measureAll
        self.measureCompleteTime = measureCompleteTime
        for f in self.FIELDS:
            setattr(self, f, 0.0)

    def __iadd__(self, b):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) + getattr(b, f))
        return self

    def __itruediv__(self, x):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) / x)
        return self

    def _to_c(self):
        t = CTimings()
        t.measureAll = int(self.measureAll)
        t.measureCompleteTime = int(self.measureCompleteTime)
        return t

    def _from_c(self, t):
        for f in self.FIELDS:
            setattr(self, f, float(getattr(t, f)))


class dCSR:
    """Device CSR (reference include/dCSR.h:9-22).  Owns its buffers unless built as a view."""

    def __init__(self, dtype=np.float64):
        self._c = DCsr()
        self._owner = True
        self._keep = None
        self.dtype = np.dtype(dtype)
        self._host_row_offsets = None

    rows = property(lambda s: int(s._c.rows))
    cols = property(lambda s: int(s._c.cols))
    nnz = property(lambda s: int(s._c.nnz))

    def alloc(self, rows, cols, nnz, allocOffsets=True):
        _check(_lib.load().speck_dcsr_alloc(C.byref(self._c), rows, cols, nnz, int(allocOffsets),
                                            self.dtype.itemsize), "dCSR.alloc")

    def reset(self):
        if self._owner:
            _lib.load().speck_dcsr_free(C.byref(self._c))
        else:
            # in place: a BoundMultiply (or any other holder of byref(self._c)) keeps pointing at THIS struct
            C.memset(C.byref(self._c), 0, C.sizeof(DCsr))
        self._keep = None

    def __del__(self):
        try:
            self.reset()
        except Exception:
            pass

    # convert(dCSR <- CSR), source/dCSR.cpp:51-65
    @staticmethod
    def from_host(h):
        d = dCSR(h.data.dtype)
        base = int(h.row_offsets[0])
        ro = (h.row_offsets - np.uint32(base)).astype(np.uint32) if base else h.row_offsets
        ci = np.ascontiguousarray(h.col_ids[base:base + h.nnz])
        da = np.ascontiguousarray(h.data[base:base + h.nnz])
        _check(_lib.load().speck_dcsr_upload(C.byref(d._c), h.rows, h.cols, h.nnz, ro.ctypes.data,
                                             ci.ctypes.data, da.ctypes.data, d.dtype.itemsize),
               "convert(dCSR<-CSR)")
        d._host_row_offsets = np.array(ro, dtype=np.uint32)
        return d

    # convert(CSR <- dCSR), source/dCSR.cpp:67-76
    def to_host(self):
        ro = np.zeros(self.rows + 1, dtype=np.uint32)
        ci = np.zeros(self.nnz, dtype=np.uint32)
        da = np.zeros(self.nnz, dtype=self.dtype)
        if self._c.row_offsets:
            _check(_lib.load().speck_dcsr_download(C.byref(self._c), ro.ctypes.data, ci.ctypes.data,
                                                   da.ctypes.data, self.dtype.itemsize),
                   "convert(CSR<-dCSR)")
        return HostCSR(self.rows, self.cols, ro, ci, da)

    # convert(dCSR <- dCSR, padding), source/dCSR.cpp:81-89: device to device
    def copy(self, padding=0):
        d = dCSR(self.dtype)
        _check(_lib.load().speck_dcsr_copy(C.byref(d._c), C.byref(self._c), self.dtype.itemsize, int(padding)),
               "convert(dCSR<-dCSR)")
        if self._host_row_offsets is not None:
            d._host_row_offsets = (self._host_row_offsets - self._host_row_offsets[0]).astype(np.uint32)
        return d

    def row_view(self, r0, r1):
        """Non-owning view of rows [r0, r1): row_offsets stay absolute (shard of A)."""
        if self._host_row_offsets is None:
            raise ValueError("row_view needs the host row offsets (build with from_host/from_device)")
        v = dCSR(self.dtype)
        v._owner = False
        v._keep = self
        v._c.rows = r1 - r0
        v._c.cols = self._c.cols
        v._c.nnz = int(self._host_row_offsets[r1]) - int(self._host_row_offsets[r0])
        v._c.data = self._c.data
        v._c.col_ids = self._c.col_ids
        v._c.row_offsets = (self._c.row_offsets or 0) + 4 * r0
        v._host_row_offsets = self._host_row_offsets[r0:r1 + 1]
        return v

    @staticmethod
    def from_device(rows, cols, nnz, row_offsets_ptr, col_ids_ptr, data_ptr, dtype=np.float64,
                    keep=None, host_row_offsets=None):
        """Non-owning wrapper of caller-owned device buffers (e.g. torch tensors)."""
        v = dCSR(dtype)
        v._owner = False
        v._keep = keep
        v._c.rows, v._c.cols, v._c.nnz = rows, cols, nnz
        v._c.row_offsets, v._c.col_ids, v._c.data = row_offsets_ptr, col_ids_ptr, data_ptr
        v._host_row_offsets = host_row_offsets
        return v


class spECKConfig:
    """reference include/spECKConfig.h:8-53."""

    def __init__(self):
        raise TypeError("use spECKConfig.initialize(device)")  # private ctor in the reference

    @classmethod
    def initialize(cls, device=0):
        self = object.__new__(cls)
        self._h = C.c_void_p()
        _check(_lib.load().speck_config_create(int(device), C.byref(self._h)), "spECKConfig.initialize")
        sm, st, dy = C.c_int(), C.c_int(), C.c_int()
        _lib.load().speck_config_info(self._h, C.byref(sm), C.byref(st), C.byref(dy))
        self.sm = sm.value
        self.maxStaticSharedMemoryPerBlock = st.value
        self.maxDynamicSharedMemoryPerBlock = dy.value
        self.device = device
        return self

    def cleanup(self):
        if getattr(self, "_h", None):
            _lib.load().speck_config_destroy(self._h)
            self._h = None

    def set_stream(self, hip_stream_ptr):
        _check(_lib.load().speck_config_set_stream(self._h, hip_stream_ptr))

    def set_option(self, name, value):
        _check(_lib.load().speck_config_set_option(self._h, name.encode(), int(value)), f"set_option({name})")

    def profile_kernels(self, enable=True):
        _check(_lib.load().speck_config_profile_kernels(self._h, int(enable)))

    def last_stats(self):
        s = CStats()
        _check(_lib.load().speck_last_stats(self._h, C.byref(s)))
        return dict(
            sum_products=int(s.sum_products), nnz_c=int(s.nnz_c), max_row_ops=int(s.max_row_ops),
            max_row_nnz_c=int(s.max_row_nnz_c),
            sym_bin_rows=dict(zip(SYM_CLASS_NAMES, list(s.sym_bin_rows))),
            num_bin_rows=dict(zip(NUM_CLASS_NAMES, list(s.num_bin_rows))),
            sym_bin_bytes=dict(zip(SYM_CLASS_NAMES, list(s.sym_bin_bytes))),
            num_bin_bytes=dict(zip(NUM_CLASS_NAMES, list(s.num_bin_bytes))),
            sym_bin_ms=dict(zip(SYM_CLASS_NAMES, list(s.sym_bin_ms))),
            num_bin_ms=dict(zip(NUM_CLASS_NAMES, list(s.num_bin_ms))),
            analysis_ms=float(s.analysis_ms), scan_ms=float(s.scan_ms),
            sym_light_ms=float(s.sym_light_ms), num_light_ms=float(s.num_light_ms),
            sym_tiny_ms=float(s.sym_tiny_ms), num_tiny_ms=float(s.num_tiny_ms),
            kernel_events_valid=bool(s.kernel_events_valid), numeric_reruns=int(s.numeric_reruns),
            graph_replays=int(s.graph_replays), graph_captures=int(s.graph_captures),
            sym_phase_ms=float(s.sym_phase_ms), num_phase_ms=float(s.num_phase_ms),
            replayed=bool(s.replayed), nf_direct=bool(s.nf_direct), esc_fused=bool(s.esc_fused), pool_fallbacks=int(s.pool_fallbacks),
            scratch_pool_bytes=int(s.scratch_pool_bytes), pred_stages=int(s.pred_stages),
            eager_speculated=int(s.eager_speculated), one_walk=int(s.one_walk), walk_misses=int(s.walk_misses),
            eager_through=int(s.eager_through))


_NO_TIMINGS = CTimings()  # scratch for calls that do not ask for stage times


def MultiplyspECK(A, B, matOut, config, timings=None):
    """spECK::MultiplyspECK<T,...>(A, B, matOut, config, timings), include/Multiply.h:15-16."""
    L = _lib.load()
    t = timings._to_c() if timings is not None else _NO_TIMINGS
    if A.dtype != B.dtype:
        raise TypeError("A and B must share a value type")
    fn = L.speck_multiply_f64 if A.dtype == np.float64 else L.speck_multiply_f32
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    _check(fn(config._h, C.byref(A._c), C.byref(B._c), C.byref(matOut._c), C.byref(t)), "MultiplyspECK")
    if timings is not None:
        timings._from_c(t)
    return matOut


class BoundMultiply:
    """MultiplyspECK(A, B, matOut, config) with its arguments bound once: the benchmark loop of the reference calls
    the SAME multiply again and again (source/Executor.cpp:59-72), and at ~90 us per call the interpreter's share of a
    call -- attribute lookups, four byref objects, a status check through two frames -- is worth measuring out.
    Each __call__ is still exactly one speck_multiply_* call of the C ABI."""

    def __init__(self, A, B, matOut, config):
        if A.dtype != B.dtype:
            raise TypeError("A and B must share a value type")
        L = _lib.load()
        self._fn = L.speck_multiply_f64 if A.dtype == np.float64 else L.speck_multiply_f32
        if matOut.dtype != A.dtype:
            matOut.reset()
            matOut.dtype = A.dtype
        self._keep = (A, B, matOut, config)
        self._args = (config._h, C.byref(A._c), C.byref(B._c), C.byref(matOut._c), C.byref(_NO_TIMINGS))

    def __call__(self):
        rc = self._fn(*self._args)
        if rc:
            _check(rc, "MultiplyspECK")


def _dev_u32(n):
    """Scratch device array through the library's own allocator (a 1 x n dCSR col_ids buffer)."""
    d = dCSR()
    d.alloc(0, 0, max(int(n), 1), allocOffsets=False)
    return d


def analysis(A, B, config):
    """Stage entry point: the reference's readOperations quantities (include/common.cuh:321-459)."""
    L = _lib.load()
    m = A.rows
    bufs = [_dev_u32(m) for _ in range(4)]
    P, M = C.c_uint64(), C.c_uint32()
    _check(L.speck_analysis(config._h, C.byref(A._c), C.byref(B._c), *[b._c.col_ids for b in bufs],
                            C.byref(P), C.byref(M)), "analysis")
    out = {}
    for name, b in zip(("row_ops", "row_max_ops", "row_col_min", "row_col_max"), bufs):
        h = np.zeros(max(m, 1), dtype=np.uint32)
        b._c.nnz = max(m, 1)
        b._c.rows = 0
        _check(L.speck_dcsr_download(C.byref(b._c), None, h.ctypes.data, None, 8))
        out[name] = h[:m]
    out["sum_products"] = int(P.value)
    out["max_row_ops"] = int(M.value)
    return out


def symbolic(A, B, config):
    """Stage entry point: C.row_offsets (host copy) and nnz(C)."""
    L = _lib.load()
    buf = _dev_u32(A.rows + 1)
    n = C.c_uint64()
    _check(L.speck_symbolic(config._h, C.byref(A._c), C.byref(B._c), buf._c.col_ids, C.byref(n)), "symbolic")
    h = np.zeros(A.rows + 1, dtype=np.uint32)
    buf._c.nnz = A.rows + 1
    _check(L.speck_dcsr_download(C.byref(buf._c), None, h.ctypes.data, None, 8))
    return h, int(n.value)


def partition_rows(A, B, config, parts):
    b = (C.c_uint64 * (parts + 1))()
    _check(_lib.load().speck_partition_rows(config._h, C.byref(A._c), C.byref(B._c), parts, b), "partition_rows")
    return [int(x) for x in b]


def compare(ref, cmp, config, compare_data=False, rel_tol=1e-12):
    """spECK::Compare(reference_mat, compare_mat, compare_data) -> bool, include/Compare.h:5-6."""
    n = C.c_uint64()
    fn = _lib.load().speck_compare_f32 if ref.dtype == np.float32 else _lib.load().speck_compare_f64
    _check(fn(config._h, C.byref(ref._c), C.byref(cmp._c), int(compare_data), float(rel_tol), C.byref(n)), "Compare")
    return n.value == 0


def compare_bounded(ref, cmp, abs_products, config, tol=1e-12):
    """(rows differing in structure, rows of equal structure with |ref - cmp| > tol * sum|a*b|); abs_products = |A|*|B|."""
    ns, nv = C.c_uint64(), C.c_uint64()
    _check(_lib.load().speck_compare_bounded_f64(config._h, C.byref(ref._c), C.byref(cmp._c),
                                                 C.byref(abs_products._c), float(tol), C.byref(ns), C.byref(nv)),
           "compare_bounded")
    return int(ns.value), int(nv.value)


def transpose(A, config):
    """spECK::Transpose(matIn, matTransposeOut), include/Transpose.h (float and double)."""
    At = dCSR(A.dtype)
    fn = _lib.load().speck_transpose_f32 if A.dtype == np.float32 else _lib.load().speck_transpose_f64
    _check(fn(config._h, C.byref(A._c), C.byref(At._c)), "Transpose")
    return At


# include/speck_c_api.h: SPECK_SORT_REG_MAX / SPECK_SORT_LDS_MAX (rows up to this many entries are sorted in registers / in LDS)
SORT_REG_MAX = 256
SORT_LDS_MAX = 4096
# speck_amd/csrc/extras.hip: the radix sort behind transpose walks tiles of TRANSPOSE_TILE entries (kRadixThreads x
# kRadixItems; a wave's share of a tile is TRANSPOSE_WAVE_SHARE = 64 x kRadixItems) in TRANSPOSE_BLOCKS workgroups
# (kRadixBlocks); compare runs at most COMPARE_MAX_WAVES waves (8192 workgroups of 4), one row per wave and trip;
# speck_amd/csrc/dcsr.hip: the device copy runs at most COPY_MAX_THREADS threads (8192 workgroups of 256), a word per trip
TRANSPOSE_TILE = 2048
TRANSPOSE_BLOCKS = 1024
TRANSPOSE_WAVE_SHARE = 512
COMPARE_MAX_WAVES = 32768
COPY_MAX_THREADS = 2097152


class _Info:
    """What a call reports: the fields of its C struct (include/speck_c_api.h, _lib.C*Info) as int, an array field as a
    tuple of ints.  A subclass is a name, a docstring and `_fields`."""
    _fields = ()

    def __init__(self, c):
        for f in self._fields:
            v = getattr(c, f)
            setattr(self, f, int(v) if isinstance(v, int) else tuple(int(x) for x in v))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{f}={getattr(self, f)}' for f in self._fields)})"


class SortInfo(_Info):
    """speck_sort_info: what a sort_rows call found and did."""
    _fields = ("rows_in_order", "rows_sorted", "duplicates", "nnz_out")  # rows_sorted: register / LDS / global-memory class


def sort_rows(M, config, sum_duplicates=False):
    """Sort every row of the device matrix M in place by column id (stable); sum_duplicates merges equal columns
    (speck_sort_rows_f64 / _f32).  config may be None.  Returns a SortInfo; M.nnz is the new count."""
    L = _lib.load()
    fn = L.speck_sort_rows_f32 if M.dtype == np.float32 else L.speck_sort_rows_f64
    info = _lib.CSortInfo()
    _check(fn(config._h if config is not None else None, C.byref(M._c), 1 if sum_duplicates else 0, C.byref(info)),
           "sort_rows")
    if sum_duplicates and info.duplicates and M._host_row_offsets is not None:
        M._host_row_offsets = None  # (row_offsets were rewritten on the device)
    return SortInfo(info)


# include/speck_c_api.h: SPECK_MASK_GROUP_MAX / SPECK_MASK_LDS_MAX (mask rows up to this many entries: several rows per
# workgroup / one workgroup per row with its table in LDS; longer ones go through global memory)
MASK_GROUP_MAX = 256
MASK_LDS_MAX = 4096


class MaskedInfo(_Info):
    """speck_masked_info: what a multiply_masked call found and did."""
    _fields = ("rows_idle", "rows_class", "products", "hits", "nnz_out")  # rows_class: group / LDS / global-memory class


def multiply_masked(A, B, M, config, matOut=None, full_pattern=False):
    """C = M o (A B): the product kept only where the mask M has an entry (speck_multiply_masked_f64 / _f32).  Only the
    pattern of M is read.  full_pattern: C takes exactly M's pattern, +0.0 where no product falls; otherwise an entry
    exists where M has one AND a product falls.  config may be None.  Returns (matOut, MaskedInfo)."""
    L = _lib.load()
    if A.dtype != B.dtype:
        raise TypeError("A and B must share a value type")
    fn = L.speck_multiply_masked_f32 if A.dtype == np.float32 else L.speck_multiply_masked_f64
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    info = _lib.CMaskedInfo()
    _check(fn(config._h if config is not None else None, C.byref(A._c), C.byref(B._c), C.byref(M._c), C.byref(matOut._c),
              1 if full_pattern else 0, C.byref(info)), "multiply_masked")
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    return matOut, MaskedInfo(info)


# include/speck_c_api.h: SPECK_SELECT_* flags; SPECK_SELECT_TILE_ROWS_LONG / _SHORT (rows per tile of the marking pass: the
# first where a row of A and of the pattern holds SELECT_LONG_ROW_AVG entries or more on average, the second elsewhere)
SELECT_BAND, SELECT_ABS, SELECT_PATTERN = 1, 2, 4
SELECT_NOT_BAND, SELECT_NOT_ABS, SELECT_NOT_PATTERN = 16, 32, 64
SELECT_TILE_ROWS = (256, 1024)
SELECT_LONG_ROW_AVG = 32
_INT64_MIN, _INT64_MAX = -(1 << 63), (1 << 63) - 1


class SelectInfo(_Info):
    """speck_select_info: what a select call kept and dropped."""
    _fields = ("kept", "dropped", "rows_unchanged", "nnz_out")


def select(A, config, band=None, abs_gt=None, pattern=None, negate=(), row_base=0, matOut=None):
    """C = the entries of A that every given predicate keeps, in input order, bit for bit (speck_select_f64 / _f32).
    band=(lo, hi): lo <= col - (row_base + row) <= hi, None leaves a side open; abs_gt=t: not (|v| <= t), so a NaN is kept;
    pattern=M: (row, col) is an entry of the device matrix M (only its pattern is read).  negate: those of "band", "abs",
    "pattern" whose predicate is to be inverted.  No predicate: a copy.  config may be None.  Returns (matOut, SelectInfo)."""
    L = _lib.load()
    negate = (negate,) if isinstance(negate, str) else tuple(negate)
    unknown = set(negate) - {"band", "abs", "pattern"}
    if unknown:
        raise ValueError(f"negate: unknown predicate(s) {sorted(unknown)}")
    p = _lib.CSelectParams()
    flags = 0
    p.band_lo, p.band_hi = _INT64_MIN, _INT64_MAX
    if band is not None:
        lo, hi = band
        p.band_lo = _INT64_MIN if lo is None else int(lo)
        p.band_hi = _INT64_MAX if hi is None else int(hi)
        flags |= SELECT_BAND
    if abs_gt is not None:
        p.abs_threshold = float(abs_gt)
        flags |= SELECT_ABS
    if pattern is not None:
        p.pattern = C.pointer(pattern._c)
        flags |= SELECT_PATTERN
    for name, bit in (("band", SELECT_NOT_BAND), ("abs", SELECT_NOT_ABS), ("pattern", SELECT_NOT_PATTERN)):
        if name in negate:
            flags |= bit     # (without its predicate: the library refuses it)
    p.flags = flags
    p.row_base = int(row_base)
    fn = L.speck_select_f32 if A.dtype == np.float32 else L.speck_select_f64
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    info = _lib.CSelectInfo()
    _check(fn(config._h if config is not None else None, C.byref(A._c), C.byref(p), C.byref(matOut._c), C.byref(info)),
           "select")
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    return matOut, SelectInfo(info)


def tril(A, config, k=0):
    """The entries of A on and below the k-th diagonal (scipy.sparse.tril), made on the device."""
    return select(A, config, band=(None, k))[0]


def triu(A, config, k=0):
    """The entries of A on and above the k-th diagonal (scipy.sparse.triu), made on the device."""
    return select(A, config, band=(k, None))[0]


# include/speck_c_api.h: SPECK_ADD_UNION; SPECK_ADD_TILE_ROWS_LONG / _SHORT (rows per tile of the marking pass: the first
# where a row of A and of B together hold ADD_LONG_ROW_AVG entries or more on average, the second elsewhere);
# SPECK_ADD_TILE_ENTRIES (entries of an operand per tile of the pass that writes C)
ADD_UNION = 0
ADD_TILE_ROWS = (256, 1024)
ADD_LONG_ROW_AVG = 32
ADD_TILE_ENTRIES = 4096


class AddInfo(_Info):
    """speck_add_info: where the entries of the sum come from."""
    _fields = ("only_a", "only_b", "both", "nnz_out")


def add(A, B, config, alpha=1.0, beta=1.0, matOut=None):
    """C = alpha A + beta B on the union of the two patterns (speck_add_f64 / _f32): rows ascending, every value computed
    in double and rounded once, an entry that cancels to 0.0 stays.  A and B have the same shape and value type and sorted
    rows; they may be the same matrix.  config may be None.  Returns (matOut, AddInfo)."""
    L = _lib.load()
    if A.dtype != B.dtype:
        raise ValueError("A and B must share a value type")
    fn = L.speck_add_f32 if A.dtype == np.float32 else L.speck_add_f64
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    info = _lib.CAddInfo()
    _check(fn(config._h if config is not None else None, float(alpha), C.byref(A._c), float(beta), C.byref(B._c),
              C.byref(matOut._c), ADD_UNION, C.byref(info)), "add")
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    return matOut, AddInfo(info)


def symmetrize(A, config):
    """A + A^T of a square device matrix, made on the device: add(A, transpose(A))."""
    if A.rows != A.cols:
        raise ValueError("symmetrize: A must be square")
    return add(A, transpose(A, config), config)[0]


# include/speck_c_api.h: SPECK_REDUCE_*; the entries of a tile, of a thread and of a wave of the pass that walks them
REDUCE_SUM, REDUCE_ABS_SUM, REDUCE_SQ_SUM, REDUCE_MAX, REDUCE_MIN, REDUCE_ABS_MAX = range(6)
REDUCE_OPS = {"sum": REDUCE_SUM, "abs_sum": REDUCE_ABS_SUM, "sq_sum": REDUCE_SQ_SUM, "max": REDUCE_MAX, "min": REDUCE_MIN,
              "abs_max": REDUCE_ABS_MAX}
REDUCE_TILE_ENTRIES = 4096
REDUCE_THREAD_ENTRIES = 16
REDUCE_WAVE_ENTRIES = 1024


class ReduceInfo(_Info):
    """speck_reduce_info: what the reduction walked."""
    _fields = ("rows_empty", "rows_split", "tiles", "entries")


def _dev_f64(n):
    """n doubles (one at least) from the library's allocator: the data array of a dCSR without rows"""
    d = dCSR(np.float64)
    d.alloc(0, 0, max(int(n), 1), allocOffsets=False)
    return d


def _download_f64(buf, n, who):
    """the first n doubles of a _dev_f64 buffer as a numpy array"""
    out = np.zeros(max(int(n), 1), dtype=np.float64)
    _check(_lib.load().speck_dcsr_download(C.byref(buf._c), None, None, out.ctypes.data, 8), f"{who}: download")
    return out[:n]


def reduce(A, config, op="sum", rows=True, total=True, out_ptr=None):
    """Per row and over all entries of a device matrix (speck_reduce_f64 / _f32): op is "sum", "abs_sum", "sq_sum", "max",
    "min" or "abs_max" (or its REDUCE_* number); results are float64 for both value types.  A row without entries is 0.0,
    -inf for "max", +inf for "min"; a NaN entry makes its row and the total NaN for every op.  Bit-reproducible, and a
    row_view gives the rows of the whole matrix bit for bit.  Column quantities: reduce(transpose(A)).
    Returns (row_values, total, ReduceInfo).  row_values is a numpy array downloaded from a buffer of the library's
    allocator; None when rows=False, and None when out_ptr -- a device address of A.rows float64, e.g. a torch tensor's
    data_ptr() -- keeps the result on the device.  total is None when total=False.  config may be None."""
    if isinstance(op, str):
        if op not in REDUCE_OPS:
            raise ValueError(f"reduce: unknown op {op!r} (one of {', '.join(REDUCE_OPS)})")
        op = REDUCE_OPS[op]
    elif op not in REDUCE_OPS.values():
        raise ValueError(f"reduce: unknown op {op!r}")
    L = _lib.load()
    fn = L.speck_reduce_f32 if A.dtype == np.float32 else L.speck_reduce_f64
    buf = None
    if out_ptr is None and rows:
        buf = _dev_f64(A.rows)
        out_ptr = buf._c.data
    t = C.c_double()
    info = _lib.CReduceInfo()
    _check(fn(config._h if config is not None else None, C.byref(A._c), int(op), out_ptr if rows else None,
              C.byref(t) if total else None, C.byref(info)), "reduce")
    row_values = _download_f64(buf, A.rows, "reduce") if buf is not None else None
    return row_values, (float(t.value) if total else None), ReduceInfo(info)


# include/speck_c_api.h: SPECK_MAP_*, SPECK_SCALE_*; the entries of a tile of the pass that walks them with a row vector
MAP_IDENTITY, MAP_ABS, MAP_SQUARE, MAP_ONE = range(4)
SCALE_MAPS = {"identity": MAP_IDENTITY, "abs": MAP_ABS, "square": MAP_SQUARE, "one": MAP_ONE}
SCALE_NONE, SCALE_MUL, SCALE_DIV = range(3)
SCALE_TILE_ENTRIES = 4096


class ScaleInfo(_Info):
    """speck_scale_info: what the scaling wrote."""
    _fields = ("entries", "nonfinite", "tiles")


def _device_vector(v, n, what, who="scale"):
    """The device address of a vector of n float64: an address as it is, a torch tensor (anything with data_ptr()) checked"""
    if v is None:
        return None
    if not hasattr(v, "data_ptr"):
        return int(v)
    if hasattr(v, "dtype") and str(v.dtype) not in ("torch.float64", "float64"):
        raise ValueError(f"{who}: {what} must be float64, not {v.dtype}")
    if hasattr(v, "is_contiguous") and not v.is_contiguous():
        raise ValueError(f"{who}: {what} must be contiguous")
    if hasattr(v, "numel") and v.numel() != n:
        raise ValueError(f"{who}: {what} holds {v.numel()} values, the matrix asks for {n}")
    return int(v.data_ptr())


def scale(A, config, alpha=1.0, map="identity", row=None, col=None, row_div=False, col_div=False, matOut=None, inplace=False):
    """C(i,j) = ((alpha g(A(i,j))) (.) row[i]) (.) col[j] on A's pattern (speck_scale_f64 / _f32).  map is g: "identity",
    "abs", "square" or "one" (1.0 whatever the entry holds, a NaN included), or its MAP_* number.  row (A.rows float64) and
    col (A.cols float64) are optional device vectors -- a device address or an object with data_ptr(), e.g. a torch tensor;
    they may be one array; row is indexed by the row inside A, so for a row_view pass the slice.  Each multiplies, or divides
    with row_div / col_div.  Every step is computed in double and rounded once to A's value type: bit for bit numpy's
    (((alpha * g(a.astype(f64))) (.) row[i]) (.) col[j]).astype(dtype), NaN where numpy has NaN.  Nothing is hidden or
    dropped: 0 * inf, x / 0 and a NaN of a vector land in the entry and are counted in info.nonfinite; a result of 0.0 stays.
    inplace=True overwrites A's values (on a row_view: the view's entries only) and leaves its structure alone; otherwise
    the result goes to matOut (a new matrix when None) with A's pattern, offsets rebased to 0.  Rows need not be sorted;
    col_ids is read only for col or a new matrix.  config may be None.  Returns (matOut or A, ScaleInfo)."""
    if isinstance(map, str):
        if map not in SCALE_MAPS:
            raise ValueError(f"scale: unknown map {map!r} (one of {', '.join(SCALE_MAPS)})")
        map = SCALE_MAPS[map]
    elif map not in SCALE_MAPS.values():
        raise ValueError(f"scale: unknown map {map!r}")
    if inplace and matOut is not None:
        raise ValueError("scale: inplace=True and matOut exclude each other")
    p = _lib.CScaleParams()
    p.map = int(map)
    p.alpha = float(alpha)
    p.d_row = _device_vector(row, A.rows, "row")
    p.d_col = _device_vector(col, A.cols, "col")
    p.row_mode = SCALE_NONE if row is None else SCALE_DIV if row_div else SCALE_MUL
    p.col_mode = SCALE_NONE if col is None else SCALE_DIV if col_div else SCALE_MUL
    L = _lib.load()
    fn = L.speck_scale_f32 if A.dtype == np.float32 else L.speck_scale_f64
    info = _lib.CScaleInfo()
    h = config._h if config is not None else None
    if inplace:
        _check(fn(h, C.byref(A._c), C.byref(p), None, C.byref(info)), "scale")
        return A, ScaleInfo(info)
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    _check(fn(h, C.byref(A._c), C.byref(p), C.byref(matOut._c), C.byref(info)), "scale")
    ro = A._host_row_offsets   # (C's offsets are A's, from 0: the host copy is shared where A's start there)
    matOut._host_row_offsets = ro if ro is None or ro[0] == 0 else (ro - ro[0]).astype(np.uint32)
    return matOut, ScaleInfo(info)


_ROW_NORMS = ("abs_sum", "sum", "abs_max")


def normalize_rows(A, config, norm="abs_sum", inplace=False):
    """Every row of A divided by its norm -- "abs_sum" (row-stochastic where the entries are not negative), "sum" or
    "abs_max" -- without leaving the device: reduce(A, norm) into a device buffer, then scale(A, row=that, row_div=True).
    A row whose norm is 0 (explicit zeros only, or values that cancel under "sum") becomes NaN (0 / 0) or inf (x / 0): such
    entries are not hidden and show up in info.nonfinite.  Rows without entries stay empty.  Returns (matrix, ScaleInfo)."""
    if norm not in _ROW_NORMS:
        raise ValueError(f"normalize_rows: unknown norm {norm!r} (one of {', '.join(_ROW_NORMS)})")
    buf = _dev_f64(A.rows)
    reduce(A, config, norm, total=False, out_ptr=buf._c.data)
    return scale(A, config, row=buf._c.data, row_div=True, inplace=inplace)


def pattern_ones(A, config):
    """The indicator matrix of A: its pattern with every value 1.0 (scale with map "one"), made on the device -- what a
    triangle count L o (L L) needs of a weighted graph."""
    return scale(A, config, map="one")[0]


# include/speck_c_api.h: the entries of a tile of the pass that walks them (the reduction's)
SPMV_TILE_ENTRIES = 4096


class SpmvInfo(_Info):
    """speck_spmv_info: what the matrix-vector product walked."""
    _fields = ("rows_empty", "rows_split", "tiles", "entries")


def spmv(A, x, config, alpha=1.0, beta=0.0, y=None):
    """y = alpha A x + beta y on a device matrix (speck_spmv_f64 / _f32).  x (A.cols float64, indexed by the column id) and
    y (A.rows float64, indexed by the row inside A: for a row_view pass the slice) are device vectors -- a device address
    or an object with data_ptr(), e.g. a torch tensor -- float64 for both value types.  Every term a x[j] and every sum is
    rounded on its own; the row sums come from the tree of reduce(A, "sum"): bit-reproducible, a row_view gives the rows
    of the whole matrix bit for bit, and for float64 spmv(A, x) equals reduce(scale(A, col=x), "sum") bit for bit.
    beta == 0 does not read y (a NaN in it does not survive); alpha is always applied; a NaN or 0 * inf lands in exactly the
    rows that reference it.  Rows need not be sorted, duplicates add.  y=None is allowed only with beta == 0: the result is
    then a numpy array downloaded from a buffer of the library's allocator.  config may be None.
    Returns (that array, or None where y was given and holds the result on the device, SpmvInfo)."""
    if y is None and float(beta) != 0.0:
        raise ValueError("spmv: beta != 0 needs a y to read")
    x_ptr = _device_vector(x, A.cols, "x", "spmv")
    y_ptr = _device_vector(y, A.rows, "y", "spmv")
    L = _lib.load()
    fn = L.speck_spmv_f32 if A.dtype == np.float32 else L.speck_spmv_f64
    buf = None
    if y is None:
        buf = _dev_f64(A.rows)
        y_ptr = buf._c.data
    info = _lib.CSpmvInfo()
    _check(fn(config._h if config is not None else None, float(alpha), C.byref(A._c), x_ptr, float(beta), y_ptr,
              C.byref(info)), "spmv")
    return (_download_f64(buf, A.rows, "spmv") if buf is not None else None), SpmvInfo(info)


# include/speck_c_api.h: the most right-hand sides one call takes
SPMM_MAX_RHS = 1024
# ... and the columns a tile takes per round (SPECK_SPMM_COLUMN_BLOCK; SPECK_SPMM_COLUMN_BLOCK_B32 with float blocks)
SPMM_COLUMN_BLOCK = 4
SPMM_COLUMN_BLOCK_B32 = 4
# the element types of the dense blocks of spmm, spmm_t and sddmm (the keyword `blocks`): numpy's type, torch's names
_BLOCK_TYPES = {"float64": (np.float64, ("torch.float64", "float64")), "float32": (np.float32, ("torch.float32", "float32"))}


def _block_type(blocks, op):
    """the name of a block type as the keyword `blocks` takes it; anything else is refused"""
    if not isinstance(blocks, str) or blocks not in _BLOCK_TYPES:
        raise ValueError(f"{op}: blocks must be 'float64' or 'float32', not {blocks!r}")
    return blocks


def _dev_block_buffer(n, blocks):
    """a device buffer of n block elements from the library's allocator"""
    d = dCSR(_BLOCK_TYPES[blocks][0])     # (as _dev_f64: the data array of a dCSR without rows)
    d.alloc(0, 0, max(int(n), 1), allocOffsets=False)
    return d


def _download_block(buf, n, who, blocks):
    """the first n elements of a _dev_block_buffer as a numpy array of the block type"""
    dtype = np.dtype(_BLOCK_TYPES[blocks][0])
    out = np.zeros(max(int(n), 1), dtype=dtype)
    _check(_lib.load().speck_dcsr_download(C.byref(buf._c), None, None, out.ctypes.data, dtype.itemsize), f"{who}: download")
    return out[:n]


class SpmmInfo(_Info):
    """speck_spmm_info: what the product with several right-hand sides walked (A's counts, and terms = entries * k)."""
    _fields = ("rows_empty", "rows_split", "tiles", "entries", "terms")


def _device_block(v, n, k, ld, what, op="spmm", blocks="float64"):
    """(address, k, ld) of a row-major n x k block of `blocks` elements: a device address with k and ld given, or a 2-D
    object with data_ptr(), shape, stride() and dtype (a torch tensor, a column slice of one) checked -- a tensor of
    another type is refused, never converted"""
    who = f"{op}: {what}"
    if hasattr(v, "data_ptr"):
        if not all(hasattr(v, a) for a in ("shape", "stride", "dtype")):
            raise ValueError(f"{who} must have shape, stride() and dtype beside data_ptr()")
        if str(v.dtype) not in _BLOCK_TYPES[blocks][1]:
            raise ValueError(f"{who} must be {blocks}, not {v.dtype}")
        shape = tuple(int(d) for d in v.shape)
        if len(shape) != 2 or shape[0] != n or (k is not None and shape[1] != int(k)):
            raise ValueError(f"{who} has shape {shape}, the call asks for ({n}, {'k' if k is None else int(k)})")
        k = shape[1]
        s0, s1 = int(v.stride(0)), int(v.stride(1))
        if k > 1 and s1 != 1:
            raise ValueError(f"{who} must be row-major (stride(1) == 1), not stride {s1}")
        if n > 1 and s0 < k:
            raise ValueError(f"{who} has rows {s0} apart, fewer than its {k} columns")
        if ld is not None and n > 1 and int(ld) != s0:
            raise ValueError(f"{who} has rows {s0} apart, not ld = {int(ld)}")
        return int(v.data_ptr()), k, max(s0, k) if n > 1 else (k if ld is None else int(ld))
    if isinstance(v, (bool, float)) or not hasattr(v, "__index__"):
        raise ValueError(f"{who} must be a 2-D {blocks} device tensor or a device address, not {type(v).__name__}")
    if k is None:
        raise ValueError(f"{who} is a device address: k must be given")
    return int(v), int(k), int(k) if ld is None else int(ld)


def spmm(A, X, config, alpha=1.0, beta=0.0, Y=None, k=None, ldx=None, ldy=None, blocks="float64"):
    """Y = alpha A X + beta Y on a device matrix with k right-hand sides (speck_spmm_f64 / _f32).  X (A.cols x k) and Y
    (A.rows x k, indexed by the row inside A: for a row_view pass the slice) are row-major device blocks of float64 for both
    value types: a 2-D object with data_ptr(), shape, stride() and dtype -- a torch tensor or a column slice Z[:, a:b] of
    one, with stride(1) == 1 and stride(0) >= k -- or a device address with k (and ldx / ldy, default k) given.  A is read
    once for all columns; column c of Y is bit for bit spmv(A, X[:, c], ..., y=Y[:, c]) on contiguous copies, so all that
    spmv promises holds per column; the padding between the rows of Y is neither read nor written.  The memory X spans
    and the memory Y spans must not overlap (two column slices of one tensor do and are refused).  Y=None is allowed only
    with beta == 0: the result is then a (rows, k) numpy array downloaded from a buffer of the library's allocator.
    blocks="float32" (speck_spmm_f64_b32 / _f32_b32): X and Y are float32 blocks, ldx and ldy count floats, and the result is
    bit for bit the float64 call's on X.double(), Y.double(), rounded to float32 once; a float64 tensor is then refused as a
    float32 one is by default -- a block is never converted.  config may be None.
    Returns (that array, or None where Y was given and holds the result on the device, SpmmInfo)."""
    blocks = _block_type(blocks, "spmm")
    if Y is None and float(beta) != 0.0:
        raise ValueError("spmm: beta != 0 needs a Y to read")
    x_ptr, k, ldx = _device_block(X, A.cols, k, ldx, "X", blocks=blocks)
    if Y is not None:
        y_ptr, _, ldy = _device_block(Y, A.rows, k, ldy, "Y", blocks=blocks)
    if k < 0 or ldx < k or (Y is not None and ldy < k):
        raise ValueError(f"spmm: k = {k} with ldx = {ldx}, ldy = {ldy}: a leading dimension is at least k >= 0")
    L = _lib.load()
    if blocks == "float32":
        fn = L.speck_spmm_f32_b32 if A.dtype == np.float32 else L.speck_spmm_f64_b32
    else:
        fn = L.speck_spmm_f32 if A.dtype == np.float32 else L.speck_spmm_f64
    buf = None
    if Y is None:
        buf = _dev_block_buffer(A.rows * k, blocks)
        y_ptr, ldy = buf._c.data, k
    info = _lib.CSpmmInfo()
    _check(fn(config._h if config is not None else None, float(alpha), C.byref(A._c), x_ptr, ldx, k, float(beta), y_ptr, ldy,
              C.byref(info)), "spmm")
    return (_download_block(buf, A.rows * k, "spmm", blocks).reshape(A.rows, k) if buf is not None else None), SpmmInfo(info)


# include/speck_c_api.h: SPECK_SR_*
SR_MIN_PLUS, SR_MAX_PLUS, SR_MIN_TIMES, SR_MAX_TIMES, SR_MIN_SECOND, SR_MAX_SECOND = range(6)
SEMIRINGS = {"min_plus": SR_MIN_PLUS, "max_plus": SR_MAX_PLUS, "min_times": SR_MIN_TIMES, "max_times": SR_MAX_TIMES,
             "min_second": SR_MIN_SECOND, "max_second": SR_MAX_SECOND}


class SemiringInfo(_Info):
    """speck_semiring_info: A's counts as SpmmInfo has them, terms = entries * k, and changed: the elements of the result
    that differ from z (0 without a z)."""
    _fields = ("rows_empty", "rows_split", "tiles", "entries", "terms", "changed")


def _semiring(semiring, op):
    if isinstance(semiring, str):
        if semiring not in SEMIRINGS:
            raise ValueError(f"{op}: unknown semiring {semiring!r} (one of {', '.join(SEMIRINGS)})")
        return SEMIRINGS[semiring]
    if isinstance(semiring, (bool, float)) or not hasattr(semiring, "__index__") or int(semiring) not in SEMIRINGS.values():
        raise ValueError(f"{op}: unknown semiring {semiring!r}")
    return int(semiring)


def spmv_sr(A, x, config, semiring="min_plus", z=None, y=None):
    """y = [z (+)] A (x) x over a semiring on a device matrix (speck_spmv_sr_f64 / _f32): s_i = (+) over the entries (i, j) of
    a_ij (x) x[j], where (+) is min or max and (x) is a + x[j] ("plus"), a * x[j] ("times") or x[j] alone ("second": A's
    values are never read).  semiring is "min_plus", "max_plus", "min_times", "max_times", "min_second" or "max_second" (or
    its SR_* number).  y = s without z, y = z (+) s with one; a row without entries has s_i = +inf (min) or -inf (max).
    x (A.cols), z and y (A.rows, indexed by the row inside A) are float64 device vectors as spmv takes them.  z may be x (a
    relaxation step between two buffers) or y (in place); y may not overlap x.  min and max are exact and propagate a NaN:
    the result equals numpy's minimum / maximum.reduceat in value, NaN where that has one, from run to run and on a
    row_view.  info.changed counts the elements with y != z (NaN equal to NaN): a loop ends on it without a download.
    y=None: the result is a numpy array downloaded from a buffer of the library's allocator.  config may be None.
    Returns (that array, or None where y was given and holds the result on the device, SemiringInfo)."""
    sr = _semiring(semiring, "spmv_sr")
    x_ptr = _device_vector(x, A.cols, "x", "spmv_sr")
    z_ptr = _device_vector(z, A.rows, "z", "spmv_sr")
    y_ptr = _device_vector(y, A.rows, "y", "spmv_sr")
    L = _lib.load()
    fn = L.speck_spmv_sr_f32 if A.dtype == np.float32 else L.speck_spmv_sr_f64
    buf = None
    if y is None:
        buf = _dev_f64(A.rows)
        y_ptr = buf._c.data
    info = _lib.CSemiringInfo()
    _check(fn(config._h if config is not None else None, sr, C.byref(A._c), x_ptr, z_ptr, y_ptr, C.byref(info)), "spmv_sr")
    return (_download_f64(buf, A.rows, "spmv_sr") if buf is not None else None), SemiringInfo(info)


def spmm_sr(A, X, config, semiring="min_plus", Z=None, Y=None, k=None, ldx=None, ldz=None, ldy=None):
    """Y = [Z (+)] A (x) X over a semiring with k right-hand sides (speck_spmm_sr_f64 / _f32): spmv_sr per column, A read once
    for all of them.  X (A.cols x k), Z and Y (A.rows x k) are row-major float64 device blocks as spmm takes them: a 2-D
    object with data_ptr(), shape, stride() and dtype, or a device address with k (and ldx / ldz / ldy, default k).  Column
    c equals spmv_sr on contiguous copies of column c; the padding between the rows of Y is neither read nor written.  Z
    may be X, or Y with the same leading dimension (in place); the memory Y spans may not overlap what X spans (two
    column slices of one tensor do and are refused).  Y=None: the result is a (rows, k) numpy array.  config may be None.
    Returns (that array, or None where Y was given and holds the result on the device, SemiringInfo)."""
    sr = _semiring(semiring, "spmm_sr")
    x_ptr, k, ldx = _device_block(X, A.cols, k, ldx, "X", op="spmm_sr")
    z_ptr, ldz_ = None, k
    if Z is not None:
        z_ptr, _, ldz_ = _device_block(Z, A.rows, k, ldz, "Z", op="spmm_sr")
    if Y is not None:
        y_ptr, _, ldy = _device_block(Y, A.rows, k, ldy, "Y", op="spmm_sr")
    if k < 0 or ldx < k or ldz_ < k or (Y is not None and ldy < k):
        raise ValueError(f"spmm_sr: k = {k} with ldx = {ldx}, ldz = {ldz_}, ldy = {ldy}: a leading dimension is at least k >= 0")
    L = _lib.load()
    fn = L.speck_spmm_sr_f32 if A.dtype == np.float32 else L.speck_spmm_sr_f64
    buf = None
    if Y is None:
        buf = _dev_f64(A.rows * k)
        y_ptr, ldy = buf._c.data, k
    info = _lib.CSemiringInfo()
    _check(fn(config._h if config is not None else None, sr, C.byref(A._c), x_ptr, ldx, k, z_ptr, ldz_, y_ptr, ldy, C.byref(info)),
           "spmm_sr")
    return (_download_f64(buf, A.rows * k, "spmm_sr").reshape(A.rows, k) if buf is not None else None), SemiringInfo(info)


class TplanInfo(_Info):
    """speck_tplan_info: the matrix a transpose plan was made from, its empty and longest columns, the plan's device bytes."""
    _fields = ("rows", "cols", "nnz", "cols_empty", "max_col_entries", "bytes")


class SpmmTInfo(_Info):
    """speck_spmm_t_info: what the transposed product walked (the counts of A's columns, and terms = entries * k)."""
    _fields = ("cols_empty", "cols_split", "tiles", "entries", "terms")


class TransposePlan:
    """speck_tplan: the pattern of a device matrix sorted by column once (speck_tplan_create), for any number of spmm_t /
    spmv_t calls on matrices with that pattern -- the values may change between them, the plan is verified in every call.
    `info` is a TplanInfo.  free() releases the device buffers (also at the end of a `with` block, and with the object);
    a freed plan raises SpeckError where it is used."""

    def __init__(self, A, config=None):
        self._h = C.c_void_p()
        info = _lib.CTplanInfo()
        _check(_lib.load().speck_tplan_create(config._h if config is not None else None, C.byref(A._c), C.byref(self._h),
                                              C.byref(info)), "transpose_plan")
        self.info = TplanInfo(info)

    def _handle(self, who):
        if not self._h:
            raise SpeckError(1, f"{who}: the plan was freed")
        return self._h

    def free(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            _check(_lib.load().speck_tplan_destroy(h), "TransposePlan.free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def transpose_plan(A, config=None):
    """The TransposePlan of A's pattern (A's values are not read).  The creation checks A -- offsets, every column id --
    before it follows anything; unsound input raises SpeckError (SPECK_ERR_INVALID)."""
    return TransposePlan(A, config)


def spmm_t(A, X, config, plan=None, alpha=1.0, beta=0.0, Y=None, k=None, ldx=None, ldy=None, blocks="float64"):
    """Y = alpha A^T X + beta Y on a device matrix through a TransposePlan (speck_spmm_t_f64 / _f32): X is A.rows x k
    (indexed by the row inside A), Y is A.cols x k, row-major device blocks of float64 passed as spmm takes them.  Column c
    of Y is bit for bit spmm(transpose(A), X, ...)'s, so all that spmm promises holds per column; a row_view gives the
    partial sum of its rows.  The plan is verified against A in every call: another pattern raises SpeckError
    (SPECK_ERR_INVALID) with nothing of Y written.  plan=None builds a plan for this one call and frees it -- a training
    loop makes one with transpose_plan(A) and keeps it.  Y=None is allowed only with beta == 0: the result is then a
    (cols, k) numpy array.  blocks="float32" (speck_spmm_t_f64_b32 / _f32_b32): X and Y are float32 blocks as spmm takes
    them, the result bit for bit the float64 call's with the same plan rounded to float32 once; one plan serves both.
    config may be None.  Returns (that array, or None where Y was given, SpmmTInfo)."""
    return _spmm_t("spmm_t", A, X, config, plan, alpha, beta, Y, k, ldx, ldy, _block_type(blocks, "spmm_t"))


def _spmm_t(who, A, X, config, plan, alpha, beta, Y, k, ldx, ldy, blocks="float64"):
    if Y is None and float(beta) != 0.0:
        raise ValueError(f"{who}: beta != 0 needs a Y to read")
    if plan is not None and not isinstance(plan, TransposePlan):
        raise ValueError(f"{who}: plan must be a TransposePlan, not {type(plan).__name__}")
    x_ptr, k, ldx = _device_block(X, A.rows, k, ldx, "X", who, blocks)
    if Y is not None:
        y_ptr, _, ldy = _device_block(Y, A.cols, k, ldy, "Y", who, blocks)
    if k < 0 or ldx < k or (Y is not None and ldy < k):
        raise ValueError(f"{who}: k = {k} with ldx = {ldx}, ldy = {ldy}: a leading dimension is at least k >= 0")
    L = _lib.load()
    if blocks == "float32":
        fn = L.speck_spmm_t_f32_b32 if A.dtype == np.float32 else L.speck_spmm_t_f64_b32
    else:
        fn = L.speck_spmm_t_f32 if A.dtype == np.float32 else L.speck_spmm_t_f64
    own = None
    if plan is None:
        plan = own = TransposePlan(A, config)
    try:
        handle = plan._handle(who)
        buf = None
        if Y is None:
            buf = _dev_block_buffer(A.cols * k, blocks)
            y_ptr, ldy = buf._c.data, k
        info = _lib.CSpmmTInfo()
        _check(fn(config._h if config is not None else None, handle, float(alpha), C.byref(A._c), x_ptr, ldx, k, float(beta),
                  y_ptr, ldy, C.byref(info)), who)
    finally:
        if own is not None:
            own.free()
    return (_download_block(buf, A.cols * k, who, blocks).reshape(A.cols, k) if buf is not None else None), SpmmTInfo(info)


def spmv_t(A, x, config, plan=None, alpha=1.0, beta=0.0, y=None):
    """y = alpha A^T x + beta y: spmm_t with k = 1 and ld = 1.  x (A.rows float64) and y (A.cols float64) are device vectors
    as spmv takes them.  Returns (a numpy array of A.cols values, or None where y was given, SpmmTInfo)."""
    if y is None and float(beta) != 0.0:
        raise ValueError("spmv_t: beta != 0 needs a y to read")
    x_ptr = _device_vector(x, A.rows, "x", "spmv_t")
    y_ptr = _device_vector(y, A.cols, "y", "spmv_t")
    out, info = _spmm_t("spmv_t", A, x_ptr if x_ptr is not None else 0, config, plan, alpha, beta, y_ptr, 1, 1, 1)
    return (out.reshape(A.cols) if out is not None else None), info


# include/speck_c_api.h: SPECK_COO_TILE_ENTRIES (the entries of a tile of from_coo's check pass); the limit on rows and cols
COO_TILE_ENTRIES = 2048
_DIM_MAX = 1 << 27
_ID_BYTES = {"torch.int64": 8, "int64": 8, "torch.int32": 4, "int32": 4}
_VALUE_TYPES = {"torch.float64": np.float64, "float64": np.float64, "torch.float32": np.float32, "float32": np.float32}


class FromCooInfo(_Info):
    """speck_from_coo_info: the entries grouped, the empty and the longest row, whether the row ids came in order (then
    nothing was sorted) and the radix passes that ran."""
    _fields = ("entries", "rows_empty", "max_row_entries", "sorted_input", "sort_passes")


def _coo_array(v, what, who, types, nnz, width):
    """What from_coo needs of one of its arrays, checked WITHOUT asking for its address: (object or address, entries, bytes per
    entry or the value type).  A 1-D tensor of one of `types` with unit stride, or a device address with nnz and `width`."""
    if hasattr(v, "data_ptr"):
        kind = types.get(str(getattr(v, "dtype", None)))
        if kind is None:
            raise ValueError(f"{who}: {what} must be {' or '.join(t for t in types if '.' not in t)}, not {getattr(v, 'dtype', None)}")
        if len(v.shape) != 1:
            raise ValueError(f"{who}: {what} must have one dimension, not {len(v.shape)}")
        if v.shape[0] > 1 and v.stride(0) != 1:
            raise ValueError(f"{who}: {what} must be contiguous (stride {v.stride(0)})")
        return v, int(v.shape[0]), kind
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {what} must be a tensor or a device address, not {type(v).__name__}")
    if nnz is None or width is None:
        raise ValueError(f"{who}: {what} is an address: pass nnz and {'index_bytes' if types is _ID_BYTES else 'dtype'}")
    return int(v), int(nnz), width


def _address(v):
    return int(v.data_ptr()) if hasattr(v, "data_ptr") else v


def _coo_shape(shape, who):
    try:
        rows, cols = (int(x) for x in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: shape must be (rows, cols), not {shape!r}") from None
    if not (0 <= rows <= _DIM_MAX and 0 <= cols <= _DIM_MAX):
        raise ValueError(f"{who}: shape {(rows, cols)} is beyond the limit of {_DIM_MAX} rows and columns")
    return rows, cols


def from_coo(row, col, val, shape, config, dtype=None, canonical=False, sum_duplicates=False, matOut=None, nnz=None,
             index_bytes=None, who="from_coo"):
    """Device COO triplets grouped by row into a device CSR (speck_from_coo_f64 / _f32), stable: row i holds the triplets with
    row id i in input order, bit for bit.  row and col are 1-D int64 or int32 tensors of one type (anything with data_ptr(),
    shape, dtype and stride()), or device addresses with nnz and index_bytes (4: uint32, 8: int64); val is a float64 or
    float32 tensor, an address with dtype, or None: every value is 1.0 in `dtype` (float64 by default).  shape is
    (rows, cols).  An id out of range -- negative, >= its limit, an int64 beyond 32 bits -- raises SpeckError
    (SPECK_ERR_INVALID) with matOut untouched.  Rows are not sorted by column and duplicates stay: canonical=True calls
    sort_rows on the result, sum_duplicates=True (which implies it) merges equal columns.  config may be None.
    Returns (matOut, FromCooInfo)."""
    rows, cols = _coo_shape(shape, who)
    r, n_r, w_r = _coo_array(row, "row", who, _ID_BYTES, nnz, index_bytes)
    c, n_c, w_c = _coo_array(col, "col", who, _ID_BYTES, nnz, index_bytes)
    if w_r != w_c or w_r not in (4, 8):
        raise ValueError(f"{who}: row and col must hold ids of one width, 4 or 8 bytes (got {w_r} and {w_c})")
    if n_r != n_c:
        raise ValueError(f"{who}: row holds {n_r} ids, col {n_c}")
    want = None
    if dtype is not None:
        try:
            want = _VALUE_TYPES.get(str(dtype)) or np.dtype(dtype).type
        except TypeError:
            pass
        if want not in (np.float64, np.float32):
            raise ValueError(f"{who}: dtype must be float64 or float32, not {dtype}")
    v = None
    if val is not None:
        v, n_v, vt = _coo_array(val, "val", who, _VALUE_TYPES, n_r, want if want is not None else np.float64)
        if n_v != n_r:
            raise ValueError(f"{who}: val holds {n_v} values for {n_r} ids")
        if want is not None and vt is not want:
            raise ValueError(f"{who}: val is {np.dtype(vt)}, dtype asks for {np.dtype(want)}")
        want = vt
    vtype = np.dtype(want if want is not None else np.float64)
    if n_r >= 1 << 32:
        raise ValueError(f"{who}: {n_r} entries; the limit is 2^32 - 1")
    # ---- everything was checked: the addresses
    coo = _lib.CDcoo()
    coo.rows, coo.cols, coo.nnz, coo.index_bytes = rows, cols, n_r, w_r
    coo.row_ids, coo.col_ids, coo.data = _address(r), _address(c), (_address(v) if v is not None else None)
    L = _lib.load()
    fn = L.speck_from_coo_f32 if vtype == np.float32 else L.speck_from_coo_f64
    if matOut is None:
        matOut = dCSR(vtype)
    if matOut.dtype != vtype:
        matOut.reset()
        matOut.dtype = vtype
    info = _lib.CFromCooInfo()
    _check(fn(config._h if config is not None else None, C.byref(coo), C.byref(matOut._c), C.byref(info)), who)
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    if canonical or sum_duplicates:
        sort_rows(matOut, config, sum_duplicates=sum_duplicates)
    return matOut, FromCooInfo(info)


def from_edge_index(edge_index, val, shape, config, dtype=None, canonical=False, sum_duplicates=False, matOut=None):
    """from_coo on a 2 x E int64 (or int32) tensor as graph libraries keep it: row 0 holds the row ids, row 1 the column ids.
    The entries of a row must be adjacent (stride(1) == 1); the two rows may lie anywhere (any stride(0)): their two addresses
    are passed, nothing is copied.  The other arguments and the result are from_coo's."""
    who = "from_edge_index"
    if not hasattr(edge_index, "data_ptr") or not hasattr(edge_index, "shape"):
        raise ValueError(f"{who}: edge_index must be a tensor, not {type(edge_index).__name__}")
    width = _ID_BYTES.get(str(getattr(edge_index, "dtype", None)))
    if width is None:
        raise ValueError(f"{who}: edge_index must be int64 or int32, not {getattr(edge_index, 'dtype', None)}")
    if len(edge_index.shape) != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{who}: edge_index must be 2 x E, not {tuple(edge_index.shape)}")
    n = int(edge_index.shape[1])
    if n > 1 and edge_index.stride(1) != 1:
        raise ValueError(f"{who}: edge_index must hold the ids of a row side by side (stride(1) == 1, not {edge_index.stride(1)})")
    _coo_shape(shape, who)
    if val is not None and hasattr(val, "data_ptr"):
        _coo_array(val, "val", who, _VALUE_TYPES, n, None)  # (refused before edge_index is asked for its address)
    step = int(edge_index.stride(0)) * width
    if step < 0:
        raise ValueError(f"{who}: edge_index has a negative stride")
    base = int(edge_index.data_ptr())
    return from_coo(base, base + step, val, shape, config, dtype=dtype, canonical=canonical, sum_duplicates=sum_duplicates,
                    matOut=matOut, nnz=n, index_bytes=width, who=who)


def to_coo(A, config, index_dtype=None, cols=True, row_base=0):
    """The row index of every entry of a device matrix, as torch tensors on A's device (speck_to_coo): entry e of row i inside
    A gets row_base + i.  index_dtype is torch.int64 (the default) or torch.int32; cols=True also returns the column ids
    widened to it.  Values are not touched: they are A's data from its first entry on.  A may be a row_view; row_base is the
    global index of its first row.  Unsound offsets, or with cols=True an id >= A.cols, raise SpeckError (SPECK_ERR_INVALID).
    config may be None.  Returns (row, col), col None where cols=False."""
    import torch
    index_dtype = torch.int64 if index_dtype is None else index_dtype
    if index_dtype not in (torch.int64, torch.int32):
        raise ValueError(f"to_coo: index_dtype must be torch.int64 or torch.int32, not {index_dtype}")
    row_base = int(row_base)
    limit = (1 << 63) if index_dtype is torch.int64 else (1 << 31)
    if row_base < 0 or row_base + A.rows > limit:
        raise ValueError(f"to_coo: row_base {row_base} + {A.rows} rows does not fit {index_dtype}")
    device = torch.device("cuda", config.device) if config is not None else torch.device("cuda")
    # (one index at least: a tensor without elements has no address, and the call wants one even where it writes nothing)
    row = torch.empty(max(A.nnz, 1), dtype=index_dtype, device=device)
    col = torch.empty(max(A.nnz, 1), dtype=index_dtype, device=device) if cols else None
    _check(_lib.load().speck_to_coo(config._h if config is not None else None, C.byref(A._c), 8 if index_dtype is torch.int64 else 4,
                                    row_base, row.data_ptr(), col.data_ptr() if cols else None), "to_coo")
    return row[:A.nnz], (col[:A.nnz] if cols else None)


# include/speck_c_api.h: SPECK_EXTRACT_TILE_ENTRIES (the gathered entries of a tile of extract's marking and placing passes)
EXTRACT_TILE_ENTRIES = 4096


class ExtractInfo(_Info):
    """speck_extract_info: the rows of the result and the empty ones among them, the entries of the gathered rows before
    the drop, the entries kept and dropped, the map entries that keep their column, and the longest row."""
    _fields = ("rows_out", "rows_empty", "gross", "nnz_out", "dropped", "cols_kept", "max_row_entries")


def _index_array(v, what, who, count, width):
    """An index list or a column map of extract, checked WITHOUT asking for its address: (object or address, entries, bytes per
    entry).  A 1-D int64 or int32 tensor with unit stride, or a device address with its count and index_bytes."""
    if not hasattr(v, "data_ptr") and not isinstance(v, bool) and isinstance(v, (int, np.integer)) and (count is None or width is None):
        raise ValueError(f"{who}: {what} is an address: pass {'n_rows and ' if what == 'rows' else ''}index_bytes")
    return _coo_array(v, what, who, _ID_BYTES, count, width)


def extract(A, rows=None, col_map=None, out_cols=None, config=None, matOut=None, canonical=False, sum_duplicates=False,
            n_rows=None, index_bytes=None, who="extract"):
    """C = A(rows, col_map) (speck_extract_f64 / _f32): row i of C is row rows[i] of the device matrix A -- any order,
    repeats allowed, None: every row in order -- without the entries whose column the map drops, in input order, every column
    id j replaced by col_map[j], every value copied bit for bit.  col_map holds A.cols entries: the new id, or "dropped"
    (int64: any negative value; int32: -1); it need be neither injective nor monotone; None: identity.  rows and col_map are
    1-D int64 or int32 tensors of one type (anything with data_ptr(), shape, dtype and stride()), or device addresses with
    index_bytes (4: uint32, 8: int64) and, for rows, n_rows.  out_cols is C.cols: A.cols without a map, required with one.
    An index >= A.rows, a map value >= out_cols, an id >= A.cols in a gathered row raise SpeckError (SPECK_ERR_INVALID) with
    matOut untouched.  Nothing is sorted and duplicates stay: canonical=True calls sort_rows on the result,
    sum_duplicates=True (which implies it) merges equal columns.  config may be None.  Returns (matOut, ExtractInfo)."""
    r = m = None
    w_r = w_m = None
    n = A.rows
    if rows is not None:
        r, n, w_r = _index_array(rows, "rows", who, n_rows, index_bytes)
    if col_map is not None:
        m, n_m, w_m = _index_array(col_map, "col_map", who, A.cols, index_bytes)
        if n_m != A.cols:
            raise ValueError(f"{who}: col_map holds {n_m} entries for {A.cols} columns")
        if out_cols is None:
            raise ValueError(f"{who}: out_cols is required with a col_map")
    if w_r is not None and w_m is not None and w_r != w_m:
        raise ValueError(f"{who}: rows and col_map must hold ids of one width (got {w_r} and {w_m} bytes)")
    width = w_r if w_r is not None else w_m if w_m is not None else 8
    if width not in (4, 8):
        raise ValueError(f"{who}: index_bytes must be 4 or 8, not {width}")
    out_cols = A.cols if out_cols is None else int(out_cols)
    if not (0 <= out_cols <= _DIM_MAX and 0 <= n <= _DIM_MAX):
        raise ValueError(f"{who}: {n} rows x {out_cols} columns is beyond the limit of {_DIM_MAX} rows and columns")
    # ---- everything was checked: the addresses
    p = _lib.CExtractParams()
    p.n_rows, p.out_cols, p.index_bytes = n, out_cols, width
    p.d_row_index = _address(r) if r is not None else None
    p.d_col_map = _address(m) if m is not None else None
    L = _lib.load()
    fn = L.speck_extract_f32 if A.dtype == np.float32 else L.speck_extract_f64
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    info = _lib.CExtractInfo()
    _check(fn(config._h if config is not None else None, C.byref(A._c), C.byref(p), C.byref(matOut._c), C.byref(info)), who)
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    if canonical or sum_duplicates:
        sort_rows(matOut, config, sum_duplicates=sum_duplicates)
    return matOut, ExtractInfo(info)


def _inverse_map(ids, limit, who, what):
    """The column map that sends ids[j] to j and drops every other column below `limit`, as a tensor of ids' type: ONE
    scatter (plumbing; the C call takes the map, it does not build it).  ids: a 1-D int64 or int32 device tensor without
    repeats, every id in [0, limit)."""
    import torch
    _coo_array(ids, what, who, _ID_BYTES, None, None)
    if not isinstance(ids, torch.Tensor):
        raise ValueError(f"{who}: {what} must be a torch tensor (the map is built with torch)")
    k = int(ids.shape[0])
    pos = torch.arange(k, dtype=ids.dtype, device=ids.device)
    if k and bool(((ids < 0) | (ids >= limit)).any()):
        raise ValueError(f"{who}: {what} holds an id outside [0, {limit})")
    cmap = torch.full((limit,), -1, dtype=ids.dtype, device=ids.device)
    at = ids.long()
    cmap[at] = pos
    if k and not bool((cmap[at] == pos).all()):      # a repeated id kept one of its positions, the other differs
        raise ValueError(f"{who}: {what} holds an id more than once")
    return cmap, k


def gather_rows(A, rows, config=None, matOut=None):
    """The rows of A the index list names, in its order, repeats allowed (scipy's A[rows]); the columns stay.  extract's
    arguments and result."""
    return extract(A, rows=rows, config=config, matOut=matOut, who="gather_rows")


def select_columns(A, cols, config=None, matOut=None, canonical=False):
    """scipy's A[:, cols] for a list without repeats (a repeated id is a ValueError): column cols[j] becomes column j, every
    other column is dropped.  The entries of a row keep their input order; canonical=True sorts them by their new id."""
    cmap, k = _inverse_map(cols, A.cols, "select_columns", "cols")
    return extract(A, col_map=cmap, out_cols=k, config=config, matOut=matOut, canonical=canonical, who="select_columns")


def induced_subgraph(A, nodes, config=None, matOut=None, canonical=True):
    """A[nodes][:, nodes] with the vertices renumbered 0 .. len(nodes) - 1 in the order of the list, which holds no vertex
    twice: the adjacency of a sampled mini-batch.  canonical=True (the default) sorts the rows, as the multiply wants them."""
    cmap, k = _inverse_map(nodes, A.cols, "induced_subgraph", "nodes")
    return extract(A, rows=nodes, col_map=cmap, out_cols=k, config=config, matOut=matOut, canonical=canonical, who="induced_subgraph")


def permute(A, row_perm=None, col_perm=None, config=None, matOut=None, canonical=False):
    """scipy's A[row_perm][:, col_perm]: row i of the result is row row_perm[i] of A, column j of it column col_perm[j] -- the
    map is the inverse permutation.  None leaves that side as it is; P A P^T is permute(A, perm, perm).  The entries of a row
    keep their input order: canonical=True sorts them by their new id."""
    cmap = None
    if col_perm is not None:
        cmap, k = _inverse_map(col_perm, A.cols, "permute", "col_perm")
        if k != A.cols:
            raise ValueError(f"permute: col_perm holds {k} ids for {A.cols} columns")
    if row_perm is not None and _coo_array(row_perm, "row_perm", "permute", _ID_BYTES, None, None)[1] != A.rows:
        raise ValueError(f"permute: row_perm holds {row_perm.shape[0]} ids for {A.rows} rows")
    return extract(A, rows=row_perm, col_map=cmap, out_cols=A.cols, config=config, matOut=matOut, canonical=canonical, who="permute")


# include/speck_c_api.h: SPECK_BMAT_TILE_ENTRIES (the output entries of a tile of bmat's id check and placing pass),
# SPECK_BMAT_MAX_BLOCKS (the cells a grid may name)
BMAT_TILE_ENTRIES = 4096
BMAT_MAX_BLOCKS = 65536


class BmatInfo(_Info):
    """speck_bmat_info: the blocks, the shape and the entries of the result, its pieces -- (output row, block of its block
    row) pairs --, its rows without an entry and its longest row."""
    _fields = ("blocks", "rows_out", "cols_out", "nnz_out", "pieces", "rows_empty", "max_row_entries")


class BmatLayout:
    """speck_bmat_layout_out: the shape, the entries and the pieces of a grid's result, and the origins of its block rows
    and block columns (block_rows + 1 / block_cols + 1 ints: line g covers [origins[g], origins[g + 1]))."""

    def __init__(self, rows, cols, nnz, pieces, row_origins, col_origins):
        self.rows, self.cols, self.nnz, self.pieces = rows, cols, nnz, pieces
        self.row_origins, self.col_origins = row_origins, col_origins

    def __repr__(self):
        return f"BmatLayout(rows={self.rows}, cols={self.cols}, nnz={self.nnz}, pieces={self.pieces})"


def _bmat_sizes(sizes, n, what, who):
    if sizes is None:
        return None
    sizes = list(sizes)
    if len(sizes) != n or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 for v in sizes):
        raise ValueError(f"{who}: {what} must hold {n} non-negative integers")
    return [int(v) for v in sizes]


def _bmat_cells(blocks, row_sizes, col_sizes, who):
    """A grid given as a list of lists (None: a zero block) as (cells, block_rows, block_cols): checked without asking
    any cell for an address."""
    if not isinstance(blocks, (list, tuple)) or any(not isinstance(line, (list, tuple)) for line in blocks):
        raise ValueError(f"{who}: blocks must be a list of lists of dCSR or None")
    block_rows = len(blocks)
    block_cols = len(blocks[0]) if block_rows else (len(col_sizes) if col_sizes is not None else 0)
    if any(len(line) != block_cols for line in blocks):
        raise ValueError(f"{who}: blocks is ragged: every block row must name {block_cols} cells")
    cells = []
    for g, line in enumerate(blocks):
        for q, m in enumerate(line):
            if m is None:
                continue
            if not isinstance(m, dCSR):
                raise ValueError(f"{who}: the cell ({g}, {q}) must be a dCSR or None, not {type(m).__name__}")
            cells.append((g, q, m))
    return cells, block_rows, block_cols


def _bmat_params(cells, block_rows, block_cols, row_sizes, col_sizes, who):
    """The checks the wrappers make themselves, then speck_bmat_params with everything it points to: (params, keep, dtype)."""
    row_sizes = _bmat_sizes(row_sizes, block_rows, "row_sizes", who)
    col_sizes = _bmat_sizes(col_sizes, block_cols, "col_sizes", who)
    if len(cells) > BMAT_MAX_BLOCKS:
        raise ValueError(f"{who}: {len(cells)} blocks are beyond the limit of {BMAT_MAX_BLOCKS}")
    dtypes = {m.dtype for _, _, m in cells}
    if len(dtypes) > 1:
        raise TypeError(f"{who}: the blocks hold {sorted(str(d) for d in dtypes)}: blocks of mixed value type are not converted")
    for sizes, n, at, line in ((row_sizes, block_rows, 0, "block row"), (col_sizes, block_cols, 1, "block column")):
        if sizes is None:
            named = {c[at] for c in cells}
            missing = [g for g in range(n) if g not in named]
            if missing:
                raise ValueError(f"{who}: {line} {missing[0]} has neither a block nor a size")
    arr = (_lib.CBmatBlock * max(len(cells), 1))()
    for k, (g, q, m) in enumerate(cells):
        arr[k].block_row, arr[k].block_col, arr[k].M = g, q, C.pointer(m._c)
    p = _lib.CBmatParams()
    p.block_rows, p.block_cols, p.n_blocks = block_rows, block_cols, len(cells)
    p.blocks = arr if cells else None
    rs = (C.c_uint64 * max(block_rows, 1))(*row_sizes) if row_sizes is not None else None
    cs = (C.c_uint64 * max(block_cols, 1))(*col_sizes) if col_sizes is not None else None
    p.row_sizes, p.col_sizes = rs, cs
    return p, (arr, rs, cs, cells), (dtypes.pop() if dtypes else None)


def _bmat_layout(p, who):
    out = _lib.CBmatLayoutOut()
    ro = (C.c_uint64 * (p.block_rows + 1))()
    co = (C.c_uint64 * (p.block_cols + 1))()
    out.row_origins, out.col_origins = ro, co
    _check(_lib.load().speck_bmat_layout(C.byref(p), C.byref(out)), who)
    return BmatLayout(int(out.rows), int(out.cols), int(out.nnz), int(out.pieces), tuple(int(v) for v in ro), tuple(int(v) for v in co))


def bmat_layout(blocks, row_sizes=None, col_sizes=None):
    """What bmat(blocks, ...) would build, from the host alone (speck_bmat_layout: no device, no config): a BmatLayout with the
    shape, nnz, the pieces and the origins of the block rows and block columns."""
    cells, block_rows, block_cols = _bmat_cells(blocks, row_sizes, col_sizes, "bmat_layout")
    p, keep, _ = _bmat_params(cells, block_rows, block_cols, row_sizes, col_sizes, "bmat_layout")
    return _bmat_layout(p, "bmat_layout")


def _bmat_call(cells, block_rows, block_cols, config, row_sizes, col_sizes, matOut, return_info, who, dtype=None, return_offsets=False):
    p, keep, found = _bmat_params(cells, block_rows, block_cols, row_sizes, col_sizes, who)
    if matOut is not None and any(m is matOut for _, _, m in cells):
        raise ValueError(f"{who}: matOut is one of the blocks (there is no in-place form)")
    dtype = found if found is not None else np.dtype(dtype) if dtype is not None else matOut.dtype if matOut is not None else np.dtype(np.float64)
    if dtype not in (np.float32, np.float64):
        raise TypeError(f"{who}: the values must be float32 or float64, not {dtype}")
    L = _lib.load()
    fn = L.speck_bmat_f32 if dtype == np.float32 else L.speck_bmat_f64
    if matOut is None:
        matOut = dCSR(dtype)
    if matOut.dtype != dtype:
        matOut.reset()
        matOut.dtype = np.dtype(dtype)
    info = _lib.CBmatInfo()
    _check(fn(config._h if config is not None else None, C.byref(p), C.byref(matOut._c), C.byref(info)), who)
    matOut._host_row_offsets = None  # (row_offsets were rewritten on the device)
    res = (matOut, BmatInfo(info)) if return_info else (matOut,)
    if return_offsets:
        lay = _bmat_layout(p, who)
        res += (lay.row_origins, lay.col_origins)
    del keep
    return res if len(res) > 1 else res[0]


def bmat(blocks, config, row_sizes=None, col_sizes=None, matOut=None, return_info=False, dtype=None):
    """C = the device matrix assembled from a grid of device matrices (speck_bmat_f64 / _f32; scipy.sparse.bmat without the
    sort): blocks is a list of block rows, each a list of dCSR or None (a zero block).  Row i of block row g of C is the
    concatenation, in ascending block column, of row i of its blocks, each column id shifted by its block column's origin,
    each value copied bit for bit; nothing is sorted, summed or dropped.  A block row's height is row_sizes[g] where
    row_sizes is given, else the common rows of its blocks (columns likewise): a line with neither a block nor a size, a
    ragged grid, a cell that is no dCSR and a matOut that is one of the blocks raise ValueError, blocks of mixed dtype
    TypeError (they are never converted).  A block may be a row_view, one matrix may stand in several cells.  config may be
    None; dtype names the value type of a grid without a block.  Returns matOut, or (matOut, BmatInfo) with return_info."""
    cells, block_rows, block_cols = _bmat_cells(blocks, row_sizes, col_sizes, "bmat")
    return _bmat_call(cells, block_rows, block_cols, config, row_sizes, col_sizes, matOut, return_info, "bmat", dtype)


def _bmat_list(mats, who):
    if not isinstance(mats, (list, tuple)) or any(not isinstance(m, dCSR) for m in mats):
        raise ValueError(f"{who}: mats must be a list of dCSR")
    return list(mats)


def vstack(mats, config, matOut=None, return_info=False):
    """The matrices one below the other (scipy.sparse.vstack): a bmat grid of one column.  They share their cols."""
    mats = _bmat_list(mats, "vstack")
    if not mats:
        raise ValueError("vstack: mats is empty (bmat with row_sizes and col_sizes builds a matrix without a block)")
    return _bmat_call([(g, 0, m) for g, m in enumerate(mats)], len(mats), 1, config, None, None, matOut, return_info, "vstack")


def hstack(mats, config, matOut=None, return_info=False):
    """The matrices side by side (scipy.sparse.hstack, entries of a row in the order of the list): a bmat grid of one row."""
    mats = _bmat_list(mats, "hstack")
    if not mats:
        raise ValueError("hstack: mats is empty (bmat with row_sizes and col_sizes builds a matrix without a block)")
    return _bmat_call([(0, q, m) for q, m in enumerate(mats)], 1, len(mats), config, None, None, matOut, return_info, "hstack")


def block_diag(mats, config, matOut=None, return_info=False, return_offsets=False, dtype=None):
    """block_diag(G_1 .. G_n) (scipy.sparse.block_diag): n descriptors, not n^2 cells.  One matrix of a batch of graphs, or
    the operand of a batched product: block_diag(A_i) block_diag(B_i) = block_diag(A_i B_i).  return_offsets=True also
    returns the row and the column origins (n + 1 ints each, from bmat_layout): graph i owns the rows
    [row_origins[i], row_origins[i + 1]) -- torch.repeat_interleave on their differences is the batch vector."""
    mats = _bmat_list(mats, "block_diag")
    n = len(mats)
    return _bmat_call([(i, i, m) for i, m in enumerate(mats)], n, n, config, [] if n == 0 else None, [] if n == 0 else None, matOut,
                      return_info, "block_diag", dtype, return_offsets)


# include/speck_c_api.h: SPECK_TOPK_*; SPECK_TOPK_GROUP_MAX / SPECK_TOPK_LDS_MAX (rows of more than k entries up to this many:
# ranked by a group of 8 / 16 / 32 / 64 lanes -- up to GROUP_MAX / 8, / 4, / 2, GROUP_MAX entries -- / selected by one
# workgroup with the row's keys in LDS; longer ones are selected from global memory)
TOPK_LARGEST, TOPK_SMALLEST, TOPK_LARGEST_ABS = range(3)
TOPK_MODES = {"largest": TOPK_LARGEST, "smallest": TOPK_SMALLEST, "abs": TOPK_LARGEST_ABS}
TOPK_GROUP_MAX = 256
TOPK_LDS_MAX = 4096


class TopKInfo(_Info):
    """speck_topk_info: the rows, those longer than k, the entries that went in, came out and were dropped, the longest row
    of the result, the rows in which the tie rule decided and the NaN entries of the result."""
    _fields = ("rows", "rows_cut", "entries_in", "nnz_out", "dropped", "max_row_entries", "ties_cut", "nan_kept")


def topk(A, k, by="largest", cfg=None, out=None, return_info=False):
    """C = the k best entries of every row of the device matrix A (speck_topk_f64 / _f32), in input order, ids and values
    bit for bit.  by: "largest" (the key of a value v is v), "smallest" (-v) or "abs" (|v|).  A NaN ranks above every
    number, -0.0 equals +0.0; of equal keys the entry that comes first in the row wins.  A row of at most k entries is kept
    whole, k == 0 gives empty rows, a k of 2^32 or more keeps everything.  cfg may be None; out is the dCSR that takes the
    result (its buffers are reused where their size stays).  Returns out, or (out, TopKInfo) with return_info."""
    if by not in TOPK_MODES:
        raise ValueError(f"topk: by must be one of {sorted(TOPK_MODES)}, not {by!r}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < (1 << 64):
        raise ValueError(f"topk: k must be an integer in [0, 2^64), not {k!r}")
    L = _lib.load()
    p = _lib.CTopKParams()
    p.k, p.mode, p.reserved = int(k), TOPK_MODES[by], 0
    fn = L.speck_topk_f32 if A.dtype == np.float32 else L.speck_topk_f64
    if out is None:
        out = dCSR(A.dtype)
    if out.dtype != A.dtype:
        out.reset()
        out.dtype = A.dtype
    info = _lib.CTopKInfo()
    _check(fn(cfg._h if cfg is not None else None, C.byref(A._c), C.byref(p), C.byref(out._c), C.byref(info)), "topk")
    out._host_row_offsets = None  # (row_offsets were rewritten on the device)
    return (out, TopKInfo(info)) if return_info else out


# include/speck_c_api.h: SPECK_SAMPLE_*; SPECK_SAMPLE_GROUP_MAX / SPECK_SAMPLE_LDS_MAX (cut rows up to this many entries: ranked
# by a group of 8 / 16 / 32 / 64 lanes / selected by one workgroup with the row's keys in LDS; longer ones are selected
# with their keys recomputed in every pass); the gross entries of a tile of the id check and the draws of a tile of mode 1
SAMPLE_WITHOUT_REPLACEMENT, SAMPLE_WITH_REPLACEMENT = range(2)
SAMPLE_GROUP_MAX = 256
SAMPLE_LDS_MAX = 4096
SAMPLE_TILE_ENTRIES = 4096


class SampleInfo(_Info):
    """speck_sample_info: the rows of the result and the empty ones among them, the gathered rows longer than k, the
    entries of the gathered rows, the entries of the result and its longest row."""
    _fields = ("rows_out", "rows_empty", "rows_cut", "gross", "nnz_out", "max_row_entries")


def _sample_call(A, p, cfg):
    """one speck_sample_* call into a new matrix: (dCSR, SampleInfo)"""
    L = _lib.load()
    fn = L.speck_sample_f32 if A.dtype == np.float32 else L.speck_sample_f64
    out = dCSR(A.dtype)
    info = _lib.CSampleInfo()
    _check(fn(cfg._h if cfg is not None else None, C.byref(A._c), C.byref(p), C.byref(out._c), C.byref(info)), "sample_neighbors")
    out._host_row_offsets = None  # (row_offsets were written on the device)
    return out, SampleInfo(info)


def sample_neighbors(A, k, seed, rows=None, replace=False, row_base=0, return_pos=False, cfg=None):
    """Fan-out neighbour sampling (speck_sample_f64 / _f32): row i of the result holds at most k entries of row rows[i] of the
    device matrix A, chosen uniformly at random -- rows is a 1-D int64 or int32 tensor, any order, repeats allowed; None:
    every row in order.  The random key of an entry is a pure function of (seed, row_base + rows[i], place in the row), so
    the sample is the same from run to run, does not depend on values, ids or the value type, and is restated in numpy by
    tests/test_sample_host.py; vary seed per hop or epoch.  replace=False: a row of at most k entries is kept whole, a
    longer one keeps exactly k, in input order (k == 0: empty rows; k >= 2^32: everything).  replace=True: a non-empty
    row gives exactly k entries in draw order, repeats stay.  Ids and values are copied bit for bit.  row_base is the
    global index of A's first row where A is a row_view: the view's sample is then the rows of the whole matrix's sample.
    return_pos=True also returns, per entry of the result, its position in A's data / col_ids (the edge id) as an int64
    tensor: a second call on a matrix that shares A's offsets and ids and whose values are the positions as doubles (exact:
    nnz < 2^32).  An index >= A.rows or an id >= A.cols in a gathered row raise SpeckError (SPECK_ERR_INVALID).  cfg may be
    None.  Returns (C, SampleInfo), or (C, SampleInfo, pos) with return_pos."""
    who = "sample_neighbors"
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < (1 << 64):
        raise ValueError(f"{who}: k must be an integer in [0, 2^64), not {k!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), not {seed!r}")
    if isinstance(row_base, bool) or not isinstance(row_base, (int, np.integer)) or not 0 <= int(row_base) <= (1 << 62):
        raise ValueError(f"{who}: row_base must be an integer in [0, 2^62], not {row_base!r}")
    if not isinstance(replace, (bool, np.bool_)):
        raise ValueError(f"{who}: replace must be True or False, not {replace!r}")
    r, n, width = None, A.rows, 8
    if rows is not None:
        r, n, width = _index_array(rows, "rows", who, None, None)
    if not 0 <= n <= _DIM_MAX:
        raise ValueError(f"{who}: {n} rows are beyond the limit of {_DIM_MAX}")
    # ---- everything was checked: the addresses
    p = _lib.CSampleParams()
    p.k, p.seed, p.row_base, p.n_rows, p.index_bytes = int(k), int(seed), int(row_base), n, width
    p.mode = SAMPLE_WITH_REPLACEMENT if replace else SAMPLE_WITHOUT_REPLACEMENT
    p.d_row_index = _address(r) if r is not None else None
    if r is not None and n == 0 and hasattr(r, "data_ptr"):
        import torch                     # (a tensor without elements has no address, and a NULL index names every row)
        none = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", cfg.device) if cfg is not None else torch.device("cuda"))
        p.d_row_index = none.data_ptr()
    out, info = _sample_call(A, p, cfg)
    if not return_pos:
        return out, info
    import torch
    device = torch.device("cuda", cfg.device) if cfg is not None else torch.device("cuda")
    # The positions count from the start of A's buffers, as the offsets of a row_view do: its entries start at its first offset.
    if A._host_row_offsets is not None and len(A._host_row_offsets):
        base = int(A._host_row_offsets[0])
    elif A.rows and A._c.row_offsets:
        first = np.zeros(1, dtype=np.uint32)
        probe = _lib.DCsr()                  # (no row and one entry: not a view to the download, which then rebases nothing)
        probe.nnz, probe.row_offsets = 1, A._c.row_offsets
        _check(_lib.load().speck_dcsr_download(C.byref(probe), first.ctypes.data, None, None, 8), f"{who}: download")
        base = int(first[0])
    else:
        base = 0
    # (one element at least each: a tensor without elements has no address)
    at = torch.arange(max(base + A.nnz, 1), dtype=torch.float64, device=device)
    torch.cuda.current_stream(device).synchronize()   # (the call reads them on the config's stream)
    twin = dCSR.from_device(A.rows, A.cols, A.nnz, A._c.row_offsets, A._c.col_ids, at.data_ptr(), dtype=np.float64, keep=(A, at))
    # the second result goes into torch tensors: a C of the first result's rows and entries is reused, not re-allocated
    pos = torch.empty(max(out.nnz, 1), dtype=torch.float64, device=device)
    ids = torch.empty(max(out.nnz, 1), dtype=torch.int32, device=device)
    offs = torch.empty(out.rows + 1, dtype=torch.int32, device=device)
    where = dCSR.from_device(out.rows, A.cols, out.nnz, offs.data_ptr(), ids.data_ptr(), pos.data_ptr(), dtype=np.float64,
                             keep=(pos, ids, offs))
    before = (where._c.data, where._c.col_ids, where._c.row_offsets)
    L = _lib.load()
    _check(L.speck_sample_f64(cfg._h if cfg is not None else None, C.byref(twin._c), C.byref(p), C.byref(where._c), None), who)
    if (where._c.data, where._c.col_ids, where._c.row_offsets) != before or where.nnz != out.nnz:
        raise RuntimeError(f"{who}: the call on the positions gave another structure ({where.nnz} entries, not {out.nnz})")
    return out, info, pos[:out.nnz].long()


# include/speck_c_api.h: SPECK_SDDMM_*; the most columns U and V may have, and the entries of a tile of the pass
SDDMM_AXPBY, SDDMM_HADAMARD = range(2)
SDDMM_MODES = {"axpby": SDDMM_AXPBY, "hadamard": SDDMM_HADAMARD}
SDDMM_MAX_K = 1024
SDDMM_TILE_ENTRIES = 4096


def sddmm_lanes(k):
    """L(k) of speck_sddmm_*: the lanes that serve one entry -- min(8, max(1, pow2ceil(ceil(k / 4))))"""
    lanes = 1
    while lanes < 8 and 4 * lanes < k:
        lanes *= 2
    return lanes


class SddmmInfo(_Info):
    """speck_sddmm_info: what the sampled product wrote (terms = entries * k, lanes = L(k))."""
    _fields = ("entries", "terms", "nonfinite", "tiles", "lanes")


def sddmm(A, U, V, config, alpha=1.0, beta=0.0, mode="axpby", matOut=None, inplace=False, k=None, ldu=None, ldv=None,
          blocks="float64"):
    """C = alpha (U V^T) on A's pattern + beta A (speck_sddmm_f64 / _f32): d(i,j) = sum_c U(i,c) V(j,c) only where A holds
    an entry.  mode "hadamard" gives alpha d(i,j) A(i,j) instead (beta must be 0).  U (A.rows x k, indexed by the row inside
    A: for a row_view pass the slice) and V (A.cols x k) are row-major device blocks of float64 for both value types, as
    spmm takes them: a 2-D object with data_ptr(), shape, stride() and dtype, or a device address with k (and ldu / ldv,
    default k) given.  They are only read and may be one block.  Every step in double, the sum over k in a tree that is a
    function of k alone (sddmm_lanes), one rounding to A's value type: the same bits from run to run, in place or not,
    whatever the leading dimensions.  beta == 0 does not read A's values (a NaN there does not survive); a NaN or 0 * inf
    of U or V lands in exactly the entries that reference it and is counted in info.nonfinite.  The gradient of spmm
    with respect to A's values is sddmm(A, dY, X).  inplace=True overwrites A's values (on a row_view: the view's
    entries only); otherwise the result goes to matOut (a new matrix when None) with A's pattern, offsets rebased to 0.
    blocks="float32" (speck_sddmm_f64_b32 / _f32_b32): U and V are float32 blocks, ldu and ldv count floats, and the result
    and the info are bit for bit the float64 call's on U.double(), V.double(); a float64 tensor is then refused as a
    float32 one is by default -- a block is never converted.  config may be None.  Returns (matOut or A, SddmmInfo)."""
    blocks = _block_type(blocks, "sddmm")
    if isinstance(mode, str):
        if mode not in SDDMM_MODES:
            raise ValueError(f"sddmm: unknown mode {mode!r} (one of {', '.join(SDDMM_MODES)})")
        mode = SDDMM_MODES[mode]
    elif mode not in SDDMM_MODES.values():
        raise ValueError(f"sddmm: unknown mode {mode!r}")
    if mode == SDDMM_HADAMARD and float(beta) != 0.0:
        raise ValueError("sddmm: beta must be 0 with mode 'hadamard'")
    if inplace and matOut is not None:
        raise ValueError("sddmm: inplace=True and matOut exclude each other")
    p = _lib.CSddmmParamsB32() if blocks == "float32" else _lib.CSddmmParams()
    p.mode, p.alpha, p.beta = int(mode), float(alpha), float(beta)
    p.d_U, k, p.ldu = _device_block(U, A.rows, k, ldu, "U", "sddmm", blocks)
    p.d_V, k, p.ldv = _device_block(V, A.cols, k, ldv, "V", "sddmm", blocks)
    if k < 0 or p.ldu < k or p.ldv < k:
        raise ValueError(f"sddmm: k = {k} with ldu = {p.ldu}, ldv = {p.ldv}: a leading dimension is at least k >= 0")
    p.k = k
    L = _lib.load()
    if blocks == "float32":
        fn = L.speck_sddmm_f32_b32 if A.dtype == np.float32 else L.speck_sddmm_f64_b32
    else:
        fn = L.speck_sddmm_f32 if A.dtype == np.float32 else L.speck_sddmm_f64
    info = _lib.CSddmmInfo()
    h = config._h if config is not None else None
    if inplace:
        _check(fn(h, C.byref(A._c), C.byref(p), None, C.byref(info)), "sddmm")
        return A, SddmmInfo(info)
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    _check(fn(h, C.byref(A._c), C.byref(p), C.byref(matOut._c), C.byref(info)), "sddmm")
    ro = A._host_row_offsets   # (C's offsets are A's, from 0: the host copy is shared where A's start there)
    matOut._host_row_offsets = ro if ro is None or ro[0] == 0 else (ro - ro[0]).astype(np.uint32)
    return matOut, SddmmInfo(info)


# include/speck_c_api.h: SPECK_SOFTMAX_*; the entries of a tile of the pass
SOFTMAX_NORMALIZED, SOFTMAX_EXP, SOFTMAX_BACKWARD = range(3)
SOFTMAX_MODES = {"normalized": SOFTMAX_NORMALIZED, "exp": SOFTMAX_EXP}
SOFTMAX_TILE_ENTRIES = 4096


class SoftmaxInfo(_Info):
    """speck_softmax_info: what the row softmax wrote and walked."""
    _fields = ("entries", "nonfinite", "rows_empty", "rows_split", "tiles")


def _softmax_call(who, A, p, config, matOut, inplace):
    """the call of softmax and softmax_backward behind their checks: in place, or into matOut (a new matrix when None)"""
    L = _lib.load()
    fn = L.speck_softmax_f32 if A.dtype == np.float32 else L.speck_softmax_f64
    info = _lib.CSoftmaxInfo()
    h = config._h if config is not None else None
    if inplace:
        _check(fn(h, C.byref(A._c), C.byref(p), None, C.byref(info)), who)
        return A, SoftmaxInfo(info)
    if matOut is None:
        matOut = dCSR(A.dtype)
    if matOut.dtype != A.dtype:
        matOut.reset()
        matOut.dtype = A.dtype
    _check(fn(h, C.byref(A._c), C.byref(p), C.byref(matOut._c), C.byref(info)), who)
    ro = A._host_row_offsets   # (C's offsets are A's, from 0: the host copy is shared where A's start there)
    matOut._host_row_offsets = ro if ro is None or ro[0] == 0 else (ro - ro[0]).astype(np.uint32)
    return matOut, SoftmaxInfo(info)


def softmax(A, config, alpha=1.0, mode="normalized", matOut=None, inplace=False, row_max=None, row_sum=None):
    """The softmax of every row of A over the entries the row holds (speck_softmax_f64 / _f32): p = exp(alpha a - m_i) / s_i
    with m_i the row's largest alpha a and s_i the sum of the row's exp(alpha a - m_i); mode "exp" leaves the division out.
    Every step in double, s_i in the tree of reduce(.., "sum"), one rounding to A's value type: the same bits from run to
    run, in place or not, and a row_view gives the entries of the whole matrix's result bit for bit.  As torch.softmax, a
    -inf entry (a mask) becomes 0, a row of only -inf becomes NaN, a +inf or a NaN makes its row NaN and touches no other;
    such results are counted in info.nonfinite.  alpha is the temperature, any finite number.  row_max and row_sum
    (A.rows float64 each, a device address or an object with data_ptr(); indexed by the row inside A, so for a row_view
    pass the slice) receive m_i and s_i; a row without entries gets -inf and 0.0.  inplace=True overwrites A's values
    (on a row_view: the view's entries only) and never reads col_ids; otherwise the result goes to matOut (a new matrix
    when None) with A's pattern, offsets rebased to 0.  Rows need not be sorted, duplicates are separate terms.  The
    scores of sddmm go in, the result goes into spmm.  config may be None.  Returns (matOut or A, SoftmaxInfo)."""
    if isinstance(mode, str):
        if mode not in SOFTMAX_MODES:
            raise ValueError(f"softmax: unknown mode {mode!r} (one of {', '.join(SOFTMAX_MODES)})")
        mode = SOFTMAX_MODES[mode]
    elif isinstance(mode, bool) or mode not in SOFTMAX_MODES.values():
        raise ValueError(f"softmax: unknown mode {mode!r}")
    if inplace and matOut is not None:
        raise ValueError("softmax: inplace=True and matOut exclude each other")
    p = _lib.CSoftmaxParams()
    p.mode, p.alpha = int(mode), float(alpha)
    p.d_row_max = _device_vector(row_max, A.rows, "row_max", "softmax")
    p.d_row_sum = _device_vector(row_sum, A.rows, "row_sum", "softmax")
    return _softmax_call("softmax", A, p, config, matOut, inplace)


def softmax_backward(P, G, config, alpha=1.0, matOut=None, inplace=False, row_sum=None, check_pattern=False, row_max=None):
    """The gradient of softmax(A, alpha) with respect to A's values (speck_softmax_* with SPECK_SOFTMAX_BACKWARD): P is the
    forward result, G the gradient with respect to it, a dCSR with P's rows, nnz and value type whose entries stand where
    P's do (for a row_view of P: the same row_view of G's matrix).  Every entry becomes alpha p (g - r_i), r_i the sum of
    the row's p g in the tree of reduce(.., "sum"), each step rounded to double on its own: bit for bit numpy's
    (alpha * (p * (g - r[row]))).astype(dtype).  row_sum (P.rows float64) receives r_i.  The pattern of G is not
    compared inside the call; check_pattern=True runs compare(P, G) on the structures first and raises ValueError on a
    difference (it needs a config).  inplace=True overwrites P's values.  row_max is refused: the backward has no
    maximum.  config may be None.  Returns (matOut or P, SoftmaxInfo)."""
    if row_max is not None:
        raise ValueError("softmax_backward: row_max belongs to the forward call (the backward has no maximum)")
    if inplace and matOut is not None:
        raise ValueError("softmax_backward: inplace=True and matOut exclude each other")
    if not isinstance(G, dCSR):
        raise ValueError(f"softmax_backward: G must be a dCSR with P's pattern, not {type(G).__name__}")
    if (G.rows, G.nnz) != (P.rows, P.nnz):
        raise ValueError(f"softmax_backward: G has {G.rows} rows and {G.nnz} entries, P has {P.rows} and {P.nnz}")
    if G.dtype != P.dtype:
        raise ValueError(f"softmax_backward: G holds {G.dtype}, P holds {P.dtype}")
    if check_pattern and not compare(P, G, config, compare_data=False):
        raise ValueError("softmax_backward: G does not have P's pattern")
    p = _lib.CSoftmaxParams()
    p.mode, p.alpha = SOFTMAX_BACKWARD, float(alpha)
    p.d_G = G._c.data
    p.d_row_sum = _device_vector(row_sum, P.rows, "row_sum", "softmax_backward")
    return _softmax_call("softmax_backward", P, p, config, matOut, inplace)
