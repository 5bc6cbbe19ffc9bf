"""Row-range views whose absolute offsets lie in [2^31, 2^32), through every entry point whose header says it takes a view.
row_offsets are u32 and every entry point accepts nnz < 2^32; a matrix of more than 2^31 entries cut into row views hands the
later ranks views whose every offset has the top bit set.  A stray int, a u32 sum formed before widening, a (u32) cast of a
tile end or a 32-bit address offset goes wrong exactly there.

The backing store is real: device tensors of 2^32 - 1 column ids and float32 values (16 GiB each) and, after the float32
values are released, 2^31 + 2^21 float64 values (16 GiB), made with torch.empty and never filled as a whole.  A view writes
its own region and 64 sentinel entries on each side of it; a wrapped index therefore reads a wrong value and fails an
assertion, it does not leave the allocation.  One and the same view is placed four times:
  low       base = (2^31 - T - 37) mod T + T: the control, the regime every other test file pins, through this file's code
  straddle  base = 2^31 - T - 37: the top bit flips inside a row, 2^31 is a tile boundary, the first tile is partial
  above     base = 2^31 + 5 T + 1: every offset has the top bit set
  top       base + nnz = 2^32 - 1: the last offset is 0xFFFFFFFF and the last tile ends at 2^32 (float32 only: the float64
            values up to there would take 32 GiB more)
Every expectation is numpy, math.fsum or the oracle, computed from the view's own entries (the host copy counts from 0)
through the helpers of the operation's own test file; integer values, so equality.  T = 4096 entries per tile below."""
import ctypes as C_
import math
import struct

import numpy as np
import pytest
import torch

import speck_amd as sa
import test_gpu_add as ADD
import test_gpu_masked as MSK
import test_gpu_reduce as R
import test_gpu_scale as S
import test_gpu_sddmm as D
import test_gpu_select as SEL
import test_gpu_sort_rows as SORT
import test_gpu_spmm as M
import test_gpu_spmv as V
from speck_amd import _lib
from test_gpu_parity import _assert_matches_oracle, fast_random_csr, to_sa
from test_gpu_reduce import cfg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
DEV = "cuda:0"
T = sa.REDUCE_TILE_ENTRIES
TWO31, TWO32 = 1 << 31, 1 << 32
GIB = 1 << 30
IDS_N = F32_N = TWO32 - 1
F64_N = TWO31 + (1 << 21)
SMALL_N = 1 << 22                       # the store where memory is short: the control placement alone fits
GUARD = 64                              # sentinel entries on each side of a view
ID_SENTINEL = 0xDEADBEEF
VALUE_SENTINEL = {np.dtype(np.float64): np.array([0x7FF8DEADBEEF1234], dtype=np.uint64).view(np.float64)[0],
                  np.dtype(np.float32): np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]}
COLS = 300_000                          # more than the long row holds: its ids are distinct
B_COLS = 5_000
LONG = 70 * T + 3
OPS, SUMS = R.OPS, R.SUMS
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def places(kind):
    """the placements a test runs at: PLACES[kind] of its class (pytest_generate_tests below)"""
    def mark(f):
        f.places = kind
        return f
    return mark


def pytest_generate_tests(metafunc):
    if "where" in metafunc.fixturenames and metafunc.cls is not None:
        metafunc.parametrize("where", metafunc.cls.PLACES[metafunc.function.places])


# ---------------------------------------------------------------------------------------------------- the backing store
class Store:
    """column ids and values of one value type, indexed by absolute entry"""

    def __init__(self, ids, vals, short):
        self.ids, self.vals, self.short = ids, vals, short
        self.n = min(ids.numel(), vals.numel())
        self.dtype = np.dtype(np.float32 if vals.dtype == torch.float32 else np.float64)

    def need(self, end):
        if end > self.n:
            assert self.short is not None, f"entries up to {end} lie outside the store of {self.n}"
            free, want = self.short
            pytest.skip(f"free device memory {free} B is below the store's {want} B + 8 GiB: entries up to {end} do not fit")

    def place(self, H, base):
        """H's entries at [base, base + nnz) between two rows of sentinels: a view with absolute offsets"""
        assert H.data.dtype == self.dtype and H.row_offsets[0] == 0 and base >= GUARD
        self.need(base + H.nnz)
        return Placed(self, H, base)


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _empty(n, dtype, size):
    """(tensor of n elements, None) where free memory allows, else (a small one, (free, wanted))"""
    free, want = _free(), n * size
    if free < want + 8 * GIB:
        return torch.empty(SMALL_N, dtype=dtype, device=DEV), (free, want)
    return torch.empty(n, dtype=dtype, device=DEV), None


class Stores:
    """the ids for the whole module and the values of ONE value type at a time: asking for the other releases the first"""

    def __init__(self):
        self.ids, self.ids_short = _empty(IDS_N, torch.int32, 4)
        self.store = None

    def get(self, dtype):
        dtype = np.dtype(dtype)
        if self.store is None or self.store.dtype != dtype:
            self.release()
            vals, short = _empty(F32_N if dtype == F32 else F64_N, torch.float32 if dtype == F32 else torch.float64, dtype.itemsize)
            self.store = Store(self.ids, vals, short or self.ids_short)
        return self.store

    def release(self):
        if self.store is not None:
            self.store.ids = self.store.vals = None
            self.store = None
            torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def stores():
    st = Stores()
    yield st
    st.release()
    st.ids = None
    torch.cuda.empty_cache()


class Placed:
    def __init__(self, store, H, base):
        self.store, self.H, self.base, self.n = store, H, base, H.nnz
        self.lo, self.hi = base - GUARD, min(base + H.nnz + GUARD, store.n)
        self.write()
        self.ro = (H.row_offsets.astype(np.int64) + base).astype(np.uint32)
        self.d = self.view(self.ro, self.n)

    def write(self):
        H, back = self.H, self.hi - self.base - self.n
        ci = np.concatenate([np.full(GUARD, ID_SENTINEL, np.uint32), H.col_ids, np.full(back, ID_SENTINEL, np.uint32)])
        va = np.concatenate([np.full(GUARD, VALUE_SENTINEL[H.data.dtype]), H.data, np.full(back, VALUE_SENTINEL[H.data.dtype])])
        self.store.ids[self.lo:self.hi].copy_(torch.from_numpy(ci.view(np.int32)))
        self.store.vals[self.lo:self.hi].copy_(torch.from_numpy(va))
        self.region = (ci.tobytes(), va.tobytes())
        torch.cuda.synchronize()

    def view(self, ro, nnz):
        """a dCSR over the store with these absolute offsets"""
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        t_ro = torch.from_numpy(ro.view(np.int32).copy()).to(DEV)
        d = sa.dCSR.from_device(self.H.rows, self.H.cols, nnz, t_ro.data_ptr(), self.store.ids.data_ptr(), self.store.vals.data_ptr(),
                                dtype=self.H.data.dtype, keep=(t_ro, self.store), host_row_offsets=ro)
        d._ro_bytes = ro.tobytes()
        return d

    def read(self):
        torch.cuda.synchronize()
        return (self.store.ids[self.lo:self.hi].cpu().numpy().view(np.uint32), self.store.vals[self.lo:self.hi].cpu().numpy())

    def entries(self):
        ci, va = self.read()
        return ci[GUARD:GUARD + self.n].copy(), va[GUARD:GUARD + self.n].copy()

    def check_guards(self, d=None):
        """the sentinels on both sides and the view's row_offsets keep their bytes"""
        ci, va = self.read()
        want_ci, want_va = (np.frombuffer(b, dtype=t) for b, t in zip(self.region, (np.uint32, self.H.data.dtype)))
        for a, b in ((0, GUARD), (GUARD + self.n, self.hi - self.lo)):
            assert ci[a:b].tobytes() == want_ci[a:b].tobytes(), "a sentinel id was written"
            assert va[a:b].tobytes() == want_va[a:b].tobytes(), "a sentinel value was written"
        d = d or self.d
        assert d._keep[0].cpu().numpy().tobytes() == d._ro_bytes, "row_offsets were written"

    def check_structure(self, d=None):
        """... and so do the view's column ids (an in-place call)"""
        self.check_guards(d)
        assert self.entries()[0].tobytes() == self.H.col_ids.tobytes(), "col_ids were written"

    def check_intact(self, d=None):
        """... and its values (a call that only reads the view)"""
        self.check_structure(d)
        assert self.entries()[1].tobytes() == self.H.data.tobytes(), "values were written"


def base_of(where, nnz):
    return {"low": (TWO31 - T - 37) % T + T, "straddle": TWO31 - T - 37, "above": TWO31 + 5 * T + 1, "top": TWO32 - 1 - nnz}[where]


def other_base(where, base, nnz, nnz_other):
    """where a second operand lies in the same store: behind the first, at the top in front of it"""
    return base - nnz_other - 2 * T - 77 if where == "top" else base + nnz + 2 * T + 77


def twin_base(base):
    """the low placement with the same position inside a tile"""
    return base % T + T


def check_premise(where, ro, inside_a_row=True):
    """each placement is what its name says"""
    ro = np.asarray(ro).astype(np.int64)
    s, e = ro[:-1], ro[1:]
    if where == "low":
        assert ro[-1] < 1 << 24 and ro[0] % T == (TWO31 - T - 37) % T
    elif where == "straddle":
        assert ro[0] < TWO31 <= ro[-1] and TWO31 % T == 0 and ro[0] % T and (ro[0] * 4) % 16
        assert not inside_a_row or ((s < TWO31) & (e > TWO31)).any()                # the top bit flips inside a row
    elif where == "above":
        assert ro[0] >= TWO31
    else:
        assert ro[0] >= TWO31 and ro[-1] == 0xFFFFFFFF and ro[-1] % T and (ro[-1] // T + 1) * T == TWO32


# ---------------------------------------------------------------------------------------------------- the matrices
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def distinct(rng, n, cols):
    return np.sort(rng.choice(cols, size=int(n), replace=False)).astype(np.uint32)


def view_lens():
    """about 400 rows of 0..60 entries that hold 3 T + 5 entries, one row of 70 T + 3, 20 short rows"""
    rng = np.random.default_rng(2)
    lens = [int(v) for v in rng.integers(0, 61, size=380)]
    lens[0] = lens[7] = lens[200] = 0
    while 3 * T + 5 - sum(lens) > 60:
        lens.append(60)
    lens.append(3 * T + 5 - sum(lens))
    assert 390 <= len(lens) <= 420 and sum(lens) == 3 * T + 5 and min(lens) >= 0
    tail = [int(v) for v in rng.integers(0, 61, size=20)]
    tail[4] = 0
    return lens + [LONG] + tail, len(lens)


def structure():
    """(row_offsets from 0, sorted distinct column ids, the long row)"""
    def make():
        lens, long_row = view_lens()
        rng = np.random.default_rng(3)
        ro = np.zeros(len(lens) + 1, dtype=np.uint32)
        ro[1:] = np.cumsum(lens)
        ci = np.concatenate([distinct(rng, n, COLS) for n in lens])
        ro.setflags(write=False), ci.setflags(write=False)
        return ro, ci, long_row
    return cached("structure", make)


def view_matrix(dtype, kind="int", values=None):
    """THE view: integers in [-1024, 1024] or reals over twelve decades -- or, under another name for `kind`, what
    values(n, dtype) gives (test_gpu_high_offsets_side.py: the values of an operation's own test file on this structure)"""
    def make():
        ro, ci, _ = structure()
        if values is not None:
            assert kind not in ("int", "real")
            data = np.ascontiguousarray(values(len(ci), np.dtype(dtype).type))
            assert data.dtype == np.dtype(dtype) and data.shape == (len(ci),)
        else:
            data = V.ints(len(ci), 4, dtype) if kind == "int" else V.real_values(len(ci), 4, dtype)
        data.setflags(write=False)
        return sa.HostCSR(len(ro) - 1, COLS, ro, ci, data)
    return cached(("view", np.dtype(dtype).name, kind), make)


def second_matrix(dtype):
    """the pattern of select and the B of add: every other id of the view's rows and a third as many others, integer values"""
    def make():
        ro, ci, _ = structure()
        rng = np.random.default_rng(5)
        rows = []
        for a, b in zip(ro[:-1].astype(np.int64), ro[1:].astype(np.int64)):
            extra = rng.integers(0, COLS, size=(b - a) // 3 + 1 if b > a else 0).astype(np.uint32)
            rows.append(np.unique(np.concatenate([ci[a:b:2], extra])))
        ro2 = np.zeros(len(ro), dtype=np.uint32)
        ro2[1:] = np.cumsum([len(r) for r in rows])
        ci2 = np.concatenate(rows).astype(np.uint32)
        return sa.HostCSR(len(ro) - 1, COLS, ro2, ci2, V.ints(len(ci2), 6, dtype))
    return cached(("second", np.dtype(dtype).name), make)


def b_matrix(dtype):
    """the ordinary right-hand side of the two products: 300 000 x 5 000, up to two entries a row, values +-1 .. +-4 (every
    sum of products stays an integer below 2^24: exact in float32 whatever the order)"""
    def make():
        B = fast_random_csr(COLS, B_COLS, 2, 7)
        rng = np.random.default_rng(8)
        data = (rng.integers(1, 5, size=B.nnz) * rng.choice([-1, 1], size=B.nnz)).astype(dtype)
        return sa.HostCSR(B.rows, B.cols, B.row_offsets, B.col_ids, data)
    return cached(("b", np.dtype(dtype).name), make)


def mask_matrix():
    """the mask of the masked product: rows of 0..60 ids, 4 500 for the long row (the global-memory class); of the last two
    rows of A that hold entries -- at the top they lie within 256 entries of 2^32, one step of every row kernel -- the
    earlier has 4 500 ids too and the later 1 000 (the LDS class)"""
    def make():
        ro, _, long_row = structure()
        rng = np.random.default_rng(9)
        lens = rng.integers(0, 61, size=len(ro) - 1)
        lens[long_row] = 4500
        for r, n in zip(mask_tail_rows(), (4500, 1000)):
            lens[r] = n
        assert sa.MASK_GROUP_MAX < 1000 <= sa.MASK_LDS_MAX < 4500
        return MSK.mask_from_rows([distinct(rng, n, B_COLS) for n in lens], B_COLS)
    return cached("mask", make)


def mask_tail_rows():
    """the last two rows of the view that hold entries: (global class, LDS class) of mask_matrix"""
    ro, _, _ = structure()
    full = np.nonzero(np.diff(ro.astype(np.int64)) > 0)[0]
    assert int(ro[-1]) - int(ro[full[-2]]) < 256
    return int(full[-2]), int(full[-1])


def place_view(store, where, H=None, inside_a_row=True):
    H = view_matrix(store.dtype) if H is None else H
    p = store.place(H, base_of(where, H.nnz))
    check_premise(where, p.ro, inside_a_row)
    return p


def place_second(store, where, first, H2):
    p2 = store.place(H2, other_base(where, first.base, first.n, H2.nnz))
    assert p2.hi <= first.lo or p2.lo >= first.hi
    assert where == "low" or p2.ro[-1] >= TWO31                                     # a high view too
    return p2


def place_pair(store, where, H, H2, swapped=False):
    """the view and a second operand in the same store; swapped (at the top): the SECOND ends at 0xFFFFFFFF, the view lies in
    front of it"""
    if not swapped:
        p = place_view(store, where, H)
        return p, place_second(store, where, p, H2)
    assert where == "top"
    p2 = store.place(H2, TWO32 - 1 - H2.nnz)
    p = store.place(H, p2.base - H.nnz - 2 * T - 77)
    assert p2.ro[-1] == 0xFFFFFFFF and p.ro[0] >= TWO31 and p.hi <= p2.lo
    return p, p2


def roles(where):
    return (False, True) if where == "top" else (False,)


def test_the_view_and_its_placements_are_what_this_file_says():
    ro, ci, long_row = structure()
    ro = ro.astype(np.int64)
    assert ro[long_row] == 3 * T + 5 and ro[long_row + 1] - ro[long_row] == LONG and len(ro) - 1 == long_row + 21
    assert np.diff(ro)[np.arange(len(ro) - 1) != long_row].max() <= 60 and (np.diff(ro) == 0).sum() >= 4
    for a, b in zip(ro[:-1], ro[1:]):
        assert (np.diff(ci[a:b].astype(np.int64)) > 0).all()
    for where in ("low", "straddle", "above", "top"):
        check_premise(where, ro + base_of(where, int(ro[-1])))
    assert twin_base(base_of("straddle", 0)) == base_of("low", 0)


# ---------------------------------------------------------------------------------------------------- helpers of the tests
def out_of_place_is(C, H, want, same):
    """a new matrix: offsets from 0, the ids bit for bit, the values expected"""
    G = C.to_host()
    assert (G.rows, G.cols, C.nnz) == (H.rows, H.cols, H.nnz)
    assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
    assert same(G.data, want)


def fsum_rows(t, ro):
    ro = np.asarray(ro, dtype=np.int64)
    return (np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])]),
            np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])]))


def place_with_twin(store, where, H):
    hi = place_view(store, where, H)
    lo = store.place(H, twin_base(hi.base))
    assert lo.base % T == hi.base % T and lo.ro[-1] < 1 << 24                      # the same position inside a tile
    return hi, lo


def hostile_views(p):
    """(name, dCSR): one change each, and nothing a correct library would read lies outside the placed region"""
    H, ro = p.H, p.ro
    r = next(i for i in range(H.rows // 2, H.rows) if ro[i + 1] - ro[i] >= 4)
    desc = ro.copy()
    desc[r] = desc[r + 1] + 1                                                      # a descending pair
    short = ro.copy()
    assert short[-1] > short[-2]
    short[-1] -= 1                                                                 # the declared nnz is one more than the offsets span
    below = ro.copy()
    below[r] = p.base - 1                                                          # one offset below the base (a sentinel entry)
    return [("descending", p.view(desc, p.n)), ("nnz + 1", p.view(short, p.n)), ("below the base", p.view(below, p.n))]


def sentinel_output(rows, cols, dtype, n=1234):
    dC = sa.dCSR(dtype)
    dC.alloc(rows, cols, n)
    s = (np.full(rows + 1, 0xABABABAB, dtype=np.uint32), np.full(n, 0xCDCDCDCD, dtype=np.uint32), np.full(n, -77.25, dtype=dtype))
    assert _lib.load().speck_dcsr_update(C_.byref(dC._c), s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data,
                                         np.dtype(dtype).itemsize) == 0
    return dC, bytes(dC._c), s


def untouched(dC, before, s):
    got = dC.to_host()
    return bytes(dC._c) == before and got.row_offsets.tobytes() == s[0].tobytes() and got.col_ids.tobytes() == s[1].tobytes() \
        and got.data.tobytes() == s[2].tobytes()


# ---------------------------------------------------------------------------------------------------- the tests, per value type
class HighOffsets:
    """every test at the placements of its kind; the two classes below give the value type.  The float32 class comes first
    and, for every test, the control placement"""
    dtype = None
    PLACES = {}

    @pytest.fixture
    def store(self, stores):
        return stores.get(self.dtype)

    @places("all")
    def test_reduce(self, cfg, store, where):
        H = view_matrix(store.dtype)
        p = place_view(store, where)
        for op in OPS:
            rows, total, info = sa.reduce(p.d, cfg, op)
            want_rows, want_total = R.ref_exact(H.row_offsets, H.data, op)
            assert R.same(rows, want_rows), (op, np.nonzero(rows != want_rows)[0][:8])
            assert R.same(total, want_total), (op, total, want_total)
            R.check_info(info, p.ro)
        p.check_intact()
        R.check_exact(cfg, R.edge_matrix(store.dtype.type), ops=["sum", "max"])      # an ordinary call right after

    @places("all")
    def test_spmv(self, cfg, store, where):
        H = view_matrix(store.dtype)
        p = place_view(store, where)
        x = V.ints(COLS, 10)
        dx, s, y0 = V.tv(x), V.row_sums(H, x), V.ints(H.rows, 11)
        assert np.abs(V.terms(H, x)).sum() < 2.0 ** 53
        for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
            got, info = V.run(cfg, p.d, dx, alpha, beta, y0 if beta else None)
            want = alpha * s + beta * y0 if beta else alpha * s
            assert np.array_equal(got, want), (alpha, beta, np.nonzero(got != want)[0][:8])
            V.check_info(info, p.ro)
        p.check_intact()
        V.check_edge(cfg, sa.dCSR.from_host(V.edge_case(store.dtype.type)[0]), store.dtype.type)

    @pytest.mark.parametrize("k", [1, 3, 5])
    @places("all")
    def test_spmm(self, cfg, store, where, k):
        H = view_matrix(store.dtype)
        p = place_view(store, where)
        X = cached("X", lambda: M.ints((COLS, 5), 12))[:, :k]
        S_ = M.row_sums(H, X)
        Y0 = M.ints((H.rows, k), 13)
        for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
            got, info = M.run(cfg, p.d, X, alpha, beta, Y0 if beta else None)
            want = alpha * S_ + beta * Y0 if beta else alpha * S_
            assert np.array_equal(got, want), (k, alpha, beta, np.argwhere(got != want)[:8])
            M.check_info(info, p.ro, k)
        p.check_intact()
        M.check_edge(cfg, sa.dCSR.from_host(M.edge_case(store.dtype.type)[0]), store.dtype.type, ks=(3,))

    # ------------------------------------------------------------------------------------------------ sddmm, scale

    @pytest.mark.parametrize("k", [1, 5, 9])
    @places("all")
    def test_sddmm(self, cfg, store, where, k):
        dtype = store.dtype.type
        H = view_matrix(dtype)
        p = place_view(store, where)
        U, W = D.ints((H.rows, k), 14), D.ints((COLS, k), 15)
        d = D.exact(H, U, W)
        for alpha, beta, mode in ((-3.0, 2.0, "axpby"), (0.5, 0.0, "hadamard")):
            want = D.expect(d, H.data, dtype, alpha, beta, mode)
            C, info = D.run(cfg, p.d, U, W, alpha=alpha, beta=beta, mode=mode)
            out_of_place_is(C, H, want, D.same_bytes)
            assert D.as_tuple(info) == D.counts(p.ro, k, want)
            p.check_intact()
            C, info = D.run(cfg, p.d, U, W, alpha=alpha, beta=beta, mode=mode, inplace=True)
            assert C is p.d and D.same_bytes(p.entries()[1], want), (k, mode, D.first_difference(p.entries()[1], want))
            assert D.as_tuple(info) == D.counts(p.ro, k, want)
            p.check_structure()
            p.write()
        small = D.sweep_matrix(dtype, "int")
        Us, Ws = D.blocks(5, "int")
        got, _ = D.values(cfg, small, Us, Ws)
        assert D.same_bytes(got, D.expect(D.exact(small, Us, Ws), small.data, dtype))

    @places("all")
    def test_scale(self, cfg, store, where):
        dtype = store.dtype.type
        H = view_matrix(dtype)
        p = place_view(store, where)
        rw, cl = S.rows_of(H.row_offsets), H.col_ids.astype(np.int64)
        l, r = S.vector(H.rows, 16), S.vector(COLS, 17)
        l_t, r_t = S.dev(l), S.dev(r)
        for row, col, map, alpha in (("mul", None, "identity", 1.0), (None, "div", "identity", 1.0), (None, None, "square", -1.7)):
            want = S.expected(H.data, rw, cl, dtype, alpha, map, l, row, r, col)
            C, info = S.call(p.d, cfg, l_t, r_t, row, col, alpha=alpha, map=map)
            out_of_place_is(C, H, want, S.same)
            S.check_info(info, want, p.ro, row is not None)
            p.check_intact()
            C, info = S.call(p.d, cfg, l_t, r_t, row, col, alpha=alpha, map=map, inplace=True)
            assert C is p.d and S.same(p.entries()[1], want), (row, col, map, S.first_difference(p.entries()[1], want))
            S.check_info(info, want, p.ro, row is not None)
            p.check_structure()
            p.write()
        small = S.edge_matrix(dtype)[0]
        C, _ = sa.scale(sa.dCSR.from_host(small), cfg, alpha=2.0)
        assert S.same(C.to_host().data, S.expected(small.data, None, None, dtype, 2.0))

    # ------------------------------------------------------------------------------------------------ select, add
    @places("all")
    def test_select(self, cfg, store, where):
        dtype = store.dtype.type
        H, P = view_matrix(dtype), second_matrix(dtype)
        for swapped in roles(where):                                                   # (at the top: the pattern up there too)
            p, pp = place_pair(store, where, H, P, swapped)
            SEL.check(cfg, H, dA=p.d, band=(-40_000, 90_000), row_base=1000)
            SEL.check(cfg, H, dA=p.d, abs_gt=512.0)
            _, info, _ = SEL.check(cfg, H, dA=p.d, dPattern=pp.d, pattern=P)
            assert 0 < info.kept < H.nnz
            SEL.check(cfg, H, dA=p.d, dPattern=pp.d, pattern=P, negate=("pattern",), abs_gt=100.0)
            p.check_intact(), pp.check_intact()
        SEL.check(cfg, SEL.from_lengths([5, 0, 9, 300], 400, 18, dtype), abs_gt=0.7)

    @places("all")
    def test_add(self, cfg, store, where):
        dtype = store.dtype.type
        H, B = view_matrix(dtype), second_matrix(dtype)
        for swapped in roles(where):                                                   # (at the top: B up there too)
            p, pb = place_pair(store, where, H, B, swapped)
            assert p.base % T != pb.base % T                                           # each with its own base
            _, info, _ = ADD.check(cfg, H, B, 2.5, -0.5, dA=p.d, dB=pb.d)
            assert info.only_a and info.only_b and info.both
            p.check_intact(), pb.check_intact()
        ADD.check(cfg, ADD.from_lengths([5, 0, 9, 300], 400, 19, dtype), ADD.from_lengths([0, 7, 9, 250], 400, 20, dtype), 2.5, -0.5)

    # ------------------------------------------------------------------------------------------------ sort_rows
    @pytest.mark.parametrize("sum_duplicates", [False, True], ids=["keep", "sum_duplicates"])
    @places("all")
    def test_sort_rows(self, cfg, store, where, sum_duplicates):
        """shuffled rows of every class length, the long one about 9000: in place (no column repeats: summing duplicates leaves
        the stable sort, and is allowed on a view)"""
        dtype = store.dtype.type
        ro, ci, va, cols = cached(("sort", store.dtype.name), lambda: SORT.edge_matrix(dtype, seed=6, long_row=9000))
        H = sa.HostCSR(len(ro) - 1, cols, ro, ci, va)
        p = place_view(store, where, H, inside_a_row=False)
        eci, eva = cached(("sorted", store.dtype.name), lambda: SORT.expect_keep(ro, ci, va))
        info = sa.sort_rows(p.d, cfg, sum_duplicates=sum_duplicates)
        got_ci, got_va = p.entries()
        assert SORT.same_bytes(got_ci, eci) and SORT.same_bytes(got_va, eva)
        planted = SORT.strictly_ascending_rows(ro, ci)
        assert (info.nnz_out, info.duplicates, info.rows_in_order) == (len(ci), 0, planted) and p.d.nnz == len(ci)
        assert sum(info.rows_sorted) == H.rows - planted and all(n > 0 for n in info.rows_sorted)
        p.check_guards()
        d = SORT.upload(ro, ci, va, cols)                                              # an ordinary call right after
        sa.sort_rows(d, cfg, sum_duplicates=sum_duplicates)
        got = d.to_host()
        assert SORT.same_bytes(got.col_ids, eci) and SORT.same_bytes(got.data, eva)

    # ------------------------------------------------------------------------------------------------ the two products
    @pytest.mark.parametrize("full", [False, True], ids=["structure", "full_pattern"])
    @places("all")
    def test_multiply_masked(self, cfg, store, where, full):
        dtype = store.dtype.type
        A, B, Mk = view_matrix(dtype), b_matrix(dtype), mask_matrix()
        X = cached(("masked", store.dtype.name), lambda: MSK.Expect(MSK.as_dtype(A, dtype), MSK.as_dtype(B, dtype), Mk))
        Mh = sa.HostCSR(Mk.rows, Mk.cols, Mk.row_offsets, Mk.col_ids, Mk.data.astype(dtype))
        for swapped in roles(where):                                                   # (at the top: the mask up there too)
            p, pm = place_pair(store, where, A, Mh, swapped)
            if where == "top" and not swapped:                                         # one step of a row kernel reaches 2^32
                assert all(int(p.ro[r]) + 256 >= TWO32 and p.ro[r + 1] > p.ro[r] for r in mask_tail_rows())
            _, info, _ = MSK.check(cfg, A, B, Mk, dtype, full, X=X, views=(p.d, MSK.to_dev(B), pm.d))
            assert info.hits > 0 and info.rows_class[1] >= 1 and info.rows_class[2] >= 2
            p.check_intact(), pm.check_intact()
        a, b = fast_random_csr(300, 300, 6, 21), fast_random_csr(300, 300, 6, 22)
        MSK.check(cfg, a, b, MSK.random_mask(300, 300, 8, 23), dtype, full)

    @places("all")
    def test_multiply(self, cfg, store, where):
        """at the top the header's limit for A holds: row_offsets[0] + nnz > 2^32 - 2^16 is refused by the multiply and its
        stage entry points before any kernel starts, with nothing written"""
        dtype = store.dtype.type
        A, B = view_matrix(dtype), b_matrix(dtype)
        p = place_view(store, where)
        dB = sa.dCSR.from_host(B)
        if where == "top":
            dC, before, s = sentinel_output(A.rows, B_COLS, dtype)
            for call in (lambda: sa.MultiplyspECK(p.d, dB, dC, cfg), lambda: sa.analysis(p.d, dB, cfg),
                         lambda: sa.symbolic(p.d, dB, cfg), lambda: sa.partition_rows(p.d, dB, cfg, 4)):
                with pytest.raises(sa.SpeckError) as e:
                    call()
                assert e.value.status == ERR_INVALID
                assert untouched(dC, before, s)
        else:
            dC = sa.dCSR(dtype)
            sa.MultiplyspECK(p.d, dB, dC, cfg)
            assert dC.dtype == store.dtype
            _assert_matches_oracle(dC, MSK.as_dtype(A, np.float64), MSK.as_dtype(B, np.float64))    # (integers: exact in float32 too)
        p.check_intact()
        a = fast_random_csr(300, 300, 6, 24)
        dA = sa.dCSR.from_host(to_sa(a))
        _assert_matches_oracle(sa.MultiplyspECK(dA, dA, sa.dCSR(), cfg), a, a)

    # ------------------------------------------------------------------------------------------------ download, device copy
    @places("all")
    def test_to_host_and_device_copy_rebase_to_zero(self, store, where):
        H = view_matrix(store.dtype)
        p = place_view(store, where)
        c = p.d.copy()
        assert c._c.data != p.d._c.data and c._c.col_ids != p.d._c.col_ids and c._c.row_offsets != p.d._c.row_offsets
        for G in (p.d.to_host(), c.to_host()):
            assert (G.rows, G.cols) == (H.rows, H.cols) and G.data.dtype == H.data.dtype
            assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
            assert G.data.tobytes() == H.data.tobytes()
        p.check_intact()

    # ------------------------------------------------------------------------------------------------ real values

    @places("real")
    def test_real_values_reduce_spmv_spmm_give_the_bytes_of_the_low_twin(self, cfg, store, where):
        """the headers: the tree is a function of the positions of the entries inside their tiles alone.  The low result is held
        against math.fsum first; only then is the library compared with itself"""
        H = view_matrix(store.dtype, "real")
        hi, lo = place_with_twin(store, where, H)
        ro = H.row_offsets.astype(np.int64)
        n = ro[1:] - ro[:-1]
        for op in OPS:
            rows, total, _ = sa.reduce(lo.d, cfg, op)
            t = R.terms_of(H.data, op)
            if op in SUMS:
                want, mags = fsum_rows(t, ro)
                assert (np.abs(rows - want) <= R.allowance(n, mags)).all(), op
                assert abs(total - math.fsum(t)) <= R.allowance(len(t), math.fsum(np.abs(t))), op
            else:
                want_rows, want_total = R.ref_exact(ro, H.data, op)
                assert R.same(rows, want_rows) and R.same(total, want_total), op
            rows_hi, total_hi, info = sa.reduce(hi.d, cfg, op)
            assert rows_hi.view(np.uint64).tobytes() == rows.view(np.uint64).tobytes(), op
            assert struct.pack("<d", total_hi) == struct.pack("<d", total), op
            R.check_info(info, hi.ro)
        X = cached("Xreal", lambda: M.real_values((COLS, 3), 25))
        low, _ = M.run(cfg, lo.d, X)
        for c in range(3):
            want, mags = fsum_rows(V.terms(H, X[:, c]), ro)
            col, _ = V.run(cfg, lo.d, V.tv(X[:, c]))
            assert (np.abs(col - want) <= V.allowance(n, mags)).all(), c
            assert M.bits(low[:, c]).tobytes() == V.bits(col).tobytes(), c            # (so spmm's column keeps the bound)
            col_hi, info = V.run(cfg, hi.d, V.tv(X[:, c]))
            assert V.bits(col_hi).tobytes() == V.bits(col).tobytes(), c
            V.check_info(info, hi.ro)
        high, info = M.run(cfg, hi.d, X)
        assert M.bits(high).tobytes() == M.bits(low).tobytes()
        M.check_info(info, hi.ro, 3)
        hi.check_intact(), lo.check_intact()

    @places("real")
    def test_real_values_sddmm_gives_the_bytes_of_the_low_twin(self, cfg, store, where):
        dtype = store.dtype.type
        H = view_matrix(dtype, "real")
        hi, lo = place_with_twin(store, where, H)
        k = 5
        U, W = D.real_values((H.rows, k), 26), D.real_values((COLS, k), 27)
        d = D.tree(H, U, W, D.lanes(k))                                               # (held against math.fsum in test_gpu_sddmm.py)
        Ue, We = D.gathered(H, U, W)
        t = Ue * We
        some = np.unique(np.concatenate([np.arange(2000), np.arange(0, H.nnz, 97), np.arange(H.nnz - 2000, H.nnz)]))
        exact_d = np.array([math.fsum(row) for row in t[some]])                        # (the short rows, every 97th entry, the tail)
        assert (np.abs(d[some] - exact_d) <= (k * D.EPS / (1 - k * D.EPS) + D.EPS) * np.abs(t[some]).sum(axis=1)).all()
        want = D.expect(d, H.data, dtype, -1.7, 0.9)
        C_lo, _ = D.run(cfg, lo.d, U, W, alpha=-1.7, beta=0.9)
        low = C_lo.to_host().data
        assert D.same_bytes(low, want), D.first_difference(low, want)
        C_hi, info = D.run(cfg, hi.d, U, W, alpha=-1.7, beta=0.9)
        assert C_hi.to_host().data.tobytes() == low.tobytes()
        assert D.as_tuple(info) == D.counts(hi.ro, k, want)
        D.run(cfg, hi.d, U, W, alpha=-1.7, beta=0.9, inplace=True)
        assert hi.entries()[1].tobytes() == low.tobytes()
        hi.check_structure(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ hostile input at height

    @places("hostile")
    def test_hostile_offsets_at_height_are_refused_and_nothing_is_written(self, cfg, store, where):
        """a descending pair, a declared nnz one larger than the offsets span, one offset below the base: reduce, spmv, select
        and add refuse all three, and nothing is written"""
        dtype = store.dtype.type
        H, B = view_matrix(dtype), second_matrix(dtype)
        p = place_view(store, where)
        pb = place_second(store, where, p, B)
        L = _lib.load()
        f32 = store.dtype == F32
        x = V.ints(COLS, 10)
        dx = V.tv(x)
        for name, bad in hostile_views(p):
            # reduce
            out = R.sentinel_tensor(H.rows)
            total = C_.c_double(struct.unpack("<d", struct.pack("<Q", R.SENTINEL_BITS))[0])
            before = bytes(total)
            rc = (L.speck_reduce_f32 if f32 else L.speck_reduce_f64)(cfg._h, C_.byref(bad._c), 0, out.data_ptr(), C_.byref(total), None)
            torch.cuda.synchronize()
            assert rc == ERR_INVALID and (R.bits_of(out) == R.SENTINEL_BITS).all() and bytes(total) == before, name
            # spmv
            y = V.sentinel(H.rows)
            info = _lib.CSpmvInfo(7, 7, 7, 7)
            rc = (L.speck_spmv_f32 if f32 else L.speck_spmv_f64)(cfg._h, 2.0, C_.byref(bad._c), dx.data_ptr(), 0.0, y.data_ptr(), C_.byref(info))
            torch.cuda.synchronize()
            assert rc == ERR_INVALID and (V.bits(V.host(y)) == V.SENTINEL_BITS).all(), name
            assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == (0, 0, 0, 0), name
            # select and add
            for call in (lambda dC: sa.select(bad, cfg, abs_gt=512.0, matOut=dC), lambda dC: sa.select(bad, cfg, pattern=pb.d, matOut=dC),
                         lambda dC: sa.add(bad, pb.d, cfg, alpha=2.5, beta=-0.5, matOut=dC),
                         lambda dC: sa.add(pb.d, bad, cfg, alpha=2.5, beta=-0.5, matOut=dC)):
                dC, struct_before, s = sentinel_output(H.rows, COLS, dtype)
                with pytest.raises(sa.SpeckError) as e:
                    call(dC)
                assert e.value.status == ERR_INVALID, name
                assert untouched(dC, struct_before, s), name
            p.check_intact(bad), pb.check_intact()
        # the config serves the sound view and an ordinary matrix right after
        rows, total, info = sa.reduce(p.d, cfg, "sum")
        want_rows, want_total = R.ref_exact(H.row_offsets, H.data, "sum")
        assert R.same(rows, want_rows) and R.same(total, want_total)
        got, _ = V.run(cfg, p.d, dx)
        assert np.array_equal(got, V.row_sums(H, x))
        ADD.check(cfg, H, B, 2.5, -0.5, dA=p.d, dB=pb.d)
        R.check_exact(cfg, R.edge_matrix(dtype), ops=["sum"])


class TestFloat32(HighOffsets):
    dtype = F32
    PLACES = {"all": ["low", "straddle", "above", "top"], "real": ["top"], "hostile": ["straddle", "top"]}


class TestFloat64(HighOffsets):
    """(no placement at the top: the float64 values up to 2^32 would take 32 GiB, 48 GiB with the ids)"""
    dtype = F64
    PLACES = {"all": ["low", "straddle", "above"], "real": ["straddle", "above"], "hostile": ["straddle"]}
