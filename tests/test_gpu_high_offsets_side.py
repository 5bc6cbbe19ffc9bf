"""The entry points that came after tests/test_gpu_high_offsets.py, on the same row-range view at the same four placements
(low, straddle, above, top: see that file, whose stores, placements and helpers this one imports): topk, sample, extract,
to_coo, softmax forward and backward, the transpose plan with spmm_t / spmv_t, and the float-block (_b32) forms of spmm,
spmm_t and sddmm.  Every expectation is the numpy statement of the operation's own test file, computed from the host copy of
the view, which counts from 0; beside it, the bytes of the low twin (the same position inside a tile, offsets below 2^24).
Every buffer the caller owns lies in a payload frame, every call is followed by check_intact / check_structure.

What the values are: for topk, sample, extract and to_coo test_gpu_topk.mixed_values over the view's structure (the position
in the low mantissa bits, NaNs with payloads, ties); for softmax the view's reals times 2^-16 (|x| < 31: no exp leaves the
normal doubles); integers for the products, so equality.

The gradient of the softmax backward is read at the SAME absolute entries as P (speck_softmax_params.d_G is indexed as
A->data), so at 2^31 it would need a second store of values.  It lies in a free stretch of the store of ids instead, seen
as values, and d_G is that stretch's address minus base entries: one store of ids and one of values stay the rule, and an
index that went wrong still reads allocated memory.

tests/test_high_offsets_host.py proves without a GPU that the lists, the classes and the placements below are what their
names say."""
import numpy as np
import pytest
import torch

import speck_amd as sa
import test_gpu_blocks32 as B32
import test_gpu_extract as EX
import test_gpu_from_coo as COO
import test_gpu_reduce as R
import test_gpu_sample as SP
import test_gpu_sddmm as D
import test_gpu_softmax as SM
import test_gpu_spmm as M
import test_gpu_spmm_t as SPT
import test_gpu_spmv as V
import test_gpu_topk as TK
from test_gpu_high_offsets import (COLS, ERR_INVALID, F32, GUARD, T, TWO31, VALUE_SENTINEL, base_of,  # noqa: F401
                                   cached, fsum_rows, hostile_views, other_base, out_of_place_is, place_view, place_with_twin,
                                   places, pytest_generate_tests, sentinel_output, stores, structure, twin_base, untouched,
                                   view_matrix)
from test_gpu_reduce import cfg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
OK = 0
DEV = "cuda:0"
KS = (5, 40)                            # below and above the length of the row that holds entry 2^31 (29 entries)
ROW_BASE = 1_000_003
SEED = 2026
B32_LDS = ("odd", "aligned")            # leading dimensions k + 3 / k + 2, and 8 / 8 (16-byte rows)


# ---------------------------------------------------------------------------------------------------- matrices, lists (numpy only)
def tagged_matrix(dtype):
    """the view with test_gpu_topk's values: an entry that comes from another place shows in its low mantissa bits"""
    return view_matrix(dtype, "tagged", values=lambda n, t: TK.mixed_values(n, t, 31))


def softmax_matrix(dtype):
    """the view's reals over twelve decades times 2^-16: |x| < 31, so with |alpha| = 1 every exp(x - m) is a normal double"""
    H = view_matrix(dtype, "softmax", values=lambda n, t: view_matrix(t, "real").data * t(2.0 ** -16))
    assert np.abs(H.data).max() < 31
    return H


def marked_rows():
    """(the row entry 2^31 lies inside at `straddle`, the long row, the last row with entries, the last empty row)"""
    ro, _, long_row = structure()
    ro = ro.astype(np.int64)
    a = ro + base_of("straddle", int(ro[-1]))
    inside = np.nonzero((a[:-1] < TWO31) & (a[1:] > TWO31))[0]
    assert len(inside) == 1
    lens = np.diff(ro)
    return int(inside[0]), int(long_row), int(np.nonzero(lens > 0)[0][-1]), int(np.nonzero(lens == 0)[0][-1])


def row_list():
    """the index list of sample and extract: forty rows at random, then the straddling row, an empty row, the long row, the
    last row with entries, the straddling row again and the last row again"""
    inside, long_row, last, empty = marked_rows()
    rows = len(structure()[0]) - 1
    return np.concatenate([np.random.default_rng(41).integers(0, rows, size=40), [inside, empty, long_row, last, inside, last]]).astype(np.int64)


def sparse_list():
    """extract's list with thousands of empty rows: 5000 between two copies of the straddling row (the first tile of gross
    entries), 4500 between two copies of the long row (the tile the first copy ends in): more rows than LDS holds ends of"""
    inside, long_row, last, empty = marked_rows()
    return np.concatenate([[inside], [empty] * 5000, [inside, long_row], [empty] * 4500, [long_row, last, last]]).astype(np.int64)


def column_map():
    """(map, out_cols): every third id dropped, the others renumbered in order"""
    keep = np.arange(COLS) % 3 != 0
    m = np.full(COLS, -1, dtype=np.int64)
    m[keep] = np.arange(int(keep.sum()))
    return m, int(keep.sum())


def extract_cases():
    """name -> (index list or None, map or None, out_cols)"""
    m, oc = column_map()
    return {"identity": (None, None, COLS), "list": (row_list(), None, COLS), "list and map": (row_list(), m, oc), "map": (None, m, oc),
            "empty rows and map": (sparse_list(), m, oc), "empty rows": (sparse_list(), None, COLS)}


def class_of(length, k, limits, maxima):
    """the kernel of topk.hip / sample.hip a row of `length` entries goes to under the options `limits` = (group_max, lds_max),
    which the library clamps to its constants `maxima`"""
    if length <= k:
        return "copy"
    return "group" if length <= min(limits[0], maxima[0]) else "lds" if length <= min(limits[1], maxima[1]) else "long"


# ---------------------------------------------------------------------------------------------------- helpers of the tests
def u_of(dtype):
    return np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32


def framed_c(want, cols, dtype):
    """(C, frames, its struct): a C whose three arrays are payload frames of exactly the expected sizes -- the call reuses them"""
    C, frames = TK.framed_c(len(want[0]) - 1, cols, len(want[1]), dtype)
    return C, frames, TK.struct_of(C)


def framed_result(C, frames, before, want, dtype):
    """C's struct stayed, the pads of the three frames hold the payload, the arrays are the expected ones: their bytes"""
    ro, ci, vb = want[:3]
    assert TK.struct_of(C) == before, "C's struct changed"
    got = (TK.framed(frames[2], len(ro) * 4, np.uint32), TK.framed(frames[1], len(ci) * 4, np.uint32),
           TK.framed(frames[0], len(ci) * np.dtype(dtype).itemsize, u_of(dtype)))
    assert np.array_equal(got[0], ro), ("row_offsets", np.nonzero(got[0] != ro)[0][:8])
    assert np.array_equal(got[1], ci), ("col_ids", np.nonzero(got[1] != ci)[0][:8])
    assert np.array_equal(got[2], vb), ("values", np.nonzero(got[2] != vb)[0][:8])
    return b"".join(g.tobytes() for g in got)


def twins(hi, lo, where):
    """the placements a case runs at: the view, and its low twin unless the view is the control itself"""
    return (hi,) if where == "low" else (hi, lo)


OUT_AT = 4 << 20                          # to_coo's outputs: this many bytes into the store of values


def to_coo_clear_of_the_values(cfg, p, iw, row_base, with_cols):
    """(status, row indices, column indices or None where none were asked for -- or written): speck_to_coo with both outputs
    clear of the bytes it takes for A's values.  It does not know the value type and refuses an output anywhere from 4 base
    to 8 (base + nnz) bytes behind A->data (speck_c_api.h) -- with float values up to 16 GiB behind the store, and that is
    where the allocator put this test's frames.  So the outputs lie where the place is known: in a free stretch of the
    store of values itself, 4 MiB from its start -- behind the low twin (2.4 MiB at the most) and far below every other
    placement --, each between two pads of the payload byte"""
    raw = p.store.vals.view(torch.uint8)
    nbytes, pad = p.n * iw, COO.PAD
    span = (4 * p.base, 8 * (p.base + p.n))
    assert OUT_AT >= 8 * (twin_base(p.base) + p.n) and (OUT_AT + 3 * pad + 2 * nbytes <= span[0] or OUT_AT >= span[1])
    stretch = raw[OUT_AT:OUT_AT + 3 * pad + 2 * nbytes]
    stretch.fill_(COO.PAYLOAD)
    torch.cuda.synchronize()
    at = raw.data_ptr() + OUT_AT + pad
    rc = sa._lib.load().speck_to_coo(cfg._h, COO.C_.byref(p.d._c), iw, row_base, at, at + nbytes + pad if with_cols else None)
    torch.cuda.synchronize()
    got = stretch.cpu().numpy()
    dt = np.int64 if iw == 8 else np.uint32
    row, col = got[pad:pad + nbytes], got[2 * pad + nbytes:2 * pad + 2 * nbytes]
    for a, b in ((0, pad), (pad + nbytes, 2 * pad + nbytes), (2 * pad + 2 * nbytes, len(got))):
        assert (got[a:b] == COO.PAYLOAD).all(), "a pad beside an output"
    if not with_cols or rc != OK:
        assert (col == COO.PAYLOAD).all(), "the columns' place was written"
    return rc, row.copy().view(dt), col.copy().view(dt) if with_cols else None


def tf(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


class Gradient:
    """G of the softmax backward for the placed view p: g (p's value type) in a free stretch of the store of ids, between
    sentinels; .d is a dCSR with p's offsets and ids whose data address is that stretch's minus p.base entries"""

    def __init__(self, p, where, g, slot):
        store, n, size = p.store, p.n, p.store.dtype.itemsize
        ids = store.ids
        self.vals = ids.view(torch.float32) if size == 4 else ids[:ids.numel() // 2 * 2].view(torch.float64)
        if size == 4 and slot == 0:
            at = other_base(where, p.base, n, n)
        else:
            at = twin_base(p.base) + (1 + slot) * (n + 2 * T + 77)
        self.at, self.n, self.g = at, n, g
        assert at >= GUARD and at + n + GUARD <= self.vals.numel()
        lo32, hi32 = (at - GUARD) * size // 4, (at + n + GUARD) * size // 4          # the stretch in entries of the ids
        assert hi32 <= p.lo or lo32 >= p.hi, "the gradient lies on the view's ids"
        self.span = (lo32, hi32)
        s = VALUE_SENTINEL[g.dtype]
        self.region = np.concatenate([np.full(GUARD, s), g, np.full(GUARD, s)])
        self.vals[at - GUARD:at + n + GUARD].copy_(torch.from_numpy(self.region))
        torch.cuda.synchronize()
        self.d = sa.dCSR.from_device(p.H.rows, p.H.cols, n, p.d._c.row_offsets, p.d._c.col_ids, ids.data_ptr() + (at - p.base) * size,
                                     dtype=g.dtype, keep=(p.d, ids), host_row_offsets=p.ro)

    def check_intact(self):
        torch.cuda.synchronize()
        got = self.vals[self.at - GUARD:self.at + self.n + GUARD].cpu().numpy()
        assert got.tobytes() == self.region.tobytes(), "the gradient or a sentinel beside it was written"


# ---------------------------------------------------------------------------------------------------- the tests, per value type
class HighOffsetsSide:
    """every test at the placements of its kind; the two classes below give the value type.  The float32 class comes first
    and, for every test, the control placement"""
    dtype = None
    PLACES = {}

    @pytest.fixture
    def store(self, stores):
        return stores.get(self.dtype)

    # ------------------------------------------------------------------------------------------------ topk
    @pytest.mark.parametrize("cls", list(TK.CLASSES))
    @places("all")
    def test_topk(self, cfg, store, where, cls):
        """all modes at k = 5 and 40 under the class setting `cls`: the row around 2^31 (straddle) and the last rows before
        0xFFFFFFFF (top) go through the copy kernel (k = 40) and the group, LDS or long-row kernel (k = 5); the long row is cut"""
        dtype = store.dtype.type
        H = tagged_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        try:
            TK.set_classes(cfg, cls)
            for by, mode in TK.MODES.items():
                for k in KS:
                    want = cached(("topk", store.dtype.name, by, k), lambda: TK.want_of(H, k, mode))
                    assert want[3]["rows_cut"] > 100 and want[3]["max_row_entries"] == k
                    seen = []
                    for p in twins(hi, lo, where):
                        C, frames, before = framed_c(want, H.cols, dtype)
                        rc, _, info = TK.call(cfg, p.d, k, mode, C=C)
                        assert rc == OK, (by, k)
                        seen.append(framed_result(C, frames, before, want, dtype))
                        assert vars(info) == want[3], (by, k)
                    assert len(set(seen)) == 1, (by, k)
        finally:
            TK.set_classes(cfg, "group")
        hi.check_intact(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ sample
    @pytest.mark.parametrize("cls", list(SP.CLASSES) + ["replace"])
    @places("all")
    def test_sample(self, cfg, store, where, cls):
        """without replacement under the three class settings, and with replacement; every row, and the list in both widths"""
        dtype = store.dtype.type
        H = tagged_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        mode = SP.WITH if cls == "replace" else SP.WITHOUT
        picks = row_list()
        try:
            if mode == SP.WITHOUT:
                SP.set_classes(cfg, cls)
            for k in KS:
                for itype, rows in ((torch.int64, picks), (torch.int32, picks), (torch.int64, None)):
                    want = cached(("sample", store.dtype.name, mode, k, rows is None), lambda: SP.want_of(H, k, SEED, rows, mode, ROW_BASE))
                    assert want[3]["rows_empty"] >= 1 and want[3]["max_row_entries"] == k
                    seen = []
                    for p in twins(hi, lo, where):
                        C, frames, before = framed_c(want, H.cols, dtype)
                        rc, _, info = SP.call(cfg, p.d, k, SEED, rows, mode, ROW_BASE, C=C, itype=itype)
                        assert rc == OK, (k, itype)
                        seen.append(framed_result(C, frames, before, want, dtype))
                        assert vars(info) == want[3], (k, itype)
                    assert len(set(seen)) == 1, (k, itype)
            if where == "low":
                # the wrapper's positions count from the start of A's buffers: minus the base they are the statement's, which
                # counts from the view's first entry.  (Above 2^31 the wrapper's second matrix, positions as doubles up to
                # base + nnz, would be a store of its own: the positions are held through the values' low bits there.)
                want = cached(("sample", store.dtype.name, mode, 5, False), lambda: SP.want_of(H, 5, SEED, picks, mode, ROW_BASE))
                C, info, pos = sa.sample_neighbors(hi.d, 5, SEED, rows=SP.index_tensor(picks, torch.int64), replace=mode == SP.WITH,
                                                   row_base=ROW_BASE, return_pos=True, cfg=cfg)
                SP.check(C, info, want, H.cols)
                assert np.array_equal(pos.cpu().numpy() - hi.base, want[4])
            elif store.dtype.itemsize == 8 and cls in ("group", "replace"):
                # above 2^31 the same by hand, where the doubles exist: the view's values ARE its absolute positions (what the
                # wrapper's second matrix holds), written over the view's span of the store alone
                P = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, hi.base + np.arange(H.nnz, dtype=np.float64))
                pp = place_view(store, where, P)
                assert pp.base == hi.base and float(pp.base + H.nnz - 1) == pp.base + H.nnz - 1
                want = cached(("sample", store.dtype.name, mode, 5, False), lambda: SP.want_of(H, 5, SEED, picks, mode, ROW_BASE))
                rc, C, info = SP.call(cfg, pp.d, 5, SEED, picks, mode, ROW_BASE)
                assert rc == OK and vars(info) == want[3]
                got = C.to_host()
                assert np.array_equal(got.data - pp.base, want[4].astype(np.float64)) and np.array_equal(got.col_ids, want[1])
                pp.check_intact()
                hi.write()                                                            # (the positions lay on the view's values)
        finally:
            SP.set_classes(cfg, "group")
        hi.check_intact(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ extract
    @pytest.mark.parametrize("iw", [8, 4], ids=["i64", "u32"])
    @places("all")
    def test_extract(self, cfg, store, where, iw):
        dtype = store.dtype.type
        H = tagged_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        for name, (rows, cmap, out_cols) in extract_cases().items():
            want = cached(("extract", store.dtype.name, name, iw), lambda: EX.want_of(H, rows, cmap, out_cols, iw))
            seen = []
            for p in twins(hi, lo, where):
                C, frames, before = framed_c(want, out_cols, dtype)
                rc, _, info = EX.call(cfg, p.d, rows, cmap, out_cols, iw, C=C)
                assert rc == OK, name
                seen.append(framed_result(C, frames, before, want, dtype))
                assert vars(info) == want[3], name
            assert len(set(seen)) == 1, name
            if name == "identity":                                                     # the host copy: offsets from 0
                assert want[0].tobytes() == H.row_offsets.tobytes() and want[1].tobytes() == H.col_ids.tobytes()
                assert want[2].tobytes() == H.data.tobytes()
        # the wrapper: the last row with entries alone (at the top it ends at 0xFFFFFFFF)
        last = marked_rows()[2]
        a, b = int(H.row_offsets[last]), int(H.row_offsets[last + 1])
        index = EX.dev_ids([last], iw)
        C, info = sa.gather_rows(hi.d, index, cfg)
        G = C.to_host()
        assert (C.rows, C.cols, C.nnz, info.gross) == (1, COLS, b - a, b - a) and G.row_offsets.tolist() == [0, b - a]
        assert G.col_ids.tobytes() == H.col_ids[a:b].tobytes() and G.data.tobytes() == H.data[a:b].tobytes()
        hi.check_intact(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ to_coo
    @pytest.mark.parametrize("iw", [8, 4], ids=["i64", "u32"])
    @places("all")
    def test_to_coo(self, cfg, store, where, iw):
        dtype = store.dtype.type
        H = tagged_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        dt = np.int64 if iw == 8 else np.uint32
        want_row = (np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64))) + ROW_BASE).astype(dt)
        for with_cols in (True, False):
            seen = []
            for p in twins(hi, lo, where):
                rc, got, ids = to_coo_clear_of_the_values(cfg, p, iw, ROW_BASE, with_cols)
                assert rc == OK, with_cols
                assert np.array_equal(got, want_row), np.nonzero(got != want_row)[0][:8]
                if with_cols:
                    assert np.array_equal(ids, H.col_ids.astype(dt)), np.nonzero(ids != H.col_ids.astype(dt))[0][:8]
                seen.append(got.tobytes() + (ids.tobytes() if with_cols else b""))
            assert len(set(seen)) == 1
        # there and back: the host copy, offsets from 0 (the values are the view's own, from its first entry on)
        rc, row, col = to_coo_clear_of_the_values(cfg, hi, iw, 0, True)
        assert rc == OK
        it = torch.int64 if iw == 8 else torch.int32
        row_t, col_t = (torch.from_numpy(a.view(np.int64 if iw == 8 else np.int32)).to(DEV) for a in (row, col))
        assert row_t.dtype == it
        back, info = sa.from_coo(row_t, col_t, store.vals.data_ptr() + hi.base * store.dtype.itemsize, (H.rows, H.cols), cfg, dtype=dtype,
                                 nnz=H.nnz)
        G = back.to_host()
        assert info.sorted_input == 1 and G.row_offsets.tobytes() == H.row_offsets.tobytes()
        assert G.col_ids.tobytes() == H.col_ids.tobytes() and G.data.tobytes() == H.data.tobytes()
        hi.check_intact(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ softmax
    @pytest.mark.parametrize("mode", ["normalized", "exp"])
    @places("all")
    def test_softmax_forward(self, cfg, store, where, mode):
        """into a new C and in place, m and s asked for: test_gpu_softmax's numpy_forward within the bound of its
        test_forward_accuracy (the exp alone takes fewer steps than the quotient that bound is stated for)"""
        dtype = store.dtype.type
        H = softmax_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        alpha = -1.0 if mode == "exp" else 1.0
        want, want_m, want_s = cached(("softmax", store.dtype.name, mode), lambda: SM.numpy_forward(H, alpha, mode))
        n = np.diff(H.row_offsets.astype(np.int64))
        row = SM.rows_of(H.row_offsets)
        full = n > 0
        seen = []
        for p in twins(hi, lo, where):
            m, s = SM.payload(H.rows), SM.payload(H.rows)
            C, info = sa.softmax(p.d, cfg, alpha=alpha, mode=mode, row_max=m, row_sum=s)
            G = C.to_host()
            assert (G.rows, G.cols, C.nnz) == (H.rows, H.cols, H.nnz)
            assert G.row_offsets.tobytes() == H.row_offsets.tobytes(), "C's offsets count from 0"
            assert G.col_ids.tobytes() == H.col_ids.tobytes()
            rel, floor = SM.bound(n[row], dtype)
            err = np.abs(G.data.astype(np.float64) - want)
            allowed = rel * np.abs(want) + floor
            print(f"softmax {mode} {store.dtype.name} at {where}: worst error / bound = {float((err / allowed).max()):.3f}")
            assert (err <= allowed).all(), (int((err > allowed).sum()), np.nonzero(err > allowed)[0][:8])
            got_m, got_s = SM.host(m), SM.host(s)
            assert got_m.tobytes() == want_m.tobytes(), "row_max (a maximum is exact)"
            rel, _ = SM.bound(n, np.float64)
            assert (np.abs(got_s - want_s)[full] <= (rel * want_s)[full]).all() and (got_s[~full] == 0).all()
            assert SM.as_tuple(info) == SM.counts(p.ro, G.data) and info.rows_split >= 1 and info.nonfinite == 0
            p.check_intact()
            # in place: the bytes of the new C, the structure untouched
            m2, s2 = SM.payload(H.rows), SM.payload(H.rows)
            same, info2 = sa.softmax(p.d, cfg, alpha=alpha, mode=mode, inplace=True, row_max=m2, row_sum=s2)
            assert same is p.d and p.entries()[1].tobytes() == G.data.tobytes()
            assert SM.host(m2).tobytes() == got_m.tobytes() and SM.host(s2).tobytes() == got_s.tobytes()
            assert SM.as_tuple(info2) == SM.as_tuple(info)
            p.check_structure()
            p.write()
            seen.append(G.data.tobytes() + got_m.tobytes() + got_s.tobytes())
        assert len(set(seen)) == 1

    @places("all")
    def test_softmax_backward(self, cfg, store, where):
        """r against math.fsum within reduce's bound; then the values bit for bit numpy's chain on that r (test_gpu_softmax's
        numpy_backward, whose r comes from a reduce call at offset 0 -- another tree than the one of this base)"""
        dtype = store.dtype.type
        S = softmax_matrix(dtype)
        H = cached(("probabilities", store.dtype.name), lambda: SM.probabilities(S, 71))
        g = cached(("gradient", store.dtype.name), lambda: SM.gradient(H, 72))
        hi, lo = place_with_twin(store, where, H)
        alpha = -2.0
        ro = H.row_offsets.astype(np.int64)
        p64, g64 = H.data.astype(np.float64), g.astype(np.float64)
        want_r, mags = cached(("backward sums", store.dtype.name), lambda: fsum_rows(p64 * g64, ro))
        row = SM.rows_of(ro)
        seen = []
        for slot, p in enumerate(twins(hi, lo, where)):
            G = Gradient(p, where, g, slot)
            r = SM.payload(H.rows)
            C, info = sa.softmax_backward(p.d, G.d, cfg, alpha=alpha, row_sum=r)
            got_r = SM.host(r)
            assert (np.abs(got_r - want_r) <= R.allowance(np.diff(ro), mags)).all()
            want = (alpha * (p64 * (g64 - got_r[row]))).astype(dtype)
            out_of_place_is(C, H, want, SM.same_bytes)
            assert SM.as_tuple(info) == SM.counts(p.ro, want) and info.rows_split >= 1
            p.check_intact(), G.check_intact()
            r2 = SM.payload(H.rows)
            same, info2 = sa.softmax_backward(p.d, G.d, cfg, alpha=alpha, inplace=True, row_sum=r2)
            assert same is p.d and p.entries()[1].tobytes() == C.to_host().data.tobytes() and SM.host(r2).tobytes() == got_r.tobytes()
            assert SM.as_tuple(info2) == SM.as_tuple(info)
            p.check_structure(), G.check_intact()
            p.write()
            seen.append(C.to_host().data.tobytes() + got_r.tobytes())
        assert len(set(seen)) == 1

    # ------------------------------------------------------------------------------------------------ the transpose plan
    @pytest.mark.parametrize("blocks", ["float64", "float32"])
    @places("all")
    def test_transpose_plan_spmm_t(self, cfg, store, where, blocks):
        """one plan made from the high view serves the view, its low twin and a copy; a plan made from the twin serves the
        view: integers, so numpy's A^T X exactly, and the same bytes from all of them"""
        dtype = store.dtype.type
        H = view_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        f32 = blocks == "float32"
        X5 = cached(("Xt", blocks), lambda: B32.ints((H.rows, 5), 51) if f32 else SPT.ints((H.rows, 5), 51))
        Y5 = cached(("Yt", blocks), lambda: B32.ints((COLS, 5), 52) if f32 else SPT.ints((COLS, 5), 52))
        with sa.transpose_plan(hi.d, cfg) as plan, sa.transpose_plan(lo.d, cfg) as plan_lo:
            assert (plan.info.rows, plan.info.cols, plan.info.nnz) == (H.rows, COLS, H.nnz) and vars(plan.info) == vars(plan_lo.info)
            copy = hi.d.copy()
            for k in (1, 3, 5):
                X, Y0 = X5[:, :k], Y5[:, :k]
                S = cached(("AtX", store.dtype.name, blocks, k), lambda: SPT.at_x(H, X.astype(np.float64)))
                counts = SPT.counts(SPT.t_offsets(H), k)
                for alpha, beta in ((1.0, 0.0), (2.0, -3.0)):
                    y0 = Y0 if beta else None
                    exact = alpha * S + beta * Y0.astype(np.float64) if beta else alpha * S
                    seen = []
                    for d, pl in ((hi.d, plan), (lo.d, plan), (copy, plan), (hi.d, plan_lo)):
                        if not f32:
                            got, info = SPT.run(cfg, d, X, pl, alpha, beta, y0)
                            assert np.array_equal(got, exact), (k, alpha, np.argwhere(got != exact)[:8])
                            seen.append(SPT.bits(got).tobytes())
                        else:
                            for form in B32_LDS:
                                ld = dict(ldx=8, ldy=8) if form == "aligned" else {}
                                got, info = B32.spmm_t32(cfg, d, X, alpha, beta, y0, plan=pl, **ld)
                                assert B32.same_bytes(got, B32.narrow(exact)), (k, alpha, form, B32.where_differ(got, B32.narrow(exact)))
                                seen.append(B32.b32(got).tobytes())
                        assert SPT.as_tuple(info) == counts
                        if beta:
                            break                                                      # (the other three with beta = 0 alone)
                    if not beta:                                                       # the view, its twin, the copy; both plans
                        assert len(seen) >= 4 and len(set(seen)) == 1, (k, alpha)
                if f32:                                                              # the double call on the widened blocks, narrowed
                    wide, info64 = B32.spmm_t64(cfg, hi.d, X, 2.0, -3.0, Y0, plan=plan)
                    assert B32.same_bytes(wide, B32.narrow(2.0 * S - 3.0 * Y0.astype(np.float64))) and SPT.as_tuple(info64) == counts
            if not f32:
                x = X5[:, 0]
                y, info = sa.spmv_t(hi.d, V.tv(x), cfg, plan=plan)
                assert np.array_equal(y, SPT.at_x(H, x[:, None])[:, 0]) and SPT.as_tuple(info) == SPT.counts(SPT.t_offsets(H), 1)
        hi.check_intact(), lo.check_intact()

    # ------------------------------------------------------------------------------------------------ float blocks
    @pytest.mark.parametrize("k", [3, 5])
    @places("all")
    def test_spmm_b32(self, cfg, store, where, k):
        dtype = store.dtype.type
        H = view_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        X = cached("X32", lambda: B32.ints((COLS, 5), 61))[:, :k]
        Y0 = cached("Y32", lambda: B32.ints((H.rows, 5), 62))[:, :k]
        S = cached(("S32", store.dtype.name, k), lambda: B32.row_sums(H, X))
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
            y0 = Y0 if beta else None
            want = B32.narrow(alpha * S + beta * Y0.astype(np.float64) if beta else alpha * S)
            wide, info64 = B32.spmm64(cfg, hi.d, X, alpha, beta, y0)                    # the double call, narrowed
            assert B32.same_bytes(wide, want), (alpha, B32.where_differ(wide, want))
            for form in B32_LDS:
                ld = dict(ldx=8, ldy=8) if form == "aligned" else {}
                for p in twins(hi, lo, where):
                    got, info = B32.spmm32(cfg, p.d, X, alpha, beta, y0, **ld)
                    assert B32.same_bytes(got, want), (alpha, form, B32.where_differ(got, want))
                    M.check_info(info, p.ro, k)
                    assert p is not hi or B32.as_tuple(info) == B32.as_tuple(info64)
        hi.check_intact(), lo.check_intact()

    @pytest.mark.parametrize("k", [3, 5])
    @places("all")
    def test_sddmm_b32(self, cfg, store, where, k):
        dtype = store.dtype.type
        H = view_matrix(dtype)
        hi, lo = place_with_twin(store, where, H)
        U = cached("U32", lambda: B32.ints((H.rows, 5), 63))[:, :k]
        W = cached("W32", lambda: B32.ints((COLS, 5), 64))[:, :k]
        d = cached(("d32", k), lambda: D.exact(H, U.astype(np.float64), W.astype(np.float64)))
        for alpha, beta, mode in ((-3.0, 2.0, "axpby"), (0.5, 0.0, "hadamard")):
            want = D.expect(d, H.data, dtype, alpha, beta, mode)
            kw = dict(alpha=alpha, beta=beta, mode=mode)
            wide, info64 = sa.sddmm(hi.d, tf(U).double(), tf(W).double(), cfg, **kw)    # the double call on the widened blocks
            out_of_place_is(wide, H, want, D.same_bytes)
            for form in B32_LDS:
                ldu, ldv = (8, 8) if form == "aligned" else (k + 3, k + 2)
                dU, dW = B32.padded(U, ldu), B32.padded(W, ldv)
                for p in twins(hi, lo, where):
                    C, info = sa.sddmm(p.d, dU, dW, cfg, blocks="float32", **kw)
                    out_of_place_is(C, H, want, D.same_bytes)
                    assert C.to_host().data.tobytes() == wide.to_host().data.tobytes(), (mode, form)
                    assert D.as_tuple(info) == D.counts(p.ro, k, want)
                    p.check_intact()
                    same, info = sa.sddmm(p.d, dU, dW, cfg, blocks="float32", inplace=True, **kw)
                    assert same is p.d and p.entries()[1].tobytes() == wide.to_host().data.tobytes(), (mode, form)
                    assert D.as_tuple(info) == D.counts(p.ro, k, want)
                    p.check_structure()
                    p.write()
            assert D.as_tuple(info64) == D.counts(hi.ro, k, want)

    # ------------------------------------------------------------------------------------------------ hostile input at height
    @places("hostile")
    def test_hostile_offsets_at_height_are_refused_and_nothing_is_written(self, cfg, store, where):
        """a descending pair, a declared nnz one larger than the offsets span, one offset below the base: every one of the
        seven families refuses all three with SPECK_ERR_INVALID, and nothing is written"""
        dtype = store.dtype.type
        H = view_matrix(dtype)
        p = place_view(store, where, H)
        picks, (cmap, out_cols) = row_list(), column_map()
        k = 3
        X64, X32 = SPT.ints((H.rows, k), 81), B32.ints((H.rows, k), 82)
        Xc32, U32, W32 = B32.ints((COLS, k), 83), B32.ints((H.rows, k), 84), B32.ints((COLS, k), 85)
        G = Gradient(p, where, SM.gradient(H, 73), 0)
        with sa.transpose_plan(p.d, cfg) as plan:
            for name, bad in hostile_views(p):
                # topk, sample, extract: C in frames that the call would reuse
                for call in (lambda C: TK.call(cfg, bad, 5, TK.MODES["abs"], C=C), lambda C: SP.call(cfg, bad, 5, SEED, picks, SP.WITHOUT, ROW_BASE, C=C),
                             lambda C: SP.call(cfg, bad, 5, SEED, None, SP.WITH, ROW_BASE, C=C),
                             lambda C: EX.call(cfg, bad, picks, cmap, out_cols, 8, C=C), lambda C: EX.call(cfg, bad, None, None, COLS, 4, C=C)):
                    C, frames = TK.framed_c(H.rows, COLS, 1234, dtype)
                    before = TK.struct_of(C)
                    rc, _, info = call(C)
                    assert rc == ERR_INVALID, name
                    assert TK.struct_of(C) == before and not any(vars(info).values()) and TK.untouched(*frames), name
                # to_coo
                for iw in (8, 4):
                    bad_p = type("View", (), dict(store=store, n=p.n, base=p.base, d=bad))
                    rc, row, _ = to_coo_clear_of_the_values(cfg, bad_p, iw, ROW_BASE, True)
                    assert rc == ERR_INVALID and (row.view(np.uint8) == COO.PAYLOAD).all(), name
                # softmax: into a new C, and in place
                for mode in ("normalized", "exp"):
                    dC, struct_before, s = sentinel_output(H.rows, COLS, dtype)
                    m, sm = SM.payload(H.rows), SM.payload(H.rows)
                    for kw in (dict(matOut=dC), dict(inplace=True)):
                        with pytest.raises(sa.SpeckError) as e:
                            sa.softmax(bad, cfg, mode=mode, row_max=m, row_sum=sm, **kw)
                        assert e.value.status == ERR_INVALID, name
                    assert untouched(dC, struct_before, s) and SM.is_payload(SM.host(m)) and SM.is_payload(SM.host(sm)), name
                # ... and backward, the gradient at the view's absolute entries
                dC, struct_before, s = sentinel_output(H.rows, COLS, dtype)
                r = SM.payload(H.rows)
                for kw in (dict(matOut=dC), dict(inplace=True)):
                    with pytest.raises(sa.SpeckError) as e:
                        sa.softmax_backward(bad, G.d, cfg, alpha=-2.0, row_sum=r, **kw)
                    assert e.value.status == ERR_INVALID, name
                assert untouched(dC, struct_before, s) and SM.is_payload(SM.host(r)), name
                G.check_intact()
                # the plan: none is made from such a view, and the sound view's does not fit it
                with pytest.raises(sa.SpeckError) as e:
                    sa.transpose_plan(bad, cfg)
                assert e.value.status == ERR_INVALID, name
                xb, xs = SPT.frame(H.rows, k + 3, k, X64)
                yb, ys = SPT.frame(COLS, k + 2, k)
                assert SPT.raw(cfg, plan, bad, xs.data_ptr(), k + 3, k, ys.data_ptr(), k + 2) == ERR_INVALID and SPT.untouched(yb), name
                # float blocks: spmm_t, spmm, sddmm
                for call, n_x, n_y, X in ((lambda xs, ys: sa.spmm_t(bad, xs, cfg, plan=plan, Y=ys, blocks="float32"), H.rows, COLS, X32),
                                          (lambda xs, ys: sa.spmm(bad, xs, cfg, Y=ys, blocks="float32"), COLS, H.rows, Xc32)):
                    xb, xs = B32.frame(n_x, k + 3, k, X)
                    yb, ys = B32.frame(n_y, k + 2, k)
                    with pytest.raises(sa.SpeckError) as e:
                        call(xs, ys)
                    assert e.value.status == ERR_INVALID and B32.untouched(yb), name
                dC, struct_before, s = sentinel_output(H.rows, COLS, dtype)
                dU, dW = B32.padded(U32, k + 3), B32.padded(W32, k + 2)
                for kw in (dict(matOut=dC), dict(inplace=True)):
                    with pytest.raises(sa.SpeckError) as e:
                        sa.sddmm(bad, dU, dW, cfg, blocks="float32", **kw)
                    assert e.value.status == ERR_INVALID, name
                assert untouched(dC, struct_before, s), name
                p.check_intact(bad)
            # the config and the plan serve the sound view right after
            want = TK.want_of(H, 5, TK.MODES["abs"])
            rc, C, info = TK.call(cfg, p.d, 5, TK.MODES["abs"])
            assert rc == OK
            TK.check(C, info, want, COLS)
            got, _ = SPT.run(cfg, p.d, X64, plan)
            assert np.array_equal(got, SPT.at_x(H, X64))
        p.check_intact()


class TestFloat32(HighOffsetsSide):
    dtype = F32
    PLACES = {"all": ["low", "straddle", "above", "top"], "hostile": ["straddle", "top"]}


class TestFloat64(HighOffsetsSide):
    """(no placement at the top: the float64 values up to 2^32 would take 32 GiB, 48 GiB with the ids)"""
    dtype = np.dtype(np.float64)
    PLACES = {"all": ["low", "straddle", "above"], "hostile": ["straddle"]}
