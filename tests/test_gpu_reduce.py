"""speck_reduce_* on the GPU (speck_amd/csrc/reduce.hip).  The expectation is numpy / math.fsum in this file: reduceat over
the rows that hold entries (integer values: every order gives the same bits, so equality), math.fsum for real values
with the bound of any summation order, (g_n + 2^-53) sum|term| with g_n = n 2^-53 / (1 - n 2^-53) -- the extra ulp is the
reference's own rounding.  Extrema by equality; a NaN matches a NaN.  T = 4096 entries per tile below."""
import ctypes as C_
import math
import struct

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
DTYPES = [np.float64, np.float32]
OPS = ["sum", "abs_sum", "sq_sum", "max", "min", "abs_max"]
SUMS = ("sum", "abs_sum", "sq_sum")
T = sa.REDUCE_TILE_ENTRIES
PER_THREAD, PER_WAVE = sa.REDUCE_THREAD_ENTRIES, sa.REDUCE_WAVE_ENTRIES
IDENT = {"sum": 0.0, "abs_sum": 0.0, "sq_sum": 0.0, "abs_max": 0.0, "max": -math.inf, "min": math.inf}
U = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def mk(lens, data):
    """rows of the given lengths over `data`; the column ids (never read) count up inside a row"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = (np.arange(len(data), dtype=np.int64) - np.repeat(ro[:-1].astype(np.int64), lens)).astype(np.uint32)
    return sa.HostCSR(len(lens), int(lens.max(initial=0)) + 1, ro, ci, np.asarray(data))


def ints(n, seed, dtype):
    return np.random.default_rng(seed).integers(-1024, 1025, size=n).astype(dtype)


def terms_of(data, op):
    d = np.asarray(data).astype(np.float64)
    return np.abs(d) if op in ("abs_sum", "abs_max") else d * d if op == "sq_sum" else d


def ref_exact(ro, data, op):
    """(row results, total) by numpy: ro counts from the first entry of data"""
    t = terms_of(data, op)
    ro = np.asarray(ro, dtype=np.int64)
    rows = np.full(len(ro) - 1, IDENT[op])
    full = np.nonzero(ro[1:] > ro[:-1])[0]
    with np.errstate(invalid="ignore"):
        if len(full):
            fn = np.add if op in SUMS else np.minimum if op == "min" else np.maximum
            rows[full] = fn.reduceat(t, ro[:-1][full])
        if len(t) == 0:
            total = IDENT[op]
        else:
            total = float(np.sum(t)) if op in SUMS else float(np.min(t)) if op == "min" else float(np.max(t))
    return rows, total


def same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True)


def counts(ro):
    """what speck_reduce_info reports, counted on the host (ro absolute)"""
    ro = np.asarray(ro, dtype=np.int64)
    s, e = ro[:-1], ro[1:]
    full = e > s
    nnz = int(ro[-1] - ro[0])
    return dict(rows_empty=int((~full).sum()), rows_split=int(((e[full] - 1) // T > s[full] // T).sum()),
                tiles=int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0, entries=nnz)


def check_info(info, ro):
    want = counts(ro)
    assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == \
        (want["rows_empty"], want["rows_split"], want["tiles"], want["entries"]), (info, want)


def check_exact(cfg, H, dA=None, ops=OPS):
    dA = dA if dA is not None else sa.dCSR.from_host(H)
    for op in ops:
        rows, total, info = sa.reduce(dA, cfg, op)
        want_rows, want_total = ref_exact(H.row_offsets, H.data, op)
        assert same(rows, want_rows), (op, np.nonzero(~((rows == want_rows) | (np.isnan(rows) & np.isnan(want_rows))))[0][:8])
        assert same(total, want_total), (op, total, want_total)
        check_info(info, H.row_offsets)
    return dA


def edge_lens():
    """case 1: (row lengths) laid out against the tile edges; the comments give the entries a row holds"""
    return ([0,                # an empty first row
             T,                # [0, T): a row that is a tile
             0,                # an empty row exactly at T
             1,                # [T, T + 1): the first entry of a tile
             T - 3,            # [T + 1, 2T - 2)
             1,                # [2T - 2, 2T - 1): ends at T - 1 of its tile
             1,                # [2T - 1, 2T): the last entry of a tile
             0,                # an empty row exactly at 2T
             T - 1,            # [2T, 3T - 1)
             2 * T + 2,        # [3T - 1, 5T + 1): four tiles, two of them wholly inside
             99,               # [5T + 1, 5T + 100)
             T - 50,           # [5T + 100, 6T + 50): split ...
             T - 40,           # [6T + 50, 7T + 10): ... and split: the two meet in tile 6
             T - 10]           # [7T + 10, 8T)
            + [0] * 5000 +     # more rows without entries than a tile has entries, between two tiles
            [5,                # [8T, 8T + 5)
             2,                # [8T + 5, 8T + 7)
             0])               # an empty last row


_EDGE = {}


def edge_matrix(dtype):
    key = np.dtype(dtype).name
    if key not in _EDGE:
        lens = edge_lens()
        _EDGE[key] = mk(lens, ints(sum(lens), 11, dtype))
    return _EDGE[key]


def real_values(n, seed, dtype):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.random(n)) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(dtype)


_REAL = {}


def real_matrix(dtype):
    """case 3: row lengths from 0 to 3T, with the reference per op, computed once: (H, {op: (rows, sum|term| per row, ...)})"""
    key = np.dtype(dtype).name
    if key not in _REAL:
        rng = np.random.default_rng(5)
        lens = [0, 1, 7, 100, T - 1, T, T + 1, 3 * T, 0, 2 * T + 5, 33, 1000, 3 * T - 1, 17, 0, 0, 2, T + T // 2]
        lens += [int(x) for x in rng.integers(0, 60, size=400)]
        H = mk(lens, real_values(sum(lens), 6, dtype))
        ref = {}
        ro = H.row_offsets.astype(np.int64)
        for op in OPS:
            t = terms_of(H.data, op)
            if op in SUMS:
                rows = np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])])
                mags = np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])])
                ref[op] = (rows, mags, math.fsum(t), math.fsum(np.abs(t)))
            else:
                ref[op] = ref_exact(ro, H.data, op)
        _REAL[key] = (H, ref)
    return _REAL[key]


def allowance(n, mag):
    n = np.asarray(n, dtype=np.float64)
    return (n * U / (1.0 - n * U) + U) * mag


def check_bound(H, ref, op, rows, total, r0=0, r1=None):
    r1 = H.rows if r1 is None else r1
    ro = H.row_offsets.astype(np.int64)
    if op in SUMS:
        want, mags = ref[op][0][r0:r1], ref[op][1][r0:r1]
        if rows is not None:
            err = np.abs(rows - want)
            ok = err <= allowance(ro[r0 + 1:r1 + 1] - ro[r0:r1], mags)
            assert ok.all(), (op, np.nonzero(~ok)[0][:8], err[~ok][:8])
        if total is not None:
            t = terms_of(H.data[ro[r0]:ro[r1]], op)
            assert abs(total - math.fsum(t)) <= allowance(len(t), math.fsum(np.abs(t))), (op, total)
    else:
        if rows is not None:
            assert same(rows, ref[op][0][r0:r1]), op
        if total is not None:
            assert same(total, ref_exact([0, ro[r1] - ro[r0]], H.data[ro[r0]:ro[r1]], op)[1]), op


def sentinel_tensor(n):
    return torch.from_numpy(np.full(max(n, 1), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)


def bits_of(t):
    return t.cpu().numpy().view(np.uint64)


def on_torch(H, ro=None, col="ids", nnz=None, r0=0, r1=None):
    """H in torch tensors, as a dCSR that owns nothing: other offsets, garbage or no column ids, a declared nnz, a view"""
    ro = H.row_offsets if ro is None else ro
    r1 = H.rows if r1 is None else r1
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    t_va = torch.from_numpy(np.ascontiguousarray(H.data).copy()).to(DEV) if H.nnz else torch.zeros(1, dtype=torch.float64, device=DEV)
    t_ci = torch.full((max(H.nnz, 1),), -1, dtype=torch.int32, device=DEV)
    if nnz is None:
        nnz = int(H.row_offsets[r1]) - int(H.row_offsets[r0])
    return sa.dCSR.from_device(r1 - r0, H.cols, nnz, t_ro.data_ptr() + 4 * r0, t_ci.data_ptr() if col == "ids" else None,
                               t_va.data_ptr(), dtype=H.data.dtype, keep=(t_ro, t_va, t_ci))


# ---------------------------------------------------------------------------------------------------- 1: tile edges, exact
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_at_every_tile_edge(cfg, dtype):
    H = edge_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    assert {T - 1, 0, 1} <= set((ro % T).tolist()) and T in ro and 2 * T in ro and 8 * T in ro   # rows end at T - 1, T, T + 1
    want = counts(ro)
    assert want["tiles"] == 9 and want["rows_split"] == 3 and want["rows_empty"] == 5004
    check_exact(cfg, H)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_smallest_matrices(cfg, dtype):
    check_exact(cfg, mk([1], np.array([-3], dtype=dtype)))
    check_exact(cfg, mk([0, 0, 0], np.zeros(0, dtype=dtype)))
    empty = sa.HostCSR(0, 1, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))
    dA = sa.dCSR.from_host(empty)
    for op in OPS:
        rows, total, info = sa.reduce(dA, cfg, op)
        assert len(rows) == 0 and struct.pack("<d", total) == struct.pack("<d", IDENT[op])
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == (0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------- 2: lane, thread, wave edges
LENGTHS = [1, 2, 3, 4, 5, PER_THREAD - 1, PER_THREAD, PER_THREAD + 1, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, T - 1, T, T + 1]


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_one_length(cfg, dtype, length):
    n = (2 * T + 100) // length + 3
    check_exact(cfg, mk([length] * n, ints(n * length, 20 + length, dtype)))


# ---------------------------------------------------------------------------------------------------- 3: the bound
@pytest.mark.parametrize("dtype", DTYPES)
def test_real_values_within_the_bound_of_any_order(cfg, dtype):
    H, ref = real_matrix(dtype)
    dA = sa.dCSR.from_host(H)
    for op in OPS:
        rows, total, info = sa.reduce(dA, cfg, op)
        check_bound(H, ref, op, rows, total)
        check_info(info, H.row_offsets)


# ---------------------------------------------------------------------------------------------------- 4: reproducible; views
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_a_view_gives_the_rows_of_the_whole(cfg, dtype):
    H, ref = real_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    dA = sa.dCSR.from_host(H)
    # r0: behind a split row, in the tile that row ends in, not on a tile edge; r1: in the middle of a tile
    r0 = next(r for r in range(1, H.rows) if ro[r] % T and ro[r] > ro[r - 1] and (ro[r] - 1) // T > ro[r - 1] // T)
    r1 = next(r for r in range(H.rows - 1, r0, -1) if ro[r] % T and ro[r] // T > ro[r0] // T + 2)
    assert ro[r0] % T and ro[r1] % T and ro[r1] < ro[-1]
    for op in OPS:
        out1, out2 = sentinel_tensor(H.rows), sentinel_tensor(H.rows)
        _, t1, _ = sa.reduce(dA, cfg, op, out_ptr=out1.data_ptr())
        _, t2, _ = sa.reduce(dA, cfg, op, out_ptr=out2.data_ptr())
        torch.cuda.synchronize()
        whole = bits_of(out1)
        assert whole.tobytes() == bits_of(out2).tobytes() and struct.pack("<d", t1) == struct.pack("<d", t2)
        for a, b in ((r0, H.rows), (r0, r1), (0, r1)):
            rows, total, info = sa.reduce(dA.row_view(a, b), cfg, op)
            assert rows.view(np.uint64).tobytes() == whole[a:b].tobytes(), (op, a, b)
            check_bound(H, ref, op, None, total, a, b)
            want = counts(ro[a:b + 1])
            assert (info.rows_empty, info.rows_split, info.tiles, info.entries) == \
                (want["rows_empty"], want["rows_split"], want["tiles"], want["entries"])


# ---------------------------------------------------------------------------------------------------- 5: special values
def special_matrix(dtype, with_nan):
    nan = np.nan if with_nan else 1.0
    tiny = float(np.finfo(dtype).smallest_subnormal)
    long_row = ints(3 * T, 31, np.float64)
    rows = [[1, 2, 3], [1, nan, 2], [4, -5], [nan, nan], [7], [np.inf, 1, -np.inf], [-6, 2], [np.inf, 3], [9],
            [-0.0, -0.0], [-8], [tiny, 3 * tiny, -2 * tiny], [], [5, 5], list(long_row), [-4, 1], []]
    start = sum(len(r) for r in rows[:14])
    mid = start + T + T // 2                                  # in a tile that lies wholly inside the long row
    assert start // T + 1 <= mid // T < (start + 3 * T - 1) // T
    rows[14][mid - start] = nan
    data = np.array([x for r in rows for x in r], dtype=np.float64).astype(dtype)
    return mk([len(r) for r in rows], data), ([1, 3, 14] if with_nan else [])


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inf_zero_and_subnormal_rows(cfg, dtype):
    H, nan_rows = special_matrix(dtype, True)
    dA = sa.dCSR.from_host(H)
    for op in OPS:
        rows, total, _ = sa.reduce(dA, cfg, op)
        assert np.isnan(rows[nan_rows]).all() and math.isnan(total), op       # a NaN is never hidden ...
        want, _ = ref_exact(H.row_offsets, H.data, op)
        assert same(rows, want), op                                            # ... and touches no other row
        for r in (12, 16):                                                     # the identities, as bit patterns
            assert struct.pack("<d", rows[r]) == struct.pack("<d", IDENT[op]), (op, r)
    check_exact(cfg, special_matrix(dtype, False)[0])                          # the IEEE results without the NaNs


# ---------------------------------------------------------------------------------------------------- 6: hostile offsets
def hostile(H):
    """(offsets, declared nnz, first row, last row) -- one change each"""
    ro, rows, nnz = H.row_offsets, H.rows, H.nnz
    for i in (1, rows - 1, 1023, 1024, 1025):                      # a descending pair
        bad = ro.copy()
        bad[i] = bad[i + 1] + 1
        yield bad, nnz, 0, rows
    bad = ro.copy()
    bad[rows] = nnz + 5                                            # above base + nnz
    yield bad, nnz, 0, rows
    bad = ro.copy()
    bad[0] = bad[1] + 1                                            # the first above the second
    yield bad, nnz, 0, rows
    yield ro, nnz + 1, 0, rows                                     # the last offset does not span nnz: an owner ...
    yield ro, nnz - 1, 0, rows
    a, b = 3, rows - 2                                             # ... and a view
    span = int(ro[b]) - int(ro[a])
    yield ro, span + 1, a, b
    yield ro, span - 1, a, b


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_offsets_are_refused_and_nothing_is_written(cfg, dtype):
    H = edge_matrix(dtype)
    good = sa.dCSR.from_host(H)
    L = _lib.load()
    fn = L.speck_reduce_f32 if dtype == np.float32 else L.speck_reduce_f64
    for k, (ro, nnz, a, b) in enumerate(hostile(H)):
        dA = on_torch(H, ro=ro, nnz=nnz, r0=a, r1=b)
        out = sentinel_tensor(b - a)
        total = C_.c_double(struct.unpack("<d", struct.pack("<Q", SENTINEL_BITS))[0])
        before = bytes(total)
        torch.cuda.synchronize()
        op = k % len(OPS)
        rc = fn(cfg._h, C_.byref(dA._c), op, out.data_ptr(), C_.byref(total), None)
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, k
        assert (bits_of(out) == SENTINEL_BITS).all() and bytes(total) == before, k
        check_exact(cfg, H, dA=good, ops=[OPS[op]])                # the config serves a valid call right after


# ---------------------------------------------------------------------------------------------------- 7: column ids are not read
@pytest.mark.parametrize("col", ["ids", None])
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_ids_are_never_read(cfg, dtype, col):
    H = edge_matrix(dtype)
    check_exact(cfg, H, dA=on_torch(H, col=col))


# ---------------------------------------------------------------------------------------------------- 8: plumbing
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config(dtype):
    check_exact(None, edge_matrix(dtype), ops=["sum", "min"])


def test_runs_on_the_callers_stream(cfg):
    """the values are written by a copy on the caller's stream right before the call: ordering against the producer is by
    the stream alone"""
    H = edge_matrix(np.float64)
    dA = on_torch(H)
    t_va = dA._keep[1]
    real = t_va.clone()
    t_va.zero_()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream sums zeros
            t_va.copy_(real, non_blocking=True)
        check_exact(cfg, H, dA=dA, ops=["abs_sum"])
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        check_exact(cfg, edge_matrix(dtype))                                   # (a touched zone is status 3)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_alone_total_alone_and_a_result_that_stays_on_the_device(cfg, dtype):
    H = edge_matrix(dtype)
    dA = sa.dCSR.from_host(H)
    for op in ("sq_sum", "max"):
        want_rows, want_total = ref_exact(H.row_offsets, H.data, op)
        rows, total, info = sa.reduce(dA, cfg, op, total=False)
        assert total is None and same(rows, want_rows)
        check_info(info, H.row_offsets)
        rows, total, info = sa.reduce(dA, cfg, op, rows=False)
        assert rows is None and same(total, want_total)
        check_info(info, H.row_offsets)
        out = torch.zeros(H.rows, dtype=torch.float64, device=DEV)
        rows, total, _ = sa.reduce(dA, cfg, op, out_ptr=out.data_ptr())
        torch.cuda.synchronize()
        assert rows is None and same(total, want_total) and same(out.cpu().numpy(), want_rows)


def test_a_reduce_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.08, 7, signed=True)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()
    for _ in range(3):
        sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"]
    sa.MultiplyspECK(dS, dS, dC, cfg)
    without = cfg.last_stats()["replayed"]
    first = dC.to_host()
    _, total, _ = sa.reduce(dS, cfg, "sum")
    assert abs(total - math.fsum(h.data)) <= allowance(h.nnz, math.fsum(np.abs(h.data)))
    sa.reduce(dC, cfg, "abs_max")                                              # ... and of the product itself, where it lies
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == without
    again = dC.to_host()                                                       # (the product sums through atomics: last bits move)
    assert again.col_ids.tobytes() == first.col_ids.tobytes() and np.allclose(again.data, first.data, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------- 9: the triangle count
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_triangle_count_ends_on_the_device(cfg, dtype):
    P = sp.random(300, 300, density=4 / 300, random_state=91, format="csr")
    P.data[:] = 1.0
    P.sort_indices()
    S = ((P + P.T) != 0).astype(np.float64).tocsr()
    Ls = sp.tril(S, k=-1).tocsr()
    per_row = np.asarray((Ls @ Ls).multiply(Ls).sum(axis=1)).ravel()
    triangles = int(per_row.sum())
    assert triangles > 0
    HP = sa.HostCSR(300, 300, P.indptr.astype(np.uint32), P.indices.astype(np.uint32), P.data.astype(dtype))
    dL = sa.tril(sa.symmetrize(sa.dCSR.from_host(HP), cfg), cfg, k=-1)
    dC, minfo = sa.multiply_masked(dL, dL, dL, cfg)
    rows, total, info = sa.reduce(dC, cfg, "sum")                              # (the product is never downloaded)
    assert total == minfo.hits == triangles
    assert same(rows, per_row) and info.entries == dC.nnz


# ---------------------------------------------------------------------------------------------------- 10: real row laws, small
@pytest.mark.parametrize("kind", ["webbase", "cant"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_standins_and_their_squares(cfg, dtype, kind):
    h = sa.gen_matrix(kind, 0.05, 3, signed=True)
    h = sa.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data.astype(dtype))
    dS, dC = sa.dCSR.from_host(h), sa.dCSR(dtype)
    sa.MultiplyspECK(dS, dS, dC, cfg)
    for d, H in ((dS, h), (dC, dC.to_host())):
        ro = H.row_offsets.astype(np.int64)
        t = H.data.astype(np.float64)
        n = ro[1:] - ro[:-1]
        rows, total, info = sa.reduce(d, cfg, "sum")
        want = np.array([math.fsum(t[a:b]) for a, b in zip(ro[:-1], ro[1:])])
        mags = np.array([math.fsum(np.abs(t[a:b])) for a, b in zip(ro[:-1], ro[1:])])
        assert (np.abs(rows - want) <= allowance(n, mags)).all()
        assert abs(total - math.fsum(t)) <= allowance(len(t), math.fsum(np.abs(t)))
        check_info(info, ro)
        rows, total, _ = sa.reduce(d, cfg, "abs_max")
        want_rows, want_total = ref_exact(ro, H.data, "abs_max")
        assert same(rows, want_rows) and total == want_total
