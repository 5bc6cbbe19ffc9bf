"""speck_spmv_sr_* / speck_spmm_sr_* on the GPU (speck_amd/csrc/semiring.hip) and the two loops of speck_amd/graph.py.  The
expectation is the numpy restatement of tests/test_semiring_host.py (`restate`): min and max are exact and every term is one
IEEE operation, so the comparison is np.array_equal(..., equal_nan=True) -- exact in value, blind only to the sign of a
zero, never a tolerance.  Every y lives in a tensor or frame filled with a payload NaN: what a call must not write still
holds the payload afterwards.  T = 4096 entries per tile below."""
import ctypes as C_
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse import csgraph

import speck_amd as sa
from speck_amd import _lib
from test_semiring_host import NAMES, cc_case, restate, same_partition, sssp_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
DTYPES = [np.float64, np.float32]
T = sa.SPMV_TILE_ENTRIES
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
COLS = 3000
TAIL = 8                                # payload words behind the last row of a frame
INF, NAN = np.inf, np.nan


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def mk(lens, data, cols=COLS, seed=1, col=None):
    """rows of the given lengths over `data`; column ids random in [0, cols) unless given, duplicates allowed, unsorted"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = np.random.default_rng(seed).integers(0, cols, size=len(data)).astype(np.uint32) if col is None else np.asarray(col, np.uint32)
    return sa.HostCSR(len(lens), cols, ro, ci, np.asarray(data))


def ints(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).integers(-1024, 1025, size=shape).astype(dtype)


def real_values(shape, seed, dtype=np.float64):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(dtype)


def want(H, X, name, Z=None, r0=0, r1=None):
    """(Y, changed) by numpy for the rows [r0, r1) of H; X and Z with one column per right-hand side"""
    r1 = H.rows if r1 is None else r1
    return restate(H.row_offsets[r0:r1 + 1], H.col_ids, H.data, X, name, Z)


def counts(ro, k=1):
    """what speck_semiring_info reports about A, counted on the host (ro absolute)"""
    ro = np.asarray(ro, dtype=np.int64)
    s, e = ro[:-1], ro[1:]
    full = e > s
    nnz = int(ro[-1] - ro[0]) if len(ro) else 0
    return (int((~full).sum()), int(((e[full] - 1) // T > s[full] // T).sum()),
            int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0, nnz, nnz * k)


def check_info(info, ro, k, changed):
    got = (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms, info.changed)
    assert got == counts(ro, k) + (changed,), (got, counts(ro, k), changed)


def tv(a):
    """a float64 vector on the device (one element at least, so that it has an address)"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(1)).to(DEV)


def sentinel(n):
    return torch.from_numpy(np.full(max(n, 1), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, expect):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(expect, dtype=np.float64), equal_nan=True)


def frame(n, ld, k, vals=None, lead=0):
    """(buffer, block): a device buffer of the payload NaN that holds an n x k block in rows ld apart, `lead` words from its
    start and TAIL words from its end; the block is the torch view [:, :k] of those rows and holds vals"""
    buf = torch.from_numpy(np.full(lead + n * ld + TAIL, SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
    blk = buf[lead:lead + n * ld].view(n, ld)[:, :k]
    if vals is not None and n and k:
        blk.copy_(torch.from_numpy(np.array(vals, dtype=np.float64)).to(DEV))
    return buf, blk


def read_frame(buf, n, ld, k, lead=0):
    """the n x k block of a frame on the host, after checking that every other word still holds the payload"""
    full = host(buf)
    rows = full[lead:lead + n * ld].reshape(n, ld)
    assert (bits(full[:lead]) == SENTINEL_BITS).all(), "in front of Y"
    assert (bits(rows[:, k:]) == SENTINEL_BITS).all(), "the padding of Y"
    assert (bits(full[lead + n * ld:]) == SENTINEL_BITS).all(), "behind the last row of Y"
    return rows[:, :k].copy()


def run_v(cfg, dA, x, name, z=None):
    """one spmv_sr into a y that held the payload: (y on the host as a column, info); x, z numpy or tensors"""
    dx = x if torch.is_tensor(x) else tv(x)
    dz = z if z is None or torch.is_tensor(z) else tv(z)
    y = sentinel(dA.rows)
    torch.cuda.synchronize()
    out, info = sa.spmv_sr(dA, dx, cfg, semiring=name, z=dz, y=y[:max(dA.rows, 1)] if dA.rows else y.data_ptr())
    assert out is None
    return host(y)[:dA.rows].reshape(-1, 1), info


def run_b(cfg, dA, X, name, Z=None, ldx=None, ldy=None, ldz=None, x_lead=0):
    """one spmm_sr on padded blocks (ldx = k + 3, ldy = k + 2, ldz = k + 1 unless given) passed as torch column slices: (Y on
    the host, info); Y held the payload"""
    k = X.shape[1]
    ldx = k + 3 if ldx is None else ldx
    ldy = k + 2 if ldy is None else ldy
    ldz = k + 1 if ldz is None else ldz
    xb, xs = frame(dA.cols, ldx, k, X, lead=x_lead)
    yb, ys = frame(dA.rows, ldy, k)
    zs = None if Z is None else frame(dA.rows, ldz, k, Z)[1]
    torch.cuda.synchronize()                                      # (torch filled the frames on its own stream)
    out, info = sa.spmm_sr(dA, xs, cfg, semiring=name, Z=zs, Y=ys)
    assert out is None
    return read_frame(yb, dA.rows, ldy, k), info


def edge_lens():
    """(row lengths) laid out against the tile edges; the comments give the entries a row holds"""
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


_CACHE = {}
K_MAX = 9


def edge_case(dtype, real=False):
    """(H, X with K_MAX columns, Z with K_MAX columns), computed once: integers, or values over twelve decades"""
    key = ("edge", np.dtype(dtype).name, real)
    if key not in _CACHE:
        lens = edge_lens()
        gen = real_values if real else ints
        H = mk(lens, gen(sum(lens), 11, dtype), seed=12)
        X, Z = gen((COLS, K_MAX), 13), gen((H.rows, K_MAX), 14)
        for a in (H.row_offsets, H.col_ids, H.data, X, Z):
            a.setflags(write=False)
        _CACHE[key] = (H, X, Z)
    return _CACHE[key]


def edge_want(dtype, real, name, k, with_z):
    """the restatement for the first k columns of edge_case, computed once"""
    key = ("want", np.dtype(dtype).name, real, name, k, with_z)
    if key not in _CACHE:
        H, X, Z = edge_case(dtype, real)
        _CACHE[key] = want(H, X[:, :k], name, Z[:, :k] if with_z else None)
    return _CACHE[key]


def on_torch(H, ro=None, col=None, nnz=None, r0=0, r1=None, shift=0, data="own"):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz, a view; shift = 1 puts
    a dummy entry in front of data and col_ids and advances both pointers by one element; data = None: a NULL data pointer,
    "nan": an array of NaNs"""
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    r1 = H.rows if r1 is None else r1
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    vals = np.full(len(H.data), NAN, dtype=H.data.dtype) if isinstance(data, str) and data == "nan" else H.data
    va = np.concatenate([np.full(shift, 77, dtype=H.data.dtype), vals, np.zeros(1, dtype=H.data.dtype)])
    ci = np.concatenate([np.zeros(shift, dtype=np.uint32), np.asarray(col, dtype=np.uint32), np.zeros(1, dtype=np.uint32)])
    t_va = torch.from_numpy(va).to(DEV)
    t_ci = torch.from_numpy(ci.view(np.int32)).to(DEV)
    if nnz is None:
        nnz = int(H.row_offsets[r1]) - int(H.row_offsets[r0])
    return sa.dCSR.from_device(r1 - r0, H.cols, nnz, t_ro.data_ptr() + 4 * r0, t_ci.data_ptr() + 4 * shift,
                               None if data is None else t_va.data_ptr() + H.data.itemsize * shift, dtype=H.data.dtype,
                               keep=(t_ro, t_va, t_ci))


# ---------------------------------------------------------------------------------------------------- 1: tile edges
@pytest.mark.parametrize("real", [False, True], ids=["integers", "twelve_decades"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_at_every_tile_edge(cfg, dtype, real):
    H, X, Z = edge_case(dtype, real)
    dA, dx, dz = sa.dCSR.from_host(H), tv(X[:, 0]), tv(Z[:, 0])
    for name in NAMES:
        expect, _ = edge_want(dtype, real, name, 1, False)
        got, info = run_v(cfg, dA, dx, name)
        assert same(got, expect), (name, np.nonzero(got != expect)[0][:8])
        check_info(info, H.row_offsets, 1, 0)
        expect, changed = edge_want(dtype, real, name, 1, True)
        got, info = run_v(cfg, dA, dx, name, z=dz)
        assert same(got, expect), (name, "z", np.nonzero(got != expect)[0][:8])
        check_info(info, H.row_offsets, 1, changed)
        assert 0 < changed < H.rows
    empty = np.nonzero(np.diff(H.row_offsets.astype(np.int64)) == 0)[0]
    assert (run_v(cfg, dA, dx, "min_times")[0][empty] == INF).all() and (run_v(cfg, dA, dx, "max_second")[0][empty] == -INF).all()


# ---------------------------------------------------------------------------------------------------- 2: a long chain
CHAIN_LEAD, CHAIN_LEN = 100, 70 * T     # the long row holds the absolute entries [100, 100 + 70 T): tiles 0 .. 70
CHAIN_SPOTS = {"head tile": 50, "whole tile 1": T - CHAIN_LEAD + 7, "whole tile 65": 65 * T - CHAIN_LEAD + 7,
               "tail tile": 70 * T - CHAIN_LEAD + 50, "first entry": 0, "last entry": CHAIN_LEN - 1}


def test_a_row_of_seventy_tiles_finds_its_extremum_wherever_it_lies(cfg):
    """chain_finish's lane loop goes past 64 tiles: the one entry that decides the row lies, in turn, in every part of it"""
    lens = [CHAIN_LEAD - 40, 40, CHAIN_LEN, 3, 0, 7]
    n = sum(lens)
    rng = np.random.default_rng(21)
    special = COLS - 1                                             # the column only the deciding entry points at
    col = rng.integers(0, special, size=n).astype(np.uint32)
    data = 1.0 + rng.random(n)                                     # in [1, 2)
    dA_cache = {}
    for spot, idx in CHAIN_SPOTS.items():
        p = CHAIN_LEAD + idx
        c, a = col.copy(), data.copy()
        c[p], a[p] = special, 1.0
        H = mk(lens, a, col=c)
        assert H.row_offsets[2] == CHAIN_LEAD and p // T == {"head tile": 0, "whole tile 1": 1, "whole tile 65": 65,
                                                             "tail tile": 70, "first entry": 0, "last entry": 70}[spot]
        dA_cache[spot] = (H, sa.dCSR.from_host(H))
    for name in NAMES:
        x = 1.0 + rng.random((COLS, 1))
        x[special] = -1.0e6 if name.startswith("min") else 1.0e6
        decided = {"plus": x[special, 0] + 1.0, "times": x[special, 0], "second": x[special, 0]}[name.split("_")[1]]
        dx = tv(x)
        for spot, (H, dA) in dA_cache.items():
            got, info = run_v(cfg, dA, dx, name)
            expect, _ = want(H, x, name)
            assert same(got, expect), (name, spot)
            assert got[2, 0] == decided, (name, spot)
            check_info(info, H.row_offsets, 1, 0)
            assert info.tiles == 71 and info.rows_split == 1


# ---------------------------------------------------------------------------------------------------- 3: views, alignment
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_with_an_odd_base_and_arrays_off_their_boundaries_give_the_same_values(cfg, dtype):
    H, X, Z = edge_case(dtype, True)
    whole = sa.dCSR.from_host(H)
    r0, r1 = 4, H.rows - 2
    assert H.row_offsets[r0] % 2 == 1
    view = whole.row_view(r0, r1)
    shifted = on_torch(H, shift=1)
    assert shifted._c.data % 16 and shifted._c.col_ids % 16
    dx = tv(X[:, 0])
    for name in NAMES:
        full, _ = run_v(cfg, whole, dx, name)
        assert same(full, edge_want(dtype, True, name, 1, False)[0])
        part, info = run_v(cfg, view, dx, name, z=Z[r0:r1, 0])
        expect, changed = want(H, X[:, :1], name, Z[r0:r1, :1], r0, r1)
        assert same(part, expect) and same(expect, np.minimum(Z[r0:r1, :1], full[r0:r1]) if name.startswith("min")
                                           else np.maximum(Z[r0:r1, :1], full[r0:r1])), name
        check_info(info, H.row_offsets[r0:r1 + 1], 1, changed)
        got, _ = run_v(cfg, shifted, dx, name)                     # entry by entry
        assert bits(got).tobytes() == bits(full).tobytes(), name
    # the block: X on a 16-byte boundary with an even ld (16-byte gathers), off it by one element, and with an odd ld
    k = 5
    for name in ("min_plus", "max_times", "min_second"):
        expect, _ = edge_want(dtype, True, name, k, False)
        seen = []
        for ldx, lead in ((k + 3, 0), (k + 3, 1), (k + 2, 0), (k + 2, 1)):
            for dA in (whole, shifted):
                got, _ = run_b(cfg, dA, X[:, :k], name, ldx=ldx, x_lead=lead)
                assert same(got, expect), (name, ldx, lead)
                seen.append(bits(got).tobytes())
        assert len(set(seen)) == 1, name
        part, _ = run_b(cfg, view, X[:, :k], name, ldx=k + 2, x_lead=1)
        assert same(part, expect[r0:r1]), name


# ---------------------------------------------------------------------------------------------------- 4: special values
def special_case(dtype):
    """eight rows over eight columns; column 7 of x is +inf, column 6 NaN, column 5 -inf"""
    #        row 0       1        2         3          4            5        6       7
    lens = [2,          1,       2,        2,         2,           0,       1,      3]
    col = [0, 1,        7,       7, 2,     7, 3,      6, 0,                 5,      1, 2, 3]
    a = [1.0, 2.0,      3.0,     -INF, 1,  0.0, 1.0,  1.0, 1.0,             2.0,    NAN, 1.0, 1.0]
    return mk(lens, np.array(a, dtype=dtype), cols=8, col=col)


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinities_and_nans_land_in_the_rows_and_the_column_that_reference_them(cfg, dtype):
    H = special_case(dtype)
    dA = sa.dCSR.from_host(H)
    x = np.array([4.0, 5.0, 6.0, 7.0, 8.0, -INF, NAN, INF])
    nan_rows = {"min_plus": [2, 4, 7],        # -inf + inf; a NaN of x; a NaN of A
                "max_plus": [2, 4, 7],
                "min_times": [3, 4, 7],       # 0 * inf
                "max_times": [3, 4, 7],
                "min_second": [4],            # the NaN of x alone: A's values are not read
                "max_second": [4]}
    for name in NAMES:
        got, _ = run_v(cfg, dA, x, name)
        expect, _ = want(H, x[:, None], name)
        assert same(got, expect), name
        assert np.nonzero(np.isnan(got[:, 0]))[0].tolist() == nan_rows[name], name
    got, _ = run_v(cfg, dA, x, "min_plus")
    assert got[1, 0] == INF and got[5, 0] == INF and got[6, 0] == -INF and got[0, 0] == 5.0     # unreached stays +inf
    # a NaN of z lands in its row and nowhere else, and counts as unchanged where the result is a NaN as well
    z = np.array([1.0, NAN, 100.0, 1.0, NAN, 3.0, 0.0, 2.0])
    got, info = run_v(cfg, dA, x, "min_plus", z=z)
    expect, changed = want(H, x[:, None], "min_plus", z[:, None])
    assert same(got, expect) and np.nonzero(np.isnan(got[:, 0]))[0].tolist() == [1, 2, 4, 7]
    assert info.changed == changed == 3                           # rows 2 and 7 became NaN, row 6 -inf; rows 1 and 4: NaN on both sides
    # the block: the specials in column 1 of three only
    X = np.tile(np.array([4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])[:, None], (1, 3))
    X[:, 1] = x
    for name in NAMES:
        got, _ = run_b(cfg, dA, X, name)
        expect, _ = want(H, X, name)
        assert same(got, expect), name
        assert np.nonzero(np.isnan(got[:, 1]))[0].tolist() == nan_rows[name], name
        other = [7] if "second" not in name else []               # the NaN of A reaches every column
        assert np.nonzero(np.isnan(got[:, 0]))[0].tolist() == other == np.nonzero(np.isnan(got[:, 2]))[0].tolist(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_never_reads_the_values(cfg, dtype):
    H, X, _ = edge_case(dtype, False)
    for data in ("nan", None):
        dA = on_torch(H, data=data)
        assert data is not None or not dA._c.data
        for name in ("min_second", "max_second"):
            got, info = run_v(cfg, dA, X[:, 0], name)
            assert same(got, edge_want(dtype, False, name, 1, False)[0]) and not np.isnan(got).any(), (data, name)
            check_info(info, H.row_offsets, 1, 0)
            got, _ = run_b(cfg, dA, X[:, :3], name)
            assert same(got, edge_want(dtype, False, name, 3, False)[0]), (data, name)
    L = _lib.load()
    fn = L.speck_spmv_sr_f32 if dtype == np.float32 else L.speck_spmv_sr_f64
    y, dx, hollow = sentinel(H.rows), tv(X[:, 0]), on_torch(H, data=None)
    assert fn(cfg._h, sa.SR_MIN_PLUS, C_.byref(hollow._c), dx.data_ptr(), None, y.data_ptr(), None) == ERR_INVALID   # read there
    assert (bits(host(y)) == SENTINEL_BITS).all()


# ---------------------------------------------------------------------------------------------------- 5: z
@pytest.mark.parametrize("dtype", DTYPES)
def test_z_absent_in_place_equal_to_x_and_apart(cfg, dtype):
    rng = np.random.default_rng(31)
    n = 1500
    lens = rng.integers(0, 12, size=n)
    lens[700] = T + 9                                             # one split row
    H = mk(lens, ints(int(lens.sum()), 32, dtype), cols=n, seed=33)
    dA = sa.dCSR.from_host(H)
    x = ints((n, 1), 34)
    x[::50] = NAN                                                 # rows that are NaN before and after
    for name in ("min_plus", "max_plus", "min_second", "max_times"):
        s, _ = want(H, x, name)
        # no z: the payload is wholly overwritten, nothing counts as changed
        got, info = run_v(cfg, dA, x, name)
        assert same(got, s) and info.changed == 0, name
        # z == x on a square matrix: a relaxation step between two buffers
        expect, changed = want(H, x, name, x)
        dx = tv(x)
        got, info = run_v(cfg, dA, dx, name, z=dx)
        assert same(got, expect) and info.changed == changed and 0 < changed < n, name
        assert same(host(dx), x[:, 0])
        nan_both = int((np.isnan(expect) & np.isnan(x)).sum())
        assert nan_both >= n // 50 and changed <= n - nan_both
        # z == y: in place
        y = tv(x)
        out, info = sa.spmv_sr(dA, dx, cfg, semiring=name, z=y, y=y)
        assert out is None and same(host(y), expect[:, 0]) and info.changed == changed, name
        out, info = sa.spmv_sr(dA, dx, cfg, semiring=name, z=y, y=y)            # (+) is idempotent
        assert same(host(y), expect[:, 0]) and info.changed == 0, name
        # z apart from both
        z = ints((n, 1), 35)
        expect, changed = want(H, x, name, z)
        got, info = run_v(cfg, dA, dx, name, z=z)
        assert same(got, expect) and info.changed == changed, name
    # the library's own result buffer
    out, info = sa.spmv_sr(dA, tv(x), cfg, semiring="min_plus")
    assert same(out[:, None], want(H, x, "min_plus")[0])
    out, info = sa.spmm_sr(dA, tv(x).view(n, 1), None, semiring="max_plus", Z=tv(x).view(n, 1))   # no config
    expect, changed = want(H, x, "max_plus", x)
    assert same(out, expect) and info.changed == changed


# ---------------------------------------------------------------------------------------------------- 6: hostile input
def hostile(H):
    """(offsets, column ids, declared nnz) -- one change each"""
    ro, nnz = H.row_offsets, H.nnz
    assert nnz % T and nnz > 8 * T
    for p in (0, T - 1, T, 5 * T - 1, 8 * T, nnz - 1):               # the first and last entry of a tile, the partial last tile
        col = H.col_ids.copy()
        col[p] = H.cols
        yield ro, col, nnz
    bad = ro.copy()
    bad[1024] = bad[1025] + 1                                      # a descending pair
    yield bad, None, nnz
    yield ro, None, nnz + 1                                        # the last offset is short of nnz
    yield ro, None, nnz - 1                                        # ... and beyond it


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_of_y_is_written(cfg, dtype):
    H, X, Z = edge_case(dtype, False)
    good, dx, dz = sa.dCSR.from_host(H), tv(X[:, 0]), tv(Z[:, 0])
    L = _lib.load()
    fv, fb = (L.speck_spmv_sr_f32, L.speck_spmm_sr_f32) if dtype == np.float32 else (L.speck_spmv_sr_f64, L.speck_spmm_sr_f64)
    k, ldx, ldy = 3, 4, 5
    xb, xs = frame(H.cols, ldx, k, X[:, :k])
    for i, (ro, col, nnz) in enumerate(hostile(H)):
        dA = on_torch(H, ro=ro, col=col, nnz=nnz)
        sr = i % 6
        y = sentinel(H.rows)
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)
        torch.cuda.synchronize()
        rc = fv(cfg._h, sr, C_.byref(dA._c), dx.data_ptr(), dz.data_ptr() if i % 2 else None, y.data_ptr(), C_.byref(info))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, i
        assert (bits(host(y)) == SENTINEL_BITS).all(), i
        assert tuple(getattr(info, f) for f, _ in info._fields_) == (0,) * 6, i
        yb, ys = frame(H.rows, ldy, k)
        info = _lib.CSemiringInfo(7, 7, 7, 7, 7, 7)
        rc = fb(cfg._h, sr, C_.byref(dA._c), xs.data_ptr(), ldx, k, None, 0, ys.data_ptr(), ldy, C_.byref(info))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, i
        assert (bits(host(yb)) == SENTINEL_BITS).all(), i
        assert tuple(getattr(info, f) for f, _ in info._fields_) == (0,) * 6, i
        got, _ = run_v(cfg, good, dx, NAMES[sr])                   # the config serves a valid call right after
        assert same(got, edge_want(dtype, False, NAMES[sr], 1, False)[0]), i


# ---------------------------------------------------------------------------------------------------- 7: blocks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9])
def test_every_block_form_and_each_column_equal_to_the_vector_call(cfg, dtype, k):
    H, X, Z = edge_case(dtype, True)
    dA = sa.dCSR.from_host(H)
    for name in ("min_plus", "max_times", "max_second"):
        expect, changed = edge_want(dtype, True, name, k, True)
        for ldx in (k + 3, k + 2):                                 # pairs of columns in one load, and single loads
            got, info = run_b(cfg, dA, X[:, :k], name, Z=Z[:, :k], ldx=ldx)
            assert same(got, expect), (name, ldx)
            check_info(info, H.row_offsets, k, changed)
        for c in sorted({0, k // 2, k - 1}):
            col, _ = run_v(cfg, dA, np.ascontiguousarray(X[:, c]), name, z=np.ascontiguousarray(Z[:, c]))
            assert bits(col[:, 0]).tobytes() == bits(got[:, c]).tobytes(), (name, c)


def test_thirty_three_columns_and_a_thousand_on_three_rows(cfg):
    H, X9, _ = edge_case(np.float64, True)
    X = np.concatenate([X9, real_values((COLS, 24), 41)], axis=1)
    got, info = run_b(cfg, sa.dCSR.from_host(H), X, "min_plus")
    assert same(got, want(H, X, "min_plus")[0])
    check_info(info, H.row_offsets, 33, 0)
    k = sa.SPMM_MAX_RHS
    small = mk([T + 5, 0, 40], ints(T + 45, 42), cols=50, seed=43)
    X, Z = ints((50, k), 44), ints((3, k), 45) * 1000.0
    for name in ("max_plus", "min_times"):
        expect, changed = want(small, X, name, Z)
        got, info = run_b(cfg, sa.dCSR.from_host(small), X, name, Z=Z)
        assert same(got, expect), name
        check_info(info, small.row_offsets, k, changed)


def test_slices_of_wider_tensors_in_place_blocks_and_interleaved_ones(cfg):
    H, X, Z = edge_case(np.float64, False)
    dA = sa.dCSR.from_host(H)
    k = 4
    expect, changed = edge_want(np.float64, False, "min_plus", k, True)
    # Y and Z are the same column slice of a wider tensor: in place, the padding keeps the payload
    ld, lead = 7, 2
    xs = frame(H.cols, k + 1, k, X[:, :k])[1]
    wide = torch.from_numpy(np.full((H.rows, ld), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
    ys = wide[:, lead:lead + k]
    ys.copy_(torch.from_numpy(Z[:, :k].copy()).to(DEV))
    torch.cuda.synchronize()
    out, info = sa.spmm_sr(dA, xs, cfg, semiring="min_plus", Z=ys, Y=ys)
    after = host(wide)
    assert out is None and same(after[:, lead:lead + k], expect) and info.changed == changed
    assert (bits(after[:, :lead]) == SENTINEL_BITS).all() and (bits(after[:, lead + k:]) == SENTINEL_BITS).all()
    # Z == X on a square matrix, blocks
    n = 600
    lens = np.random.default_rng(51).integers(0, 9, size=n)
    sq = mk(lens, ints(int(lens.sum()), 53), cols=n, seed=52)
    D = ints((n, 3), 54)
    xs = frame(n, 3, 3, D)[1]
    yb, ys = frame(n, 5, 3)
    torch.cuda.synchronize()
    out, info = sa.spmm_sr(sa.dCSR.from_host(sq), xs, cfg, semiring="max_plus", Z=xs, Y=ys)
    expect, changed = want(sq, D, "max_plus", D)
    assert same(read_frame(yb, n, 5, 3), expect) and info.changed == changed and same(host(xs), D)
    # two column slices of ONE tensor interleave: refused, nothing written; the same for Z against Y
    both = torch.from_numpy(np.full((max(COLS, H.rows), 2 * k), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
    apart = frame(H.cols, k, k, X[:, :k])[1]
    for kwargs in ({"X": both[:COLS, :k], "Y": both[:H.rows, k:]}, {"X": apart, "Z": both[:H.rows, :k], "Y": both[:H.rows, 1:k + 1]}):
        with pytest.raises(sa.SpeckError) as e:
            sa.spmm_sr(dA, kwargs.pop("X"), cfg, **kwargs)
        assert e.value.status == ERR_INVALID
    assert (bits(host(both)) == SENTINEL_BITS).all()


# ---------------------------------------------------------------------------------------------------- 8: twice, streams
def test_two_calls_give_the_same_bytes_and_the_callers_stream_is_honoured(cfg):
    H, X, Z = edge_case(np.float64, True)
    dA = sa.dCSR.from_host(H)
    for name in NAMES:
        a, _ = run_b(cfg, dA, X[:, :5], name, Z=Z[:, :5])
        b, _ = run_b(cfg, dA, X[:, :5], name, Z=Z[:, :5])
        assert bits(a).tobytes() == bits(b).tobytes(), name
        a, _ = run_v(cfg, dA, X[:, 0], name)
        b, _ = run_v(cfg, dA, X[:, 0], name)
        assert bits(a).tobytes() == bits(b).tobytes(), name
    # x is written by a copy on the caller's stream right before the call: ordering against the producer is by the stream
    real, dx, y = tv(X[:, 0]), tv(np.zeros(COLS)), sentinel(H.rows)
    real5 = frame(COLS, 5, 5, X[:, :5])[1]
    xb, xs = frame(COLS, 5, 5, np.zeros((COLS, 5)))
    yb, ys = frame(H.rows, 6, 5)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream works on zeros
            dx.copy_(real, non_blocking=True)
            xs.copy_(real5, non_blocking=True)
        sa.spmv_sr(dA, dx, cfg, semiring="min_plus", y=y)
        sa.spmm_sr(dA, xs, cfg, semiring="max_times", Y=ys)
        assert same(host(y)[:, None], edge_want(np.float64, True, "min_plus", 1, False)[0])
        assert same(read_frame(yb, H.rows, 6, 5), edge_want(np.float64, True, "max_times", 5, False)[0])
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched_and_degenerate_shapes(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        H, X, Z = edge_case(dtype, False)
        dA = sa.dCSR.from_host(H)
        for name in ("min_plus", "max_second"):                    # (a touched zone is status 3)
            assert same(run_v(cfg, dA, X[:, 0], name, z=Z[:, 0])[0], edge_want(dtype, False, name, 1, True)[0])
            assert same(run_b(cfg, dA, X[:, :9], name, Z=Z[:, :9])[0], edge_want(dtype, False, name, 9, True)[0])
        # no entry at all: the identity, or z
        none = mk([0] * 300, np.zeros(0, dtype=dtype), cols=7)
        d0 = sa.dCSR.from_host(none)
        z = ints((300, 2), 61)
        got, info = run_v(cfg, d0, np.ones(7), "min_plus")
        assert (got == INF).all() and (info.rows_empty, info.tiles, info.changed) == (300, 0, 0)
        got, info = run_b(cfg, d0, np.ones((7, 2)), "max_times", Z=z)
        assert same(got, z) and info.changed == 0
        got, info = run_b(cfg, d0, np.ones((7, 2)), "max_times")
        assert (got == -INF).all()
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_the_caller_that_includes_semiring_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_semiring.cpp")
    out = str(tmp_path / "caller_semiring")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "semiring caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)


# ---------------------------------------------------------------------------------------------------- 9: the two loops
def to_device(M, dtype=np.float64):
    M = M.tocsr()
    M.sort_indices()
    return sa.dCSR.from_host(sa.HostCSR(M.shape[0], M.shape[1], M.indptr.astype(np.uint32), M.indices.astype(np.uint32),
                                        M.data.astype(dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sssp_equals_dijkstra(cfg, dtype):
    A, At, sources = sssp_case()
    dist, iterations, converged = sa.sssp(to_device(At, dtype), sources, cfg)
    assert converged and iterations == 20
    assert np.array_equal(dist, csgraph.dijkstra(A, directed=True, indices=sources).T)
    assert int(np.isinf(dist).sum()) == 625 and (dist[np.isinf(dist)] > 0).all()


def test_connected_components_gives_scipys_partition_and_the_smallest_id(cfg):
    S = cc_case()
    labels, iterations = sa.connected_components(to_device(S), cfg)
    n_comp, ref = csgraph.connected_components(S, directed=False)
    assert iterations == 16 and n_comp == 291 == len(set(labels.tolist()))
    assert same_partition(labels, ref)
    smallest = np.full(n_comp, S.shape[0])
    np.minimum.at(smallest, ref, np.arange(S.shape[0]))
    assert np.array_equal(labels, smallest[ref])
    # the values are never read: the same labels from the pattern alone
    P = S.copy()
    P.data[:] = NAN
    assert np.array_equal(sa.connected_components(to_device(P), cfg)[0], labels)


def test_a_path_needs_as_many_steps_as_vertices_and_a_negative_cycle_stops_at_the_bound(cfg):
    path = sp.csr_matrix((np.ones(299), (np.arange(1, 300), np.arange(299))), shape=(300, 300))     # in-edges: i-1 -> i
    dist, iterations, converged = sa.sssp(to_device(path), [0], cfg)
    assert (iterations, converged) == (300, True) and np.array_equal(dist[:, 0], np.arange(300.0))
    cyc = sp.csr_matrix((np.array([1.0, 1.0, -3.0]), (np.array([1, 2, 0]), np.array([0, 1, 2]))), shape=(3, 3))
    dist, iterations, converged = sa.sssp(to_device(cyc), [0], cfg, max_iters=10)
    assert (iterations, converged) == (10, False) and (dist < 0).any()
