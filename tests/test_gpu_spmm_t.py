"""speck_tplan_* and speck_spmm_t_* on the GPU (speck_amd/csrc/extras.hip, spmm_t.hip): Y = alpha A^T X + beta Y through a
transpose plan, X (rows x k) and Y (cols x k) in padded row-major blocks.  The expectation is numpy / scipy / math.fsum in
this file: with integer values every order gives the same bits, so equality (every sum stays below 2^53); for real values
the defining property, byte equality of every column with speck_spmm_* on speck_transpose_*(A), and against math.fsum the
bound of any summation order, (g_n + 2^-53) sum|t| with g_n = n 2^-53 / (1 - n 2^-53) and t = a.astype(f64) * X[row, c]
-- the extra ulp is the reference's own rounding.  Every Y lives in a frame filled with a payload NaN: the padding between
its rows and the words around it must still hold the payload after every call, and after a refused call the whole frame
does.  Every hostile input is refused by a check before anything is followed.  T = 4096 plan entries per tile below; CB is
the number of columns the tile kernel takes per round."""
import ctypes as C_
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
OK, ERR_INVALID, ERR_DIM_LIMIT = 0, 1, 2
DTYPES = [np.float64, np.float32]
T = sa.SPMV_TILE_ENTRIES
CB = sa.SPMM_COLUMN_BLOCK
KS = sorted({1, 2, 3, CB, CB + 1, 2 * CB + 1, 9})
K_MAX = max(KS)
U = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
TAIL = 8                                # payload words behind the last row of a frame
LEAD = 4                                # ... and in front of the first


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def from_pairs(rows, cols, r, c, data, seed=1):
    """the CSR of the entries (r[i], c[i], data[i]): inside a row in a shuffled order, so rows are unsorted and duplicates
    of one (i, j) lie apart"""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    p = np.random.default_rng(seed).permutation(len(r))
    p = p[np.argsort(r[p], kind="stable")]
    ro = np.zeros(rows + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(np.bincount(r, minlength=rows))
    return sa.HostCSR(rows, cols, ro, c[p].astype(np.uint32), np.asarray(data)[p])


def with_col_lens(rows, col_lens, dtype, seed, values):
    """a matrix whose column j holds col_lens[j] entries, in random rows (few rows: many duplicates)"""
    col_lens = np.asarray(col_lens, dtype=np.int64)
    n = int(col_lens.sum())
    c = np.repeat(np.arange(len(col_lens)), col_lens)
    r = np.random.default_rng(seed).integers(0, rows, size=n)
    return from_pairs(rows, len(col_lens), r, c, values(n, seed + 1, dtype), seed=seed + 2)


def ints(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).integers(-1024, 1025, size=shape).astype(dtype)


def real_values(shape, seed, dtype=np.float64):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(dtype)


def row_of(H):
    return np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))


def at_x(H, X):
    """scipy's A^T X (exact for integers: every order gives the same bits)"""
    A = sp.csr_matrix((H.data.astype(np.float64), H.col_ids.astype(np.int64), H.row_offsets.astype(np.int64)), shape=(H.rows, H.cols))
    return np.asarray(A.T @ X)


def t_offsets(H):
    """t_ro on the host"""
    t_ro = np.zeros(H.cols + 1, dtype=np.int64)
    t_ro[1:] = np.cumsum(np.bincount(H.col_ids.astype(np.int64), minlength=H.cols))
    return t_ro


def counts(t_ro, k):
    """what speck_spmm_t_info reports, counted on the host's t_ro"""
    s, e = t_ro[:-1], t_ro[1:]
    full = e > s
    nnz = int(t_ro[-1]) if len(t_ro) else 0
    return (int((~full).sum()), int(((e[full] - 1) // T > s[full] // T).sum()), (nnz + T - 1) // T, nnz, nnz * k)


def as_tuple(info):
    return (info.cols_empty, info.cols_split, info.tiles, info.entries, info.terms)


def frame(n, ld, k, vals=None, lead=LEAD):
    """(buffer, block): a device buffer of the payload NaN that holds an n x k block in rows ld apart, `lead` words from its
    start and TAIL words from its end; the block is the torch view [:, :k] of those rows and holds vals"""
    buf = torch.from_numpy(np.full(lead + n * ld + TAIL, SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
    blk = buf[lead:lead + n * ld].view(n, ld)[:, :k]
    if vals is not None and n and k:
        blk.copy_(torch.from_numpy(np.array(vals, dtype=np.float64)).to(DEV))
    return buf, blk


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def read_frame(buf, n, ld, k, lead=LEAD):
    """the n x k block of a frame on the host, after checking that every other word still holds the payload"""
    full = host(buf)
    rows = full[lead:lead + n * ld].reshape(n, ld)
    assert (bits(full[:lead]) == SENTINEL_BITS).all(), "in front of Y"
    assert (bits(rows[:, k:]) == SENTINEL_BITS).all(), "the padding of Y"
    assert (bits(full[lead + n * ld:]) == SENTINEL_BITS).all(), "behind the last row of Y"
    return rows[:, :k].copy()


def untouched(buf):
    return bool((bits(host(buf)) == SENTINEL_BITS).all())


def run(cfg, dA, X, plan=None, alpha=1.0, beta=0.0, Y0=None, ldx=None, ldy=None):
    """one call on padded blocks (ldx = k + 3, ldy = k + 2 unless given) passed as torch column slices: (Y on the host,
    info); without Y0 the block holds the payload too"""
    k = X.shape[1]
    ldx = k + 3 if ldx is None else ldx
    ldy = k + 2 if ldy is None else ldy
    xb, xs = frame(dA.rows, ldx, k, X)
    yb, ys = frame(dA.cols, ldy, k, Y0)
    out, info = sa.spmm_t(dA, xs, cfg, plan=plan, alpha=alpha, beta=beta, Y=ys)
    assert out is None
    assert bits(host(xb)).tobytes() == bits(host(frame(dA.rows, ldx, k, X)[0])).tobytes(), "X was written"
    return read_frame(yb, dA.cols, ldy, k), info


def on_torch(H, ro=None, col=None, nnz=None, rows=None, cols=None):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz or shape"""
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    t_ro = torch.from_numpy(np.ascontiguousarray(ro, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    va = np.concatenate([H.data, np.zeros(1, dtype=H.data.dtype)])
    ci = np.concatenate([np.asarray(col, dtype=np.uint32), np.zeros(1, dtype=np.uint32)])
    t_va = torch.from_numpy(va).to(DEV)
    t_ci = torch.from_numpy(ci.view(np.int32)).to(DEV)
    return sa.dCSR.from_device(H.rows if rows is None else rows, H.cols if cols is None else cols, H.nnz if nnz is None else nnz,
                               t_ro.data_ptr(), t_ci.data_ptr(), t_va.data_ptr(), dtype=H.data.dtype, keep=(t_ro, t_va, t_ci))


def raw(cfg, plan, dA, x, ldx, k, y, ldy, alpha=1.0, beta=0.0):
    """the status of the C call on addresses"""
    fn = _lib.load().speck_spmm_t_f32 if dA.dtype == np.float32 else _lib.load().speck_spmm_t_f64
    return fn(cfg._h if cfg is not None else None, plan._h if plan is not None else None, alpha, C_.byref(dA._c), x, ldx, k, beta,
              y, ldy, None)


def edge_col_lens():
    """(column lengths) laid out against the tile edges of the plan; the comments give the plan entries a column holds"""
    return ([0,                # an empty first column
             T,                # [0, T): a column that is a tile, and ends exactly on a tile edge
             0,                # an empty column exactly at T
             1,                # [T, T + 1): starts on the edge
             T - 3,            # [T + 1, 2T - 2)
             1,                # [2T - 2, 2T - 1)
             1,                # [2T - 1, 2T): the last entry of a tile
             0,                # an empty column exactly at 2T
             T - 1,            # [2T, 3T - 1)
             2 * T + 2,        # [3T - 1, 5T + 1): a hub column over four tiles, two of them wholly inside
             99,               # [5T + 1, 5T + 100)
             T - 50,           # [5T + 100, 6T + 50): split ...
             T - 40,           # [6T + 50, 7T + 10): ... and split: the two meet in tile 6
             T - 10]           # [7T + 10, 8T)
            + [0] * 5000 +     # more columns without entries than a tile has entries, in the middle
            [5,                # [8T, 8T + 5)
             2,                # [8T + 5, 8T + 7)
             0])               # an empty last column


EDGE_ROWS = 37                  # few rows: every row holds hundreds of entries, many of them duplicates of the hub's id
_CACHE = {}


def edge_case(dtype):
    """(H, X of K_MAX columns, A^T X by scipy), computed once; a test with k columns takes the first k"""
    key = ("edge", np.dtype(dtype).name)
    if key not in _CACHE:
        H = with_col_lens(EDGE_ROWS, edge_col_lens(), dtype, 11, lambda n, s, d: ints(n, s, d))
        X = ints((H.rows, K_MAX), 13)
        S = at_x(H, X)
        assert np.abs(H.data.astype(np.float64)).sum() * 1024 < 2.0 ** 53
        for a in (H.row_offsets, H.col_ids, H.data, X, S):
            a.setflags(write=False)
        _CACHE[key] = (H, X, S)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- 1: exact, integers
COEFFS = [(1.0, 0.0), (2.0, -3.0), (0.0, 1.0)]


def check_exact(cfg, H, X, S, ks, coeffs=COEFFS, plan=None):
    dA = sa.dCSR.from_host(H)
    own = plan is None
    plan = sa.transpose_plan(dA, cfg) if own else plan
    try:
        t_ro = t_offsets(H)
        for k in ks:
            Y0 = ints((H.cols, k), 14)
            for alpha, beta in coeffs:
                got, info = run(cfg, dA, X[:, :k], plan, alpha, beta, Y0 if beta else None)
                want = alpha * S[:, :k] + beta * Y0 if beta else alpha * S[:, :k]
                assert np.array_equal(got, want), (k, alpha, beta, np.argwhere(got != want)[:8])
                assert as_tuple(info) == counts(t_ro, k), (info, counts(t_ro, k))
    finally:
        if own:
            plan.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_against_every_tile_edge_exact_with_the_padding_untouched(cfg, dtype):
    H, X, S = edge_case(dtype)
    t_ro = t_offsets(H)
    assert {T - 1, 0, 1} <= set((t_ro % T).tolist()) and T in t_ro and 2 * T in t_ro and 8 * T in t_ro
    assert counts(t_ro, 2) == (5004, 3, 9, 8 * T + 7, 2 * (8 * T + 7))
    ro = H.row_offsets.astype(np.int64)                                            # unsorted rows with duplicates
    assert any(len(set(H.col_ids[a:b].tolist())) < b - a and (np.diff(H.col_ids[a:b].astype(np.int64)) < 0).any()
               for a, b in zip(ro[:-1], ro[1:]))
    check_exact(cfg, H, X, S, KS)


def shapes_case(name, dtype):
    rng = np.random.default_rng(len(name))
    if name == "wide":                                                             # rows < cols
        rows, cols, n = 50, 700, 3000
        return from_pairs(rows, cols, rng.integers(0, rows, n), rng.integers(0, cols, n), ints(n, 21, dtype))
    if name == "tall":                                                             # rows > cols
        rows, cols, n = 700, 50, 3000
        return from_pairs(rows, cols, rng.integers(0, rows, n), rng.integers(0, cols, n), ints(n, 22, dtype))
    if name == "gaps":                                                             # empty columns in front, in the middle, at the end
        rows, cols, n = 90, 400, 2500
        live = np.concatenate([np.arange(5, 300), np.arange(320, 393)])
        return from_pairs(rows, cols, rng.integers(0, rows, n), rng.choice(live, n), ints(n, 23, dtype))
    n = {"one": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+5": 2 * T + 5}[name]
    rows, cols = 61, 130
    return from_pairs(rows, cols, rng.integers(0, rows, n), rng.integers(0, cols, n), ints(n, 24, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["wide", "tall", "gaps", "one", "T-1", "T", "T+1", "2T+5"])
def test_shapes_gaps_and_entry_counts_exact(cfg, dtype, name):
    H = shapes_case(name, dtype)
    t_ro = t_offsets(H)
    if name == "gaps":
        lens = np.diff(t_ro)
        assert not lens[:5].any() and not lens[300:320].any() and not lens[393:].any() and lens[5:300].all()
    X = ints((H.rows, K_MAX), 25)
    check_exact(cfg, H, X, at_x(H, X), KS, coeffs=[(2.0, -3.0), (1.0, 0.0)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_of_66_tiles_through_the_chain_finish(cfg, dtype):
    # column 2 holds 66 T + 3 entries in six rows: more tile records in one chain than a wave has lanes
    lens = [7, 0, 66 * T + 3, 5, 0]
    H = with_col_lens(6, lens, dtype, 31, lambda n, s, d: ints(n, s, d))
    assert counts(t_offsets(H), 1)[:3] == (2, 1, 67)
    X = ints((H.rows, 2), 32)
    assert np.abs(H.data.astype(np.float64)).sum() * 1024 < 2.0 ** 53
    check_exact(cfg, H, X, at_x(H, X), (1, 2), coeffs=[(2.0, -3.0)])


# ---------------------------------------------------------------------------------------------------- 2: the defining property
REAL_K = 5


def real_case(dtype):
    """column lengths from 0 to 3T, real values; (H, X of REAL_K columns, fsum per column of A and of X, sum|t| likewise)"""
    key = ("real", np.dtype(dtype).name)
    if key not in _CACHE:
        rng = np.random.default_rng(5)
        lens = [T - 1, 1, 7, 0, 100, T, T + 1, 3 * T, 0, 2 * T + 5, 33, 1000, 3 * T - 1, 17, 0, 0, 2, T + T // 2]
        lens += [int(v) for v in rng.integers(0, 60, size=400)]
        H = with_col_lens(257, lens, dtype, 6, real_values)
        X = real_values((H.rows, REAL_K), 8)
        order = np.argsort(H.col_ids, kind="stable")
        t_ro = t_offsets(H)
        a, r = H.data.astype(np.float64)[order], row_of(H)[order]
        want, mags = np.zeros((H.cols, 3)), np.zeros((H.cols, 3))
        for c in range(3):                                                         # (the bound test takes three columns)
            t = a * X[r, c]
            want[:, c] = [math.fsum(t[b:e]) for b, e in zip(t_ro[:-1], t_ro[1:])]
            mags[:, c] = [math.fsum(np.abs(t[b:e])) for b, e in zip(t_ro[:-1], t_ro[1:])]
        for v in (H.row_offsets, H.col_ids, H.data, X, want, mags):
            v.setflags(write=False)
        _CACHE[key] = (H, X, want, mags)
    return _CACHE[key]


def spmm_on_transpose(cfg, dA, X, alpha, beta, Y0):
    """what the parent offers: speck_transpose_*, then speck_spmm_*"""
    k = X.shape[1]
    dAt = sa.transpose(dA, cfg)
    _, xs = frame(dA.rows, k + 1, k, X)
    yb, ys = frame(dA.cols, k + 4, k, Y0)
    sa.spmm(dAt, xs, cfg, alpha=alpha, beta=beta, Y=ys)
    return read_frame(yb, dA.cols, k + 4, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_column_is_spmm_on_the_transpose_bit_for_bit(cfg, dtype):
    H, X, _, _ = real_case(dtype)
    dA = sa.dCSR.from_host(H)
    rng = np.random.default_rng(40)
    Y0 = rng.choice([-1.0, 1.0], size=(H.cols, REAL_K)) * (0.5 + rng.random((H.cols, REAL_K)))
    with sa.transpose_plan(dA, cfg) as plan:
        for alpha, beta in ((-1.5, 0.25), (1.0, 0.0)):
            got, info = run(cfg, dA, X, plan, alpha, beta, Y0 if beta else None)
            again, _ = run(cfg, dA, X, plan, alpha, beta, Y0 if beta else None)
            assert bits(got).tobytes() == bits(again).tobytes()                    # two consecutive calls: the same bits
            assert as_tuple(info) == counts(t_offsets(H), REAL_K)
            assert not np.isnan(got).any()
            want = spmm_on_transpose(cfg, dA, X, alpha, beta, Y0 if beta else None)
            assert bits(got).tobytes() == bits(want).tobytes(), (alpha, beta, np.argwhere(bits(got) != bits(want))[:8])


def allowance(n, mag):
    n = np.asarray(n, dtype=np.float64)[:, None]
    return (n * U / (1.0 - n * U) + U) * mag


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_values_within_the_bound_of_any_order(cfg, dtype):
    H, X, want, mags = real_case(dtype)
    got, _ = run(cfg, sa.dCSR.from_host(H), X[:, :3])
    err = np.abs(got - want)
    lens = np.diff(t_offsets(H))
    print("largest error / allowance:", float(np.max(err / np.maximum(allowance(lens, mags), 1e-300))))
    ok = err <= allowance(lens, mags)
    assert ok.all(), (np.argwhere(~ok)[:8], err[~ok][:8])


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_of_one_entry_are_added_in_their_input_order(cfg, dtype):
    # (0,0) three times: 1e16, 1, -1e16; (1,1) three times in the other order; column 2 holds both triples, row 0's first
    big = float(dtype(1e16))
    ro = np.array([0, 6, 12], dtype=np.uint32)
    ci = np.array([0, 2, 0, 2, 0, 2, 1, 2, 1, 2, 1, 2], dtype=np.uint32)
    da = np.array([big, big, 1, 1, -big, -big, -big, -big, 1, 1, big, big], dtype=dtype)
    H = sa.HostCSR(2, 3, ro, ci, da)
    dA = sa.dCSR.from_host(H)
    X = np.ones((2, 1))
    got, _ = run(cfg, dA, X)

    def serial(vals):
        acc = np.float64(0.0)
        for v in vals:
            acc = acc + np.float64(v)
        return float(acc)

    want = [serial([big, 1, -big]), serial([-big, 1, big]), serial([big, 1, -big, -big, 1, big])]
    assert serial([big, -big, 1]) == 1.0 and want[0] == 0.0                        # (another order gives another sum)
    assert got[:, 0].tolist() == want
    assert bits(got).tobytes() == bits(spmm_on_transpose(cfg, dA, X, 1.0, 0.0, None)).tobytes()


# ---------------------------------------------------------------------------------------------------- 3: the plan and the pattern
def update_values(d, data):
    data = np.ascontiguousarray(data)
    assert _lib.load().speck_dcsr_update(C_.byref(d._c), None, None, data.ctypes.data, data.dtype.itemsize) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_plan_of_a_view_fits_the_view_its_copy_and_a_scaled_copy(cfg, dtype):
    rng = np.random.default_rng(50)
    rows, cols, n = 120, 90, 2 * T + 300
    H = from_pairs(rows, cols, rng.integers(0, rows, n), rng.integers(0, cols, n), ints(n, 51, dtype))
    ro = H.row_offsets.astype(np.int64)
    dA = sa.dCSR.from_host(H)
    k = 3
    X = ints((rows, k), 52)
    seen = set()
    for want_mod in (1, 3):
        a = next(r for r in range(1, rows // 2) if ro[r] % 4 == want_mod)
        b = rows - 7
        seen.add(int(ro[a] % 4))
        view = dA.row_view(a, b)
        sub = sa.HostCSR(b - a, cols, (H.row_offsets[a:b + 1] - H.row_offsets[a]).astype(np.uint32), H.col_ids[ro[a]:ro[b]],
                         H.data[ro[a]:ro[b]])
        want = at_x(sub, X[a:b])                                                   # the partial sum of the view's rows
        with sa.transpose_plan(view, cfg) as plan:
            assert (plan.info.rows, plan.info.cols, plan.info.nnz) == (b - a, cols, ro[b] - ro[a])
            r_view, info = run(cfg, view, X[a:b], plan)
            assert as_tuple(info) == counts(t_offsets(sub), k)
            copy = view.copy()
            r_copy, _ = run(cfg, copy, X[a:b], plan)
            scaled, _ = sa.scale(view, cfg, alpha=2.0)
            r_scaled, _ = run(cfg, scaled, X[a:b], plan)
            assert np.array_equal(r_view, want)
            assert bits(r_view).tobytes() == bits(r_copy).tobytes() == bits(r_scaled / 2.0).tobytes()
            assert np.array_equal(r_scaled, 2.0 * want)
            # the values change, the pattern stays: the same plan gives the new values' product
            fresh = ints(sub.nnz, 53, dtype)
            update_values(copy, fresh)
            r_new, _ = run(cfg, copy, X[a:b], plan)
            assert np.array_equal(r_new, at_x(sa.HostCSR(sub.rows, cols, sub.row_offsets, sub.col_ids, fresh), X[a:b]))
            # one plan, two configs -- and no config
            other = sa.spECKConfig.initialize(0)
            try:
                r_other, _ = run(other, view, X[a:b], plan)
            finally:
                other.cleanup()
            r_none, _ = run(None, view, X[a:b], plan)
            assert bits(r_other).tobytes() == bits(r_view).tobytes() == bits(r_none).tobytes()
            # plan=None builds one for the call
            r_own, _ = run(cfg, view, X[a:b], None)
            assert bits(r_own).tobytes() == bits(r_view).tobytes()
    assert seen == {1, 3}


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmv_t_is_column_zero(cfg, dtype):
    H, X, S = edge_case(dtype)
    dA = sa.dCSR.from_host(H)
    x = torch.from_numpy(X[:, 0].copy()).to(DEV)
    y, info = sa.spmv_t(dA, x, cfg)
    assert np.array_equal(y, S[:, 0]) and as_tuple(info) == counts(t_offsets(H), 1)
    yt = torch.from_numpy(np.ones(H.cols)).to(DEV)
    out, _ = sa.spmv_t(dA, x, cfg, alpha=2.0, beta=-3.0, y=yt)
    assert out is None and np.array_equal(host(yt), 2.0 * S[:, 0] - 3.0)


# ---------------------------------------------------------------------------------------------------- 4: special values
@pytest.mark.parametrize("dtype", DTYPES)
def test_beta_zero_does_not_read_y_and_nan_and_inf_land_where_a_holds_an_entry(cfg, dtype):
    rng = np.random.default_rng(70)
    rows, cols, n = 40, 60, T + 500
    r, c = rng.integers(0, rows, n), rng.integers(0, cols, n)
    data = rng.integers(1, 100, size=n).astype(dtype)
    data[r == 9] = 0.0                                                             # row 9: 0 * inf
    H = from_pairs(rows, cols, r, c, data)
    X = ints((rows, 3), 71)
    X[7, 1], X[9, 2] = np.nan, np.inf                                              # ONE element each
    got, _ = run(cfg, sa.dCSR.from_host(H), X)                                     # (Y held the payload NaN: beta == 0)
    rr = row_of(H)
    hit7 = np.zeros(cols, dtype=bool)
    hit7[H.col_ids[rr == 7]] = True
    hit9 = np.zeros(cols, dtype=bool)
    hit9[H.col_ids[rr == 9]] = True
    assert hit7.any() and not hit7.all() and hit9.any() and not hit9.all()
    nan = np.isnan(got)
    assert not nan[:, 0].any()
    assert np.array_equal(nan[:, 1], hit7) and np.array_equal(nan[:, 2], hit9)
    clean = X.copy()
    clean[7, 1], clean[9, 2] = 0.0, 0.0
    want = at_x(H, clean)
    assert np.array_equal(got[~nan], want[~nan])


# ---------------------------------------------------------------------------------------------------- 5: refusals, Y untouched
def hostile_variants(H):
    """(name, dCSR) of matrices with H's shape and nnz and another pattern: one id changed, two entries of one row swapped to
    different columns, one interior offset moved by one -- each at the first entry, at the last, and on a tile edge of the plan"""
    ro, ci = H.row_offsets.astype(np.int64), H.col_ids.astype(np.int64)
    order = np.argsort(ci, kind="stable")                                          # t_pos
    rr = row_of(H)
    out = []
    for where, p in (("first", 0), ("last", H.nnz - 1), ("edge", int(order[T])), ("edge-1", int(order[T - 1]))):
        col = ci.copy()
        col[p] = (col[p] + 1) % H.cols
        out.append((f"id changed at the {where} entry", on_torch(H, col=col)))
        # a neighbour in p's row with another id
        row = rr[p]
        q = next(q for q in list(range(p + 1, ro[row + 1])) + list(range(p - 1, ro[row] - 1, -1)) if ci[q] != ci[p])
        col = ci.copy()
        col[p], col[q] = ci[q], ci[p]
        out.append((f"entries swapped at the {where} entry", on_torch(H, col=col)))
    inner = [r for r in range(1, H.rows) if ro[r - 1] < ro[r] < ro[r + 1]]
    near = min(inner, key=lambda r: abs(ro[r] - T))
    for where, r in (("first", inner[0]), ("last", inner[-1]), ("edge", near)):
        for step in (1, -1):
            moved = ro.copy()
            moved[r] += step
            out.append((f"offset {r} moved by {step} ({where})", on_torch(H, ro=moved)))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_another_pattern_is_refused_with_y_untouched(cfg, dtype):
    H, X, S = edge_case(dtype)
    k = 5
    dA = sa.dCSR.from_host(H)
    with sa.transpose_plan(dA, cfg) as plan:
        _, xs = frame(H.rows, k + 3, k, X[:, :k])
        for name, bad in hostile_variants(H):
            yb, ys = frame(H.cols, k + 2, k)
            with pytest.raises(sa.SpeckError) as e:
                sa.spmm_t(bad, xs, cfg, plan=plan, Y=ys)
            assert e.value.status == ERR_INVALID, name
            assert untouched(yb), name
        # nnz or a dimension differing from the plan's: refused before anything runs
        short = H.row_offsets.copy()
        short[-1] -= 1
        for name, bad in (("nnz", on_torch(H, ro=short, nnz=H.nnz - 1)), ("cols", on_torch(H, cols=H.cols + 1)),
                          ("rows", on_torch(H, rows=H.rows - 1, nnz=H.nnz))):
            yb, ys = frame(H.cols + 1, k + 2, k)
            assert raw(cfg, plan, bad, xs.data_ptr(), k + 3, k, ys.data_ptr(), k + 2) == ERR_INVALID, name
            assert untouched(yb), name
        # ... and the plan still serves the matrix it was made from
        got, _ = run(cfg, dA, X[:, :k], plan)
        assert np.array_equal(got, S[:, :k])


def test_argument_refusals_leave_y_untouched(cfg):
    H, X, S = edge_case(np.float64)
    k, ldx, ldy = 3, 6, 5
    dA = sa.dCSR.from_host(H)
    nan = float("nan")
    with sa.transpose_plan(dA, cfg) as plan:
        _, xs = frame(H.rows, ldx, k, X[:, :k])
        yb, ys = frame(H.cols, ldy, k)
        px, py = xs.data_ptr(), ys.data_ptr()
        assert raw(cfg, None, dA, px, ldx, k, py, ldy) == ERR_INVALID              # no plan
        assert raw(cfg, plan, dA, px, ldx, k, py, ldy, alpha=nan) == ERR_INVALID
        assert raw(cfg, plan, dA, px, ldx, k, py, ldy, beta=nan) == ERR_INVALID
        assert raw(cfg, plan, dA, px, k - 1, k, py, ldy) == ERR_INVALID            # ld < k
        assert raw(cfg, plan, dA, px, ldx, k, py, k - 1) == ERR_INVALID
        assert raw(cfg, plan, dA, px, 2000, 1025, py, 2000) == ERR_DIM_LIMIT
        assert raw(cfg, plan, dA, px, (1 << 32) + 1, k, py, ldy) == ERR_DIM_LIMIT
        for ptr in (dA._c.data, dA._c.col_ids, dA._c.row_offsets):                 # a block is one of A's buffers
            assert raw(cfg, plan, dA, ptr, ldx, k, py, ldy) == ERR_INVALID
            assert raw(cfg, plan, dA, px, ldx, k, ptr, ldy) == ERR_INVALID
        assert raw(cfg, plan, dA, None, ldx, k, py, ldy) == ERR_INVALID
        assert raw(cfg, plan, dA, px, ldx, k, None, ldy) == ERR_INVALID
        assert untouched(yb)
        # X and Y in one buffer: X spans [x, x + (rows - 1) ldx + k), Y spans [y, y + (cols - 1) ldy + k)
        x_span, y_span = (H.rows - 1) * ldx + k, (H.cols - 1) * ldy + k
        both = torch.from_numpy(np.full(x_span + y_span + 16, SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)
        p0 = both.data_ptr()
        xrows = torch.from_numpy(X[:, :k].copy()).to(DEV)
        for i in range(H.rows):
            both[i * ldx:i * ldx + k] = xrows[i]
        before = bits(host(both)).copy()
        for off in (0, 1, k, ldx, x_span - 1):                                     # Y begins inside X's span
            assert raw(cfg, plan, dA, p0, ldx, k, p0 + 8 * off, ldy) == ERR_INVALID, off
        for off in (1, y_span - 1):                                                # X begins inside Y's span
            assert raw(cfg, plan, dA, p0 + 8 * off, ldx, k, p0, ldy) == ERR_INVALID, off
        assert np.array_equal(bits(host(both)), before)
        # spans that touch are served: Y right behind X
        assert raw(cfg, plan, dA, p0, ldx, k, p0 + 8 * x_span, ldy) == OK
        after = host(both)
        assert np.array_equal(bits(after)[:x_span], before[:x_span])
        assert (bits(after[x_span + y_span:]) == SENTINEL_BITS).all()
        block = np.concatenate([after[x_span:x_span + y_span], after[-(ldy - k):]]).reshape(H.cols, ldy)
        assert np.array_equal(block[:, :k], S[:, :k]) and (bits(block[:, k:]) == SENTINEL_BITS).all()
        # a freed plan, in the wrapper
        plan.free()
        with pytest.raises(sa.SpeckError) as e:
            sa.spmm_t(dA, xs, cfg, plan=plan, Y=ys)
        assert e.value.status == ERR_INVALID and untouched(yb)
        plan.free()                                                                # (twice is once)


# ---------------------------------------------------------------------------------------------------- 6: the creation
def small_case(dtype=np.float64):
    rng = np.random.default_rng(80)
    rows, cols, n = 30, 50, 300
    return from_pairs(rows, cols, rng.integers(0, rows, n), rng.integers(3, cols - 2, n), ints(n, 81, dtype))


def create_raw(dA):
    h = C_.c_void_p()
    rc = _lib.load().speck_tplan_create(None, C_.byref(dA._c), C_.byref(h), None)
    return rc, h


def test_plan_creation_refuses_hostile_input_and_then_serves_a_sound_one(cfg):
    H = small_case()
    ro, ci = H.row_offsets.astype(np.int64), H.col_ids.astype(np.int64)
    cases = []
    r = H.rows // 2
    desc = ro.copy()
    desc[r] = ro[r + 1] + 1                                                        # (inside [0, nnz]: only the descent is wrong)
    assert desc[r] > desc[r + 1] and desc[r] <= H.nnz
    cases.append(("a descending offset", on_torch(H, ro=desc)))
    beyond = ro.copy()
    beyond[H.rows - 1] = H.nnz + 1
    cases.append(("an offset beyond nnz", on_torch(H, ro=beyond)))
    short = ro.copy()
    short[-1] = H.nnz - 1
    cases.append(("a last offset short of nnz", on_torch(H, ro=short)))
    for name, v in (("an id == cols", H.cols), ("an id == 0xFFFFFFFF", 0xFFFFFFFF)):
        for p in (0, H.nnz // 2, H.nnz - 1):
            col = ci.copy()
            col[p] = v
            cases.append((f"{name} at {p}", on_torch(H, col=col)))
    for name, bad in cases:
        rc, h = create_raw(bad)
        assert rc == ERR_INVALID and not h, name
        with pytest.raises(sa.SpeckError) as e:
            sa.transpose_plan(bad, cfg)
        assert e.value.status == ERR_INVALID, name
    rc, h = create_raw(on_torch(H))
    assert rc == OK and h
    assert _lib.load().speck_tplan_destroy(h) == OK


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_plan_is_the_transpose_read_through_the_product_with_the_identity(cfg, dtype):
    H = small_case(dtype)
    dA = sa.dCSR.from_host(H)
    valueless = sa.dCSR.from_device(H.rows, H.cols, H.nnz, dA._c.row_offsets, dA._c.col_ids, None, dtype=dtype, keep=dA)
    with sa.transpose_plan(valueless, cfg) as plan:                                # (the values are not read)
        t_ro = t_offsets(H)
        lens = np.diff(t_ro)
        assert repr(plan.info).startswith("TplanInfo(rows=30, cols=50, nnz=300, ")
        assert (plan.info.cols_empty, plan.info.max_col_entries) == (int((lens == 0).sum()), int(lens.max()))
        assert plan.info.cols_empty >= 5                                           # columns 0..2 and the last two
        assert plan.info.bytes >= 4 * (H.cols + 1 + 2 * H.nnz + H.rows + 1)
        got, _ = run(cfg, dA, np.eye(H.rows), plan)                                # Y = A^T, duplicates added
    At = sa.transpose(dA, cfg).to_host()
    dense = sp.csr_matrix((At.data.astype(np.float64), At.col_ids.astype(np.int64), At.row_offsets.astype(np.int64)),
                          shape=(H.cols, H.rows)).toarray()
    assert np.array_equal(got, dense)
    assert np.array_equal(At.row_offsets.astype(np.int64), t_ro)


# ---------------------------------------------------------------------------------------------------- 7: valid and empty
def test_sizes_that_are_valid_but_empty(cfg):
    z = np.zeros(0)
    # nnz == 0 with rows and columns: Y = alpha * (+0.0) + beta * Y
    H = sa.HostCSR(4, 6, np.zeros(5, dtype=np.uint32), np.zeros(0, dtype=np.uint32), z)
    dA = on_torch(H)
    with sa.transpose_plan(dA, cfg) as plan:
        assert (plan.info.nnz, plan.info.cols_empty, plan.info.max_col_entries) == (0, 6, 0)
        got, info = run(cfg, dA, np.ones((4, 2)), plan, alpha=2.0)
        assert (bits(got) == 0).all() and as_tuple(info) == (6, 0, 0, 0, 0)
        Y0 = ints((6, 2), 90)
        got, _ = run(cfg, dA, np.ones((4, 2)), plan, alpha=2.0, beta=0.5, Y0=Y0)
        assert np.array_equal(got, 0.5 * Y0)
        # k == 0: nothing written
        yb, ys = frame(6, 2, 2)
        _, xs = frame(4, 2, 2, np.ones((4, 2)))
        assert raw(cfg, plan, dA, xs.data_ptr(), 0, 0, ys.data_ptr(), 0) == OK
        assert untouched(yb)
    # no row: every column is empty
    H = sa.HostCSR(0, 6, np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), z)
    dA = on_torch(H)
    with sa.transpose_plan(dA, cfg) as plan:
        assert (plan.info.rows, plan.info.cols_empty) == (0, 6)
        yb, ys = frame(6, 4, 2)
        _, xs = frame(1, 2, 2)
        assert raw(cfg, plan, dA, xs.data_ptr(), 2, 2, ys.data_ptr(), 4, alpha=3.0) == OK
        assert (bits(read_frame(yb, 6, 4, 2)) == 0).all()
    # no column: nothing to write
    H = sa.HostCSR(4, 0, np.zeros(5, dtype=np.uint32), np.zeros(0, dtype=np.uint32), z)
    dA = on_torch(H)
    with sa.transpose_plan(dA, cfg) as plan:
        assert (plan.info.cols, plan.info.cols_empty) == (0, 0)
        yb, ys = frame(1, 2, 2)
        _, xs = frame(4, 2, 2, np.ones((4, 2)))
        assert raw(cfg, plan, dA, xs.data_ptr(), 2, 2, ys.data_ptr(), 2) == OK
        assert untouched(yb)


# ---------------------------------------------------------------------------------------------------- 8: guards, streams
def test_no_canary_zone_is_touched():
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        H, X, S = edge_case(np.float64)
        check_exact(cfg, H, X, S, (1, 3, 9))                                       # (a touched zone is status 3)
        dA = sa.dCSR.from_host(H)
        with sa.transpose_plan(dA, cfg) as plan:
            col = H.col_ids.astype(np.int64)
            col[0] = (col[0] + 1) % H.cols
            yb, ys = frame(H.cols, 5, 3)
            _, xs = frame(H.rows, 6, 3, X[:, :3])
            with pytest.raises(sa.SpeckError) as e:
                sa.spmm_t(on_torch(H, col=col), xs, cfg, plan=plan, Y=ys)
            assert e.value.status == ERR_INVALID and untouched(yb)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_the_call_runs_on_the_configs_stream(cfg):
    H, X, S = edge_case(np.float64)
    dA = sa.dCSR.from_host(H)
    stream = torch.cuda.Stream()
    with sa.transpose_plan(dA, cfg) as plan:
        cfg.set_stream(stream.cuda_stream)
        try:
            yb, ys = frame(H.cols, 4, 3)
            with torch.cuda.stream(stream):
                dX = torch.empty((H.rows, 3), dtype=torch.float64, device=DEV)
                dX.copy_(torch.from_numpy(X[:, :3].copy()).pin_memory(), non_blocking=True)
            sa.spmm_t(dA, dX, cfg, plan=plan, Y=ys)
            assert np.array_equal(read_frame(yb, H.cols, 4, 3), S[:, :3])
        finally:
            cfg.set_stream(None)
            torch.cuda.synchronize()
