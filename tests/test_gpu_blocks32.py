"""Float blocks on the GPU: speck_spmm_*_b32, speck_spmm_t_*_b32 and speck_sddmm_*_b32 (spmm.hip, spmm_t.hip, sddmm.hip with
B = float).  No tolerance appears anywhere.  The expectations are (i) the existing double-block call on the widened
blocks (X.double(), Y.double()), narrowed with .float() and compared as BYTES -- the defining property of the contract --
and (ii) numpy on the host for integer inputs, where every order of summation is exact:
(alpha * S + beta * Y.astype(f64)).astype(f32).  Every Y lives in a frame filled with a payload float NaN: the padding
between its rows, what lies in front of it and behind its last row must still hold the payload after every call.
T = 4096 entries per tile; CB is the number of float columns the tile kernels take per round."""
import ctypes as C_
import warnings

import numpy as np
import pytest
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_DIM_LIMIT = 1, 2
DTYPES = [np.float64, np.float32]
T = sa.SPMV_TILE_ENTRIES
CB = sa.SPMM_COLUMN_BLOCK_B32
KS = sorted({1, 2, 3, 4, 5, 7, 8, 9, CB, CB + 1, 2 * CB + 1})
K_MAX = max(KS)
SDDMM_KS = [1, 3, 4, 5, 8, 9, 16, 17, 33]           # both sides of every switch of L(k): 4|5, 8|9, 16|17
PAYLOAD = 0x7FC0BEEF                                # a float NaN with a payload
DEV = "cuda:0"
COLS = 3000
TAIL = 8                                            # payload words behind the last row of a frame
F32 = "float32"


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
    if col is None:
        col = np.random.default_rng(seed).integers(0, cols, size=len(data))
    return sa.HostCSR(len(lens), cols, ro, np.asarray(col, dtype=np.uint32), np.asarray(data))


def ints(shape, seed, dtype=np.float32, lim=64):
    """integers without a zero: no term is a signed zero (the sign of a zero SUM is the same in every order: +0.0)"""
    v = np.random.default_rng(seed).integers(-lim, lim + 1, size=shape)
    return np.where(v == 0, lim, v).astype(dtype)


def reals(shape, seed, dtype=np.float32):
    """mixed signs over six decades: products and sums round in double AND in the last conversion"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(dtype)


def row_sums(H, X):
    """numpy's row sums of the terms a.astype(f64) * X.astype(f64), column by column; +0.0 for a row without entries"""
    ro = H.row_offsets.astype(np.int64)
    X = np.asarray(X, dtype=np.float64)
    S = np.zeros((H.rows, X.shape[1]))
    full = np.nonzero(ro[1:] > ro[:-1])[0]
    with np.errstate(invalid="ignore"):
        for c in range(X.shape[1]):
            if len(full):
                S[full, c] = np.add.reduceat(H.data.astype(np.float64) * X[H.col_ids.astype(np.int64), c], ro[:-1][full])
    return S


def narrow(a):
    """numpy's rounding of doubles to float: to nearest even, subnormals kept, beyond FLT_MAX inf"""
    with warnings.catch_warnings(), np.errstate(over="ignore", invalid="ignore"):
        warnings.simplefilter("ignore")
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bytes(got, want):
    return b32(got).tobytes() == b32(want).tobytes()


def where_differ(got, want):
    return np.argwhere(b32(got) != b32(want))[:8].tolist()


def frame(n, ld, k, vals=None, lead=0):
    """(buffer, block): a device buffer of the payload NaN that holds an n x k block of floats in rows ld apart, `lead`
    floats from its start (the allocation lies on a 16-byte boundary, so lead is the block's offset from one) and TAIL
    floats from its end; the block is the torch view [:, :k] of those rows and holds vals"""
    buf = torch.from_numpy(np.full(lead + n * ld + TAIL, PAYLOAD, dtype=np.uint32).view(np.float32)).to(DEV)
    assert buf.data_ptr() % 16 == 0
    blk = buf[lead:lead + n * ld].view(n, ld)[:, :k]
    if vals is not None and n and k:
        blk.copy_(torch.from_numpy(np.array(vals, dtype=np.float32)).to(DEV))
    return buf, blk


def read_frame(buf, n, ld, k, lead=0):
    """the n x k block of a frame on the host, after checking that every other word still holds the payload"""
    full = host(buf)
    rows = full[lead:lead + n * ld].reshape(n, ld)
    assert (b32(full[:lead]) == PAYLOAD).all(), "in front of the block"
    assert (b32(rows[:, k:]) == PAYLOAD).all(), "the padding of the block"
    assert (b32(full[lead + n * ld:]) == PAYLOAD).all(), "behind the last row of the block"
    return rows[:, :k].copy()


def untouched(buf):
    return bool((b32(host(buf)) == PAYLOAD).all())


def run32(call, cfg, dA, n_x, n_y, X, alpha=1.0, beta=0.0, Y0=None, ldx=None, ldy=None, x_lead=0, y_lead=0, **kw):
    """one float-block call (sa.spmm or sa.spmm_t) on padded blocks (ldx = k + 3, ldy = k + 2 unless given) passed as
    torch column slices: (Y on the host, info); without Y0 the block holds the payload NaN too"""
    k = X.shape[1]
    ldx = k + 3 if ldx is None else ldx
    ldy = k + 2 if ldy is None else ldy
    xb, xs = frame(n_x, ldx, k, X, lead=x_lead)
    yb, ys = frame(n_y, ldy, k, Y0, lead=y_lead)
    before = b32(host(xb)).copy()
    out, info = call(dA, xs, cfg, alpha=alpha, beta=beta, Y=ys, blocks=F32, **kw)
    assert out is None
    assert np.array_equal(b32(host(xb)), before), "X was written"
    return read_frame(yb, n_y, ldy, k, lead=y_lead), info


def run64(call, cfg, dA, n_y, X, alpha=1.0, beta=0.0, Y0=None, **kw):
    """what a caller has without float blocks: the double-block call on X.double(), Y.double(), the result narrowed with
    .float() on the device: (Y on the host as floats, info)"""
    k = X.shape[1]
    dX = torch.from_numpy(np.array(X, dtype=np.float32)).to(DEV).double()
    if Y0 is None:
        dY = torch.full((n_y, k), float("nan"), dtype=torch.float64, device=DEV)
    else:
        dY = torch.from_numpy(np.array(Y0, dtype=np.float32)).to(DEV).double()
    out, info = call(dA, dX, cfg, alpha=alpha, beta=beta, Y=dY, **kw)
    assert out is None
    return host(dY.float()), info


def spmm32(cfg, dA, X, *a, **kw):
    return run32(sa.spmm, cfg, dA, dA.cols, dA.rows, X, *a, **kw)


def spmm64(cfg, dA, X, *a, **kw):
    return run64(sa.spmm, cfg, dA, dA.rows, X, *a, **kw)


def spmm_t32(cfg, dA, X, *a, **kw):
    return run32(sa.spmm_t, cfg, dA, dA.rows, dA.cols, X, *a, **kw)


def spmm_t64(cfg, dA, X, *a, **kw):
    return run64(sa.spmm_t, cfg, dA, dA.cols, X, *a, **kw)


def as_tuple(info):
    return tuple(getattr(info, f) for f in info._fields)


def on_torch(H, ro=None, col=None, nnz=None, r0=0, r1=None):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz, a view"""
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    r1 = H.rows if r1 is None else r1
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    t_va = torch.from_numpy(np.concatenate([H.data, np.zeros(1, dtype=H.data.dtype)])).to(DEV)
    t_ci = torch.from_numpy(np.concatenate([np.asarray(col, dtype=np.uint32), np.zeros(1, dtype=np.uint32)]).view(np.int32)).to(DEV)
    if nnz is None:
        nnz = int(H.row_offsets[r1]) - int(H.row_offsets[r0])
    return sa.dCSR.from_device(r1 - r0, H.cols, nnz, t_ro.data_ptr() + 4 * r0, t_ci.data_ptr(), t_va.data_ptr(), dtype=H.data.dtype,
                               keep=(t_ro, t_va, t_ci))


_CACHE = {}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def main_lens():
    """about 3 T entries: short rows, empty rows, one row of 2 T + 5 entries (the chain finish over three tiles)"""
    rng = np.random.default_rng(3)
    head = [int(v) for v in rng.integers(0, 9, size=400)]
    tail = [int(v) for v in rng.integers(0, 9, size=420)]
    return head + [0, 0, 2 * T + 5, 0, 1] + tail


def main_case(dtype):
    """(H with real values, X real of K_MAX columns, Y0 real), computed once; a test with k columns takes the first k"""
    key = ("main", np.dtype(dtype).name)
    if key not in _CACHE:
        lens = main_lens()
        H = mk(lens, reals(sum(lens), 11, dtype), seed=12)
        assert 3 * T - T // 2 < H.nnz < 3 * T + T // 4 and 0 in lens
        X, Y0 = reals((COLS, K_MAX), 13), reals((H.rows, K_MAX), 14)
        frozen(H.row_offsets, H.col_ids, H.data, X, Y0)
        _CACHE[key] = (H, X, Y0)
    return _CACHE[key]


def int_case(dtype):
    """the same structure with integers: (H, X, Y0, row sums by numpy); every sum stays far below 2^53"""
    key = ("int", np.dtype(dtype).name)
    if key not in _CACHE:
        lens = main_lens()
        H = mk(lens, ints(sum(lens), 15, dtype, lim=16), seed=12)
        X, Y0 = ints((COLS, K_MAX), 16), ints((H.rows, K_MAX), 17)
        S = row_sums(H, X)
        frozen(H.row_offsets, H.col_ids, H.data, X, Y0, S)
        _CACHE[key] = (H, X, Y0, S)
    return _CACHE[key]


COEFFS = [(1.0, 0.0), (-2.0, 0.5)]


# ==================================================================================================== spmm
@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_every_k_is_the_double_call_narrowed_with_the_padding_untouched(cfg, dtype):
    H, X, Y0 = main_case(dtype)
    dA = sa.dCSR.from_host(H)
    for k in KS:
        for alpha, beta in COEFFS:
            y0 = Y0[:, :k] if beta else None
            got, info = spmm32(cfg, dA, X[:, :k], alpha, beta, y0)
            want, info64 = spmm64(cfg, dA, X[:, :k], alpha, beta, y0)
            assert same_bytes(got, want), (k, alpha, beta, where_differ(got, want))
            assert as_tuple(info) == as_tuple(info64) and info.terms == H.nnz * k
            again, _ = spmm32(cfg, dA, X[:, :k], alpha, beta, y0)                  # two calls, the same bytes
            assert same_bytes(again, got), (k, alpha, beta)
        assert not np.isnan(got).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_integers_equal_numpy_and_beta_zero_does_not_read_y(cfg, dtype):
    H, X, Y0, S = int_case(dtype)
    dA = sa.dCSR.from_host(H)
    for k in (1, CB + 1, 9):
        # beta == 0: Y holds the payload NaN in every word and is not read
        got, _ = spmm32(cfg, dA, X[:, :k])
        assert same_bytes(got, narrow(S[:, :k])), (k, where_differ(got, narrow(S[:, :k])))
        # beta = 0.5, alpha = -2: Y is read as float, widened, and the sum rounded ONCE
        got, _ = spmm32(cfg, dA, X[:, :k], -2.0, 0.5, Y0[:, :k])
        want = narrow(-2.0 * S[:, :k] + 0.5 * Y0[:, :k].astype(np.float64))
        assert same_bytes(got, want), (k, where_differ(got, want))
    # results that do not fit a float's 24 bits: the one rounding is to nearest even, as numpy's
    big = (X[:, :3].astype(np.float64) * 65537.0).astype(np.float32)
    assert (big.astype(np.float64) == X[:, :3].astype(np.float64) * 65537.0).all()
    got, _ = spmm32(cfg, dA, big, 3.0, 0.0)
    want = narrow(3.0 * row_sums(H, big))
    assert (want.astype(np.float64) != 3.0 * row_sums(H, big)).any()               # (some results were rounded)
    assert same_bytes(got, want), where_differ(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_every_alignment_form_gives_the_same_bytes(cfg, dtype):
    """d_X 0, 1, 2 and 3 floats from a 16-byte boundary, crossed with ldx mod 4 = 0, 1, 2, 3: 16-byte, 8-byte and 4-byte
    gathers; Y offset likewise.  All give the bytes of the aligned call and of the contiguous one."""
    H, X, Y0 = main_case(dtype)
    dA = sa.dCSR.from_host(H)
    k = 9
    for alpha, beta in COEFFS:
        y0 = Y0[:, :k] if beta else None
        base, _ = spmm32(cfg, dA, X[:, :k], alpha, beta, y0, ldx=12, ldy=12)      # on 16 bytes, ld % 4 == 0
        contiguous, _ = spmm32(cfg, dA, X[:, :k], alpha, beta, y0, ldx=k, ldy=k)
        assert same_bytes(contiguous, base)
        for lead in range(4):
            for ldx in (12, 13, 14, 15):
                got, _ = spmm32(cfg, dA, X[:, :k], alpha, beta, y0, ldx=ldx, ldy=ldx - 2, x_lead=lead, y_lead=(lead + 1) % 4)
                assert same_bytes(got, base), (lead, ldx, where_differ(got, base))
    # what k leaves over a block of CB, in every form: k = CB + 3 takes a block, a pair and a column alone
    k = CB + 3
    base, _ = spmm32(cfg, dA, X[:, :k], ldx=12, ldy=12)
    for lead, ldx in ((0, 12), (2, 12), (0, 14), (1, 12), (0, 13), (3, 15)):
        got, _ = spmm32(cfg, dA, X[:, :k], ldx=ldx, x_lead=lead)
        assert same_bytes(got, base), (lead, ldx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_entry_counts_around_the_tile_on_a_view_with_an_odd_base(cfg, dtype):
    k, ldy = 5, 7
    for n in (T - 1, T, T + 1, 2 * T + 5):
        lens = [3, 40, 0, n - 40 - 9, 9]                                            # the view [1, 5) holds n entries from offset 3
        H = mk(lens, reals(sum(lens), 20 + n % 7, dtype), seed=21)
        X = reals((COLS, k), 22)
        dA = sa.dCSR.from_host(H)
        whole, _ = spmm32(cfg, dA, X, ldy=ldy)
        view = dA.row_view(1, 5)
        assert view.nnz == n and int(H.row_offsets[1]) % 2 == 1
        _, xs = frame(COLS, k + 3, k, X)
        yb, ys = frame(H.rows, ldy, k)                                              # the frame of the WHOLE result
        assert ys[1:].data_ptr() == ys.data_ptr() + 4 * ldy                         # Y + r0 ldy, in floats
        _, info = sa.spmm(view, xs, cfg, Y=ys[1:], blocks=F32)
        got = read_frame(yb, H.rows, ldy, k)
        assert same_bytes(got[1:], whole[1:]), (n, where_differ(got[1:], whole[1:]))
        assert (b32(got[:1]) == PAYLOAD).all(), n
        want, info64 = spmm64(cfg, view, X)
        assert same_bytes(got[1:], want) and as_tuple(info) == as_tuple(info64), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_nan_and_inf_land_in_their_column_of_the_rows_that_reference_them(cfg, dtype):
    lens = [3, 2, 0, 5, 2 * T + 10, 4, 1, 6]
    ro = np.concatenate([[0], np.cumsum(lens)])
    n = int(ro[-1])
    rng = np.random.default_rng(70)
    data = rng.integers(1, 100, size=n).astype(dtype)
    col = rng.integers(10, 50, size=n).astype(np.uint32)                           # nobody references 7 or 9 by chance
    X = ints((50, 3), 71)
    X[7, 1], X[9, 2] = np.nan, np.inf                                              # ONE element each
    col[ro[0] + 1] = 7                                                             # row 0: the NaN, in column 1
    col[ro[1]] = 9
    data[ro[1]] = 0.0                                                              # row 1: 0 * inf, in column 2
    col[ro[3] + 4] = 9                                                             # row 3: 12 * inf = inf in column 2, no NaN
    data[ro[3] + 4] = 12
    col[ro[4] + T + T // 2] = 7                                                    # row 4, split over three tiles
    H = sa.HostCSR(len(lens), 50, ro.astype(np.uint32), col, data)
    dA = sa.dCSR.from_host(H)
    got, _ = spmm32(cfg, dA, X)
    want = narrow(row_sums(H, X))
    assert np.argwhere(np.isnan(want)).tolist() == [[0, 1], [1, 2], [4, 1]] and want[3, 2] == np.inf
    assert np.isinf(want).sum() == 1
    assert np.array_equal(got, want, equal_nan=True), (got[:8], want[:8])
    via64, _ = spmm64(cfg, dA, X)
    assert same_bytes(got, via64), where_differ(got, via64)
    # beta = 1: a NaN of Y0 stays in its element
    clean = ints((50, 3), 72)
    Y0 = ints((H.rows, 3), 73)
    at = [(0, 2), (2, 0), (4, 1), (7, 2)]                                          # (row 2 holds no entry, row 4 is split)
    for i, c in at:
        Y0[i, c] = np.nan
    got, _ = spmm32(cfg, dA, clean, 1.0, 1.0, Y0)
    assert [tuple(p) for p in np.argwhere(np.isnan(got)).tolist()] == at
    assert np.array_equal(got, narrow(row_sums(H, clean) + Y0.astype(np.float64)), equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_subnormals_are_widened_exactly_rounded_not_flushed_and_overflow_is_inf(cfg, dtype):
    """one entry per row, alpha = 1: Y(i, c) = float(double(a_i) * double(X(i, c))) -- numpy's astype on the host"""
    tiny = np.float32(1e-45)                                                        # the smallest subnormal float
    assert tiny > 0 and tiny.view(np.uint32) == 1
    a = np.array([1.0, 1.0, 0.5, 0.75, 3.0, 2.0, -2.0, 1.0, 0.5, 0.25], dtype=dtype)
    x = np.array([tiny, np.float32(1e-40), tiny * 3, tiny * 2, np.float32(5e-39), np.float32(3e38), np.float32(3e38),
                  np.float32(3.4028235e38), np.float32(1.1754944e-38), np.float32(1.1754944e-38)], dtype=np.float32)
    n = len(a)
    H = mk([1] * n, a, cols=n, col=np.arange(n))
    X = np.stack([x, -x, x * np.float32(0.5)], axis=1).astype(np.float32)
    want = narrow(a.astype(np.float64)[:, None] * X.astype(np.float64))
    # a subnormal comes through with its bits; a result in the subnormal range is rounded to one (ties to even), a result
    # below half the smallest becomes zero with its sign, one above FLT_MAX inf
    assert want[0, 0].view(np.uint32) == 1 and want[1, 0] == np.float32(1e-40)
    assert want[2, 0].view(np.uint32) == 2 and want[3, 0].view(np.uint32) == 2      # 1.5 -> 2 (even), 1.5 -> 2
    assert want[5, 0] == np.inf and want[6, 0] == -np.inf and want[5, 1] == -np.inf and np.isfinite(want[7, 0])
    assert 0 < want[8, 0] < np.float32(1.1754944e-38) and 0 < want[9, 0] < want[8, 0]
    dA = sa.dCSR.from_host(H)
    got, _ = spmm32(cfg, dA, X)
    assert same_bytes(got, want), (got, want)
    via64, _ = spmm64(cfg, dA, X)
    assert same_bytes(got, via64)
    # through beta: a subnormal Y is widened exactly too
    Y0 = np.full((n, 3), tiny, dtype=np.float32)
    got, _ = spmm32(cfg, dA, X, 1.0, 1.0, Y0)
    assert same_bytes(got, narrow(a.astype(np.float64)[:, None] * X.astype(np.float64) + Y0.astype(np.float64)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_hostile_input_is_refused_with_every_word_of_the_frame_intact(cfg, dtype):
    H, X, Y0, S = int_case(dtype)
    k, ldx, ldy = 3, 6, 5
    good = sa.dCSR.from_host(H)
    _, xs = frame(COLS, ldx, k, X[:, :k])
    L = _lib.load()
    fn = L.speck_spmm_f32_b32 if dtype == np.float32 else L.speck_spmm_f64_b32
    ro, nnz = H.row_offsets, H.nnz
    cases = []
    bad = ro.copy()
    bad[60] = bad[61] + 1                                                           # a descending pair
    cases.append((bad, None, nnz))
    cases.append((ro, None, nnz + 1))                                               # the last offset is short of nnz
    for p in (0, T - 1, T, nnz - 1, T + T // 2):                                    # an id = cols: first, tile edges, last, inside the long row
        col = H.col_ids.copy()
        col[p] = H.cols
        cases.append((ro, col, nnz))
    col = H.col_ids.copy()
    col[7] = 0xFFFFFFFF
    cases.append((ro, col, nnz))
    for n, (r, c, z) in enumerate(cases):
        dA = on_torch(H, ro=r, col=c, nnz=z)
        yb, ys = frame(H.rows, ldy, k)
        info = _lib.CSpmmInfo(7, 7, 7, 7, 7)
        alpha, beta = COEFFS[n % 2]
        torch.cuda.synchronize()
        rc = fn(cfg._h, alpha, C_.byref(dA._c), xs.data_ptr(), ldx, k, beta, ys.data_ptr(), ldy, C_.byref(info))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, n
        assert untouched(yb), n
        assert (info.rows_empty, info.rows_split, info.tiles, info.entries, info.terms) == (0, 0, 0, 0, 0), n
    got, _ = spmm32(cfg, good, X[:, :k], -2.0, 0.5, Y0[:, :k])                     # the config serves a valid call right after
    assert same_bytes(got, narrow(-2.0 * S[:, :k] + 0.5 * Y0[:, :k].astype(np.float64)))
    # Y inside X's span, one float closer than touching on either side: refused with nothing written; touching: served
    x_span, y_span = (COLS - 1) * ldx + k, (H.rows - 1) * ldy + k

    def layout(x_at, y_at):
        buf, _ = frame(x_span + y_span, 1, 1)
        torch.as_strided(buf, (COLS, k), (ldx, 1), x_at).copy_(torch.from_numpy(X[:, :k].copy()).to(DEV))
        return buf, buf.data_ptr() + 4 * x_at, buf.data_ptr() + 4 * y_at

    for x_at, y_at in ((0, x_span - 1), (y_span - 1, 0)):
        buf, px, py = layout(x_at, y_at)
        before = b32(host(buf)).copy()
        with pytest.raises(sa.SpeckError) as e:
            sa.spmm(good, px, cfg, Y=py, k=k, ldx=ldx, ldy=ldy, blocks=F32)
        assert e.value.status == ERR_INVALID
        assert np.array_equal(b32(host(buf)), before)
    for x_at, y_at in ((0, x_span), (y_span, 0)):
        buf, px, py = layout(x_at, y_at)
        sa.spmm(good, px, cfg, Y=py, k=k, ldx=ldx, ldy=ldy, blocks=F32)
        full = torch.from_numpy(host(buf))
        assert same_bytes(torch.as_strided(full, (H.rows, k), (ldy, 1), y_at).numpy(), narrow(S[:, :k]))
        assert np.array_equal(torch.as_strided(full, (COLS, k), (ldx, 1), x_at).numpy(), X[:, :k])


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_degenerate_shapes_and_the_most_right_hand_sides(cfg, dtype):
    X = ints((COLS, 2), 17)
    _, xs = frame(COLS, 5, 2, X)
    H, _, _, _ = int_case(dtype)
    # k == 0: nothing is written, info is zero
    yb, ys = frame(H.rows, 4, 2)
    out, info = sa.spmm(sa.dCSR.from_host(H), xs.data_ptr(), cfg, alpha=2.0, Y=ys.data_ptr(), k=0, ldx=5, ldy=4, blocks=F32)
    assert out is None and untouched(yb) and as_tuple(info) == (0, 0, 0, 0, 0)
    # no row: nothing is written
    none = sa.HostCSR(0, COLS, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))
    out, info = sa.spmm(sa.dCSR.from_host(none), xs, cfg, alpha=2.0, Y=ys.data_ptr(), ldy=4, blocks=F32)
    assert out is None and untouched(yb) and as_tuple(info) == (0, 0, 0, 0, 0)
    # no entry: Y = alpha (+0.0) + beta Y, signed zeros included
    hollow = mk([0] * 5, np.zeros(0, dtype=dtype))
    Y0 = np.array([[1.0, -0.0], [-2.0, 0.0], [0.0, -0.0], [4.5, 1e-40], [-0.0, -7.0]], dtype=np.float32)
    got, info = spmm32(cfg, sa.dCSR.from_host(hollow), X, 3.0, 2.0, Y0)
    assert same_bytes(got, narrow(3.0 * 0.0 + 2.0 * Y0.astype(np.float64)))
    assert info.rows_empty == 5 and info.entries == 0
    # k = 1024 on 300 entries, and one more
    k = sa.SPMM_MAX_RHS
    M = mk([100, 0, 200], ints(300, 20, dtype, lim=16), cols=7, seed=21)
    dM = sa.dCSR.from_host(M)
    Xk, Yk = ints((7, k + 1), 22), ints((3, k), 23)
    got, info = spmm32(cfg, dM, Xk[:, :k], 2.0, -3.0, Yk)
    assert same_bytes(got, narrow(2.0 * row_sums(M, Xk[:, :k]) - 3.0 * Yk.astype(np.float64)))
    assert info.terms == 300 * k
    _, xs1 = frame(7, k + 1, k + 1, Xk)
    yb, ys1 = frame(3, k + 1, k + 1)
    with pytest.raises(sa.SpeckError) as e:
        sa.spmm(dM, xs1, cfg, Y=ys1, blocks=F32)
    assert e.value.status == ERR_DIM_LIMIT and untouched(yb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_without_a_config_and_a_downloaded_float32_result(cfg, dtype):
    H, X, Y0, S = int_case(dtype)
    dA = sa.dCSR.from_host(H)
    k = 5
    got, _ = spmm32(None, dA, X[:, :k], -2.0, 0.5, Y0[:, :k])
    assert same_bytes(got, narrow(-2.0 * S[:, :k] + 0.5 * Y0[:, :k].astype(np.float64)))
    Z = torch.from_numpy(ints((COLS, 8), 24)).to(DEV)
    Z[:, 2:7].copy_(torch.from_numpy(X[:, :k].copy()).to(DEV))
    for c in (None, cfg):
        out, info = sa.spmm(dA, Z[:, 2:7], c, alpha=-2.0, blocks=F32)              # Y=None: downloaded; X a column slice
        assert out.dtype == np.float32 and out.shape == (H.rows, k) and same_bytes(out, narrow(-2.0 * S[:, :k]))
        assert info.entries == H.nnz
        yb, ys = frame(H.rows, 9, k)                                               # raw addresses with k and ld
        out, _ = sa.spmm(dA, Z.data_ptr() + 8, c, Y=ys.data_ptr(), k=k, ldx=8, ldy=9, blocks=F32)
        assert out is None and same_bytes(read_frame(yb, H.rows, 9, k), narrow(S[:, :k]))
    # a block is never converted: tensors of the other type are refused, on either side of the keyword
    dX = Z[:, 2:7]
    with pytest.raises(ValueError, match="spmm: X must be float32"):
        sa.spmm(dA, dX.double(), cfg, blocks=F32)
    with pytest.raises(ValueError, match="spmm: X must be float64"):
        sa.spmm(dA, dX, cfg)
    with pytest.raises(ValueError, match="spmm: Y must be float32"):
        sa.spmm(dA, dX, cfg, Y=torch.zeros((H.rows, k), dtype=torch.float64, device=DEV), blocks=F32)


def test_spmm_runs_on_the_callers_stream(cfg):
    """X is written by a copy on the caller's stream right before the call: ordering against the producer is by the
    stream alone"""
    H, X, _, S = int_case(np.float64)
    dA = sa.dCSR.from_host(H)
    real, dX = torch.from_numpy(X[:, :3].copy()).to(DEV), torch.zeros((COLS, 3), dtype=torch.float32, device=DEV)
    yb, ys = frame(H.rows, 4, 3)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    cfg.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream multiplies zeros
            dX.copy_(real, non_blocking=True)
        sa.spmm(dA, dX, cfg, Y=ys, blocks=F32)
        assert same_bytes(read_frame(yb, H.rows, 4, 3), narrow(S[:, :3]))
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched_by_the_three_float_block_calls(dtype):
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)                                        # (a touched zone is status 3)
        H, X, Y0, S = int_case(dtype)
        dA = sa.dCSR.from_host(H)
        for k in (1, 3, 9):
            got, _ = spmm32(cfg, dA, X[:, :k], -2.0, 0.5, Y0[:, :k])
            assert same_bytes(got, narrow(-2.0 * S[:, :k] + 0.5 * Y0[:, :k].astype(np.float64)))
            U = ints((H.rows, k), 30)
            got, _ = spmm_t32(cfg, dA, U)
            assert same_bytes(got, spmm_t64(cfg, dA, U)[0])
            C32, _ = sa.sddmm(dA, tf(U), tf(X[:, :k]), cfg, blocks=F32)
            C64, _ = sa.sddmm(dA, tf(U).double(), tf(X[:, :k]).double(), cfg)
            assert C32.to_host().data.tobytes() == C64.to_host().data.tobytes()
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_a_float_block_call_between_two_multiplies_keeps_the_reuse_sequence(cfg):
    h = sa.gen_matrix("scircuit", 0.08, 7, signed=True)
    dS, dC = sa.dCSR.from_host(h), sa.dCSR()
    for _ in range(3):
        sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"]
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1
    X = reals((h.cols, 3), 21)
    out, _ = sa.spmm(dS, tf(X), cfg, blocks=F32)
    assert same_bytes(out, spmm64(cfg, dS, X)[0])
    sa.spmm(dC, tf(X), cfg, blocks=F32)                                            # ... and of the product itself, where it lies
    sa.spmm_t(dS, tf(reals((h.rows, 3), 22)), cfg, blocks=F32)
    sa.sddmm(dS, tf(reals((h.rows, 3), 23)), tf(X), cfg, blocks=F32)
    sa.MultiplyspECK(dS, dS, dC, cfg)
    assert cfg.last_stats()["replayed"] == 1


def tf(a):
    """a contiguous float32 block on the device"""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


# ==================================================================================================== spmm_t
def column_edge_matrix(n, dtype, rows=700):
    """n entries whose COLUMNS meet the plan's tile edges: for n = 2 T + 5 column 7 holds 2 T + 1 entries behind three of
    the columns in front of it -- it spans three tiles of the plan -- and one entry follows; elsewhere columns at random
    over few ids, so that every column holds many entries and some end exactly where a tile does"""
    rng = np.random.default_rng(n)
    cols = 40
    if n == 2 * T + 5:
        col = np.concatenate([[1, 3, 3], np.full(2 * T + 1, 7), [20]])
        col = col[rng.permutation(n)]
    else:
        col = rng.integers(0, cols, size=n)
    row = np.sort(rng.integers(0, rows, size=n))
    lens = np.bincount(row, minlength=rows)
    return mk(lens, reals(n, n % 11, dtype), cols=cols, col=col)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_t_is_spmm_on_the_transpose_and_the_double_call_narrowed(cfg, dtype):
    for n in (T - 1, T, T + 1, 2 * T + 5):
        H = column_edge_matrix(n, dtype)
        dA = sa.dCSR.from_host(H)
        dAt = sa.transpose(dA, cfg)
        X, Y0 = reals((H.rows, K_MAX), 41), reals((H.cols, K_MAX), 42)
        with sa.transpose_plan(dA, cfg) as plan:
            if n == 2 * T + 5:
                assert plan.info.max_col_entries == 2 * T + 1
            for k in (KS if n == 2 * T + 5 else (1, 9, CB + 1)):
                for alpha, beta in COEFFS:
                    y0 = Y0[:, :k] if beta else None
                    got, info = spmm_t32(cfg, dA, X[:, :k], alpha, beta, y0, plan=plan)
                    want, info64 = spmm_t64(cfg, dA, X[:, :k], alpha, beta, y0, plan=plan)
                    assert same_bytes(got, want), (n, k, alpha, beta, where_differ(got, want))
                    assert as_tuple(info) == as_tuple(info64)
                    fwd, _ = spmm32(cfg, dAt, X[:, :k], alpha, beta, y0)            # spmm_b32 on transpose(A)
                    assert same_bytes(got, fwd), (n, k, alpha, beta, where_differ(got, fwd))
            if n == 2 * T + 5:
                assert info.cols_split >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_t_every_alignment_form_gives_the_same_bytes(cfg, dtype):
    H = column_edge_matrix(2 * T + 5, dtype)
    dA = sa.dCSR.from_host(H)
    k = 9
    X, Y0 = reals((H.rows, k), 43), reals((H.cols, k), 44)
    with sa.transpose_plan(dA, cfg) as plan:
        for alpha, beta in COEFFS:
            y0 = Y0 if beta else None
            base, _ = spmm_t32(cfg, dA, X, alpha, beta, y0, ldx=12, ldy=12, plan=plan)
            assert same_bytes(base, spmm_t64(cfg, dA, X, alpha, beta, y0, plan=plan)[0])
            for lead in range(4):
                for ldx in (12, 13, 14, 15):
                    got, _ = spmm_t32(cfg, dA, X, alpha, beta, y0, ldx=ldx, ldy=ldx - 2, x_lead=lead, y_lead=(lead + 3) % 4,
                                      plan=plan)
                    assert same_bytes(got, base), (lead, ldx, where_differ(got, base))
        # the first block of every form carries the tile's first use: k below a block, a pair, one column
        for kk in (1, 2, 3, CB + 3):
            base, _ = spmm_t32(cfg, dA, X[:, :kk], ldx=12, plan=plan)
            for lead, ldx in ((2, 12), (0, 14), (1, 12), (0, 13)):
                got, _ = spmm_t32(cfg, dA, X[:, :kk], ldx=ldx, x_lead=lead, plan=plan)
                assert same_bytes(got, base), (kk, lead, ldx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm_t_another_pattern_is_refused_and_one_plan_serves_both_block_types(cfg, dtype):
    H = column_edge_matrix(T + 1, dtype)
    dA = sa.dCSR.from_host(H)
    k = 5
    X = reals((H.rows, k), 45)
    other = H.col_ids.copy()
    other[T // 2] = (other[T // 2] + 1) % H.cols                                    # the same shape and nnz, one id moved
    dB = on_torch(H, col=other)
    with sa.transpose_plan(dA, cfg) as plan:
        _, xs = frame(H.rows, k, k, X)
        yb, ys = frame(H.cols, k + 2, k)
        with pytest.raises(sa.SpeckError) as e:
            sa.spmm_t(dB, xs, cfg, plan=plan, Y=ys, blocks=F32)
        assert e.value.status == ERR_INVALID and untouched(yb)
        # alternately through one plan: float, double, float, double -- each the other's bytes
        want = None
        for turn in range(4):
            got = spmm_t32(cfg, dA, X, plan=plan)[0] if turn % 2 == 0 else spmm_t64(cfg, dA, X, plan=plan)[0]
            want = got if want is None else want
            assert same_bytes(got, want), turn
        out, _ = sa.spmm_t(dA, tf(X), cfg, plan=plan, blocks=F32)                   # Y=None: a float32 array
        assert out.dtype == np.float32 and same_bytes(out, want)
    # degenerate: k == 0 writes nothing; plan=None builds one for the call
    yb, ys = frame(H.cols, 4, 2)
    out, info = sa.spmm_t(dA, tf(X).data_ptr(), cfg, Y=ys.data_ptr(), k=0, ldx=5, ldy=4, blocks=F32)
    assert out is None and untouched(yb) and info.terms == 0
    out, _ = sa.spmm_t(dA, tf(X), None, blocks=F32)
    assert same_bytes(out, want)


# ==================================================================================================== sddmm
def sddmm_case(dtype):
    """(H of about T + 300 entries with short rows, an empty row and a row over a tile edge; U, V real of 33 columns)"""
    key = ("sddmm", np.dtype(dtype).name)
    if key not in _CACHE:
        rng = np.random.default_rng(50)
        lens = [int(v) for v in rng.integers(0, 12, size=300)] + [0, T // 2 + 100, 3, 0] + [int(v) for v in rng.integers(0, 12, size=150)]
        H = mk(lens, reals(sum(lens), 51, dtype), cols=500, seed=52)
        assert T + 100 < H.nnz < 2 * T
        U, V = reals((H.rows, 33), 53), reals((H.cols, 33), 54)
        frozen(H.row_offsets, H.col_ids, H.data, U, V)
        _CACHE[key] = (H, U, V)
    return _CACHE[key]


def padded(vals, ld, lead=0):
    """vals as a float block in a payload frame, rows ld apart, lead floats off a 16-byte boundary"""
    return frame(vals.shape[0], ld, vals.shape[1], vals, lead=lead)[1]


def values_of(d):
    return d.to_host().data


SDDMM_MODES = [dict(alpha=1.0, beta=0.0), dict(alpha=-0.5, beta=1.0), dict(alpha=2.0, mode="hadamard")]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sddmm_every_k_in_place_and_into_a_new_c_is_the_double_call(cfg, dtype):
    H, U, V = sddmm_case(dtype)
    for k in SDDMM_KS:
        dU, dV = padded(U[:, :k], k + 3), padded(V[:, :k], k + 1)
        wU, wV = tf(U[:, :k]).double(), tf(V[:, :k]).double()
        for kw in SDDMM_MODES:
            dA = sa.dCSR.from_host(H)
            want, info64 = sa.sddmm(dA, wU, wV, cfg, **kw)
            got, info = sa.sddmm(dA, dU, dV, cfg, blocks=F32, **kw)
            assert as_tuple(info) == as_tuple(info64) and info.lanes == sa.sddmm_lanes(k) and info.terms == H.nnz * k
            w, g = want.to_host(), got.to_host()
            assert g.data.dtype == dtype and g.data.tobytes() == w.data.tobytes(), (k, kw)
            assert np.array_equal(g.col_ids, H.col_ids) and np.array_equal(g.row_offsets, H.row_offsets)
            same, _ = sa.sddmm(dA, dU, dV, cfg, blocks=F32, inplace=True, **kw)     # in place: the same bytes
            assert same is dA and values_of(dA).tobytes() == w.data.tobytes(), (k, kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sddmm_every_alignment_form_and_one_block_for_u_and_v(cfg, dtype):
    H, U, V = sddmm_case(dtype)
    dA = sa.dCSR.from_host(H)
    for k in (9, 4):
        want = values_of(sa.sddmm(dA, tf(U[:, :k]).double(), tf(V[:, :k]).double(), cfg, alpha=-0.5, beta=1.0)[0]).tobytes()
        for lead in range(4):
            for ld in (12, 13, 14, 15):
                dU, dV = padded(U[:, :k], ld, lead), padded(V[:, :k], ld + 1, (lead + 1) % 4)
                got, _ = sa.sddmm(dA, dU, dV, cfg, alpha=-0.5, beta=1.0, blocks=F32)
                assert values_of(got).tobytes() == want, (k, lead, ld)
    # U and V one block: a Gram matrix on the edges of a square pattern
    S = mk([3, 0, 5, 2, 40], reals(50, 55, dtype), cols=5, seed=56)
    G = reals((5, 17), 57)
    dS, dG = sa.dCSR.from_host(S), tf(G)
    got, info = sa.sddmm(dS, dG, dG, cfg, blocks=F32)
    want, info64 = sa.sddmm(dS, dG.double(), dG.double(), cfg)
    assert values_of(got).tobytes() == values_of(want).tobytes() and as_tuple(info) == as_tuple(info64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sddmm_a_view_with_an_odd_base_nan_and_a_hostile_id(cfg, dtype):
    H, U, V = sddmm_case(dtype)
    k = 9
    ro = H.row_offsets.astype(np.int64)
    a = next(r for r in range(1, H.rows) if ro[r] % 2 == 1 and ro[r + 1] > ro[r])
    b = H.rows - 3
    dU, dV = padded(U[:, :k], k + 2, 1), padded(V[:, :k], k + 1, 2)
    whole = values_of(sa.sddmm(sa.dCSR.from_host(H), dU, dV, cfg, alpha=2.0, beta=1.0, blocks=F32)[0])
    dA = sa.dCSR.from_host(H)
    view = dA.row_view(a, b)
    _, info = sa.sddmm(view, dU[a:b], dV, cfg, alpha=2.0, beta=1.0, blocks=F32, inplace=True)   # U offset by r0 ldu
    got = values_of(dA)
    assert got[ro[a]:ro[b]].tobytes() == whole[ro[a]:ro[b]].tobytes() and info.entries == ro[b] - ro[a]
    assert got[:ro[a]].tobytes() == H.data[:ro[a]].tobytes() and got[ro[b]:].tobytes() == H.data[ro[b]:].tobytes()
    out, _ = sa.sddmm(view, dU[a:b], dV, cfg, alpha=2.0, blocks=F32)              # ... and into a new C, rebased
    w64, _ = sa.sddmm(view, tf(U[a:b, :k]).double(), tf(V[:, :k]).double(), cfg, alpha=2.0)
    assert values_of(out).tobytes() == values_of(w64).tobytes()
    # a NaN of U(i, c) lands in the entries of row i, one of V(j, c) in the entries with id j: where it lands today
    Un, Vn = U[:, :k].copy(), V[:, :k].copy()
    i = next(r for r in range(H.rows) if ro[r + 1] - ro[r] >= 3)
    j = int(H.col_ids[ro[-1] - 1])
    Un[i, 8], Vn[j, 0] = np.nan, np.nan
    dA = sa.dCSR.from_host(H)
    got, info = sa.sddmm(dA, tf(Un), tf(Vn), cfg, blocks=F32)
    want, info64 = sa.sddmm(dA, tf(Un).double(), tf(Vn).double(), cfg)
    hit = np.isnan(values_of(got))
    expect = np.zeros(H.nnz, dtype=bool)
    expect[ro[i]:ro[i + 1]] = True
    expect |= H.col_ids == j
    assert np.array_equal(hit, expect) and info.nonfinite == expect.sum() == info64.nonfinite
    assert values_of(got).tobytes() == values_of(want).tobytes()
    # an id = cols anywhere: refused, in place, with nothing written
    col = H.col_ids.copy()
    col[T + 5] = H.cols
    dB = on_torch(H, col=col)
    with pytest.raises(sa.SpeckError) as e:
        sa.sddmm(dB, dU, dV, cfg, blocks=F32, inplace=True)
    assert e.value.status == ERR_INVALID
    assert values_of_torch(dB, H).tobytes() == H.data.tobytes()
    with pytest.raises(sa.SpeckError) as e:
        sa.sddmm(dB, dU, dV, cfg, blocks=F32)
    assert e.value.status == ERR_INVALID


def values_of_torch(d, H):
    """the values of an on_torch matrix, from the tensor it keeps"""
    torch.cuda.synchronize()
    return next(t for t in d._keep if t.dtype in (torch.float64, torch.float32)).cpu().numpy()[:H.nnz]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sddmm_the_largest_k_and_none(cfg, dtype):
    k = sa.SDDMM_MAX_K
    M = mk([100, 0, 200], reals(300, 60, dtype), cols=7, seed=61)
    U, V = reals((3, k), 62), reals((7, k), 63)
    dM = sa.dCSR.from_host(M)
    got, info = sa.sddmm(dM, tf(U), tf(V), cfg, alpha=0.25, beta=1.0, blocks=F32)
    want, info64 = sa.sddmm(dM, tf(U).double(), tf(V).double(), cfg, alpha=0.25, beta=1.0)
    assert values_of(got).tobytes() == values_of(want).tobytes() and as_tuple(info) == as_tuple(info64) and info.lanes == 8
    got, info = sa.sddmm(dM, 0, 0, cfg, alpha=3.0, beta=2.0, k=0, blocks=F32)      # k == 0: d = +0.0, the blocks may be NULL
    assert values_of(got).tobytes() == (3.0 * 0.0 + 2.0 * M.data.astype(np.float64)).astype(dtype).tobytes()
    with pytest.raises(sa.SpeckError) as e:
        sa.sddmm(dM, tf(reals((3, k + 1), 64)), tf(reals((7, k + 1), 65)), cfg, blocks=F32)
    assert e.value.status == ERR_DIM_LIMIT


# ==================================================================================================== the layer, once
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_attention_layer_and_its_backward_on_float_blocks_equal_the_widened_chain(cfg, dtype):
    """forward S = sddmm(Q, K) on the pattern, P = softmax(S), Y = spmm(P, Vagg); backward through ONE plan: dVagg =
    spmm_t(P, dY), dP = sddmm(P, dY, Vagg), dS = softmax_backward(P, dP), dQ = spmm(dS, K), dK = spmm_t(dS, Q)"""
    n, k = 200, 9
    rng = np.random.default_rng(80)
    lens = [int(v) for v in rng.integers(0, 14, size=n)]
    H = mk(lens, np.ones(sum(lens), dtype=dtype), cols=n, seed=81)
    Q, K, Vagg, dY = (reals((n, k), 82 + i) * np.float32(0.01) for i in range(4))

    def chain(wide):
        t = (lambda a: tf(a).double()) if wide else tf
        kw = {} if wide else {"blocks": F32}
        out = lambda r: host(r.float()) if wide else host(r)
        new = lambda: torch.full((n, k), float("nan"), dtype=torch.float64 if wide else torch.float32, device=DEV)
        dA = sa.dCSR.from_host(H)
        S, _ = sa.sddmm(dA, t(Q), t(K), cfg, **kw)
        P, _ = sa.softmax(S, cfg)
        Y, dV, dQ, dK = new(), new(), new(), new()
        sa.spmm(P, t(Vagg), cfg, Y=Y, **kw)
        with sa.transpose_plan(P, cfg) as plan:
            sa.spmm_t(P, t(dY), cfg, plan=plan, Y=dV, **kw)
            dP, _ = sa.sddmm(P, t(dY), t(Vagg), cfg, **kw)
            dS, _ = sa.softmax_backward(P, dP, cfg)
            sa.spmm(dS, t(K), cfg, Y=dQ, **kw)
            sa.spmm_t(dS, t(Q), cfg, plan=plan, Y=dK, **kw)
        return [values_of(S), values_of(P), values_of(dP), values_of(dS)], [out(Y), out(dV), out(dQ), out(dK)]

    mats32, blocks32 = chain(False)
    mats64, blocks64 = chain(True)
    for name, a, b in zip(("S", "P", "dP", "dS"), mats32, mats64):
        assert a.tobytes() == b.tobytes(), name
    for name, a, b in zip(("Y", "dVagg", "dQ", "dK"), blocks32, blocks64):
        assert same_bytes(a, b), (name, where_differ(a, b))
        assert np.isfinite(a).all() and np.abs(a).max() > 0
