"""speck_sddmm_* on the GPU (speck_amd/csrc/sddmm.hip): C = alpha (U V^T) on A's pattern + beta A, or times A.  The
expectation is numpy in this file.  exact(): with integer inputs in [-1024, 1024] every order of the sum gives the same bits
(k <= 1024: every sum stays below 2^53).  tree(): the header's tree restated -- the terms, the sequential partial sum of
lane l over the pairs q = l (mod L) in ascending c, the butterfly -- compared by bytes except where both sides are zero
(the sign of a zero d is unspecified).  tree() itself is held against math.fsum within (g_k + 2^-53) sum|t|,
g_k = k 2^-53 / (1 - k 2^-53).  U and V live in frames filled with a payload NaN: were a padding word or a word behind the
last row ever read, it would show in the result.  T = 4096 entries per tile below."""
import ctypes as C_
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import speck_amd as sa
from speck_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
DTYPES = [np.float64, np.float32]
T = sa.SDDMM_TILE_ENTRIES
EPS = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
COLS = 3000
TAIL = 8                                # payload words behind the last row of a frame
# every k of the issue; both sides of every switch of L(k) -- 4|5, 8|9, 16|17 -- are among them
KS = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128, 129, 130, 257]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def lanes(k):
    """the header's formula: L(k) = min(8, max(1, pow2ceil(ceil(k / 4))))"""
    quarter = (k + 3) // 4
    return min(8, max(1, 1 << max(quarter - 1, 0).bit_length()))


def mk(lens, data, cols=COLS, seed=1):
    """rows of the given lengths over `data`; column ids random in [0, cols), duplicates allowed, unsorted"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = np.random.default_rng(seed).integers(0, cols, size=len(data)).astype(np.uint32)
    return sa.HostCSR(len(lens), cols, ro, ci, np.asarray(data))


def ints(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).integers(-1024, 1025, size=shape).astype(dtype)


def real_values(shape, seed, dtype=np.float64):
    """mixed signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(dtype)


def rows_of(ro):
    ro = np.asarray(ro, dtype=np.int64)
    return np.repeat(np.arange(len(ro) - 1), np.diff(ro))


def gathered(H, U, V):
    """(U[row of entry], V[id of entry]), nnz x k each"""
    return U[rows_of(H.row_offsets)], V[H.col_ids.astype(np.int64)]


def exact(H, U, V):
    Ue, Ve = gathered(H, U, V)
    d = (Ue * Ve).sum(axis=1) if U.shape[1] else np.zeros(H.nnz)
    assert (np.abs(Ue * Ve).sum(axis=1) < 2.0 ** 53).all()
    return d


def tree(H, U, V, L):
    """d of every entry in the header's tree"""
    Ue, Ve = gathered(H, U, V)
    n, k = Ue.shape
    with np.errstate(invalid="ignore", over="ignore"):
        t = Ue * Ve                                                    # the terms, each rounded once
        p = np.zeros((n, L))                                           # a lane that owns no column holds +0.0
        for l in range(L):
            first = True
            for q in range(l, (k + 1) // 2, L):                        # its pairs, ascending
                for c in (2 * q, 2 * q + 1):
                    if c < k:
                        p[:, l] = t[:, c] if first else p[:, l] + t[:, c]
                        first = False
        s = L // 2
        while s:                                                       # p += p[l ^ s]
            p = p + p[:, np.arange(L) ^ s]
            s //= 2
    assert L == 1 or (p.view(np.uint64) == p.view(np.uint64)[:, :1]).all() or np.isnan(p).any()
    return p[:, 0].copy()


def expect(d, a, dtype, alpha=1.0, beta=0.0, mode="axpby"):
    """the chain behind d, as the header orders it; a: A's values"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = alpha * d
        if mode == "hadamard":
            x = x * a.astype(np.float64)
        elif beta != 0.0:
            x = x + beta * a.astype(np.float64)
        return x.astype(dtype)


def same_bytes(got, want):
    """bit for bit, except where both sides are zero (or both are NaN)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = (got.view(u) == want.view(u)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    return bool(ok.all())


def first_difference(got, want):
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.nonzero(got.view(u) != want.view(u))[0]
    return (len(bad), bad[:6], got[bad[:6]], want[bad[:6]])


def frame(n, ld, k, vals=None, lead=0):
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


def run(cfg, dA, U, V, ldu=None, ldv=None, u_lead=0, v_lead=0, **kw):
    """one call on padded blocks (ldu = k + 3, ldv = k + 2 unless given) passed as torch column slices; the frames keep
    their bytes.  Returns (matrix, info)"""
    k = U.shape[1]
    ldu = k + 3 if ldu is None else ldu
    ldv = k + 2 if ldv is None else ldv
    ub, us = frame(U.shape[0], ldu, k, U, lead=u_lead)
    vb, vs = frame(V.shape[0], ldv, k, V, lead=v_lead)
    before = host(ub).tobytes(), host(vb).tobytes()
    out = sa.sddmm(dA, us, vs, cfg, **kw)
    assert (host(ub).tobytes(), host(vb).tobytes()) == before, "a block was written"
    return out


def values(cfg, H, U, V, **kw):
    """... in place on a fresh copy of H: (values on the host, info)"""
    dA = sa.dCSR.from_host(H)
    C, info = run(cfg, dA, U, V, inplace=True, **kw)
    assert C is dA
    G = dA.to_host()
    assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
    return G.data, info


def counts(ro, k, want):
    """what speck_sddmm_info reports, counted on the host (ro absolute; want: the expected values)"""
    ro = np.asarray(ro, dtype=np.int64)
    nnz = int(ro[-1] - ro[0]) if len(ro) else 0
    return (nnz, nnz * k, int((~np.isfinite(want)).sum()), int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0, lanes(k))


def as_tuple(info):
    return (info.entries, info.terms, info.nonfinite, info.tiles, info.lanes)


def on_torch(H, ro=None, col=None, nnz=None, shift=0, data=True):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz; shift = 1 puts a dummy
    entry in front of data and col_ids and advances both pointers by one element (col_ids then lies 4 bytes off)"""
    pad = 8   # (a declared nnz beyond the entries is looked at before it is refused: it stays inside the tensors)
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    va = np.concatenate([np.full(shift, 77, dtype=H.data.dtype), H.data, np.zeros(pad, dtype=H.data.dtype)])
    ci = np.concatenate([np.zeros(shift, dtype=np.uint32), np.asarray(col, dtype=np.uint32), np.zeros(pad, dtype=np.uint32)])
    t_va = torch.from_numpy(va).to(DEV)
    t_ci = torch.from_numpy(ci.view(np.int32)).to(DEV)
    return sa.dCSR.from_device(H.rows, H.cols, H.nnz if nnz is None else nnz, t_ro.data_ptr(), t_ci.data_ptr() + 4 * shift,
                               t_va.data_ptr() + H.data.itemsize * shift if data else None, dtype=H.data.dtype,
                               keep=(t_ro, t_va, t_ci), host_row_offsets=np.asarray(ro, dtype=np.uint32))


def values_of(dA, shift=0):
    """the entries of an on_torch matrix as they are on the device now"""
    return host(dA._keep[1])[shift:-8]


_CACHE = {}
ROWS = 400


def sweep_matrix(dtype, kind):
    """3 tiles + 5 entries in 400 rows of 0 .. 80 entries (and what is left in the last), 3000 columns, unsorted with
    duplicates; the values integers or reals"""
    key = ("sweep", np.dtype(dtype).name, kind)
    if key not in _CACHE:
        lens = [int(v) for v in np.random.default_rng(2).integers(0, 60, size=ROWS - 1)]
        lens.append(3 * T + 5 - sum(lens))
        assert lens[-1] > 0
        data = ints(3 * T + 5, 3, dtype) if kind == "int" else real_values(3 * T + 5, 3, dtype)
        H = mk(lens, data, seed=4)
        for a in (H.row_offsets, H.col_ids, H.data):
            a.setflags(write=False)
        _CACHE[key] = H
    return _CACHE[key]


def blocks(k, kind, rows=ROWS, cols=COLS, seed=20):
    """(U, V) of k columns; for the sweep's matrix the first k of one pair of blocks of 1024 columns made once per kind"""
    width = 1024 if (rows, cols) == (ROWS, COLS) else k
    key = ("blocks", kind, rows, cols, seed, width)
    if key not in _CACHE:
        make = ints if kind == "int" else real_values
        U, V = make((rows, width), seed), make((cols, width), seed + 1)
        U.setflags(write=False), V.setflags(write=False)
        _CACHE[key] = (U, V)
    U, V = _CACHE[key]
    return np.ascontiguousarray(U[:, :k]), np.ascontiguousarray(V[:, :k])


# ---------------------------------------------------------------------------------------------------- 1: the k sweep
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_inputs_are_exact_for_every_k(cfg, dtype, k):
    H = sweep_matrix(dtype, "int")
    assert H.nnz == 3 * T + 5 and len(np.unique(H.col_ids)) < H.nnz and (np.diff(H.col_ids.astype(np.int64)) < 0).any()
    U, V = blocks(k, "int")
    d = exact(H, U, V)
    want = expect(d, H.data, dtype)
    got, info = values(cfg, H, U, V)
    assert same_bytes(got, want), (k, first_difference(got, want))
    assert as_tuple(info) == counts(H.row_offsets, k, want) and info.lanes == lanes(k) == sa.sddmm_lanes(k)
    # ... and with both coefficients at work, still exact
    want = expect(d, H.data, dtype, -3.0, 2.0)
    got, _ = values(cfg, H, U, V, alpha=-3.0, beta=2.0)
    assert same_bytes(got, want), (k, first_difference(got, want))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_real_inputs_follow_the_tree_bit_for_bit_and_the_tree_keeps_the_bound(cfg, dtype, k):
    H = sweep_matrix(dtype, "real")
    U, V = blocks(k, "real")
    d = tree(H, U, V, lanes(k))
    want = expect(d, H.data, dtype)
    got, info = values(cfg, H, U, V)
    assert same_bytes(got, want), (k, first_difference(got, want))
    assert as_tuple(info) == counts(H.row_offsets, k, want)
    if dtype == np.float64 and k:
        # (the tree against an order-free reference: alpha = 1, beta = 0, so got is d)
        Ue, Ve = gathered(H, U, V)
        t = Ue * Ve
        ref = np.array([math.fsum(r) for r in t])
        mag = np.array([math.fsum(r) for r in np.abs(t)])
        err = np.abs(got - ref)
        allowance = (k * EPS / (1.0 - k * EPS) + EPS) * mag
        print("largest error / allowance:", float(np.max(err / np.maximum(allowance, 1e-300))))
        assert (err <= allowance).all(), (k, np.nonzero(err > allowance)[0][:8])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_largest_k_on_300_entries(cfg, dtype):
    k = sa.SDDMM_MAX_K
    lens = [0, 7, 120, 0, 3, 170]
    for kind in ("int", "real"):
        make = ints if kind == "int" else real_values
        H = mk(lens, make(300, 5, dtype), cols=50, seed=6)
        U, V = blocks(k, kind, rows=len(lens), cols=50, seed=30)
        d = exact(H, U, V) if kind == "int" else tree(H, U, V, lanes(k))
        want = expect(d, H.data, dtype, 0.5, -1.0)
        got, info = values(cfg, H, U, V, alpha=0.5, beta=-1.0)
        assert same_bytes(got, want), (kind, first_difference(got, want))
        assert as_tuple(info) == (300, 300 * k, 0, 1, 8)
    with pytest.raises(sa.SpeckError) as e:                             # one column more is refused
        sa.sddmm(sa.dCSR.from_host(H), frame(len(lens), k + 1, k + 1)[1], frame(50, k + 1, k + 1)[1], cfg)
    assert e.value.status == 2


# ---------------------------------------------------------------------------------------------------- 2: row shapes
SHAPES = {
    "a tile of one-entry rows": [1] * T,
    "one row over three tiles": [5, 3 * T, 7],
    "empty rows between two tiles and at both ends": [0] * 2000 + [T] + [0] * 2000 + [T] + [0] * 2000,
    "a last tile of one entry": [T // 2, T // 2, 1],
    "no entry": [0, 0, 0],
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_shapes(cfg, dtype, shape):
    k, lens = 9, SHAPES[shape]
    H = mk(lens, ints(sum(lens), 7, dtype), seed=8)
    U, V = blocks(k, "int", rows=len(lens), seed=40)
    want = expect(exact(H, U, V), H.data, dtype, 2.0, 1.0)
    for inplace in (True, False):
        dA = sa.dCSR.from_host(H)
        C, info = run(cfg, dA, U, V, alpha=2.0, beta=1.0, inplace=inplace)
        G = C.to_host()
        assert same_bytes(G.data, want), (inplace, first_difference(G.data, want))
        assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
        assert as_tuple(info) == counts(H.row_offsets, k, want)
        assert info.tiles == {"no entry": 0, "a tile of one-entry rows": 1, "a last tile of one entry": 2,
                              "empty rows between two tiles and at both ends": 2}.get(shape, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_without_rows(cfg, dtype):
    empty = sa.HostCSR(0, COLS, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype=dtype))
    dA = sa.dCSR.from_host(empty)
    U, V = blocks(9, "int", rows=0)
    _, info = run(cfg, dA, U, V, inplace=True)
    assert as_tuple(info) == (0, 0, 0, 0, lanes(9))
    C, info = run(cfg, dA, U, V)
    assert (C.rows, C.cols, C.nnz) == (0, COLS, 0) and C.to_host().row_offsets.tolist() == [0]
    assert as_tuple(info) == (0, 0, 0, 0, lanes(9))


# ---------------------------------------------------------------------------------------------------- 3: layout independence
@pytest.mark.parametrize("k", [3, 8, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bits_do_not_depend_on_the_layout(cfg, dtype, k):
    H = sweep_matrix(dtype, "real")
    U, V = blocks(k, "real")
    want = expect(tree(H, U, V, lanes(k)), H.data, dtype, 1.5, -0.25)
    kw = dict(alpha=1.5, beta=-0.25)
    plain, _ = values(cfg, H, U, V, ldu=k, ldv=k, **kw)                 # ld == k
    assert same_bytes(plain, want), first_difference(plain, want)
    again, _ = values(cfg, H, U, V, ldu=k, ldv=k, **kw)                 # two runs: the same bytes
    assert again.tobytes() == plain.tobytes()
    for layout in (dict(ldu=k + 1, ldv=k + 1),                          # odd and even leading dimensions
                   dict(ldu=k + 2, ldv=k + 1),
                   dict(ldu=k + (k % 2), ldv=k + (k % 2), u_lead=1),    # U 8 bytes off a 16-byte boundary, ld even
                   dict(ldu=k + (k % 2), ldv=k + (k % 2), v_lead=1),    # ... and V
                   dict(ldu=k + 5, ldv=k + 8, u_lead=3, v_lead=2)):
        got, _ = values(cfg, H, U, V, **layout, **kw)
        assert got.tobytes() == plain.tobytes(), (layout, first_difference(got, plain))
    # U and V as column slices of ONE wider tensor
    n, ld = max(ROWS, COLS), 2 * k + 3
    wb, _ = frame(n, ld, 0)
    W = wb[:n * ld].view(n, ld)
    us, vs = W[:ROWS, 1:1 + k], W[:COLS, 2 + k:2 + 2 * k]
    us.copy_(torch.from_numpy(U).to(DEV))
    vs.copy_(torch.from_numpy(V).to(DEV))
    dA = sa.dCSR.from_host(H)
    sa.sddmm(dA, us, vs, cfg, inplace=True, **kw)
    got = dA.to_host().data
    assert got.tobytes() == plain.tobytes(), first_difference(got, plain)
    # A's arrays one element off: col_ids 4 bytes off a 16-byte boundary, the ids go one by one
    for inplace in (True, False):
        dA = on_torch(H, shift=1)
        assert dA._c.col_ids % 16 == 4
        C, _ = run(cfg, dA, U, V, inplace=inplace, **kw)
        got = values_of(dA, 1) if inplace else C.to_host().data
        assert got.tobytes() == plain.tobytes(), (inplace, first_difference(got, plain))
        assert host(dA._keep[1])[0] == 77 and (inplace or values_of(dA, 1).tobytes() == H.data.tobytes())


# ---------------------------------------------------------------------------------------------------- 4: in place, out of place, views
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_place_equals_in_place_and_matout_keeps_the_buffers_that_fit(cfg, dtype):
    k = 8
    H = sweep_matrix(dtype, "real")
    U, V = blocks(k, "real")
    inplace, _ = values(cfg, H, U, V, alpha=-2.0, beta=0.5)
    dA = sa.dCSR.from_host(H)
    C, info = run(cfg, dA, U, V, alpha=-2.0, beta=0.5)
    G = C.to_host()
    assert C is not dA and G.data.tobytes() == inplace.tobytes()
    assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
    assert (G.rows, G.cols, C.nnz) == (H.rows, H.cols, H.nnz)
    assert dA.to_host().data.tobytes() == H.data.tobytes()              # A is left alone
    ptrs = (C._c.row_offsets, C._c.col_ids, C._c.data)
    C2, _ = run(cfg, dA, U, V, matOut=C)                                # same rows, same nnz: nothing re-allocated
    assert C2 is C and ptrs == (C._c.row_offsets, C._c.col_ids, C._c.data)
    assert same_bytes(C.to_host().data, expect(tree(H, U, V, lanes(k)), H.data, dtype))
    other = sa.dCSR(np.float32 if dtype == np.float64 else np.float64)  # a matOut of the other value type is reset
    C4, _ = run(cfg, dA, U, V, alpha=-2.0, beta=0.5, matOut=other)
    assert C4 is other and other.dtype == np.dtype(dtype) and other.to_host().data.tobytes() == inplace.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_with_an_odd_base_gives_the_entries_of_the_whole(cfg, dtype):
    k = 5
    H = sweep_matrix(dtype, "real")
    ro = H.row_offsets.astype(np.int64)
    U, V = blocks(k, "real")
    whole, _ = values(cfg, H, U, V, alpha=3.0, beta=1.0)
    a = next(r for r in range(3, H.rows) if ro[r] % 2 == 1 and ro[r + 1] > ro[r])
    b = next(r for r in range(H.rows - 3, a, -1) if ro[r] % T not in (0, T - 1) and ro[r] // T == 2)
    lo, hi = ro[a], ro[b]
    assert lo % 2 == 1 and lo < T < 2 * T < hi and hi % T
    ub, us = frame(ROWS, k + 3, k, U)
    vb, vs = frame(COLS, k + 2, k, V)
    # in place: the owner's entries in front of and behind the view's keep their bytes
    dA = sa.dCSR.from_host(H)
    view = dA.row_view(a, b)
    assert view.nnz == hi - lo and us[a:b].data_ptr() == us.data_ptr() + 8 * a * (k + 3)
    _, info = sa.sddmm(view, us[a:b], vs, cfg, alpha=3.0, beta=1.0, inplace=True)
    G = dA.to_host()
    assert G.data[lo:hi].tobytes() == whole[lo:hi].tobytes(), first_difference(G.data[lo:hi], whole[lo:hi])
    assert G.data[:lo].tobytes() == H.data[:lo].tobytes() and G.data[hi:].tobytes() == H.data[hi:].tobytes()
    assert G.row_offsets.tobytes() == H.row_offsets.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
    assert as_tuple(info) == counts(ro[a:b + 1], k, whole[lo:hi])
    # into a new matrix: the offsets rebased, the ids copied
    dA = sa.dCSR.from_host(H)
    C, info = sa.sddmm(dA.row_view(a, b), us[a:b], vs, cfg, alpha=3.0, beta=1.0)
    G = C.to_host()
    assert G.data.tobytes() == whole[lo:hi].tobytes()
    assert G.row_offsets.tobytes() == (ro[a:b + 1] - lo).astype(np.uint32).tobytes()
    assert G.col_ids.tobytes() == H.col_ids[lo:hi].tobytes() and (G.rows, G.cols) == (b - a, H.cols)
    assert as_tuple(info) == counts(ro[a:b + 1], k, whole[lo:hi])
    assert dA.to_host().data.tobytes() == H.data.tobytes()


# ---------------------------------------------------------------------------------------------------- 5: coefficients and modes
@pytest.mark.parametrize("dtype", DTYPES)
def test_coefficients_and_modes(cfg, dtype):
    k = 9
    H = sweep_matrix(dtype, "real")
    U, V = blocks(k, "real")
    d = tree(H, U, V, lanes(k))
    a64 = H.data.astype(np.float64)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0), (0.0, 1.0), (0.0, 0.0)):
        with np.errstate(over="ignore"):
            want = ((alpha * d) + (beta * a64)).astype(dtype) if beta else (alpha * d).astype(dtype)
        assert want.tobytes() == expect(d, H.data, dtype, alpha, beta).tobytes()
        got, info = values(cfg, H, U, V, alpha=alpha, beta=beta)
        assert same_bytes(got, want), (alpha, beta, first_difference(got, want))
        assert as_tuple(info) == counts(H.row_offsets, k, want)
    for alpha in (1.0, -0.75):
        want = ((alpha * d) * a64).astype(dtype)
        for mode in ("hadamard", sa.SDDMM_HADAMARD):
            got, info = values(cfg, H, U, V, alpha=alpha, mode=mode)
            assert same_bytes(got, want), (alpha, first_difference(got, want))
            assert as_tuple(info) == counts(H.row_offsets, k, want)
    # beta == 0: A's values are not read -- a NaN in every one of them does not survive ...
    nans = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, np.full(H.nnz, np.nan, dtype=dtype))
    got, info = values(cfg, nans, U, V, alpha=2.0)
    assert same_bytes(got, expect(d, H.data, dtype, 2.0)) and info.nonfinite == 0
    got, info = values(cfg, nans, U, V, alpha=2.0, beta=1.0)            # (beta != 0 reads them)
    assert np.isnan(got).all() and info.nonfinite == H.nnz
    # ... and out of place they may be absent
    dA = on_torch(H, data=False)
    assert not dA._c.data
    C, _ = run(cfg, dA, U, V, alpha=2.0)
    G = C.to_host()
    assert same_bytes(G.data, expect(d, H.data, dtype, 2.0)) and G.col_ids.tobytes() == H.col_ids.tobytes()
    for kw in (dict(inplace=True), dict(beta=1.0), dict(mode="hadamard")):
        with pytest.raises(sa.SpeckError) as e:
            run(cfg, dA, U, V, **kw)
        assert e.value.status == ERR_INVALID


def test_fp32_results_are_rounded_once(cfg):
    """d = 1 + 2^-24 lies half way between two floats and a = 2^-30 tips it up: x = d + a rounds to 1 + 2^-23, where a d
    rounded to float first (ties to even: 1.0) would stay 1.0"""
    H = sa.HostCSR(1, 1, np.array([0, 1], np.uint32), np.zeros(1, np.uint32), np.array([2.0 ** -30], dtype=np.float32))
    U, V = np.array([[1.0, 2.0 ** -24]]), np.array([[1.0, 1.0]])
    d = tree(H, U, V, 1)
    assert d[0] == 1.0 + 2.0 ** -24
    want = expect(d, H.data, np.float32, 1.0, 1.0)
    twice = np.float32(d[0]) + np.float32(H.data[0])
    assert want[0] == np.float32(1.0 + 2.0 ** -23) and twice == np.float32(1.0)
    got, _ = values(cfg, H, U, V, beta=1.0)
    assert got.tobytes() == want.tobytes(), (got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_u_and_v_may_be_one_block(cfg, dtype):
    k, n = 6, 500
    lens = [int(v) for v in np.random.default_rng(9).integers(0, 30, size=n)]
    H = mk(lens, real_values(sum(lens), 10, dtype), cols=n, seed=11)
    U, _ = blocks(k, "real", rows=n, cols=n, seed=50)
    want = expect(tree(H, U, U, lanes(k)), H.data, dtype)
    _, us = frame(n, k + 2, k, U)
    dA = sa.dCSR.from_host(H)
    sa.sddmm(dA, us, us, cfg, inplace=True)
    got = dA.to_host().data
    assert same_bytes(got, want), first_difference(got, want)
    diag = H.col_ids.astype(np.int64) == rows_of(H.row_offsets)                  # a Gram matrix: squares on the diagonal
    assert (got[diag] >= 0).all()


# ---------------------------------------------------------------------------------------------------- 6: the k = 1 identity
def test_k_equal_one_is_scale_with_a_row_and_a_column_vector(cfg):
    H = sweep_matrix(np.float64, "real")
    U, V = blocks(1, "real")
    got, _ = values(cfg, H, U, V, ldu=1, ldv=1)
    dA = sa.dCSR.from_host(H)
    u_t, v_t = torch.from_numpy(U[:, 0].copy()).to(DEV), torch.from_numpy(V[:, 0].copy()).to(DEV)
    S, _ = sa.scale(sa.pattern_ones(dA, cfg), cfg, row=u_t, col=v_t)
    assert S.to_host().data.tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------- 7: non-finite values
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_land_in_exactly_the_entries_that_reference_them(cfg, dtype):
    k = 5
    H = sweep_matrix(dtype, "int")
    ro, ci = H.row_offsets.astype(np.int64), H.col_ids.astype(np.int64)
    rw = rows_of(ro)
    i = next(r for r in range(H.rows) if ro[r + 1] - ro[r] >= 3)
    j = int(ci[ro[H.rows // 2]])
    for what in ("nan in U", "nan in V", "inf against 0"):
        U, V = blocks(k, "int")
        V[V == 0] = 1.0                                                # (no zero by chance)
        U[U == 0] = 1.0
        if what == "nan in U":
            U[i, 3] = np.nan
            marked = rw == i
        elif what == "nan in V":
            V[j, 4] = np.nan
            marked = ci == j
        else:
            U[i, 2] = np.inf
            j0 = int(ci[ro[i]])
            V[j0, 2] = 0.0                                             # 0 * inf: a NaN in (i, j0), an inf in the rest of row i
            marked = rw == i
        want = expect(tree(H, U, V, lanes(k)), H.data, dtype)
        assert (~np.isfinite(want) == marked).all() and marked.any() and not marked.all()
        if what == "inf against 0":
            assert (np.isnan(want) == (marked & (ci == j0))).all() and np.isinf(want[marked & (ci != j0)]).all()
        got, info = values(cfg, H, U, V)                               # (the status is SPECK_OK: no exception)
        assert same_bytes(got, want) and (np.isnan(got) == np.isnan(want)).all(), what
        assert info.nonfinite == int(marked.sum()) and as_tuple(info) == counts(ro, k, want)


def test_an_overflow_on_the_rounding_to_float_is_counted(cfg):
    k = 4
    for dtype in DTYPES:
        H = sweep_matrix(dtype, "int")
        U, V = blocks(k, "int")
        d = exact(H, U, V)
        want = expect(d, H.data, dtype, 1e35)                           # |alpha d| up to 4e41: finite in double only
        assert np.isfinite(1e35 * d).all()
        got, info = values(cfg, H, U, V, alpha=1e35)
        assert same_bytes(got, want)
        assert info.nonfinite == int((~np.isfinite(want)).sum())
        assert (info.nonfinite == 0) == (dtype == np.float64) and (dtype == np.float64 or info.nonfinite > H.nnz // 2)


# ---------------------------------------------------------------------------------------------------- 8: refusals on the device
def hostile(H, which):
    """(offsets, column ids, declared nnz)"""
    ro, ci, rows, nnz = H.row_offsets, H.col_ids, H.rows, H.nnz
    if which == "descending":
        bad = ro.copy()
        bad[rows // 2] = bad[rows // 2 + 1] + 1
        return bad, ci, nnz
    if which == "short":
        return ro, ci, nnz + 1
    at, value = {"id first of a tile": (T, H.cols), "id last of a tile": (2 * T - 1, H.cols), "id last entry": (nnz - 1, H.cols),
                 "id all ones": (T + 17, 0xFFFFFFFF)}[which]
    bad = ci.copy()
    bad[at] = value
    return ro, bad, nnz


HOSTILE = ["id first of a tile", "id last of a tile", "id last entry", "id all ones", "descending", "short"]


@pytest.mark.parametrize("which", HOSTILE)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_is_written(cfg, dtype, which):
    k = 9
    H = sweep_matrix(dtype, "real")
    ro, ci, nnz = hostile(H, which)
    U, V = blocks(k, "real")
    ub, us = frame(ROWS, k + 3, k, U)
    vb, vs = frame(COLS, k + 2, k, V)
    lens = np.diff(H.row_offsets.astype(np.int64)).tolist()
    lens[0], lens[-1] = lens[0] + 1, lens[-1] - 1
    other = mk(lens, real_values(H.nnz, 55, dtype), seed=56)       # C before the call: A's shape, so its buffers would be re-used
    assert (other.rows, other.nnz) == (H.rows, H.nnz) and other.row_offsets[1] != H.row_offsets[1]
    L = _lib.load()
    fn = L.speck_sddmm_f32 if dtype == np.float32 else L.speck_sddmm_f64
    for mode, beta in ((sa.SDDMM_AXPBY, 0.0), (sa.SDDMM_AXPBY, 1.0), (sa.SDDMM_HADAMARD, 0.0)):
        for new in (False, True):
            dA = on_torch(H, ro=ro, col=ci, nnz=nnz)
            dC = sa.dCSR.from_host(other)
            ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            p = _lib.CSddmmParams()
            p.mode, p.k, p.alpha, p.beta = mode, k, 2.0, beta
            p.d_U, p.ldu, p.d_V, p.ldv = us.data_ptr(), k + 3, vs.data_ptr(), k + 2
            info = _lib.CSddmmInfo(9, 9, 9, 9, 9)
            torch.cuda.synchronize()
            rc = fn(cfg._h, C_.byref(dA._c), C_.byref(p), C_.byref(dC._c) if new else None, C_.byref(info))
            torch.cuda.synchronize()
            assert rc == ERR_INVALID, (which, mode, beta, new)
            assert as_tuple(info) == (0, 0, 0, 0, 0)
            assert values_of(dA).tobytes() == H.data.tobytes(), (which, mode, beta, new)
            assert ptrs == (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            G = dC.to_host()
            assert G.data.tobytes() == other.data.tobytes() and G.col_ids.tobytes() == other.col_ids.tobytes() and \
                G.row_offsets.tobytes() == other.row_offsets.tobytes(), (which, mode, beta, new)
    # the config serves a valid call right after
    got, _ = values(cfg, H, U, V)
    assert same_bytes(got, expect(tree(H, U, V, lanes(k)), H.data, dtype))


# ---------------------------------------------------------------------------------------------------- 9: housekeeping
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config(dtype):
    k = 4
    H = sweep_matrix(dtype, "real")
    U, V = blocks(k, "real")
    d = tree(H, U, V, lanes(k))
    for inplace, kw in ((True, dict(alpha=1.5, beta=0.5)), (False, dict(mode="hadamard"))):
        C, info = run(None, sa.dCSR.from_host(H), U, V, inplace=inplace, **kw)
        want = expect(d, H.data, dtype, **kw)
        assert same_bytes(C.to_host().data, want) and as_tuple(info) == counts(H.row_offsets, k, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    k = 9
    H = sweep_matrix(dtype, "real")
    ro = H.row_offsets.astype(np.int64)
    U, V = blocks(k, "real")
    d = tree(H, U, V, lanes(k))
    cfg = sa.spECKConfig.initialize(0)
    try:
        cfg.set_option("guard_bytes", 4096)
        for kw in (dict(alpha=2.0, beta=1.0), dict(mode="hadamard")):
            for inplace in (True, False):
                dA = sa.dCSR.from_host(H)                                      # (allocated with zones: A's are checked in place)
                C, _ = run(cfg, dA, U, V, inplace=inplace, **kw)               # (a touched zone is status 3)
                assert same_bytes(C.to_host().data, expect(d, H.data, dtype, **kw))
                a = next(r for r in range(3, H.rows) if ro[r] % 2 == 1)        # a view with an odd base: the narrow form
                run(cfg, sa.dCSR.from_host(H).row_view(a, H.rows), U[a:], V, inplace=inplace, **kw)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_runs_on_the_callers_stream(cfg):
    """U is written by a copy on the caller's stream right before the call: ordering against the producer is by the
    stream alone"""
    k = 8
    H = sweep_matrix(np.float64, "real")
    U, V = blocks(k, "real")
    dA = sa.dCSR.from_host(H)
    u_real, v_t = torch.from_numpy(U).to(DEV), torch.from_numpy(V).to(DEV)
    u_t = torch.zeros_like(u_real)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    cfg.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(20_000_000)          # ~10 ms: whatever does not wait for the stream multiplies zeros
            u_t.copy_(u_real, non_blocking=True)
        sa.sddmm(dA, u_t, v_t, cfg, inplace=True)
        got = dA.to_host().data
        assert same_bytes(got, expect(tree(H, U, V, lanes(k)), H.data, np.float64))
    finally:
        cfg.set_stream(None)
        torch.cuda.synchronize()


def test_the_caller_that_includes_sddmm_h_only_runs(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_sddmm.cpp")
    out = str(tmp_path / "caller_sddmm")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "sddmm caller ok" in done.stdout, (done.returncode, done.stdout, done.stderr)
