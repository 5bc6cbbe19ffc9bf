"""speck_softmax_* on the GPU (speck_amd/csrc/softmax.hip): the row softmax of a device CSR, forward and backward.  The
expectation is numpy in this file.  What the contract pins bit for bit is held by same_bytes against the library's own
reduce and scale (the identities of the header) and against numpy's chain for the backward; only exp itself is left to a
tolerance, the derived bound of test_forward_accuracy.  T = 4096 entries per tile below.

U_EXP: the ROCm toolkit ships no document that states the ULP bound of the device's double exp (the HIP math tables are
not among its files), so it was measured: scripts/softmax_time.py --exp-ulp runs the
device exp -- mode "exp" on rows (0, v) -- over the arguments x - m of this file's accuracy inputs against np.exp in
np.longdouble; the worst observed error and the choice (twice it, rounded up to an integer) stand in profiles/softmax.txt."""
import ctypes as C_
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
T = sa.SOFTMAX_TILE_ENTRIES
SENTINEL_BITS = 0x7FF8DEADBEEF1234      # a NaN with a payload
DEV = "cuda:0"
COLS = 3000
U_EXP = 2                               # ULPs of the device's double exp: measured, profiles/softmax.txt
ALPHAS = [1.0, 0.125, -2.0]


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- helpers
def mk(lens, data, cols=COLS, seed=1):
    """rows of the given lengths over `data`; column ids random in [0, cols), duplicates allowed, unsorted"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum(lens)
    assert ro[-1] == len(data)
    ci = np.random.default_rng(seed).integers(0, cols, size=len(data)).astype(np.uint32)
    return sa.HostCSR(len(lens), cols, ro, ci, np.asarray(data))


def uniform(n, seed, dtype=np.float64):
    return np.random.default_rng(seed).uniform(-30.0, 30.0, size=n).astype(dtype)


def real_values(n, seed, dtype=np.float64):
    """mixed signs over seven and a half decades, 1e-6 .. 6e1: with |alpha| <= 2 every exp(x - m) stays a normal double (a
    relative bound says nothing about a subnormal one)"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.random(n)) * 10.0 ** rng.uniform(-6, 1.5, size=n)).astype(dtype)


def with_data(H, data):
    return sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, np.asarray(data))


def rows_of(ro):
    ro = np.asarray(ro, dtype=np.int64)
    return np.repeat(np.arange(len(ro) - 1), np.diff(ro))


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


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def payload(n):
    """n doubles on the device, each the payload NaN"""
    return torch.from_numpy(np.full(max(n, 1), SENTINEL_BITS, dtype=np.uint64).view(np.float64)).to(DEV)[:n]


def is_payload(a):
    return bool((np.ascontiguousarray(a).view(np.uint64) == SENTINEL_BITS).all())


def as_tuple(info):
    return (info.entries, info.nonfinite, info.rows_empty, info.rows_split, info.tiles)


def counts(ro, result):
    """what info holds for the offsets ro (absolute) and the values the call wrote"""
    ro = np.asarray(ro, dtype=np.int64)
    b, e = ro[:-1], ro[1:]
    full = e > b
    split = int((full & (b // T != (np.maximum(e, 1) - 1) // T)).sum())
    nnz = int(ro[-1] - ro[0])
    tiles = int((ro[-1] - 1) // T - ro[0] // T + 1) if nnz else 0
    return (nnz, int((~np.isfinite(result)).sum()), int((~full).sum()), split, tiles)


def forward(cfg, dA, alpha=1.0, mode="normalized", inplace=False, matOut=None):
    """(values, m, s, info) of one forward call, the vectors from buffers that held the payload NaN"""
    m, s = payload(dA.rows), payload(dA.rows)
    C, info = sa.softmax(dA, cfg, alpha=alpha, mode=mode, inplace=inplace, matOut=matOut, row_max=m, row_sum=s)
    return C.to_host().data, host(m), host(s), info


def backward(cfg, dP, dG, alpha=1.0, inplace=False):
    r = payload(dP.rows)
    C, info = sa.softmax_backward(dP, dG, cfg, alpha=alpha, inplace=inplace, row_sum=r)
    return C.to_host().data, host(r), info


def numpy_forward(H, alpha, mode="normalized"):
    """the contract's steps in float64 (the sum in numpy's order: compared within the bound, never by bytes)"""
    ro = H.row_offsets.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = alpha * H.data.astype(np.float64)
        m = np.full(H.rows, -np.inf)
        s = np.zeros(H.rows)
        out = np.zeros(H.nnz)
        for r in range(H.rows):
            b, e = ro[r] - ro[0], ro[r + 1] - ro[0]
            if b == e:
                continue
            m[r] = np.nan if np.isnan(x[b:e]).any() else x[b:e].max()
            ex = np.exp(x[b:e] - m[r])
            s[r] = ex.sum()
            out[b:e] = ex if mode == "exp" else ex / s[r]
    return out, m, s


def numpy_backward(cfg, H, g, alpha):
    """bit for bit: (alpha * (p * (g - r[row]))).astype(T), r the reduce(.., "sum") of the matrix of p g in float64"""
    p64, g64 = H.data.astype(np.float64), g.astype(np.float64)
    r, _, _ = sa.reduce(sa.dCSR.from_host(with_data(H, p64 * g64)), cfg, "sum", total=False)
    with np.errstate(invalid="ignore", over="ignore"):
        return (alpha * (p64 * (g64 - r[rows_of(H.row_offsets)]))).astype(H.data.dtype), r


def check_forward(cfg, H, alpha):
    """every identity of the contract on H (either value type), in place and out of place, both modes; returns P"""
    dtype = H.data.dtype
    H64 = with_data(H, H.data.astype(np.float64))
    ro = H.row_offsets
    # fp64: the identities with reduce and scale
    E64, m64, s64, info = forward(cfg, sa.dCSR.from_host(H64), alpha, "exp")
    assert as_tuple(info) == counts(ro, E64)
    scaled, _ = sa.scale(sa.dCSR.from_host(H64), cfg, alpha=alpha)
    m_ref, _, _ = sa.reduce(scaled, cfg, "max", total=False)
    assert same_bytes(m64, m_ref), first_difference(m64, m_ref)
    dE = sa.dCSR.from_host(with_data(H64, E64))
    s_ref = payload(H.rows)
    sa.reduce(dE, cfg, "sum", total=False, out_ptr=s_ref.data_ptr())
    assert same_bytes(s64, host(s_ref)), first_difference(s64, host(s_ref))
    P_ref = sa.scale(dE, cfg, row=s_ref, row_div=True)[0].to_host().data
    P64, m2, s2, info = forward(cfg, sa.dCSR.from_host(H64), alpha, "normalized")
    assert same_bytes(P64, P_ref), first_difference(P64, P_ref)
    assert m2.tobytes() == m64.tobytes() and s2.tobytes() == s64.tobytes()
    assert as_tuple(info) == counts(ro, P64)
    empty = np.diff(ro.astype(np.int64)) == 0
    assert (m64[empty] == -np.inf).all() and (s64[empty] == 0).all() and not np.signbit(s64[empty]).any()
    # the value type of H: the fp64 call on the widened matrix, rounded once; in place equals out of place
    for mode, want in (("exp", E64), ("normalized", P64)):
        with np.errstate(over="ignore"):
            want = want.astype(dtype)
        got, m, s, info = forward(cfg, sa.dCSR.from_host(H), alpha, mode)
        assert got.tobytes() == want.tobytes() or same_bytes(got, want), (mode, first_difference(got, want))
        assert m.tobytes() == m64.tobytes() and s.tobytes() == s64.tobytes()
        assert as_tuple(info) == counts(ro, want)
        dA = sa.dCSR.from_host(H)
        again, m, s, info = forward(cfg, dA, alpha, mode, inplace=True)
        assert again.tobytes() == got.tobytes() and m.tobytes() == m64.tobytes() and s.tobytes() == s64.tobytes()
        G = dA.to_host()
        assert G.row_offsets.tobytes() == ro.tobytes() and G.col_ids.tobytes() == H.col_ids.tobytes()
    out = sa.softmax(sa.dCSR.from_host(H), cfg, alpha=alpha)[0].to_host()
    assert out.row_offsets.tobytes() == ro.tobytes() and out.col_ids.tobytes() == H.col_ids.tobytes()
    assert out.data.tobytes() == got.tobytes()                              # two runs, with and without the vectors
    return got


def check_backward(cfg, H, g, alpha):
    """H holds P; in place and out of place against numpy's chain"""
    want, r_ref = numpy_backward(cfg, H, g, alpha)
    dG = sa.dCSR.from_host(with_data(H, g))
    got, r, info = backward(cfg, sa.dCSR.from_host(H), dG, alpha)
    assert same_bytes(got, want), first_difference(got, want)
    assert same_bytes(r, r_ref), first_difference(r, r_ref)
    assert as_tuple(info) == counts(H.row_offsets, want)
    dP = sa.dCSR.from_host(H)
    again, r2, info = backward(cfg, dP, dG, alpha, inplace=True)
    assert again.tobytes() == got.tobytes() and r2.tobytes() == r.tobytes()
    assert dG.to_host().data.tobytes() == g.tobytes()


_CACHE = {}
SMALL = [0, 1, 2, 0, 17, 16, 15, 64, 0]
# (length, what it is) with T = 4096; the offsets are in the comments
EDGES = [100, T - 100,        # [0, 100) [100, T): a row that ends exactly at entry T
         T,                   # [T, 2T): a row of exactly T entries on a tile boundary -- the tile lies inside one row
         T - 1, 51,           # [2T, 3T-1) [3T-1, 3T+50): one entry in tile 2, the rest in tile 3
         T + 1,               # [3T+50, 4T+51): T + 1 entries
         2 * T + 100,         # [4T+51, 6T+151): a row over three tiles
         2 * T - 151,         # [6T+151, 8T): a split row that ends on a tile edge ...
         0, 0,                # ... empty rows sitting on that edge ...
         T + 7,               # [8T, 9T+7): ... and a split row that starts there
         10, 0, 300, T,       # tile 9: a head (7 entries), whole rows, a tail [9T+317, 10T+317)
         33, 1, 0, 64]


def edge_matrix(dtype, kind="uniform"):
    key = ("edges", np.dtype(dtype).name, kind)
    if key not in _CACHE:
        n = sum(EDGES)
        H = mk(EDGES, uniform(n, 5, dtype) if kind == "uniform" else real_values(n, 6, dtype), seed=7)
        ro = H.row_offsets.astype(np.int64)
        assert ro[2] == T and ro[3] == 2 * T and ro[4] == 3 * T - 1 and ro[8] == ro[9] == ro[10] == 8 * T and ro[11] == 9 * T + 7
        for a in (H.row_offsets, H.col_ids, H.data):
            a.setflags(write=False)
        _CACHE[key] = H
    return _CACHE[key]


def gradient(H, seed):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, size=H.nnz).astype(H.data.dtype)


def probabilities(H, seed):
    """values as a forward call leaves them: positive, the rows summing to about 1"""
    rng = np.random.default_rng(seed)
    e = rng.random(H.nnz) + 1e-3
    sums = np.zeros(H.rows)
    np.add.at(sums, rows_of(H.row_offsets), e)
    return with_data(H, (e / sums[rows_of(H.row_offsets)]).astype(H.data.dtype))


# ---------------------------------------------------------------------------------------------------- 1: short rows
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_short_rows_every_mode_in_place_and_out_of_place(cfg, dtype, alpha):
    H = mk(SMALL, uniform(sum(SMALL), 3, dtype), seed=4)
    P = check_forward(cfg, H, alpha)
    sums = np.zeros(H.rows)
    np.add.at(sums, rows_of(H.row_offsets), P.astype(np.float64))
    assert np.allclose(sums[np.diff(H.row_offsets.astype(np.int64)) > 0], 1.0, rtol=0, atol=1e-6)
    assert P[0] == 1.0                                                      # the row of one entry
    check_backward(cfg, with_data(H, P), gradient(H, 8), alpha)


# ---------------------------------------------------------------------------------------------------- 2: tile edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_at_every_tile_edge(cfg, dtype):
    H = edge_matrix(dtype)
    P = check_forward(cfg, H, 0.125)
    assert counts(H.row_offsets, P)[3] == 6                                 # the split rows of EDGES
    check_backward(cfg, with_data(H, P), gradient(H, 9), -2.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_over_67_tiles(cfg, dtype):
    """65 whole tiles inside the row: the lanes of chain_finish take a second trip"""
    lens = [3, 66 * T + 10, 6]
    H = mk(lens, uniform(sum(lens), 11, dtype), seed=12)
    P = check_forward(cfg, H, 1.0)
    assert counts(H.row_offsets, P)[3:] == (1, 67)
    check_backward(cfg, with_data(H, P), gradient(H, 13), 1.0)


# ---------------------------------------------------------------------------------------------------- 3: views
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_with_an_odd_base_gives_the_rows_of_the_whole(cfg, dtype):
    H = edge_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    alpha = 0.125
    whole, m, s, _ = forward(cfg, sa.dCSR.from_host(H), alpha)
    g = gradient(H, 14)
    HP = with_data(H, whole)
    back, r, _ = backward(cfg, sa.dCSR.from_host(HP), sa.dCSR.from_host(with_data(H, g)), alpha)
    for a, b in ((4, 7), (6, 12), (11, 17)):                               # bases 3T - 1, 4T + 51, 9T + 7
        lo, hi = ro[a], ro[b]
        assert lo % 2 == 1
        assert lo % T and hi % T
        # forward in place: the owner's entries in front of and behind the view's keep their bytes
        dA = sa.dCSR.from_host(H)
        got, vm, vs, info = forward(cfg, dA.row_view(a, b), alpha, inplace=True)
        G = dA.to_host()
        assert G.data[lo:hi].tobytes() == whole[lo:hi].tobytes(), first_difference(G.data[lo:hi], whole[lo:hi])
        assert G.data[:lo].tobytes() == H.data[:lo].tobytes() and G.data[hi:].tobytes() == H.data[hi:].tobytes()
        assert vm.tobytes() == m[a:b].tobytes() and vs.tobytes() == s[a:b].tobytes()
        assert as_tuple(info) == counts(ro[a:b + 1], whole[lo:hi])
        # into a new matrix: the offsets rebased, the ids copied
        dA = sa.dCSR.from_host(H)
        C, info = sa.softmax(dA.row_view(a, b), cfg, alpha=alpha)
        G = C.to_host()
        assert G.data.tobytes() == whole[lo:hi].tobytes()
        assert G.row_offsets.tobytes() == (ro[a:b + 1] - lo).astype(np.uint32).tobytes()
        assert G.col_ids.tobytes() == H.col_ids[lo:hi].tobytes() and (G.rows, G.cols) == (b - a, H.cols)
        assert dA.to_host().data.tobytes() == H.data.tobytes()
        # backward: G is the same view of its owner
        dP, dG = sa.dCSR.from_host(HP), sa.dCSR.from_host(with_data(H, g))
        _, vr, info = backward(cfg, dP.row_view(a, b), dG.row_view(a, b), alpha, inplace=True)
        G = dP.to_host()
        assert G.data[lo:hi].tobytes() == back[lo:hi].tobytes(), first_difference(G.data[lo:hi], back[lo:hi])
        assert G.data[:lo].tobytes() == whole[:lo].tobytes() and G.data[hi:].tobytes() == whole[hi:].tobytes()
        assert vr.tobytes() == r[a:b].tobytes()


def on_torch(H, ro=None, col=None, nnz=None, shift=0):
    """H in torch tensors, as a dCSR that owns nothing: other offsets or column ids, a declared nnz; shift = 1 advances data
    and col_ids by one element, so neither lies on 16 bytes: the entry-by-entry path serves every tile"""
    pad = 8
    ro = H.row_offsets if ro is None else ro
    col = H.col_ids if col is None else col
    t_ro = torch.from_numpy(np.ascontiguousarray(ro).view(np.int32).copy()).to(DEV)
    va = np.concatenate([np.full(shift, 77, dtype=H.data.dtype), H.data, np.zeros(pad, dtype=H.data.dtype)])
    ci = np.concatenate([np.zeros(shift, dtype=np.uint32), np.asarray(col, dtype=np.uint32), np.zeros(pad, dtype=np.uint32)])
    t_va = torch.from_numpy(va).to(DEV)
    t_ci = torch.from_numpy(ci.view(np.int32)).to(DEV)
    return sa.dCSR.from_device(H.rows, H.cols, H.nnz if nnz is None else nnz, t_ro.data_ptr(), t_ci.data_ptr() + 4 * shift,
                               t_va.data_ptr() + H.data.itemsize * shift, dtype=H.data.dtype,
                               keep=(t_ro, t_va, t_ci), host_row_offsets=np.asarray(ro, dtype=np.uint32))


def values_of(dA, shift=0):
    return host(dA._keep[1])[shift:-8]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bits_do_not_depend_on_the_load_path(cfg, dtype):
    H = edge_matrix(dtype)
    wide, m, s, _ = forward(cfg, sa.dCSR.from_host(H), -2.0)
    for inplace in (True, False):
        dA = on_torch(H, shift=1)
        assert dA._c.data % 16 != 0
        got, vm, vs, _ = forward(cfg, dA, -2.0, inplace=inplace)
        assert got.tobytes() == wide.tobytes() and vm.tobytes() == m.tobytes() and vs.tobytes() == s.tobytes()
        assert host(dA._keep[1])[0] == 77
    # in place nobody reads col_ids: it may be NULL
    dA = on_torch(H)
    dA._c.col_ids = None
    sa.softmax(dA, cfg, alpha=-2.0, inplace=True)
    assert values_of(dA).tobytes() == wide.tobytes()


# ---------------------------------------------------------------------------------------------------- 5: accuracy
def bound(n, dtype):
    """per entry, relative: (n_i + 2 u_exp + 4) 2^-52 -- n_i - 1 additions on either side, u_exp ULPs of either exp, the
    products, the difference and the quotient; for float half an ulp of T on top and the smallest subnormal as a floor"""
    rel = (n + 2 * U_EXP + 4) * 2.0 ** -52
    return (rel + 2.0 ** -24, 2.0 ** -149) if dtype == np.float32 else (rel, 0.0)


@pytest.mark.parametrize("kind", ["uniform", "decades"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_accuracy(cfg, dtype, kind):
    H = edge_matrix(dtype, kind)
    n = np.diff(H.row_offsets.astype(np.int64))
    row = rows_of(H.row_offsets)
    for alpha in ALPHAS:
        got, _, _, _ = forward(cfg, sa.dCSR.from_host(H), alpha)
        want, _, _ = numpy_forward(H, alpha)
        rel, floor = bound(n[row], dtype)
        err = np.abs(got.astype(np.float64) - want)
        allowed = rel * np.abs(want) + floor
        print(f"softmax accuracy {np.dtype(dtype).name} {kind} alpha={alpha}: worst error / bound = {float((err / allowed).max()):.3f}")
        assert (err <= allowed).all(), (alpha, int((err > allowed).sum()), float((err / allowed).max()))
        sums = np.zeros(H.rows, dtype=np.longdouble)
        np.add.at(sums, row, got.astype(np.longdouble))
        rel, floor = bound(n, dtype)
        full = n > 0
        off = np.abs(sums - 1)[full].astype(np.float64) / (rel + n * floor)[full]
        print(f"softmax row sums {np.dtype(dtype).name} {kind} alpha={alpha}: worst |sum - 1| / bound = {float(off.max()):.3f}")
        assert (off <= 1).all(), (alpha, float(off.max()))


# ---------------------------------------------------------------------------------------------------- 6: special values
SPECIAL = ["-inf entries", "only -inf", "+inf", "nan", "overflow"]


@pytest.mark.parametrize("which", SPECIAL)
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_stay_in_their_row(cfg, dtype, which):
    lens = [5, 9, 0, 40, 7, 3]
    H = mk(lens, uniform(sum(lens), 21, dtype), seed=22)
    ro = H.row_offsets.astype(np.int64)
    alpha = 1.0
    clean, _, _, info = forward(cfg, sa.dCSR.from_host(H), alpha)
    assert info.nonfinite == 0
    v = H.data.copy()
    b, e = ro[3], ro[4]
    big = np.finfo(dtype).max
    if which == "-inf entries":
        v[b + 1] = v[b + 17] = v[e - 1] = -np.inf
    elif which == "only -inf":
        v[b:e] = -np.inf
    elif which == "+inf":
        v[b + 5] = np.inf
    elif which == "nan":
        v[b + 5] = np.nan
    else:
        v[b + 5], alpha = big, 2.0                                          # alpha a = +inf in double only for the doubles
        if dtype == np.float32:
            alpha = float(np.finfo(np.float64).max) / float(big) * 2.0
        clean, _, _, _ = forward(cfg, sa.dCSR.from_host(H), alpha)
    Hs = with_data(H, v)
    for inplace in (False, True):
        got, m, s, info = forward(cfg, sa.dCSR.from_host(Hs), alpha, inplace=inplace)
        assert got[:b].tobytes() == clean[:b].tobytes() and got[e:].tobytes() == clean[e:].tobytes()
        row = got[b:e]
        if which == "-inf entries":
            want = torch.softmax(torch.from_numpy(alpha * v[b:e].astype(np.float64)), 0).numpy()
            masked = np.isinf(v[b:e])
            assert (row[masked] == 0).all() and masked.sum() == 3 and np.isfinite(row).all()
            assert np.allclose(row[~masked], want[~masked], rtol=1e-6 if dtype == np.float32 else 1e-13, atol=0)
            assert info.nonfinite == 0
        else:
            assert np.isnan(row).all() and info.nonfinite == e - b
            with np.errstate(over="ignore"):
                scores = alpha * v[b:e].astype(np.float64)
            assert np.isnan(torch.softmax(torch.from_numpy(scores), 0).numpy()).all()
            assert np.isnan(s[3]) and (np.isnan(m[3]) if which == "nan" else m[3] == (-np.inf if which == "only -inf" else np.inf))
        assert np.isfinite(np.delete(s, 3)).all()
    # the backward hides nothing either: a NaN of G stays in its row
    HP = with_data(H, clean)
    g = gradient(H, 23)
    ok, _, _ = backward(cfg, sa.dCSR.from_host(HP), sa.dCSR.from_host(with_data(H, g)), 1.0)
    g[b + 2] = np.nan
    got, r, info = backward(cfg, sa.dCSR.from_host(HP), sa.dCSR.from_host(with_data(H, g)), 1.0)
    assert np.isnan(got[b:e]).all() and info.nonfinite == e - b and np.isnan(r[3])
    assert got[:b].tobytes() == ok[:b].tobytes() and got[e:].tobytes() == ok[e:].tobytes()


def test_an_overflow_on_the_rounding_to_float_is_counted(cfg):
    """EXP keeps e <= 1, the backward does not: alpha p (g - r) beyond float's range is inf after the rounding"""
    H = mk([4, 3], np.array([0.5, 0.25, 0.125, 0.125, 0.5, 0.25, 0.25], dtype=np.float32), seed=1)
    g = np.array([1, -1, 2, 0, 3, 1, -2], dtype=np.float32)
    want, _ = numpy_backward(cfg, H, g, 1e39)
    got, _, info = backward(cfg, sa.dCSR.from_host(H), sa.dCSR.from_host(with_data(H, g)), 1e39)
    assert same_bytes(got, want) and info.nonfinite == int(np.isinf(want).sum()) > 0


# ---------------------------------------------------------------------------------------------------- 7: hostile input
def hostile(H, which):
    """(offsets, column ids, declared nnz)"""
    ro, ci, nnz = H.row_offsets, H.col_ids, H.nnz
    if which == "descending at a tile edge":
        bad = ro.copy()
        assert bad[9] == 8 * T
        bad[9] = bad[10] + 1
        return bad, ci, nnz
    if which == "last offset short":
        return ro, ci, nnz + 1
    if which == "offset beyond":
        bad = ro.copy()
        bad[5] = nnz + 3
        return bad, ci, nnz
    bad = ci.copy()
    bad[2 * T - 1] = H.cols
    return ro, bad, nnz


HOSTILE = ["descending at a tile edge", "last offset short", "offset beyond", "id"]


@pytest.mark.parametrize("which", HOSTILE)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_input_is_refused_and_nothing_is_written(cfg, dtype, which):
    H = edge_matrix(dtype)
    ro, ci, nnz = hostile(H, which)
    lens = list(EDGES)
    lens[0], lens[-1] = lens[0] + 1, lens[-1] - 1
    other = mk(lens, uniform(H.nnz, 55, dtype), seed=56)           # C before the call: A's shape, so its buffers would be re-used
    g = torch.from_numpy(np.concatenate([gradient(H, 57), np.zeros(8, dtype=dtype)])).to(DEV)
    L = _lib.load()
    fn = L.speck_softmax_f32 if dtype == np.float32 else L.speck_softmax_f64
    for mode in (sa.SOFTMAX_NORMALIZED, sa.SOFTMAX_EXP, sa.SOFTMAX_BACKWARD):
        for new in (False, True):
            if which == "id" and not new:
                continue                                            # (in place nobody reads the ids)
            dA = on_torch(H, ro=ro, col=ci, nnz=nnz)
            dC = sa.dCSR.from_host(other)
            ptrs = (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            m, s = payload(H.rows), payload(H.rows)
            p = _lib.CSoftmaxParams()
            p.mode, p.alpha = mode, 0.5
            p.d_G = g.data_ptr() if mode == sa.SOFTMAX_BACKWARD else None
            p.d_row_max = m.data_ptr() if mode != sa.SOFTMAX_BACKWARD else None
            p.d_row_sum = s.data_ptr()
            info = _lib.CSoftmaxInfo(9, 9, 9, 9, 9)
            torch.cuda.synchronize()
            rc = fn(cfg._h, C_.byref(dA._c), C_.byref(p), C_.byref(dC._c) if new else None, C_.byref(info))
            torch.cuda.synchronize()
            assert rc == ERR_INVALID, (which, mode, new)
            assert as_tuple(info) == (0, 0, 0, 0, 0)
            assert values_of(dA).tobytes() == H.data.tobytes(), (which, mode, new)
            assert is_payload(host(m)) and is_payload(host(s)), (which, mode, new)
            assert ptrs == (dC._c.data, dC._c.col_ids, dC._c.row_offsets, dC.nnz, dC.rows)
            G = dC.to_host()
            assert G.data.tobytes() == other.data.tobytes() and G.col_ids.tobytes() == other.col_ids.tobytes() and \
                G.row_offsets.tobytes() == other.row_offsets.tobytes(), (which, mode, new)
    # the config serves a valid call right after
    got, _, _, _ = forward(cfg, sa.dCSR.from_host(H), 0.5)
    want, _, _ = numpy_forward(H, 0.5)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-30)


# ---------------------------------------------------------------------------------------------------- 8: housekeeping
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_without_rows_or_without_entries(cfg, dtype):
    none = sa.HostCSR(0, 7, np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=dtype))
    C, info = sa.softmax(sa.dCSR.from_host(none), cfg)
    assert (C.rows, C.cols, C.nnz) == (0, 7, 0) and as_tuple(info) == (0, 0, 0, 0, 0)
    _, info = sa.softmax(sa.dCSR.from_host(none), cfg, inplace=True)
    assert as_tuple(info) == (0, 0, 0, 0, 0)
    hollow = sa.HostCSR(5, 7, np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=dtype))
    got, m, s, info = forward(cfg, sa.dCSR.from_host(hollow))
    assert as_tuple(info) == (0, 0, 5, 0, 0) and (m == -np.inf).all() and (s == 0).all() and len(got) == 0
    dG = sa.dCSR.from_host(hollow)
    got, r, info = backward(cfg, sa.dCSR.from_host(hollow), dG)
    assert as_tuple(info) == (0, 0, 5, 0, 0) and (r == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_without_a_config(dtype):
    H = edge_matrix(dtype)
    cfg = sa.spECKConfig.initialize(0)
    try:
        want, m, s, _ = forward(cfg, sa.dCSR.from_host(H), 0.125)
    finally:
        cfg.cleanup()
    for inplace in (True, False):
        got, vm, vs, info = forward(None, sa.dCSR.from_host(H), 0.125, inplace=inplace)
        assert got.tobytes() == want.tobytes() and vm.tobytes() == m.tobytes() and vs.tobytes() == s.tobytes()
        assert as_tuple(info) == counts(H.row_offsets, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_canary_zone_is_touched(dtype):
    H = edge_matrix(dtype)
    ro = H.row_offsets.astype(np.int64)
    g = gradient(H, 31)
    cfg = sa.spECKConfig.initialize(0)
    try:
        want, _, _, _ = forward(cfg, sa.dCSR.from_host(H), 1.0)
        back, _ = numpy_backward(cfg, with_data(H, want), g, 1.0)
        cfg.set_option("guard_bytes", 4096)
        for inplace in (True, False):
            dA = sa.dCSR.from_host(H)                                      # (allocated with zones: A's are checked in place)
            got, _, _, _ = forward(cfg, dA, 1.0, inplace=inplace)          # (a touched zone is status 3)
            assert got.tobytes() == want.tobytes()
            dP, dG = sa.dCSR.from_host(with_data(H, want)), sa.dCSR.from_host(with_data(H, g))
            got, _, _ = backward(cfg, dP, dG, 1.0, inplace=inplace)
            assert same_bytes(got, back)
            assert ro[4] % 2 == 1                                           # a view with an odd base: the narrow form
            forward(cfg, sa.dCSR.from_host(H).row_view(4, H.rows), 1.0, inplace=inplace)
    finally:
        cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


def test_the_wrapper_checks_the_pattern_of_g_where_asked(cfg):
    H = probabilities(mk(SMALL, uniform(sum(SMALL), 3), seed=4), 41)
    g = gradient(H, 42)
    dP = sa.dCSR.from_host(H)
    same = sa.dCSR.from_host(with_data(H, g))
    got = sa.softmax_backward(dP, same, cfg, check_pattern=True)[0].to_host().data
    assert same_bytes(got, numpy_backward(cfg, H, g, 1.0)[0])
    ci = H.col_ids.copy()
    ci[3] = (ci[3] + 1) % H.cols
    moved = sa.dCSR.from_host(sa.HostCSR(H.rows, H.cols, H.row_offsets, ci, g))
    with pytest.raises(ValueError, match="softmax_backward: G does not have P's pattern"):
        sa.softmax_backward(dP, moved, cfg, check_pattern=True)
    assert dP.to_host().data.tobytes() == H.data.tobytes()


def test_the_caller_that_includes_softmax_h_only_runs(tmp_path):
    out = str(tmp_path / "caller_softmax")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "caller_softmax.cpp"),
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert subprocess.run([out], capture_output=True, text=True).stdout.strip() == "softmax caller ok"
