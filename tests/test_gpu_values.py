"""Values through every numeric class: special and extreme values, asserted bit for bit.

Every other module checks values against |c - c_ref| <= tol * sum|a*b| with O(1) inputs.  Here the inputs are built so
that every entry of C has exactly ONE right answer, whatever the summation order, and the GPU result must be that answer:

  * values are dyadic (+-k * 2^e, small k) with exponents in a window narrow enough that no f64 partial sum rounds;
  * the value contract ("Values"): each product is rounded to T, the products of an entry are summed in
    f64 (Acc<T> = double) and the sum is rounded to T once;
  * IEEE special values, all order-independent: a NaN product makes the entry NaN, +Inf and -Inf products in one entry
    make NaN, an Inf of one sign beside anything finite gives that Inf.

`exact_spgemm` is that reference in numpy (independent of oracle/speck_oracle.c; its own checks are in
test_values_reference.py).  The sign of a zero result is NOT asserted: NUM_DIRECT writes a*b (-0 for a negative a
times +0), the table classes start their sums from +0.  NaN is compared by position (isnan), not by payload.

One CARRIER per value-producing path: a fixed structure whose rows all fall into the named class -- asserted from
last_stats() as "the class holds every row of A" (no bare > 0) -- filled with the values of each FAMILY:
  exact      dyadic baseline
  round32    1 + k 2^-12: f32 products must round; only f32(sum_exact f32(a*b)) is right (not f32(sum a*b))
  overflow32 +1.5 2^127, +1.5 2^127, -1.5 2^127 into the column every B row shares: finite in the contract, Inf for a
             class that accumulates in f32
  special    NaN and +-Inf in A and B, 0 * Inf pairs, entries with both infinities, Inf beside finite products
  zeros      stored zeros in A and B, an all-zero row of A and of B: the entries stay in C, value 0
  subnormal  f64 products and sums in the subnormal range (exact); f32 products that are subnormal
  huge       positive products only: entries whose exact sum exceeds the largest finite T are +Inf, the rest exact
"""
import ctypes as C_
import functools

import numpy as np
import pytest

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po

gpu = pytest.mark.gpu

FAMILIES = ["exact", "round32", "overflow32", "special", "zeros", "subnormal", "huge"]
MODE_FAMILIES = ["exact", "round32", "special", "subnormal"]
DTYPES = [np.float64, np.float32]
_ODD = np.array([1.0, 3.0, 5.0, 7.0])


# ----------------------------------------------------------------------------------------------- the exact reference
def _expand(A, B):
    """Every product of A * B: (row of C, column of C, index into A.data, index into B.data)."""
    a_ro = A.row_offsets.astype(np.int64)
    b_ro = B.row_offsets.astype(np.int64)
    a_row = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(a_ro))
    k = A.col_ids[a_ro[0]:a_ro[-1]].astype(np.int64)
    lens = b_ro[k + 1] - b_ro[k]
    ia = np.repeat(np.arange(a_ro[0], a_ro[-1], dtype=np.int64), lens)
    start = np.repeat(b_ro[k] - (np.cumsum(lens) - lens), lens)
    ib = start + np.arange(int(lens.sum()), dtype=np.int64)
    return np.repeat(a_row, lens), B.col_ids[ib].astype(np.int64), ia, ib


def exact_spgemm(A, B):
    """C = A * B under the value contract, exact for inputs whose f64 sums never round (checked: the f64 sums must equal
    sums in extended precision wherever the latter are finite in f64).  Returns a po.HostCSR of A's value type; the
    structure is the symbolic one (stored zeros and cancellations keep their entries)."""
    T = A.data.dtype
    row, col, ia, ib = _expand(A, B)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (A.data[ia] * B.data[ib]).astype(T)      # the product, rounded to T (numpy: IEEE, no flush)
    p64 = prod.astype(np.float64)
    key = row * max(B.cols, 1) + col
    order = np.argsort(key, kind="stable")
    key, p64 = key[order], p64[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    starts = np.flatnonzero(first)
    nan = np.isnan(p64)
    pinf = p64 == np.inf
    ninf = p64 == -np.inf
    fin = np.where(nan | pinf | ninf, 0.0, p64)
    if starts.size:
        with np.errstate(over="ignore"):
            s64 = np.add.reduceat(fin, starts)
        sld = np.add.reduceat(fin.astype(np.longdouble), starts)
        has_nan = np.add.reduceat(nan.astype(np.int64), starts) > 0
        has_p = np.add.reduceat(pinf.astype(np.int64), starts) > 0
        has_n = np.add.reduceat(ninf.astype(np.int64), starts) > 0
    else:
        s64 = sld = np.zeros(0)
        has_nan = has_p = has_n = np.zeros(0, dtype=bool)
    in_range = np.abs(sld) <= np.longdouble(np.finfo(np.float64).max)
    assert (s64[in_range] == sld[in_range]).all(), "inputs outside the exact window: an f64 sum rounded"
    val = np.where(has_nan | (has_p & has_n), np.nan, np.where(has_p, np.inf, np.where(has_n, -np.inf, s64)))
    with np.errstate(over="ignore"):
        val = val.astype(T)                                # rounded to T once
    ukey = key[starts]
    crow = ukey // max(B.cols, 1)
    ro = np.zeros(A.rows + 1, dtype=np.int64)
    np.add.at(ro, crow + 1, 1)
    return po.HostCSR(A.rows, B.cols, np.cumsum(ro).astype(np.uint32), (ukey % max(B.cols, 1)).astype(np.uint32), val)


def assert_same_values(got, exp, what=""):
    """Structure bit-exact; values: NaN exactly where expected, every other value equal (== : bit-exact but for the sign
    of a zero)."""
    assert got.rows == exp.rows and got.cols == exp.cols and got.nnz == exp.nnz, f"{what}: shape / nnz differ"
    assert (got.row_offsets == exp.row_offsets).all(), f"{what}: row_offsets differ"
    assert (got.col_ids == exp.col_ids).all(), f"{what}: col_ids differ"
    assert got.data.dtype == exp.data.dtype
    gn, en = np.isnan(got.data), np.isnan(exp.data)
    bad = (gn != en) | (~en & (got.data != exp.data))
    if bad.any():
        i = np.flatnonzero(bad)
        row = np.searchsorted(exp.row_offsets.astype(np.int64), i, side="right") - 1
        show = ", ".join(f"C[{r},{c}] = {g!r} want {e!r}" for r, c, g, e in
                         zip(row[:5], exp.col_ids[i[:5]], got.data[i[:5]], exp.data[i[:5]]))
        pytest.fail(f"{what}: {i.size} of {exp.nnz} values differ: {show}")


# ----------------------------------------------------------------------------------------------- carriers (structure)
def _distinct_rows(rng, n_rows, k, pool):
    """n_rows sorted rows of k distinct draws from range(pool)."""
    if k * 4 >= pool:
        return np.sort(np.argsort(rng.random((n_rows, pool)), axis=1)[:, :k], axis=1)
    out = np.sort(rng.integers(0, pool, size=(n_rows, k)), axis=1)
    while True:
        dup = (out[:, 1:] == out[:, :-1]).any(axis=1)
        if not dup.any():
            return out
        out[dup] = np.sort(rng.integers(0, pool, size=(int(dup.sum()), k)), axis=1)


def _uniform(rows, len_a, kb, m, pool, cols, seed):
    """A: rows x kb, every row len_a entries; B: kb x cols, every row m entries -- column S (the smallest column of the
    pool) and m - 1 more from a pool of `pool` columns spread over [0, cols).  Every row of C has len_a * m products and
    one entry (at S) that takes len_a of them."""
    rng = np.random.default_rng(seed)
    colpool = np.sort(rng.choice(cols, size=pool, replace=False)).astype(np.int64)
    bsel = _distinct_rows(rng, kb, m - 1, pool - 1) + 1
    bcol = np.concatenate([np.full((kb, 1), colpool[0]), colpool[bsel]], axis=1)
    B = po.HostCSR(kb, cols, np.arange(kb + 1, dtype=np.uint32) * m, bcol.reshape(-1).astype(np.uint32), np.ones(kb * m))
    acol = _distinct_rows(rng, rows, len_a, kb)
    A = po.HostCSR(rows, kb, np.arange(rows + 1, dtype=np.uint32) * len_a, acol.reshape(-1).astype(np.uint32),
                   np.ones(rows * len_a))
    return A, B


# name: (rows, len_a, kb, m, pool, cols, seed), the numeric class every row takes in a complete call
CARRIERS = {
    "direct": ((3000, 1, 2000, 6, 5000, 1 << 20, 1), "direct"),          # one entry per row of A
    "g8": ((3000, 4, 2000, 6, 5000, 1 << 20, 2), "g8"),                  # 24 products from 4 entries
    "g16": ((2000, 12, 2000, 5, 5000, 1 << 20, 3), "g16"),               # 60 products from 12 entries
    "r32": ((2000, 20, 2000, 6, 5000, 1 << 20, 4), "r32"),               # 120 products from 20 entries
    "r64": ((1500, 40, 2000, 6, 5000, 1 << 20, 5), "r64"),               # 240 products from 40 entries
    "wave128": ((1500, 20, 2000, 16, 70, 1 << 20, 6), "wave128"),        # 320 products onto <= 70 columns
    "wave256": ((1500, 20, 2000, 16, 150, 1 << 20, 7), "wave256"),       # ... onto ~130 of 150
    "wave512": ((1000, 30, 2000, 20, 330, 1 << 20, 8), "wave512"),       # 600 onto ~270 of 330
    "block2k": ((400, 40, 3000, 30, 1200, 1 << 20, 9), "block2k"),       # 1200 onto ~740
    "block8k_half": ((160, 60, 4000, 60, 4000, 1 << 20, 10), "block8k"),    # ~2350 columns: the half-size table
    "block8k_full": ((160, 100, 4000, 80, 10000, 1 << 20, 11), "block8k"),  # ~5460 columns: the full table
    "dense4k": ((600, 30, 3000, 15, 4000, 4000, 12), "dense4k"),         # 450 products over 4000 columns
    "dense16k": ((24, 150, 3000, 150, 60000, 60000, 13), "dense16k"),    # ~18.7k columns over 60k: 4 windows
    "global": ((16, 150, 3000, 150, 200000, 1 << 20, 14), "global"),     # ~22k columns over 1 Mi: the spill
    "nfcopy": ((1000, 40, 2000, 20, 3000, 3000, 15), "nfcopy"),          # 800 products over 3000 columns
}
_HALF_MAX_NNZ = 4096 * 85 // 100    # kNumB8KHalfMaxNnz (device_common.hpp)


@functools.lru_cache(maxsize=None)
def carrier(name):
    return _uniform(*CARRIERS[name][0])


# ----------------------------------------------------------------------------------------------- value families
def _dyadic(rng, n, lo, hi):
    """+-k * 2^e, k odd in 1..7, e in [lo, hi]."""
    return rng.choice(_ODD, size=n) * np.exp2(rng.integers(lo, hi + 1, size=n)) * rng.choice([-1.0, 1.0], size=n)


def family_values(name, fam, dtype):
    """(A, B) of carrier `name` filled with the values of family `fam` in `dtype` (deterministic)."""
    A, B = carrier(name)
    rng = np.random.default_rng([FAMILIES.index(fam), sorted(CARRIERS).index(name)])
    na, nb = A.nnz, B.nnz
    f32 = dtype == np.float32
    a_first = np.zeros(na, dtype=bool)
    a_first[A.row_offsets[:-1].astype(np.int64)] = True
    a_last = np.zeros(na, dtype=bool)
    a_last[A.row_offsets[1:].astype(np.int64) - 1] = True
    b_shared = np.zeros(nb, dtype=bool)
    b_shared[B.row_offsets[:-1].astype(np.int64)] = True         # column S is every B row's first entry
    if fam == "exact":
        a, b = _dyadic(rng, na, -3, 3), _dyadic(rng, nb, -3, 3)
    elif fam == "round32":
        a = (1.0 + rng.integers(1, 256, size=na) * 2.0 ** -12) * rng.choice([-1.0, 1.0], size=na)
        b = (1.0 + rng.integers(1, 256, size=nb) * 2.0 ** -12) * rng.choice([-1.0, 1.0], size=nb)
    elif fam == "overflow32":
        # the first two entries of a row of A: +1.5 2^64, its last: -1.5 2^64; the rest +-k 2^40.  b at S: 2^63, else
        # +-k 2^[-3, 3].  At S: +X +X -X (X = 1.5 2^127 <= FLT_MAX < 2X) + sum +-k 2^103 -- finite, exact in f64
        a = rng.choice(_ODD, size=na) * 2.0 ** 40 * rng.choice([-1.0, 1.0], size=na)
        second = np.roll(a_first, 1) & ~a_first
        a[a_first | second] = 1.5 * 2.0 ** 64
        a[a_last & ~a_first] = -1.5 * 2.0 ** 64
        b = _dyadic(rng, nb, -3, 3)
        b[b_shared] = 2.0 ** 63
    elif fam == "special":
        a, b = _dyadic(rng, na, -3, 3), _dyadic(rng, nb, -3, 3)
        len_a = int(A.row_offsets[1] - A.row_offsets[0])
        p = min(0.05, 0.25 / len_a)
        specials = np.array([np.nan, np.inf, -np.inf, 0.0])
        ka = rng.random(na) < p
        a[ka] = rng.choice(specials, size=int(ka.sum()))
        kb_ = rng.random(nb) < p
        b[kb_] = rng.choice(specials[:3], size=int(kb_.sum()))
        # 0 * Inf pairs: a stored 0 of A against an Inf at S of the B row it points to; +Inf and -Inf into one entry
        ro = A.row_offsets.astype(np.int64)
        for r in range(0, A.rows, max(1, A.rows // 8)):
            e = ro[r]
            a[e] = 0.0
            b[B.row_offsets[A.col_ids[e]]] = np.inf
            if ro[r + 1] - ro[r] > 1:
                a[e + 1] = np.inf
                a[ro[r + 1] - 1] = -np.inf
    elif fam == "zeros":
        a, b = _dyadic(rng, na, -3, 3), _dyadic(rng, nb, -3, 3)
        a[rng.random(na) < 0.15] = 0.0
        b[rng.random(nb) < 0.15] = 0.0
        a[A.row_offsets[0]:A.row_offsets[1]] = 0.0                 # an all-zero row of A
        k = int(A.col_ids[A.row_offsets[1]])                       # ... and of B, referenced by row 1 of A
        b[B.row_offsets[k]:B.row_offsets[k + 1]] = 0.0
    elif fam == "subnormal":
        # products k k' 2^[-1066, -1060] (f64) / 2^[-146, -140] (f32): subnormal, on the grid, sums exact
        e = -70 if f32 else -530
        a, b = _dyadic(rng, na, e - 3, e), _dyadic(rng, nb, e - 3, e)
    elif fam == "huge":
        # positive products k k' 2^1018 (f64) / 2^121 (f32): an entry overflows iff sum k k' >= 64
        ea, eb = (61, 60) if f32 else (509, 509)
        a = rng.choice(_ODD, size=na) * 2.0 ** ea
        b = rng.choice(_ODD, size=nb) * 2.0 ** eb
    else:
        raise ValueError(fam)
    return (po.HostCSR(A.rows, A.cols, A.row_offsets, A.col_ids, a.astype(dtype)),
            po.HostCSR(B.rows, B.cols, B.row_offsets, B.col_ids, b.astype(dtype)))


@functools.lru_cache(maxsize=64)
def expected(name, fam, dtype):
    return exact_spgemm(*family_values(name, fam, dtype))


# ----------------------------------------------------------------------------------------------- running a carrier
def _to_sa(h):
    return sa.HostCSR(h.rows, h.cols, h.row_offsets, h.col_ids, h.data)


def _scribble(dC, dtype, cols=True):
    """junk over C between two calls (finite: a NaN the call failed to overwrite must not pass as an expected NaN)"""
    n = dC.nnz
    junk_c = np.full(n, 0xDEADBEEF, dtype=np.uint32) if cols else None
    junk_v = np.full(n, -1234.567, dtype=dtype)
    assert _lib.load().speck_dcsr_update(C_.byref(dC._c), None, None if junk_c is None else junk_c.ctypes.data,
                                         junk_v.ctypes.data, np.dtype(dtype).itemsize) == 0


def _assert_class(st, name, cls=None):
    """every row of A went through `cls` (default: the carrier's class)"""
    A, _ = carrier(name)
    cls = cls or CARRIERS[name][1]
    rows = st["num_bin_rows"]
    assert rows[cls] == A.rows, f"{name}: not every row of A is a {cls} row: {rows}"
    assert sum(rows.values()) == A.rows, f"{name}: rows outside {cls}: {rows}"


def _upload(name, fam, dtype):
    A, B = family_values(name, fam, dtype)
    return sa.dCSR.from_host(_to_sa(A)), sa.dCSR.from_host(_to_sa(B)), sa.dCSR(dtype)


@pytest.fixture(scope="module")
def vcfg():
    c = sa.spECKConfig.initialize(0)
    c.set_option("reuse", 0)        # every call a complete two-phase call: no replay of an earlier identical shape
    yield c
    c.cleanup()


@pytest.fixture
def fresh():
    made = []

    def make(**opts):
        c = sa.spECKConfig.initialize(0)
        for k, v in opts.items():
            c.set_option(k, v)
        made.append(c)
        return c
    yield make
    for c in made:
        c.cleanup()


def _ids(x):
    return x.__name__ if isinstance(x, type) else str(x)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(CARRIERS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_complete_call(vcfg, fam, name, dtype):
    dA, dB, dC = _upload(name, fam, dtype)
    sa.MultiplyspECK(dA, dB, dC, vcfg)
    st = vcfg.last_stats()
    assert not st["replayed"] and not st["eager_through"] and not st["one_walk"], st
    _assert_class(st, name)
    if name.startswith("block8k"):     # which of the two NUM_B8K launches: by the rows' nnz
        nnz = np.diff(expected(name, fam, dtype).row_offsets.astype(np.int64))
        assert (nnz <= _HALF_MAX_NNZ).all() if name == "block8k_half" else (nnz > _HALF_MAX_NNZ).all()
    assert_same_values(dC.to_host(), expected(name, fam, dtype), f"{name}/{fam}/{np.dtype(dtype).name}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(CARRIERS))
@pytest.mark.parametrize("fam", MODE_FAMILIES)
def test_through_call(fresh, fam, name, dtype):
    """reuse=0, eager_through: the second call of the same shapes into C's buffers is one batch"""
    cfg = fresh(reuse=0, eager_through=1)
    dA, dB, dC = _upload(name, fam, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    assert cfg.last_stats()["eager_through"] == 0
    _scribble(dC, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    assert st["eager_through"] == 1 and not st["replayed"], st
    _assert_class(st, name)
    assert_same_values(dC.to_host(), expected(name, fam, dtype), f"through {name}/{fam}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["g8", "g16", "r32", "r64"])
@pytest.mark.parametrize("fam", MODE_FAMILIES)
def test_replay_with_register_rows_fused(fresh, fam, name, dtype):
    """a replayed sequence finishes the register-class rows in its symbolic phase (esc_fused): they count as nfcopy"""
    cfg = fresh()
    dA, dB, dC = _upload(name, fam, dtype)
    for _ in range(3):
        sa.MultiplyspECK(dA, dB, dC, cfg)
    _scribble(dC, dtype, cols=False)       # (the column ids stay: the replay checks them against the fresh ones)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    assert st["replayed"] and st["esc_fused"], st
    _assert_class(st, name, "nfcopy")
    assert_same_values(dC.to_host(), expected(name, fam, dtype), f"fused {name}/{fam}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name,walk", [("g8", "one_walk"), ("g16", "one_walk"), ("r32", "one_walk"), ("r64", "one_walk"),
                                       ("wave128", "one_walk_hash"), ("wave256", "one_walk_hash")])
@pytest.mark.parametrize("fam", MODE_FAMILIES)
def test_walk_call(fresh, fam, name, walk, dtype):
    """one_walk (register classes) / one_walk_hash (rows of <= 170 entries): no symbolic pass, no scan"""
    cfg = fresh(reuse=0, **{walk: 2})
    dA, dB, dC = _upload(name, fam, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    assert cfg.last_stats()["one_walk"] == 0
    _scribble(dC, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    assert st["one_walk"] == (1 if walk == "one_walk" else 2) and st["walk_misses"] == 0, st
    # (a one_walk call reports the classes of the two-phase call; a one_walk_hash call counts every row under wave256:
    #  every row went through the walk kernel's 256-entry sub-wave body)
    _assert_class(st, name, "wave256" if walk == "one_walk_hash" else None)
    assert_same_values(dC.to_host(), expected(name, fam, dtype), f"{walk} {name}/{fam}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["block8k_half", "block8k_full"])
@pytest.mark.parametrize("fam", MODE_FAMILIES)
def test_sliced_rows(fresh, fam, name, dtype):
    """slice_rows: the NUM_B8K rows in column slices of the 2 Ki table"""
    cfg = fresh(reuse=0, slice_rows=1)
    dA, dB, dC = _upload(name, fam, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    _assert_class(cfg.last_stats(), name)
    assert_same_values(dC.to_host(), expected(name, fam, dtype), f"sliced {name}/{fam}")


# ----------------------------------------------------------------------------------------------- compare / transpose
def _special_matrix(dtype):
    """8 x 8, every row 4 entries: NaN, +-Inf, -0.0, a NaN with a payload, finite values"""
    rng = np.random.default_rng(3)
    col = np.sort(np.argsort(rng.random((8, 8)), axis=1)[:, :4], axis=1).reshape(-1)
    v = np.array([np.nan, np.inf, -np.inf, -0.0, 1.5, -2.25, 3.0, 0.0] * 4)
    v = v.astype(dtype)
    payload = np.array([0x7FF8DEADBEEF0001 if dtype == np.float64 else 0x7FC0BEEF], dtype=np.uint64 if dtype == np.float64
                       else np.uint32).view(dtype)
    v[9] = payload[0]
    return po.HostCSR(8, 8, np.arange(9, dtype=np.uint32) * 4, col.astype(np.uint32), v)


def _with_value(M, j, x):
    d = M.data.copy()
    d[j] = x
    return po.HostCSR(M.rows, M.cols, M.row_offsets, M.col_ids, d)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_compare_special_values(vcfg, dtype):
    """compare / compare_bounded: values match iff both NaN, or equal, or both finite and within the bound"""
    M = _special_matrix(dtype)
    dM, dM2 = sa.dCSR.from_host(_to_sa(M)), sa.dCSR.from_host(_to_sa(M))
    for tol in (1e-12, 0.5):
        assert sa.compare(dM, dM2, vcfg, compare_data=True, rel_tol=tol)
    fin = po.HostCSR(M.rows, M.cols, M.row_offsets, M.col_ids, np.ones(M.nnz))
    dS = sa.dCSR.from_host(_to_sa(fin))                          # sum |a*b| = 1 everywhere
    if dtype == np.float64:
        assert sa.compare_bounded(dM, dM2, dS, vcfg, tol=1e-12) == (0, 0)
    # one entry changed at a time: each pair is a mismatch of exactly one row, for any tolerance
    cases = [(1, np.finfo(dtype).max), (1, -np.inf), (2, np.inf), (2, 7.0), (0, 1.5), (4, np.nan), (4, np.inf), (3, np.nan)]
    for j, x in cases:
        X = sa.dCSR.from_host(_to_sa(_with_value(M, j, x)))
        for tol in (1e-12, 1e6):
            assert not sa.compare(dM, X, vcfg, compare_data=True, rel_tol=tol), (j, M.data[j], x, tol)
            assert not sa.compare(X, dM, vcfg, compare_data=True, rel_tol=tol), (j, x, M.data[j], tol)
            if dtype == np.float64:
                assert sa.compare_bounded(dM, X, dS, vcfg, tol=tol) == (0, 1), (j, M.data[j], x, tol)
                assert sa.compare_bounded(X, dM, dS, vcfg, tol=tol) == (0, 1), (j, x, M.data[j], tol)
    # -0.0 == +0.0, and another NaN payload is still NaN
    X = sa.dCSR.from_host(_to_sa(_with_value(_with_value(M, 3, 0.0), 0, M.data[9])))
    assert sa.compare(dM, X, vcfg, compare_data=True, rel_tol=1e-12)
    if dtype == np.float64:
        assert sa.compare_bounded(dM, X, dS, vcfg, tol=1e-12) == (0, 0)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_transpose_moves_values_bit_for_bit(vcfg, dtype):
    M = _special_matrix(dtype)
    rng = np.random.default_rng(8)
    big = carrier("r32")[1]                                       # 2000 x 1 Mi, 12 000 entries
    u = np.uint64 if dtype == np.float64 else np.uint32
    vals = rng.integers(0, np.iinfo(u).max, size=big.nnz, dtype=u, endpoint=True).view(dtype)   # any bit pattern
    for H in (M, po.HostCSR(big.rows, big.cols, big.row_offsets, big.col_ids, vals)):
        H64 = po.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, np.arange(H.nnz, dtype=np.float64))
        R = po.transpose(H64)                                     # where each entry goes: its position as the value
        T = sa.transpose(sa.dCSR.from_host(_to_sa(H)), vcfg).to_host()
        assert (T.row_offsets == R.row_offsets).all() and (T.col_ids == R.col_ids).all()
        assert (T.data.view(u) == H.data.view(u)[R.data.astype(np.int64)]).all()
