"""The exact value reference of test_gpu_values.py on the CPU: against Fraction brute force and the C oracle's f64 path
(its first check under NaN and Inf), and the value families against the slips they are meant to catch."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_values import CARRIERS, FAMILIES, exact_spgemm, expected, family_values

_SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0]


def _small_case(seed, dtype, specials):
    """rows x inner x cols with ~45 % density; dyadic values, subnormal ones among them, and the IEEE specials."""
    rng = np.random.default_rng(seed)
    r, k, c = rng.integers(1, 7, size=3)

    def mat(n, m):
        keep = rng.random((n, m)) < 0.45
        ro = np.zeros(n + 1, dtype=np.uint32)
        ro[1:] = np.cumsum(keep.sum(axis=1))
        ci = np.nonzero(keep)[1].astype(np.uint32)
        e = rng.integers(-4, 5, size=ci.size).astype(float)
        tiny = rng.random(ci.size) < 0.2                       # products in the subnormal range of T
        e[tiny] = -75 if dtype == np.float32 else -535
        v = rng.choice([1.0, 3.0, 5.0, 7.0], size=ci.size) * np.exp2(e) * rng.choice([-1.0, 1.0], size=ci.size)
        if specials:
            s = rng.random(ci.size) < 0.15
            v[s] = rng.choice(_SPECIALS, size=int(s.sum()))
        return po.HostCSR(n, m, ro, ci, v.astype(dtype))
    return mat(r, k), mat(k, c)


def _brute(A, B):
    """dense, entry by entry: products rounded to T, finite ones summed as Fractions, IEEE rules for the rest"""
    T = A.data.dtype
    out = {}
    for i in range(A.rows):
        for p in range(A.row_offsets[i], A.row_offsets[i + 1]):
            kk, a = int(A.col_ids[p]), A.data[p]
            for q in range(B.row_offsets[kk], B.row_offsets[kk + 1]):
                with np.errstate(invalid="ignore"):
                    prod = T.type(a * B.data[q])                  # (numpy scalar multiply in T: one rounding)
                out.setdefault((i, int(B.col_ids[q])), []).append(float(prod))
    res = {}
    for key, ps in out.items():
        if any(math.isnan(x) for x in ps) or (math.inf in ps and -math.inf in ps):
            res[key] = math.nan
        elif math.inf in ps or -math.inf in ps:
            res[key] = math.inf if math.inf in ps else -math.inf
        else:
            s = sum((Fraction(x) for x in ps), Fraction(0))
            res[key] = float(T.type(float(s)))                    # exact sums here are f64 numbers: one rounding to T
    return res


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("specials", [False, True], ids=["finite", "specials"])
def test_reference_matches_fraction_brute_force(dtype, specials):
    for seed in range(60):
        A, B = _small_case(seed, dtype, specials)
        R = exact_spgemm(A, B)
        want = _brute(A, B)
        got = {}
        for i in range(R.rows):
            for p in range(R.row_offsets[i], R.row_offsets[i + 1]):
                got[(i, int(R.col_ids[p]))] = float(R.data[p])
        assert got.keys() == want.keys(), seed
        for key, w in want.items():
            g = got[key]
            assert (math.isnan(g) and math.isnan(w)) or g == w, (seed, key, g, w)
        assert R.data.dtype == dtype


def _same(R, O):
    assert (R.row_offsets == O.row_offsets).all() and (R.col_ids == O.col_ids).all()
    rn, on = np.isnan(R.data), np.isnan(O.data)
    assert (rn == on).all(), f"NaN at {np.flatnonzero(rn != on)[:5]}"
    assert (R.data[~rn] == O.data[~rn]).all()


def test_reference_matches_the_oracle_f64_path_on_special_values():
    for seed in range(40):
        A, B = _small_case(100 + seed, np.float64, True)
        O, _ = po.spgemm(A, B)
        _same(exact_spgemm(A, B), O)
    for name in ("g16", "wave512", "dense4k", "nfcopy"):
        for fam in ("special", "zeros", "huge", "subnormal"):
            A, B = family_values(name, fam, np.float64)
            O, _ = po.spgemm(A, B)
            _same(expected(name, fam, np.float64), O)


def test_reference_keeps_the_symbolic_structure():
    """stored zeros and exact cancellations keep their entries: the pattern is that of the oracle's symbolic pass"""
    for name in CARRIERS:
        A, B = family_values(name, "zeros", np.float64)
        cnt, total = po.symbolic(A, B)
        R = expected(name, "zeros", np.float64)
        assert R.nnz == total and (np.diff(R.row_offsets.astype(np.int64)) == cnt[:A.rows]).all()


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_every_family_is_exact_in_every_carrier(fam, dtype):
    """exact_spgemm asserts its own premise (no f64 sum rounds) -- for every carrier and family"""
    for name in CARRIERS:
        assert expected(name, fam, dtype).data.dtype == dtype


def _per_entry(A, B):
    """the products sorted by entry of C (A-row order inside an entry): rounded to T, exact in f64; the entries' starts"""
    from test_gpu_values import _expand
    row, col, ia, ib = _expand(A, B)
    T = A.data.dtype
    key = row * B.cols + col
    order = np.argsort(key, kind="stable")
    prod = (A.data[ia] * B.data[ib]).astype(T)[order]
    exact64 = A.data[ia].astype(np.float64)[order] * B.data[ib].astype(np.float64)[order]
    key = key[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    return prod, exact64, starts


@pytest.mark.parametrize("name", [n for n in CARRIERS if n != "direct"])
def test_families_tell_the_contract_from_the_slips(name):
    """What each family is for, checked on the structure of every carrier (but NUM_DIRECT's, one product per entry):
    round32 -- f32 products formed in f64 give another f32 result in some entries; overflow32 -- f32 accumulation in
    the order of A overflows while the contract is finite; special -- NaN, +-Inf, finite entries, and a finite entry
    right behind a non-finite one in some row (a sum masked by multiplying with 0 turns it into NaN)."""
    A, B = family_values(name, "round32", np.float32)
    _, exact64, starts = _per_entry(A, B)
    slip = np.add.reduceat(exact64, starts).astype(np.float32)
    assert (slip != expected(name, "round32", np.float32).data).sum() > 0
    A, B = family_values(name, "overflow32", np.float32)
    prod, _, starts = _per_entry(A, B)
    with np.errstate(over="ignore", invalid="ignore"):
        f32acc = np.array([np.cumsum(seg, dtype=np.float32)[-1] for seg in np.split(prod, starts[1:])])
    want = expected(name, "overflow32", np.float32).data
    assert np.isfinite(want).all() and (~np.isfinite(f32acc)).sum() >= A.rows
    S = expected(name, "special", np.float64)
    d = S.data
    assert np.isnan(d).any() and (d == np.inf).any() and (d == -np.inf).any() and np.isfinite(d).sum() > d.size // 2
    same_row = np.ones(d.size, dtype=bool)
    same_row[S.row_offsets[1:-1].astype(np.int64)] = False
    assert (~np.isfinite(d[:-1]) & np.isfinite(d[1:]) & same_row[1:]).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_extreme_families_reach_their_ranges(dtype):
    fi = np.finfo(dtype)
    for name in CARRIERS:
        sub = expected(name, "subnormal", dtype).data
        nz = sub[sub != 0]
        assert nz.size > sub.size // 2 and (np.abs(nz) < fi.tiny).all(), name        # every nonzero result subnormal
        huge = expected(name, "huge", dtype).data
        assert (huge > 0).all() and (huge >= fi.max / 64).any(), name
        if name not in ("direct",):
            assert (huge == np.inf).any() and np.isfinite(huge).any(), name
        z = expected(name, "zeros", dtype)
        assert (z.data[z.row_offsets[0]:z.row_offsets[1]] == 0).all(), name            # the all-zero row of A
        assert (z.data == 0).sum() > z.row_offsets[1], name                              # ... and stored zeros elsewhere
