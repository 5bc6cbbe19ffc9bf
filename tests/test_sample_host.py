"""speck_sample_* without a GPU: the declarations, the exports, the ctypes mirrors and the Python info class, a C++ caller that
includes Sample.h only, the keys' anchors, the contract as numpy (numpy_sample: what tests/test_gpu_sample.py compares the
device with, byte for byte) against a brute-force count of smaller (key, t), the uniformity of the places the restatement
takes, the argument checks that come before anything touches a device, the Python wrapper's refusals, and the loud failure
where no device exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import speck_amd
from speck_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_DIM_LIMIT, ERR_NNZ_OVERFLOW = 0, 1, 2, 5
INFO_FIELDS = ["rows_out", "rows_empty", "rows_cut", "gross", "nnz_out", "max_row_entries"]
WITHOUT, WITH = 0, 1
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------------------------------- the contract
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def mix(z):
    """the SplitMix64 finaliser on an array of uint64 (numpy's unsigned arithmetic is modulo 2^64)"""
    z = np.array(z, dtype=np.uint64, ndmin=1)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def row_key(seed, g):
    return mix(np.uint64(seed) + np.uint64(GOLDEN) * (np.array(g, dtype=np.uint64, ndmin=1) + np.uint64(1)))


def key(seed, g, t):
    return mix(row_key(seed, g) + np.uint64(GOLDEN) * (np.array(t, dtype=np.uint64, ndmin=1) + np.uint64(1)))


def mulhi(a, b):
    """(a * b) >> 64 for uint64 a and b < 2^32"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    lo, hi = a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)
    return (hi * b + ((lo * b) >> np.uint64(32))) >> np.uint64(32)


def numpy_sample(ro, col, val, k, seed, rows=None, mode=WITHOUT, row_base=0):
    """The sample as the header states it: (row_offsets, col_ids, the values' bits, info, pos) -- pos the place of every entry
    of the result in A's buffers.  ro may be a view's absolute offsets; rows indexes the rows inside it.  Mode 0, per row:
    kept = np.sort(np.lexsort((t, key))[:k]) -- here for all rows at once, the row as the first sort key."""
    ro = np.asarray(ro, dtype=np.int64)
    idx = np.arange(len(ro) - 1, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    n = len(idx)
    glen = ro[idx + 1] - ro[idx]
    first = ro[idx]
    g = (np.uint64(row_base) + idx.astype(np.uint64))
    if mode == WITHOUT:
        k = min(int(k), 1 << 32)                          # (a row holds fewer than 2^32 entries: such a k cuts none)
        gross = int(glen.sum())
        G = np.concatenate([[0], np.cumsum(glen)])
        row = np.repeat(np.arange(n), glen)
        t = np.arange(gross, dtype=np.int64) - np.repeat(G[:-1], glen)
        keys = key(seed, g[row], t) if gross else np.zeros(0, dtype=np.uint64)
        order = np.lexsort((t, keys, row))
        rank = t                                          # (the sorted entries of a row take the row's places)
        kept = np.sort(order[rank < k])
        out_len = np.minimum(glen, k)
        pos = (first[row] + t)[kept]
    else:
        k = int(k)
        out_len = np.where(glen > 0, k, 0).astype(np.int64)
        total = int(out_len.sum())
        O = np.concatenate([[0], np.cumsum(out_len)])
        row = np.repeat(np.arange(n), out_len)
        u = np.arange(total, dtype=np.int64) - np.repeat(O[:-1], out_len)
        place = mulhi(key(seed, g[row], u), glen[row]) if total else np.zeros(0, dtype=np.uint64)
        pos = first[row] + place.astype(np.int64)
    new_ro = np.concatenate([[0], np.cumsum(out_len)]).astype(np.uint32)
    info = dict(rows_out=n, rows_empty=int((out_len == 0).sum()), rows_cut=int((glen > min(int(k), M64)).sum()), gross=int(glen.sum()),
                nnz_out=len(pos), max_row_entries=int(out_len.max()) if n else 0)
    return new_ro, np.asarray(col)[pos].astype(np.uint32), bits(np.asarray(val))[pos], info, pos


# plain Python integers: what the array arithmetic above must agree with
def py_mix(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def py_row_key(seed, g):
    return py_mix(seed + GOLDEN * (g + 1))


def py_key(seed, g, t):
    return py_mix(py_row_key(seed, g) + GOLDEN * (t + 1))


def brute_sample(ro, k, seed, rows, mode, row_base):
    """entry by entry: (positions in A's buffers, output lengths)"""
    pos, lens = [], []
    for i in rows:
        a, b = int(ro[i]), int(ro[i + 1])
        g, n = row_base + int(i), b - a
        if mode == WITHOUT:
            keys = [py_key(seed, g, t) for t in range(n)]
            kept = [t for t in range(n) if sum(1 for q in range(n) if (keys[q], q) < (keys[t], t)) < k]
        else:
            kept = [(py_key(seed, g, u) * n) >> 64 for u in range(k)] if n else []
        pos += [a + t for t in kept]
        lens.append(len(kept))
    return np.asarray(pos, dtype=np.int64), lens


def test_anchors():
    assert [py_mix(GOLDEN * (t + 1)) for t in range(4)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
    assert py_row_key(1, 0) == 0x910A2DEC89025CC1
    assert [py_key(1, 0, t) for t in range(3)] == [0x5E41AB087439611E, 0xF18D6CE93D6CF1EE, 0x0B95F66D327E8D78]
    assert [py_key(M64, 5, t) for t in range(2)] == [0x0159EA98CB5D2474, 0x83B7622CCCFC4EDD]
    # the array forms are the same functions
    assert mix(np.uint64(GOLDEN) * np.arange(1, 5, dtype=np.uint64)).tolist() == [py_mix(GOLDEN * (t + 1)) for t in range(4)]
    assert int(row_key(1, 0)[0]) == 0x910A2DEC89025CC1
    assert key(1, 0, np.arange(3)).tolist() == [0x5E41AB087439611E, 0xF18D6CE93D6CF1EE, 0x0B95F66D327E8D78]
    assert key(M64, 5, np.arange(2)).tolist() == [0x0159EA98CB5D2474, 0x83B7622CCCFC4EDD]
    assert key(7, [3, (1 << 62) + 9], [0, 1 << 31]).tolist() == [py_key(7, 3, 0), py_key(7, (1 << 62) + 9, 1 << 31)]
    for a, b in ((M64, 1), (M64, (1 << 32) - 1), (0x5E41AB087439611E, 300), (1 << 63, 5), (0, 17)):
        assert int(mulhi(np.uint64(a), b)) == (a * b) >> 64


@pytest.mark.parametrize("mode", [WITHOUT, WITH])
@pytest.mark.parametrize("vdtype", [np.float64, np.float32])
def test_numpy_statement_is_the_count_of_smaller_keys(vdtype, mode):
    rng = np.random.default_rng(3 + mode)
    lens = np.concatenate([np.arange(24), rng.integers(0, 24, size=30)])
    ro = np.concatenate([[5], 5 + np.cumsum(lens)])       # (a view: the offsets are absolute)
    n = int(ro[-1])
    val = rng.standard_normal(n).astype(vdtype)
    col = rng.integers(0, 50, size=n).astype(np.uint32)
    lists = [None, np.arange(len(lens))[::-1].copy(), rng.integers(0, len(lens), size=70), np.zeros(0, dtype=np.int64)]
    for k in (0, 1, 2, 5, 13, 23, 24) + ((1 << 40, M64) if mode == WITHOUT else (40,)):
        for rows in lists:
            for seed, row_base in ((0, 0), (2026, 1000), (M64, 1 << 62)):
                new_ro, ci, vb, info, pos = numpy_sample(ro, col, val, k, seed, rows, mode, row_base)
                named = range(len(lens)) if rows is None else rows
                want_pos, want_lens = brute_sample(ro, min(k, 1 << 20), seed, named, mode, row_base)
                assert np.array_equal(pos, want_pos), (k, seed)
                assert np.array_equal(ci, col[want_pos]) and np.array_equal(vb, bits(val)[want_pos])
                assert np.array_equal(np.diff(new_ro.astype(np.int64)), want_lens)
                glen = lens[np.asarray(list(named), dtype=np.int64)]
                assert info == dict(rows_out=len(glen), rows_empty=sum(x == 0 for x in want_lens), rows_cut=int((glen > k).sum()),
                                    gross=int(glen.sum()), nnz_out=len(want_pos), max_row_entries=max(want_lens, default=0))


def test_numpy_statement_by_hand():
    # seed 1, global row 0: key(1, 0, 0..2) = 5E41.., F18D.., 0B95..: the order of the places is 2, 0, 1
    ro = np.array([0, 3, 3, 4], dtype=np.uint32)
    col = np.array([7, 8, 9, 4], dtype=np.uint32)
    val = np.array([1.5, -0.0, np.nan, 2.0])
    got = numpy_sample(ro, col, val, 1, 1)
    assert got[0].tolist() == [0, 1, 1, 2] and got[1].tolist() == [9, 4] and got[4].tolist() == [2, 3]
    got = numpy_sample(ro, col, val, 2, 1)
    assert got[0].tolist() == [0, 2, 2, 3] and got[1].tolist() == [7, 9, 4]                 # places 0 and 2, in input order
    assert got[3] == dict(rows_out=3, rows_empty=1, rows_cut=1, gross=4, nnz_out=3, max_row_entries=2)
    assert np.array_equal(got[2], bits(val)[[0, 2, 3]])
    # with replacement: place (key * 3) >> 64 = 1, 2, 0 in draw order; a row of one entry gives k copies
    got = numpy_sample(ro, col, val, 3, 1, mode=WITH)
    assert got[0].tolist() == [0, 3, 3, 6] and got[1].tolist() == [8, 9, 7, 4, 4, 4]
    assert got[3] == dict(rows_out=3, rows_empty=1, rows_cut=0, gross=4, nnz_out=6, max_row_entries=3)
    # the view of rows 1 .. 2 with row_base = 1 gives the rows of the whole matrix's sample; the same row twice: the same sample
    whole = numpy_sample(ro, col, val, 1, 9)
    view = numpy_sample(ro[1:], col, val, 1, 9, row_base=1)
    assert np.array_equal(view[4], whole[4][whole[0][1]:])
    twice = numpy_sample(ro, col, val, 2, 9, rows=[0, 2, 0])
    assert np.array_equal(twice[4][:2], twice[4][3:])


# ---------------------------------------------------------------------------------------------------- uniformity
R = 20000
CAP = {4: 33.4, 16: 58.4, 63: 131.4, 299: 430.0}          # the 1 - 1e-6 quantile of chi-square with n - 1 degrees of freedom
SEEDS = (0, 1, 2026)


def _place_counts(n, k, seed, mode):
    """how often each place of a row is taken over the rows g = 0 .. R - 1 of n entries each: the rows are equally long, so
    the keys are a matrix and a row's sample is a sort along it (a stable one: of equal keys the smaller t) -- on the first
    200 rows the same places as numpy_sample's"""
    g = np.repeat(np.arange(R), min(n, k) if mode == WITHOUT else k)
    if mode == WITHOUT:
        keys = key(seed, np.repeat(np.arange(R), n), np.tile(np.arange(n), R)).reshape(R, n)
        places = np.sort(np.argsort(keys, axis=1, kind="stable")[:, :k], axis=1).ravel()
    else:
        places = mulhi(key(seed, g, np.tile(np.arange(k), R)), n).astype(np.int64)
    few = 200
    ro = np.arange(few + 1, dtype=np.int64) * n
    pos = numpy_sample(ro, np.zeros(few * n, dtype=np.uint32), np.zeros(few * n, dtype=np.float32), k, seed, None, mode)[4]
    assert np.array_equal(pos, (g * n + places)[:len(pos)]) and len(pos) == few * len(places) // R
    return np.bincount(places, minlength=n).astype(np.float64)


@pytest.mark.parametrize("n,k", [(5, 2), (17, 4), (64, 63), (300, 32)])
def test_places_without_replacement_are_uniform(n, k):
    e, p = R * k / n, k / n
    for seed in SEEDS:
        cnt = _place_counts(n, k, seed, WITHOUT)
        stat = ((cnt - e) ** 2).sum() / (e * (1 - p)) * (n - 1) / n
        print(f"without replacement n={n} k={k} seed={seed}: {stat:.1f} (cap {CAP[n - 1]})")
        assert stat <= CAP[n - 1], (seed, stat)


@pytest.mark.parametrize("n,k", [(5, 8), (17, 4), (300, 32)])
def test_places_with_replacement_are_uniform(n, k):
    e = R * k / n
    for seed in SEEDS:
        cnt = _place_counts(n, k, seed, WITH)
        stat = ((cnt - e) ** 2).sum() / e
        print(f"with replacement n={n} k={k} seed={seed}: {stat:.1f} (cap {CAP[n - 1]})")
        assert stat <= CAP[n - 1], (seed, stat)


# ---------------------------------------------------------------------------------------------------- declarations
def _header():
    return open(os.path.join(ROOT, "include", "speck_c_api.h")).read()


def _kinds(header, name):
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in proto.split(",")]


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"((?:const )?\w+)\s*(.*)$", decl, re.S).groups()
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_header_library_and_table_agree():
    header = _header()
    declared = set(re.findall(r"\b(speck_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    P = ctypes.POINTER
    for name in ("speck_sample_f64", "speck_sample_f32"):
        assert name in declared
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
        res, mirror = _lib._SIGS[name]
        assert res is ctypes.c_int and mirror == [ctypes.c_void_p, P(_lib.DCsr), P(_lib.CSampleParams), P(_lib.DCsr), P(_lib.CSampleInfo)]
        assert _kinds(header, name) == ["speck_config*", "constspeck_dcsr*", "constspeck_sample_params*", "speck_dcsr*", "speck_sample_info*"]


def test_structs_hold_exactly_the_listed_fields():
    header = _header()
    fields = _struct_fields(header, "speck_sample_info")
    assert [f for f, _ in fields] == [f[0] for f in _lib.CSampleInfo._fields_] == INFO_FIELDS
    assert all(ctype == "uint64_t" for _, ctype in fields) and all(m is ctypes.c_uint64 for _, m in _lib.CSampleInfo._fields_)
    assert ctypes.sizeof(_lib.CSampleInfo) == 8 * len(INFO_FIELDS)
    assert [getattr(_lib.CSampleInfo, f).offset for f in INFO_FIELDS] == [8 * i for i in range(len(INFO_FIELDS))]
    fields = _struct_fields(header, "speck_sample_params")
    want = [("k", "uint64_t"), ("seed", "uint64_t"), ("row_base", "uint64_t"), ("n_rows", "uint64_t"), ("*d_row_index", "const void"),
            ("index_bytes", "uint32_t"), ("mode", "uint32_t")]
    assert fields == want
    mirror = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "const void": ctypes.c_void_p}
    assert _lib.CSampleParams._fields_ == [(n.lstrip("*"), mirror[t]) for n, t in want]
    assert ctypes.sizeof(_lib.CSampleParams) == 48
    assert [getattr(_lib.CSampleParams, f.lstrip("*")).offset for f, _ in want] == [0, 8, 16, 24, 32, 40, 44]


def test_defines_are_the_python_constants_and_what_the_kernels_use():
    header = _header()
    assert int(re.search(r"#define SPECK_SAMPLE_GROUP_MAX (\d+)", header).group(1)) == speck_amd.SAMPLE_GROUP_MAX
    assert int(re.search(r"#define SPECK_SAMPLE_LDS_MAX (\d+)", header).group(1)) == speck_amd.SAMPLE_LDS_MAX
    assert int(re.search(r"#define SPECK_SAMPLE_TILE_ENTRIES (\d+)", header).group(1)) == speck_amd.SAMPLE_TILE_ENTRIES
    assert speck_amd.SAMPLE_GROUP_MAX % 8 == 0 and speck_amd.SAMPLE_GROUP_MAX < speck_amd.SAMPLE_LDS_MAX
    enum = re.search(r"enum \{ SPECK_SAMPLE_WITHOUT_REPLACEMENT = (\d), SPECK_SAMPLE_WITH_REPLACEMENT = (\d) \};", header).groups()
    assert tuple(int(x) for x in enum) == (speck_amd.SAMPLE_WITHOUT_REPLACEMENT, speck_amd.SAMPLE_WITH_REPLACEMENT) == (WITHOUT, WITH)
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "sample.hip")).read()
    assert "kGroupMax = SPECK_SAMPLE_GROUP_MAX, kLdsMax = SPECK_SAMPLE_LDS_MAX" in source and "kTile = SPECK_SAMPLE_TILE_ENTRIES" in source
    for constant in ("0x9E3779B97F4A7C15ull", "0xBF58476D1CE4E5B9ull", "0x94D049BB133111EBull", "__umul64hi"):
        assert constant in source, constant
    scratch = open(os.path.join(ROOT, "speck_amd", "csrc", "sample.hpp")).read()
    assert "group_max = SPECK_SAMPLE_GROUP_MAX" in scratch and "lds_max = SPECK_SAMPLE_LDS_MAX" in scratch
    options = open(os.path.join(ROOT, "speck_amd", "csrc", "pipeline.hip")).read()
    for name, define in (("sample_group_max", "SPECK_SAMPLE_GROUP_MAX"), ("sample_lds_max", "SPECK_SAMPLE_LDS_MAX")):
        assert re.search(r'n == "%s"\) c->sample\.\w+ = \(u32\)std::min<int64_t>\(std::max<int64_t>\(value, 0\), %s\);' % (name, define), options)
    assert options.count("c->sample.release();") == 2 and "SampleScratch* sample_scratch(speck_config* c) { return &c->sample; }" in options


def test_the_header_states_the_contract_and_names_what_is_not_built():
    block = re.search(r"/\* ---- fan-out neighbour sampling.*?---- \*/", _header(), re.S).group(0)
    flat = re.sub(r"\n\s*\*\s+", " ", block)
    not_built = flat[flat.index("Not built:"):]
    for what in ("weighted sampling", "a per-row k", "several hops in one call", "sampling by column", "an O(k) draw for hub rows"):
        assert what in not_built, what
    for what in ("GOLDEN = 0x9E3779B97F4A7C15", "z *= 0xBF58476D1CE4E5B9", "z *= 0x94D049BB133111EB", "np.sort(np.lexsort((t, key))[:k])",
                 "(key(seed, g, u) * len) >> 64", "below len / 2^64", "Integer arithmetic and integer atomics only"):
        assert what in flat, what
    # "uniform sampling" joins nobody else's list of what is not built
    others = _header().replace(block, "")
    assert "uniform sampling" not in others and "neighbour sampling" not in others


def test_info_class_and_exports():
    values = dict(zip(INFO_FIELDS, range(1, 7)))
    c = _lib.CSampleInfo()
    for field, v in values.items():
        setattr(c, field, v)
    cls = speck_amd.SampleInfo
    assert cls is speck_amd.api.SampleInfo and cls.__name__ == "SampleInfo" and issubclass(cls, speck_amd.api._Info)
    info = cls(c)
    assert vars(info) == values and all(type(getattr(info, f)) is int for f in values)
    assert repr(info) == "SampleInfo(rows_out=1, rows_empty=2, rows_cut=3, gross=4, nnz_out=5, max_row_entries=6)"
    assert speck_amd.sample_neighbors is speck_amd.api.sample_neighbors
    assert (speck_amd.SAMPLE_GROUP_MAX, speck_amd.SAMPLE_LDS_MAX, speck_amd.SAMPLE_TILE_ENTRIES) == (256, 4096, 4096)


def test_caller_that_includes_sample_h_only_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "caller_sample.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["Sample.h"]
    out = str(tmp_path / "caller_sample")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-L", os.path.join(ROOT, "speck_amd"), "-lspeck_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "speck_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    assert os.path.exists(out)


def test_the_callers_expectation_is_the_numpy_statement():
    # tests/cpp/caller_sample.cpp: the 3 x 4 matrix, seed 1
    ro = np.array([0, 4, 5, 8])
    col = np.array([0, 1, 2, 3, 2, 0, 1, 3], dtype=np.uint32)
    val = np.array([1, -5, 3, 3, 7, -2, -1, -9], dtype=np.float64)
    source = open(os.path.join(ROOT, "tests", "cpp", "caller_sample.cpp")).read()

    def listed(name):
        return [int(x) for x in re.search(r"%s\[\d+\] = \{([^}]*)\}" % name, source).group(1).split(",")]
    got = numpy_sample(ro, col, val, 2, 1)
    assert listed("want_ro") == got[0].tolist() and listed("want_ci") == got[1].tolist() and listed("want_v") == val[got[4]].tolist()
    got = numpy_sample(ro, col, val, 2, 1, rows=[2, 0], mode=WITH)
    assert listed("draw_ro") == got[0].tolist() and listed("draw_ci") == got[1].tolist() and listed("draw_v") == val[got[4]].tolist()


def test_atomics_run_on_integer_counts_only():
    source = open(os.path.join(ROOT, "speck_amd", "csrc", "sample.hip")).read()
    code = re.sub(r"//[^\n]*", "", source)
    targets = re.findall(r"atomic\w+\(\s*&?\s*([^,]+),", code)
    # (the four sums go through row_tiles.hpp -- wave_counter_to_lds, lds_counter_to_status)
    assert targets and set(targets) <= {"st->max_row", "st->cnt[c]", "s_hist[d0]", "s_hist[digit]"}, targets
    status = re.search(r"struct SampleStatus \{(.*?)\};", code, re.S).group(1)
    assert "float" not in status and "double" not in status
    # no floating-point arithmetic: values are copied, the keys are unsigned integers
    assert not re.search(r"\bfabs|\bisnan|\bfmax|\bfmin|\blog\(|\bpow\(|\brand", code)


# ---------------------------------------------------------------------------------------------------- argument checks
def _mat(rows, cols, nnz, buf):
    m = _lib.DCsr()
    m.rows, m.cols, m.nnz = rows, cols, nnz
    m.data = m.col_ids = m.row_offsets = buf
    return m


def _a(rows, cols, nnz, pa):
    A = _mat(rows, cols, nnz, pa)
    A.row_offsets, A.col_ids, A.data = pa, pa + 1024, pa + 2048
    return A


def _params(k, n_rows, index=None, index_bytes=8, mode=WITHOUT, seed=3, row_base=0):
    p = _lib.CSampleParams()
    p.k, p.seed, p.row_base, p.n_rows, p.d_row_index, p.index_bytes, p.mode = k, seed, row_base, n_rows, index, index_bytes, mode
    return p


def _no_device_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fake pointers would be followed")
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.spECKConfig.initialize(0)
    return e.value.status


def test_sample_checks_its_arguments_before_anything_runs():
    L = _lib.load()
    ka, kc, ki = (np.zeros(1024, dtype=np.uint64) for _ in range(3))
    pa, pc, pi = ka.ctypes.data, kc.ctypes.data, ki.ctypes.data
    ref = ctypes.byref
    for fn, vsize in ((L.speck_sample_f64, 8), (L.speck_sample_f32, 4)):
        def call(A, p, out=True, C=None):
            C = _mat(9, 9, 9, pc) if C is None else C
            before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
            info = _lib.CSampleInfo(*([7] * 6))
            rc = fn(None, ref(A) if A is not None else None, ref(p) if p is not None else None, ref(C) if out else None, ref(info))
            assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before       # the struct keeps its sentinel
            assert [getattr(info, f) for f in INFO_FIELDS] == [7] * 6                        # ... and so does *info
            return rc

        A = _a(4, 6, 3, pa)
        good = _params(2, 4)
        assert call(None, good) == ERR_INVALID                                      # NULL A
        assert call(A, None) == ERR_INVALID                                         # NULL params
        assert call(A, good, out=False) == ERR_INVALID                              # NULL C
        for mode in (2, 3, 0xFFFFFFFF):
            assert call(A, _params(2, 4, mode=mode)) == ERR_INVALID
        for width in (0, 2, 16, 0xFFFFFFFF):
            assert call(A, _params(2, 4, index_bytes=width)) == ERR_INVALID
            assert call(A, _params(2, 5, index=pi, index_bytes=width)) == ERR_INVALID
        assert call(A, _params(2, 4, row_base=(1 << 62) + 1)) == ERR_INVALID
        assert call(A, _params(2, 4, row_base=M64)) == ERR_INVALID
        big = (1 << 27) + 1
        assert call(_a(big, 6, 3, pa), _params(2, big)) == ERR_DIM_LIMIT
        assert call(_a(4, big, 3, pa), good) == ERR_DIM_LIMIT
        assert call(A, _params(2, big, index=pi)) == ERR_DIM_LIMIT
        assert call(_a(big, 6, 3, pa), _params(2, big, mode=2)) == ERR_INVALID      # the mode is asked first
        assert call(_a(4, 6, 1 << 32, pa), good) == ERR_NNZ_OVERFLOW
        assert call(_a(4, 6, 1 << 40, pa), _params(0, 4, mode=WITH)) == ERR_NNZ_OVERFLOW
        for field in ("row_offsets", "col_ids", "data"):                            # NULL buffers with a count
            hollow = _a(4, 6, 3, pa)
            setattr(hollow, field, None)
            assert call(hollow, good) == ERR_INVALID, field
        assert call(_a(0, 6, 3, pa), _params(2, 0)) == ERR_INVALID                  # entries, but no row
        assert call(_a(4, 0, 3, pa), good) == ERR_INVALID                           # entries, but no column
        for n_rows in (0, 3, 5):                                                    # a NULL index names every row
            assert call(A, _params(2, n_rows)) == ERR_INVALID
        for field in ("row_offsets", "col_ids", "data"):                            # C sharing a buffer with A
            C = _mat(9, 9, 9, pc)
            setattr(C, field, getattr(A, field))
            assert call(A, good, C=C) == ERR_INVALID, field
        # the index inside a buffer of A or of C (spans: the last byte of one, the first of the other)
        for width in (4, 8):
            for at in (pa + 16, pa + 19, pa + 1024 + 8, pa + 1024 - 2 * width + 1, pa + 2048 + 3 * vsize - 1,
                       pc + 39, pc - 2 * width + 1, pc + 9 * vsize - 1):
                assert call(A, _params(2, 2, index=at, index_bytes=width)) == ERR_INVALID, (width, at - pa)
    assert not ka.any() and not kc.any() and not ki.any()


def test_without_a_gpu_it_fails_loudly():
    no_device = _no_device_status()
    L = _lib.load()
    ka, kc, ki = (np.zeros(1024, dtype=np.uint64) for _ in range(3))
    pa, pi = ka.ctypes.data, ki.ctypes.data
    for fn in (L.speck_sample_f64, L.speck_sample_f32):
        for A, p in ((_a(4, 6, 3, pa), _params(2, 4)), (_a(4, 6, 3, pa), _params(0, 9, index=pi, index_bytes=4, mode=WITH)),
                     (_mat(0, 0, 0, None), _params(1 << 40, 0)), (_a(4, 6, 0, pa), _params(1, 0, index=pi, row_base=1 << 62)),
                     (_a(4, 6, 3, pa), _params(2, 2, index=pa + 20))):              # (the index just behind A's offsets)
            for C in (_lib.DCsr(), _mat(9, 9, 9, kc.ctypes.data)):
                before = (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets)
                info = _lib.CSampleInfo(*([7] * 6))
                assert fn(None, ctypes.byref(A), ctypes.byref(p), ctypes.byref(C), ctypes.byref(info)) == no_device
                assert (C.rows, C.cols, C.nnz, C.data, C.col_ids, C.row_offsets) == before
                assert [getattr(info, f) for f in INFO_FIELDS] == [0] * 6           # the arguments have passed: *info is zero
    dA = speck_amd.dCSR.from_device(4, 6, 3, pa, pa + 1024, pa + 2048)
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.sample_neighbors(dA, 2, 7)
    assert e.value.status == no_device
    with pytest.raises(speck_amd.SpeckError) as e:
        speck_amd.sample_neighbors(dA, 2, 7, replace=True, row_base=5)
    assert e.value.status == no_device
    assert not ka.any() and not kc.any() and not ki.any()


class _FakeTensor:
    """what the wrappers ask of an index tensor; its address is never taken where the call is refused"""

    def __init__(self, n, dtype="torch.int64", shape=None, stride=1):
        self.shape, self.dtype, self._stride = (n,) if shape is None else shape, dtype, stride

    def stride(self, d=0):
        return self._stride

    def data_ptr(self):
        raise AssertionError("the address was asked for before the arguments had passed")


def test_python_refuses_wrong_arguments_before_the_library_is_asked():
    A = speck_amd.dCSR.from_device(4, 6, 3, 4096, 8192, 12288)
    for k in (-1, 1.5, "3", None, True, 1 << 64):
        with pytest.raises(ValueError, match="sample_neighbors: k must be an integer"):
            speck_amd.sample_neighbors(A, k, 0)
    for seed in (-1, 0.5, None, False, 1 << 64):
        with pytest.raises(ValueError, match="sample_neighbors: seed must be an integer"):
            speck_amd.sample_neighbors(A, 2, seed)
    for row_base in (-1, 2.0, None, True, (1 << 62) + 1):
        with pytest.raises(ValueError, match="sample_neighbors: row_base must be an integer"):
            speck_amd.sample_neighbors(A, 2, 0, row_base=row_base)
    for replace in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="sample_neighbors: replace must be True or False"):
            speck_amd.sample_neighbors(A, 2, 0, replace=replace)
    with pytest.raises(ValueError, match="sample_neighbors: rows must be int64 or int32"):
        speck_amd.sample_neighbors(A, 2, 0, rows=_FakeTensor(3, "torch.float32"))
    with pytest.raises(ValueError, match="sample_neighbors: rows must have one dimension"):
        speck_amd.sample_neighbors(A, 2, 0, rows=_FakeTensor(3, shape=(3, 1)))
    with pytest.raises(ValueError, match="sample_neighbors: rows must be contiguous"):
        speck_amd.sample_neighbors(A, 2, 0, rows=_FakeTensor(3, stride=2))
    with pytest.raises(ValueError, match="sample_neighbors: rows is an address"):
        speck_amd.sample_neighbors(A, 2, 0, rows=123456)
    with pytest.raises(ValueError, match="beyond the limit"):
        speck_amd.sample_neighbors(A, 2, 0, rows=_FakeTensor((1 << 27) + 1))
