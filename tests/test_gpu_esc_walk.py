"""The class-list walks of the register classes (G8 / G16 / R32 / R64, both phases of a complete call): a lane group that
walks several rows holds the NEXT row's entries of A while it works on the current one (esc_rows.hpp, num_esc_body).

What that could get wrong is a read for a row that is not there, or past a row's end; which group takes which row moves
with option esc_walk_rows (R rows per group once the chip is full).  The chip is never full of a test's rows, so the tests
declare it full at ONE workgroup (debug option esc_walk_resident = 1): a class' range is then ceil(workgroups / R).

Inputs are dyadic (exact_spgemm is THE answer, bit for bit) and built row by row from the shapes the edge table of
test_edges_host.py shows to land in each class: full rows (L entries, 4 L products), rows shorter than the group (lanes that
must not prefetch), rows whose entries point at empty rows of B.  The last row of A is a full row of the class: its
entries -- prefetched by the group that worked on its predecessor -- end exactly at nnz(A).

List lengths per class of L lanes (G = 256 / L rows per workgroup) and R: 1, G - 1, G, G + 1, R G - 1, R G, R G + 1 (groups
with R rows, with R - 1, with none), and 16 R G + G + 1 (17 workgroups: the XCD-aware slices, taken with a stride).  Every
case runs in fp64 and fp32 as a complete call (class counts checked against the generator), a through call and a reuse
sequence; the longer ones also with A as a row-range view (absolute offsets: b_sl is rebased).  Then all four classes mixed.
test_walks_under_canary_zones runs the file once more in a child process whose device buffers carry canary zones.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import speck_amd as sa
from oracle import pyoracle as po
from test_edges_host import NUM_NAMES, SYM_NAMES, R, W, _b_rows, as_dtype
from test_gpu_values import _dyadic, _scribble, _to_sa, assert_same_values, exact_spgemm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LANES = {"g8": 8, "g16": 16, "r32": 32, "r64": 64}
# (len_a, products, nnz) of rows of each class (test_edges_host.py, "register" probes): the first is the full row
SHAPES = {
    "g8": [(8, 32, 32), (2, 4, 4), (8, 3, 3), (5, 16, 16)],
    "g16": [(16, 64, 64), (9, 18, 18), (9, 3, 3), (8, 33, 33)],
    "r32": [(32, 128, 128), (17, 34, 34), (17, 5, 5), (16, 65, 65)],
    "r64": [(64, 256, 256), (33, 66, 66), (33, 7, 7), (32, 129, 129), (64, 9, 9)],
}
WALK_ROWS = [1, 2, 3, 7]
# options that are not the config's own: back to their defaults (symbolic.hip) after a test
PROCESS_WIDE = {"esc_walk_rows": 4, "esc_walk_resident": 0}
ZONES = bool(os.environ.get("SPECK_GUARD_BYTES"))


def _rows_of(cls, n):
    """n rows of class `cls`: the shapes in turn, the last one full"""
    s = SHAPES[cls]
    return [R(1, *s[0 if i == n - 1 else i % len(s)], W, cls, cls) for i in range(n)]


@functools.lru_cache(maxsize=None)
def build(classes, counts, seed, shuffle=False):
    """(A, B, {class: rows}) of counts[k] rows of classes[k]; every row of A owns its rows of B; the last row of A is a
    full row of the last class whatever the order of the others"""
    rng = np.random.default_rng([seed, 77])
    specs = [r for cls, n in zip(classes, counts) for r in _rows_of(cls, n)]
    if shuffle:
        order = rng.permutation(len(specs) - 1)
        specs = [specs[i] for i in order] + specs[-1:]
    b_len, b_col, a_cols, next_b = [], [], [], 0
    for r in specs:
        lengths, col = _b_rows(rng, r)
        b_len.append(lengths)
        b_col.append(col)
        a_cols.append(np.arange(next_b, next_b + r.len_a, dtype=np.int64))
        next_b += r.len_a
    b_len, b_col = np.concatenate(b_len), np.concatenate(b_col)
    a_ro = np.concatenate([[0], np.cumsum([c.size for c in a_cols])]).astype(np.uint32)
    a_ci = np.concatenate(a_cols).astype(np.uint32)
    A = po.HostCSR(len(specs), next_b, a_ro, a_ci, _dyadic(rng, a_ci.size, -3, 3))
    B = po.HostCSR(next_b, W + 9, np.concatenate([[0], np.cumsum(b_len)]).astype(np.uint32), b_col.astype(np.uint32),
                   _dyadic(rng, b_col.size, -3, 3))
    assert specs[-1].len_a == LANES[classes[-1]] and int(a_ro[-1]) == A.nnz
    return A, B, dict(zip(classes, counts))


def _rows(M, r0, r1):
    """rows [r0, r1) of M as a matrix of its own"""
    ro = M.row_offsets.astype(np.int64)
    return po.HostCSR(r1 - r0, M.cols, (ro[r0:r1 + 1] - ro[r0]).astype(np.uint32), M.col_ids[ro[r0]:ro[r1]], M.data[ro[r0]:ro[r1]])


@pytest.fixture
def configs():
    """complete / through / reuse configs with the walk forced to R rows per group; a config serves every case of a test"""
    made = []

    def make(walk_rows):
        kinds = dict(complete=dict(reuse=0), through=dict(reuse=0, eager_through=1), reuse={})
        out = {}
        for kind, opts in kinds.items():
            c = sa.spECKConfig.initialize(0)
            made.append(c)
            for k, v in dict(opts, esc_walk_rows=walk_rows, esc_walk_resident=1).items():
                c.set_option(k, v)
            out[kind] = c
        return out
    yield make
    for c in made:
        for k, v in PROCESS_WIDE.items():
            c.set_option(k, v)
        c.cleanup()


def _run_case(cfgs, A, B, per_class, what, view=False):
    for dtype in (np.float64, np.float32):
        At, Bt = as_dtype(A, dtype), as_dtype(B, dtype)
        exp = exact_spgemm(At, Bt)
        dA, dB = sa.dCSR.from_host(_to_sa(At)), sa.dCSR.from_host(_to_sa(Bt))
        tag = f"{what}/{np.dtype(dtype).name}"
        # ---- a complete call: values, and every row in the class the generator gave it
        dC = sa.dCSR(dtype)
        sa.MultiplyspECK(dA, dB, dC, cfgs["complete"])
        st = cfgs["complete"].last_stats()
        assert not st["replayed"] and not st["eager_through"] and not st["one_walk"], st
        assert_same_values(dC.to_host(), exp, f"complete {tag}")
        sym, num = dict.fromkeys(SYM_NAMES, 0), dict.fromkeys(NUM_NAMES, 0)
        sym.update(per_class)
        num.update(per_class)
        assert st["sym_bin_rows"] == sym, (tag, "symbolic classes", st["sym_bin_rows"], sym)
        assert st["num_bin_rows"] == num, (tag, "numeric classes", st["num_bin_rows"], num)
        # ---- a through call: the same call again on one config, reuse = 0
        dC = sa.dCSR(dtype)
        sa.MultiplyspECK(dA, dB, dC, cfgs["through"])
        _scribble(dC, dtype)
        sa.MultiplyspECK(dA, dB, dC, cfgs["through"])
        st = cfgs["through"].last_stats()
        # (with canary zones the batch was seen to fall back behind its front -- the scan objects, the call goes on as a
        #  two-phase one, eager_through = -1 -- in one case of the file: there the call must have been attempted, no more)
        assert st["eager_through"] in ((1, -1) if ZONES else (1,)) and not st["replayed"], st
        assert_same_values(dC.to_host(), exp, f"through {tag}")
        # ---- a reuse sequence: the last call replayed (its register-class rows finished by the one-row form)
        dC = sa.dCSR(dtype)
        for _ in range(3):
            sa.MultiplyspECK(dA, dB, dC, cfgs["reuse"])
        _scribble(dC, dtype, cols=False)       # (the column ids stay: the replay checks them against the fresh ones)
        sa.MultiplyspECK(dA, dB, dC, cfgs["reuse"])
        st = cfgs["reuse"].last_stats()
        assert st["replayed"], st
        assert_same_values(dC.to_host(), exp, f"reuse {tag}")
        # ---- A as a row-range view that ends with the last row of A: absolute offsets, b_sl rebased
        if view:
            r0 = 3
            dC = sa.dCSR(dtype)
            sa.MultiplyspECK(dA.row_view(r0, A.rows), dB, dC, cfgs["complete"])
            assert not cfgs["complete"].last_stats()["replayed"]
            assert_same_values(dC.to_host(), exact_spgemm(_rows(At, r0, A.rows), Bt), f"view {tag}")


def _lengths(cls, walk_rows):
    g = 256 // LANES[cls]
    return sorted({1, g - 1, g, g + 1, walk_rows * g - 1, walk_rows * g, walk_rows * g + 1})


@pytest.mark.parametrize("walk_rows", WALK_ROWS)
@pytest.mark.parametrize("cls", list(LANES))
def test_one_class_list_edges(configs, cls, walk_rows):
    """lists of 1 row, of one workgroup -1 / 0 / +1, of R workgroups -1 / 0 / +1: groups with R rows, R - 1, none"""
    cfgs = configs(walk_rows)
    g = 256 // LANES[cls]
    for n in _lengths(cls, walk_rows):
        A, B, per_class = build((cls,), (n,), 1)
        _run_case(cfgs, A, B, per_class, f"{cls} R={walk_rows} n={n}", view=n > g + 3)


@pytest.mark.parametrize("walk_rows", WALK_ROWS)
@pytest.mark.parametrize("cls", list(LANES))
def test_one_class_seventeen_workgroups(configs, cls, walk_rows):
    """17 workgroups of the class (>= 16: the XCD-aware slices, eight contiguous parts walked with a stride), the last rows
    of every part short of a full round"""
    g = 256 // LANES[cls]
    n = 16 * walk_rows * g + g + 1
    A, B, per_class = build((cls,), (n,), 2)
    _run_case(configs(walk_rows), A, B, per_class, f"{cls} R={walk_rows} n={n}", view=True)


@pytest.mark.parametrize("walk_rows", WALK_ROWS)
def test_all_four_classes_mixed(configs, walk_rows):
    """the four classes in one call, shuffled over the rows of A: R workgroups + 1 row of each"""
    classes = tuple(LANES)
    counts = tuple(walk_rows * (256 // LANES[c]) + 1 for c in classes)
    A, B, per_class = build(classes, counts, 3, shuffle=True)
    _run_case(configs(walk_rows), A, B, per_class, f"mixed R={walk_rows}", view=True)


def test_walks_under_canary_zones():
    """Every case above once more in a process whose device buffers carry canary zones: a prefetch past the end of the
    entries of A (or a store past a row of C) touches a zone, the call returns SPECK_ERR_HIP and the child fails.  (The
    child deselects this test: it cannot start itself again.)"""
    env = dict(os.environ, SPECK_GUARD_BYTES="4096", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-k", "not canary",
                        os.path.join(ROOT, "tests", "test_gpu_esc_walk.py")], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    n = 2 * len(LANES) * len(WALK_ROWS) + len(WALK_ROWS)
    assert f"{n} passed" in r.stdout and "guard_bytes" not in r.stderr, tail
