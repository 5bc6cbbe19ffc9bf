"""scan_kernel keeps what it classified a row from: the registers of ONE thread, rows beyond the end, the early gate.

scan_kernel (speck_amd/csrc/stages.hip) requests what a thread's rows are classified from in one round -- counts, the
a_ro pairs, row_ops, row_col_min, row_col_max -- and, up to four rows per thread, writes the records from those registers;
with eight rows per thread it does so in two groups of four, and reads the groups again for the records.  The layouts of
test_stages_host.py put classed rows at tile edges; here ONE thread's consecutive rows all carry different numeric classes
and different (len_a, ops, cmin, cmax), and so do the rows of its two neighbours: a value of row i used for row j, or a
register that went stale between the two groups, is a wrong record, and a wrong record is a wrong C.

  kept_items_2 / 3 / 4   m = 2 T + 1 rows (T = 256 ITEMS): thread 0 and thread 255 of tile 0, thread 0 of tile 1
  kept_items_8           m = 2^19 + 9: eight classed rows in a thread at the start, in the middle and at the end -- the last
                         tile holds nine rows, its second thread one row of eight
  views                  the same layouts through row_view, cut one and two rows into a thread's rows, classed rows (a
                         NUM_B2K row among them) directly behind the cut: nnz, offsets and class counts of the view
                         must not see them.  m = 1 and 2 (mod 3) with three rows per thread, 1 (mod 8) with eight.
Every case: the first call on a config with its defaults, a complete call (reuse = 0), and the through call that follows
it over a scribbled C (eager_through == 1).  Dyadic values: C equals exact_spgemm bit for bit, the rows per numeric class
equal the host classifier's.
  gate                   through calls on one config: good B, the same B with two column ids of one row swapped in place,
                         good B again.  The last tile of the scan asks for the input check's ticket when it starts: the
                         middle call must find ITS check (status 8, the scribbled C untouched), not the ticket of the call
                         before it.
The host half (no GPU): the generator's claims for these layouts against the oracle and scan_shape.
"""
import ctypes as C_

import numpy as np
import pytest

import speck_amd as sa
import test_stages_host as H
from oracle import pyoracle as po
from speck_amd import _lib
from test_edges_host import CP_DEFAULT, NUM_NAMES, _classify_line, classify  # noqa: F401
from test_gpu_stages import fresh  # noqa: F401
from test_gpu_values import _scribble, _to_sa, assert_same_values
from test_stages_host import KINDS, K, Layout, Placed, build, class_counts, expected, layout, rows_of, scan_shape

gpu = pytest.mark.gpu
T_ = K["kScanThreads"]
M8 = (1 << 19) + 9


def _kind(name, k, len_a=None):
    """KINDS[name] with a column range and a length of its own: [5 + 3 k, ...) instead of [5, ...)"""
    r = KINDS[name]
    return r._replace(len_a=len_a or r.len_a, cmin=r.cmin + 3 * k, cmax=r.cmax + 3 * k)


# six numeric classes (the SCAN_KINDS of test_stages_host.py) + NUM_R64, no two with the same len_a, ops, cmin or cmax;
# light and heavy rows in turn: of any three consecutive rows one has >= 400 products
KEPT = [_kind("direct", 0), _kind("block2k", 1, 66), _kind("g8", 2), _kind("nf", 3, 67), _kind("wave128", 4, 65),
        _kind("dense4k", 5, 68), _kind("r64", 6)]
KEPT_CLASSES = ["direct", "block2k", "g8", "nfcopy", "wave128", "dense4k", "r64"]
HEAVY = 400


def _thread_rows(items, tile, thread):
    first = (tile * T_ + thread) * items
    return list(range(first, first + items))


def _kept(m, items, threads, kinds, opts):
    """classed rows in every row of the threads named and of their two neighbours (a neighbour may lie in the next or the
    previous tile), kinds in turn: any len(kinds) consecutive rows differ"""
    pos = {m - 1}
    for tile, thread in threads:
        for n in (-1, 0, 1):
            pos.update(_thread_rows(items, tile, thread + n))
    pos = sorted(p for p in pos if 0 <= p < m)
    placed = [Placed(p, kinds[i % len(kinds)], (), False) for i, p in enumerate(pos)]
    return Layout(m, placed, H._derived_subs(m, 32, placed), opts, {})


# name -> (rows per thread, rows of A, [(tile, thread)] whose rows are all classed)
KEPT_LAYOUTS = {f"kept_items_{i}": (i, 2 * T_ * i + 1, [(0, 0), (0, 255), (1, 0)]) for i in (2, 3, 4)}
KEPT_LAYOUTS["kept_items_8"] = (8, M8, [(0, 0), (128, 100), (256, 0)])
for _n, (_i, _m, _th) in KEPT_LAYOUTS.items():
    H.LAYOUTS[_n] = (lambda i, m, th: lambda R: _kept(m, i, th, KEPT[:6] if i < 8 else KEPT,
                                                      dict(scan_small_items=i) if i < 8 else {}))(_i, _m, _th)
# (layout, rows of the view): cut one / two rows into a thread's rows
VIEWS = [("kept_items_3", 254 * 3 + 1), ("kept_items_3", 254 * 3 + 2), ("kept_items_3", T_ * 3 + 2), ("kept_items_8", (1 << 19) + 1)]
CASES = [(n, None) for n in KEPT_LAYOUTS] + VIEWS
IDS = [n if r1 is None else f"{n}-view-{r1}" for n, r1 in CASES]


def _claims_of(name, r1):
    """the claims of rows [0, r1) of a layout"""
    c = build(name, 32)[2]
    if r1 is None:
        return c
    keep = c.rows < r1
    return c._replace(m=r1, rows=c.rows[keep], len_a=c.len_a[keep], ops=c.ops[keep], mx=c.mx[keep], cmin=c.cmin[keep],
                      cmax=c.cmax[keep], nnz=c.nnz[keep], b_first=c.b_first[keep])


# ------------------------------------------------------------------------------------------------------------ host half
def test_the_kept_kinds_are_seven_classes_with_nothing_in_common(classify):
    got = classify([_classify_line(r.len_a, r.ops, r.nnz, r.cmin, r.cmax, CP_DEFAULT) for r in KEPT])
    assert [NUM_NAMES[n] for _, n in got] == KEPT_CLASSES
    for field in ("len_a", "ops", "cmin", "cmax"):
        assert len({getattr(r, field) for r in KEPT}) == len(KEPT), field


@pytest.mark.parametrize("name", list(KEPT_LAYOUTS))
def test_generator_builds_the_kept_layouts(name):
    H.test_generator_builds_the_layout_it_claims(name, 32)


@pytest.mark.parametrize("name", list(KEPT_LAYOUTS))
def test_the_kept_layouts_hold_what_they_promise(name):
    items, m, threads = KEPT_LAYOUTS[name]
    L = layout(name, 32)
    at = {p.row: p.spec for p in L.placed}
    assert L.m == m and scan_shape(m, items if items < 8 else None)[:2] == (items, 1)
    tiles = scan_shape(m, items if items < 8 else None)[2]
    assert tiles == (3 if items < 8 else 257) and m - (tiles - 1) * T_ * items == (1 if items < 8 else 9)
    for tile, thread in threads:
        for n in (-1, 0, 1):
            rows = [r for r in _thread_rows(items, tile, thread + n) if 0 <= r < m]
            if not rows:
                continue                                             # (thread 0 of tile 0 has one neighbour)
            assert all(r in at for r in rows), (tile, thread + n)
            for field in ("num", "len_a", "ops", "cmin", "cmax"):
                distinct = len({getattr(at[r], field) for r in rows})
                # seven kinds in eight rows: the eighth row repeats the first one's kind (its a_ro pair and row id differ)
                assert distinct == min(len(rows), 7), (tile, thread + n, field)
    if items == 8:
        # the last tile: eight rows in thread 0, ONE row of eight in thread 1
        assert all(r in at for r in range(m - 9, m)) and (m - 9) % (T_ * 8) == 0


@pytest.mark.parametrize("name, r1", VIEWS, ids=IDS[len(KEPT_LAYOUTS):])
def test_the_views_cut_into_a_thread(name, r1):
    items = KEPT_LAYOUTS[name][0]
    at = {p.row: p.spec for p in layout(name, 32).placed}
    assert scan_shape(r1, items if items < 8 else None)[0] == items
    assert r1 % items in ((1, 2) if items == 3 else (1,)) and r1 - 1 in at
    behind = [at[r] for r in range(r1, r1 + 3)]                       # classed rows directly behind the cut, a heavy one among them
    assert any(s.ops >= HEAVY for s in behind) and all(s.nnz for s in behind)
    c = _claims_of(name, r1)
    assert c.rows.size and c.rows.max() == r1 - 1 and c.nnz.sum() < build(name, 32)[2].nnz.sum()


# ------------------------------------------------------------------------------------------------------------- GPU half
def _assert_call(cfg, dC, name, r1, classify, through, what):
    st = cfg.last_stats()
    claims = _claims_of(name, r1)
    want = expected(name, 32) if r1 is None else rows_of(expected(name, 32), 0, r1)
    print(f"{name} {r1} {what}: through {st['eager_through']} nnz {st['nnz_c']} num {({k: v for k, v in st['num_bin_rows'].items() if v})}")
    if through is not None:
        assert st["eager_through"] == through and not st["replayed"], (what, st["eager_through"], st["replayed"])
    assert_same_values(dC.to_host(), want, f"{name} rows [0, {r1}): {what}")
    assert st["nnz_c"] == claims.nnz.sum() and st["max_row_nnz_c"] == claims.nnz.max(), what
    assert st["num_bin_rows"] == class_counts(claims, classify)[1], (what, st["num_bin_rows"])


@gpu
@pytest.mark.parametrize("name, r1", CASES, ids=IDS)
def test_kept_rows(fresh, classify, name, r1):
    A, B, _ = build(name, 32)
    dA, dB = sa.dCSR.from_host(_to_sa(A)), sa.dCSR.from_host(_to_sa(B))
    dV = dA if r1 is None else dA.row_view(0, r1)
    # the first call on a config, everything at its default
    cfg = fresh(name, 32)
    dC = sa.dCSR(np.float64)
    sa.MultiplyspECK(dV, dB, dC, cfg)
    _assert_call(cfg, dC, name, r1, classify, None, "first call on a config")
    # a complete call, and the through call behind it
    cfg = fresh(name, 32, reuse=0)
    dC = sa.dCSR(np.float64)
    sa.MultiplyspECK(dV, dB, dC, cfg)
    _assert_call(cfg, dC, name, r1, classify, 0, "complete call")
    _scribble(dC, np.float64)
    sa.MultiplyspECK(dV, dB, dC, cfg)
    _assert_call(cfg, dC, name, r1, classify, 1, "through call")


def _swapped_row(B):
    """B's column ids with the first two ids of its first row of >= 2 entries swapped in place"""
    ro = B.row_offsets.astype(np.int64)
    e = int(ro[np.flatnonzero(np.diff(ro) >= 2)[0]])
    col = B.col_ids.copy()
    col[e], col[e + 1] = col[e + 1], col[e]
    return np.ascontiguousarray(col)


@gpu
def test_the_early_gate_takes_this_calls_ticket(fresh, classify):
    name = "kept_items_3"
    A, B, _ = build(name, 32)
    dA, dB, dC = sa.dCSR.from_host(_to_sa(A)), sa.dCSR.from_host(_to_sa(B)), sa.dCSR(np.float64)
    cfg = fresh(name, 32, reuse=0)
    update = lambda col: _lib.load().speck_dcsr_update(C_.byref(dB._c), None, col.ctypes.data, None, 8)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    _scribble(dC, np.float64)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    _assert_call(cfg, dC, name, None, classify, 1, "good B")
    # the same B, two ids of one row swapped: the check of THIS call objects, the ticket of the call before says nothing
    _scribble(dC, np.float64)
    scribbled = dC.to_host()
    assert update(_swapped_row(B)) == 0
    with pytest.raises(sa.SpeckError) as e:
        sa.MultiplyspECK(dA, dB, dC, cfg)
    assert e.value.status == 8
    after = dC.to_host()
    assert (after.row_offsets == scribbled.row_offsets).all() and (after.col_ids == 0xDEADBEEF).all()
    assert (after.col_ids == scribbled.col_ids).all() and (after.data == scribbled.data).all()
    # good again: the verdict of the rejected call is not held against this one
    assert update(np.ascontiguousarray(B.col_ids)) == 0
    sa.MultiplyspECK(dA, dB, dC, cfg)
    _assert_call(cfg, dC, name, None, classify, 1, "good B after the rejected one")
