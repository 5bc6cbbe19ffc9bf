"""The layouts of test_stages_host.py through analysis_kernel and scan_kernel: rows at every positional switch of the two.

For every layout (the analysis layouts in both shapes -- 8 waves x 32 rows forced with analysis_wide_rows = 0, 4 x 64 with
1 << 30 -- the scan layouts with the default):
  1. test_analysis_entry: sa.analysis == the oracle's analysis == the generator's claims, all four arrays and both totals;
  2. test_symbolic_entry: sa.symbolic's offsets == the running sum of the oracle's counts == the claims;
  3. test_complete_call: reuse = 0, fp64 -- C equals exact_spgemm bit for bit (dyadic values, no tolerance) and the call's
     statistics equal the claims: products, nnz, the two maxima, sym_bin_rows / num_bin_rows as whole dicts;
  4. test_row_view: a view of rows [5, m - 3) -- every sub-chunk boundary shifts, a_ro[0] != 0;
  5. test_replay_through_the_recomputing_verifier: verify_inputs = 0, four calls over a scribbled C, the last one replayed
     with the VERIFY analysis beside it (no false alarm on any path); then ONE column id of A moves onto another row of B in
     place -- in a lane-per-row sub-chunk, a tile-walk sub-chunk, a listed hub row, hub sub-chunks of the workgroups with 65
     and 66 of them: the replay is rejected, the re-run delivers the new product, the next replays pass;
  6. test_column_id_of_a_equal_to_the_rows_of_b: status 1, C untouched, the valid matrix multiplies on the same config;
  7. test_the_layouts_under_canary_zones: step 3 of every layout in a child whose device buffers carry canary zones.
A failure names the first rows that differ with their sub-chunk, chunk and workgroup.
No figure is compared with a tolerance anywhere.

scan_wide_2p25 / scan_wide_2p25_plus_1 (2^25 and 2^25 + 1 rows; the latter is the one launch of scan_kernel<32, true>, both
are the analysis with 129 chunks per workgroup): observed on an MI355X, scratch_pool_bytes = 29 440 (the slots of the two
numeric-first rows; the pool does not grow with the rows of A).  The arena itself is not reported by any call; by
scratch_bytes (pipeline.hip) it is 485 bytes per row of A + 16 per entry -- two record arrays of 7 regions x 32 bytes per
row are 448 of them -- 16.3 GB at 2^25 rows, not the few GB one would guess.  Each of the three steps on these two layouts
took 0.15 .. 1.5 s; the existing test_scan_tiles_at_the_capacity_of_the_chain (2^23 rows) took 0.37 s in the same run.
"""
import ctypes as C_
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import speck_amd as sa
from oracle import pyoracle as po
from speck_amd import _lib
from test_edges_host import classify  # noqa: F401  (the real classifier, compiled for the host)
from test_gpu_values import _scribble, _to_sa, assert_same_values
from test_stages_host import (ANALYSIS, CASES, CASE_IDS, build, class_counts, exact_of, expected, full, layout, movable_entry,
                              row_chunking, rows_of, with_entry)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROCESS_WIDE = {"analysis_wide_rows": 16, "scan_small_items": 3}      # not the config's own: back to their defaults after a test
SHAPE_OPT = {32: 0, 64: 1 << 30}                                      # analysis_wide_rows that forces 8 x 32 / 4 x 64


@pytest.fixture
def fresh():
    made = []

    def make(name, R, **opts):
        c = sa.spECKConfig.initialize(0)
        made.append(c)
        opts = dict(layout(name, R).opts, **opts)
        if name in ANALYSIS:
            opts["analysis_wide_rows"] = SHAPE_OPT[R]
        for k, v in opts.items():
            c.set_option(k, v)
        return c
    yield make
    for c in made:
        for k, v in PROCESS_WIDE.items():
            c.set_option(k, v)
        c.cleanup()


def _upload(name, R, A=None):
    A0, B, _ = build(name, R)
    return sa.dCSR.from_host(_to_sa(A or A0)), sa.dCSR.from_host(_to_sa(B)), sa.dCSR(np.float64)


@functools.lru_cache(maxsize=None)
def _oracle(name, R):
    """(analysis, row offsets of C, nnz of C) by the oracle"""
    A, B, _ = build(name, R)
    cnt, total = po.symbolic(A, B)
    po.lib().orc_exclusive_scan(cnt, A.rows)
    return po.analysis(A, B), cnt, total


def _same(got, want, what, name, R):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if bad.size:
        per, _ = row_chunking(build(name, R)[2].m)
        where = ", ".join(f"row {r} (workgroup {r // per}, chunk {r % per // 256}, sub-chunk {r % 256 // R}, lane {r % R}): "
                          f"{got[r]} want {want[r]}" for r in bad[:6].tolist())
        pytest.fail(f"{name} R = {R}: {what} differs in {bad.size} rows: {where}")


@pytest.mark.parametrize("name, R", CASES, ids=CASE_IDS)
def test_analysis_entry(fresh, name, R):
    _, _, claims = build(name, R)
    cfg = fresh(name, R, reuse=0)
    dA, dB, _ = _upload(name, R)
    got, (ref, _, _) = sa.analysis(dA, dB, cfg), _oracle(name, R)
    for k, field in (("row_ops", "ops"), ("row_max_ops", "mx"), ("row_col_min", "cmin"), ("row_col_max", "cmax")):
        _same(got[k], ref[k], f"{k} against the oracle", name, R)
        _same(got[k], full(claims, field), f"{k} against the layout", name, R)
    assert got["sum_products"] == ref["sum_products"] == claims.ops.sum()
    assert got["max_row_ops"] == ref["max_row_ops"] == claims.ops.max()


@pytest.mark.parametrize("name, R", CASES, ids=CASE_IDS)
def test_symbolic_entry(fresh, name, R):
    _, _, claims = build(name, R)
    cfg = fresh(name, R, reuse=0)
    dA, dB, _ = _upload(name, R)
    ro, nnz = sa.symbolic(dA, dB, cfg)
    _, want, total = _oracle(name, R)
    assert nnz == total == claims.nnz.sum()
    _same(ro, want, "row offsets of C against the oracle", name + " (row = index into the offsets)", R)
    _same(np.diff(ro.astype(np.int64)), full(claims, "nnz"), "nnz per row against the layout", name, R)


def _assert_stats(st, claims, counts, name):
    assert not st["replayed"] and not st["eager_through"] and not st["one_walk"] and not st["pool_fallbacks"], st
    assert st["sum_products"] == claims.ops.sum() and st["nnz_c"] == claims.nnz.sum(), name
    assert st["max_row_ops"] == claims.ops.max() and st["max_row_nnz_c"] == claims.nnz.max(), name
    assert st["sym_bin_rows"] == counts[0], (name, "symbolic classes", st["sym_bin_rows"], counts[0])
    assert st["num_bin_rows"] == counts[1], (name, "numeric classes", st["num_bin_rows"], counts[1])


@pytest.mark.parametrize("name, R", CASES, ids=CASE_IDS)
def test_complete_call(fresh, classify, name, R):
    """(scratch_pool_bytes is printed; what the two layouts of 2^25 rows showed is noted in the module's docstring)"""
    _, _, claims = build(name, R)
    cfg = fresh(name, R, reuse=0)
    dA, dB, dC = _upload(name, R)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    print(f"{name} R = {R}: rows {claims.m} scratch_pool_bytes {st['scratch_pool_bytes']} "
          f"sym {({k: v for k, v in st['sym_bin_rows'].items() if v})} num {({k: v for k, v in st['num_bin_rows'].items() if v})}")
    assert_same_values(dC.to_host(), expected(name, R), f"{name} R = {R}")
    _assert_stats(st, claims, class_counts(claims, classify), name)


VIEWED = [c for c in CASES if c[0] in ("tile_256_257", "hub_thresholds", "later_chunks_262145", "later_chunks_786433")]


@pytest.mark.parametrize("name, R", VIEWED, ids=[f"{n}-R{R}" for n, R in VIEWED])
def test_row_view(fresh, name, R):
    A, _, claims = build(name, R)
    r0, r1 = 5, claims.m - 3
    assert r0 % 32 and A.row_offsets[r0] != 0
    cfg = fresh(name, R, reuse=0)
    dA, dB, dC = _upload(name, R)
    sa.MultiplyspECK(dA.row_view(r0, r1), dB, dC, cfg)
    assert_same_values(dC.to_host(), rows_of(expected(name, R), r0, r1), f"{name} R = {R}, rows {r0} .. {r1}")


def _targets(pairs):
    return [(n, R, t) for n, ts in pairs for R in (32, 64) for t in ts]


MOVED = _targets([("row_path_8_9", ["lane", "tile"]), ("tile_256_257", ["tile"]), ("hub_thresholds", ["hub", "last_partial"]),
                  ("hub_list_64_65", ["hub65_0", "hub66_0", "hub66_33", "hub66_65"])])


@pytest.mark.parametrize("name, R, target", MOVED, ids=[f"{n}-R{R}-{t}" for n, R, t in MOVED])
def test_replay_through_the_recomputing_verifier(fresh, name, R, target):
    A, B, _ = build(name, R)
    cfg = fresh(name, R, verify_inputs=0)
    dA, dB, dC = _upload(name, R)

    def replays(want, calls, what):
        for call in range(calls):
            if dC.nnz:
                _scribble(dC, np.float64, cols=False)      # (the column ids stay: a replay checks them against the fresh ones)
            sa.MultiplyspECK(dA, dB, dC, cfg)
            if call == 0:
                first = cfg.last_stats()["numeric_reruns"]
        st = cfg.last_stats()
        assert st["replayed"] and st["pred_stages"] & 4, (what, st["replayed"], st["pred_stages"])
        assert st["numeric_reruns"] == first, (what, "a false alarm of the verifier")
        assert_same_values(dC.to_host(), want, f"{name} R = {R} {target}: {what}")
    replays(expected(name, R), 4, "replayed")
    # one column id of A onto the spare row of B beside it
    e, k = movable_entry(A, layout(name, R).targets[target])
    A2 = with_entry(A, e, k)
    reruns = cfg.last_stats()["numeric_reruns"]
    assert _lib.load().speck_dcsr_update(C_.byref(dA._c), None, np.ascontiguousarray(A2.col_ids).ctypes.data, None, 8) == 0
    _scribble(dC, np.float64, cols=False)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    assert cfg.last_stats()["numeric_reruns"] == reruns + 1, "the verifier did not see the entry move"
    E2 = exact_of(A2, B)
    assert_same_values(dC.to_host(), E2, f"{name} R = {R} {target}: the call that saw the change")
    replays(E2, 3, "replayed after the change")


BAD = _targets([("row_path_8_9", ["lane", "tile"]), ("hub_thresholds", ["hub", "last_partial"])])


@pytest.mark.parametrize("name, R, target", BAD, ids=[f"{n}-R{R}-{t}" for n, R, t in BAD])
def test_column_id_of_a_equal_to_the_rows_of_b(fresh, name, R, target):
    A, B, _ = build(name, R)
    row = layout(name, R).targets[target]
    Ax = with_entry(A, int(A.row_offsets[row + 1]) - 1, B.rows)       # the row's last entry: its ids still ascend
    cfg = fresh(name, R)
    dAx, dB, dC = _upload(name, R, Ax)
    with pytest.raises(sa.SpeckError) as e:
        sa.MultiplyspECK(dAx, dB, dC, cfg)
    assert e.value.status == 1
    assert dC.nnz == 0 and not dC._c.data and not dC._c.col_ids
    dA = sa.dCSR.from_host(_to_sa(A))
    sa.MultiplyspECK(dA, dB, dC, cfg)
    assert_same_values(dC.to_host(), expected(name, R), f"{name} R = {R}: the valid matrix after the rejected one")


def test_the_layouts_under_canary_zones():
    """Step 3 of every layout in a process whose device buffers carry canary zones: a record, list place or scratch slot
    written one element beside its array touches a zone, the call returns SPECK_ERR_HIP and the child fails.  (The child
    selects test_complete_call only: it cannot start itself again.)"""
    env = dict(os.environ, SPECK_GUARD_BYTES="4096", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-k", "test_complete_call",
                        os.path.join(ROOT, "tests", "test_gpu_stages.py")], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"{len(CASES)} passed" in r.stdout and "guard_bytes" not in r.stderr, tail
