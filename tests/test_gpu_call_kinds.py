"""Every kind of call a multiply can be, each right behind a call of another kind, on ONE config.

speck_amd/csrc/pipeline.hip tries the kinds in a fixed order -- reuse sequence, hash one-walk, one-walk, through call,
speculated batch, plain two-phase call (with its pool read-back) -- and each attempt either completes the call, misses and
hands over to the next, or (through call) misses and leaves its front standing.  This file pins which kind every call of
one long sequence takes and what it does to the config's counters, and checks every product against the oracle
(row_offsets and col_ids bit-exact, values within 1e-12 * sum|a*b|).  The last steps run a call with
Timings(measureAll=True) and calls under profile_kernels(1): which stage fields and phase times they fill is pinned as a
pattern of zero / positive, never as values.

Order: the issue's step 11 (scratch-pool fallback) runs LAST here, behind the timing steps: a fallback switches the
numeric-first class off for the config from then on, and the timing steps are worth more with that class on.
"""
import ctypes as C_

import numpy as np
import pytest

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po
from test_gpu_parity import _assert_matches_oracle, fast_random_csr, to_po, to_sa

pytestmark = pytest.mark.gpu

FLAGS = ("replayed", "pred_stages", "eager_through", "eager_speculated", "one_walk", "nf_direct", "esc_fused")
COUNTERS = ("numeric_reruns", "graph_replays", "graph_captures", "pool_fallbacks", "walk_misses")
STAGES = ("init", "countProducts", "loadBalanceCounting", "globalMapsCounting", "spGEMMCounting", "allocC",
          "loadBalanceNumeric", "globalMapsNumeric", "spGEMMNumeric", "sorting", "cleanup")
PHASES = ("analysis_ms", "sym_phase_ms", "scan_ms", "num_phase_ms", "kernel_events_valid")


def _observed(cfg):
    st = cfg.last_stats()
    return tuple(int(st[k]) for k in FLAGS), tuple(int(st[k]) for k in COUNTERS)


def _positive(names, get):
    """the names whose value is positive (the others are zero: nothing here is negative)"""
    vals = {k: float(get(k)) for k in names}
    print("   ", vals)
    assert all(v >= 0.0 for v in vals.values()), vals
    return tuple(k for k in names if vals[k] > 0.0)


def _rewired(H, rng):
    """Column ids of a tenth of the rows drawn again, row lengths kept: another nnz(C) under the same buffers."""
    col = H.col_ids.copy()
    ro = H.row_offsets.astype(np.int64)
    for r in rng.choice(H.rows, size=H.rows // 10, replace=False):
        n = int(ro[r + 1] - ro[r])
        if n:
            col[ro[r]:ro[r + 1]] = np.sort(rng.choice(H.cols, size=n, replace=False)).astype(np.uint32)
    return po.HostCSR(H.rows, H.cols, H.row_offsets, col, H.data)


def call_kind_sequence():
    """The steps of the test, one at a time: (name, what was observed behind the step)."""
    rng = np.random.default_rng(5)
    X = to_po(sa.gen_matrix("mac_econ", 0.08, 3, signed=True))   # register-class, hash and numeric-first rows
    L = _lib.load()
    cfg = sa.spECKConfig.initialize(0)
    try:
        A = X                                                      # what dA holds now
        dA, dB, dC = sa.dCSR.from_host(to_sa(X)), sa.dCSR.from_host(to_sa(X)), sa.dCSR()

        def multiply_x(name, timings=None):
            sa.MultiplyspECK(dA, dB, dC, cfg, timings)
            _assert_matches_oracle(dC, A, X)
            return name, _observed(cfg)

        def rewire_a():
            nonlocal A
            A = _rewired(A, rng)
            assert L.speck_dcsr_update(C_.byref(dA._c), None, np.ascontiguousarray(A.col_ids).ctypes.data, None, 8) == 0

        cfg.set_option("reuse", 0)
        yield multiply_x("1 two-phase")
        yield multiply_x("2 through")
        rewire_a()
        yield multiply_x("3 through miss, the front stands")
        cfg.set_option("eager_through", 0)
        yield multiply_x("4 speculated batch")
        cfg.set_option("eager_speculate", 0)
        yield multiply_x("5 plain two-phase")
        cfg.set_option("one_walk", 2)
        yield multiply_x("6 one-walk")
        rewire_a()
        yield multiply_x("7 one-walk miss, then two-phase")
        cfg.set_option("one_walk", 0)
        cfg.set_option("eager_speculate", 1)
        cfg.set_option("eager_through", 1)

        # the hash one-walk call, on the input of test_gpu_walk.py's test of it
        cfg.set_option("one_walk_hash", 2)
        H = to_po(sa.gen_matrix("nlpkkt", 0.01, 3, signed=True))
        dH, dCh = sa.dCSR.from_host(to_sa(H)), sa.dCSR()
        for name in ("8a other shapes: two-phase", "8b hash one-walk"):
            sa.MultiplyspECK(dH, dH, dCh, cfg)
            _assert_matches_oracle(dCh, H, H)
            yield name, _observed(cfg)
        del dH, dCh
        # ... and a row that outgrows its table under the same shapes
        G = fast_random_csr(20000, 4000, 8, 101)
        B1 = fast_random_csr(4000, 60000, 10, 102)               # rows of C up to ~100 entries
        B2 = fast_random_csr(4000, 60000, 60, 103)               # ... of several hundred
        dG, dCg = sa.dCSR.from_host(to_sa(G)), sa.dCSR()
        for name, B in (("9a other shapes: two-phase", B1), ("9b hash one-walk", B1), ("9c hash one-walk miss, through miss", B2)):
            dBg = sa.dCSR.from_host(to_sa(B))
            sa.MultiplyspECK(dG, dBg, dCg, cfg)
            _assert_matches_oracle(dCg, G, B)
            yield name, _observed(cfg)
        del dG, dBg, dCg
        cfg.set_option("one_walk_hash", 0)

        yield multiply_x("10a other shapes: two-phase")
        cfg.set_option("reuse", 1)                                 # (the switch forgets the call before: no sequence yet)
        yield multiply_x("10b through")
        yield multiply_x("10c plan made, replayed")
        yield multiply_x("10d replayed without a scan")
        cfg.set_option("reuse", 0)

        # nothing else in tests/ runs these two
        t = sa.Timings(measureAll=True)
        name, seen = multiply_x("12a measureAll", t)
        yield name, seen
        yield "12a stage fields", _positive(STAGES, lambda k: getattr(t, k))
        yield "12a phase times", _positive(PHASES, lambda k: cfg.last_stats()[k])
        cfg.profile_kernels(1)
        yield multiply_x("12b profile_kernels")
        yield "12b phase times", _positive(PHASES, lambda k: cfg.last_stats()[k])
        cfg.set_option("one_walk", 2)
        yield multiply_x("12c profile_kernels, one-walk")
        yield "12c phase times", _positive(PHASES, lambda k: cfg.last_stats()[k])
        cfg.set_option("one_walk", 0)
        cfg.profile_kernels(0)
        yield multiply_x("12d speculated batch behind a one-walk")

        # the scratch pool of the numeric-first rows does not fit its budget: as test_gpu_parity.py's test of it
        cfg.set_option("nf_pool_max_mb", 1)
        K = to_po(sa.gen_matrix("cant", 0.05, 3, signed=True))
        dK, dCk = sa.dCSR.from_host(to_sa(K)), sa.dCSR()
        sa.MultiplyspECK(dK, dK, dCk, cfg)
        _assert_matches_oracle(dCk, K, K)
        assert cfg.last_stats()["sym_bin_rows"]["numeric_first"] == 0
        yield "11 pool fallback", _observed(cfg)
    finally:
        cfg.cleanup()


# Recorded by running call_kind_sequence() on the PARENT of the commit that split multiply_impl into one function per
# call kind (twice, in two processes: the same table both times), not on the code under test.
#   flags:    replayed pred_stages eager_through eager_speculated one_walk nf_direct esc_fused
#   counters: numeric_reruns graph_replays graph_captures pool_fallbacks walk_misses (cumulative)
EXPECTED = {
    "1 two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0)),
    "2 through": ((0, 0, 1, 1, 0, 0, 0), (0, 0, 0, 0, 0)),
    "3 through miss, the front stands": ((0, 0, -1, 1, 0, 0, 0), (0, 0, 0, 0, 0)),
    "4 speculated batch": ((0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0)),
    "5 plain two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0)),
    "6 one-walk": ((0, 0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 0)),
    "7 one-walk miss, then two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1)),
    "8a other shapes: two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1)),
    "8b hash one-walk": ((0, 0, 0, 0, 2, 0, 0), (0, 0, 0, 0, 1)),
    "9a other shapes: two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1)),
    "9b hash one-walk": ((0, 0, 0, 0, 2, 0, 0), (0, 0, 0, 0, 1)),
    "9c hash one-walk miss, through miss": ((0, 0, -1, 1, 0, 0, 0), (0, 0, 0, 0, 2)),
    "10a other shapes: two-phase": ((0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 2)),
    "10b through": ((0, 0, 1, 1, 0, 0, 0), (0, 0, 0, 0, 2)),
    "10c plan made, replayed": ((1, 7, 0, 0, 0, 1, 1), (0, 1, 1, 0, 2)),
    "10d replayed without a scan": ((1, 15, 0, 0, 0, 1, 1), (0, 2, 2, 0, 2)),
    "12a measureAll": ((0, 0, 0, 1, 0, 0, 0), (0, 2, 2, 0, 2)),
    "12a stage fields": ("init", "countProducts", "spGEMMCounting", "allocC", "loadBalanceNumeric", "globalMapsNumeric", "spGEMMNumeric"),
    "12a phase times": ("analysis_ms", "sym_phase_ms", "scan_ms", "num_phase_ms", "kernel_events_valid"),
    "12b profile_kernels": ((0, 0, 0, 1, 0, 0, 0), (0, 2, 2, 0, 2)),
    "12b phase times": ("analysis_ms", "sym_phase_ms", "scan_ms", "num_phase_ms", "kernel_events_valid"),
    "12c profile_kernels, one-walk": ((0, 0, 0, 0, 1, 0, 0), (0, 2, 2, 0, 2)),
    "12c phase times": ("analysis_ms", "sym_phase_ms", "scan_ms", "num_phase_ms", "kernel_events_valid"),
    "12d speculated batch behind a one-walk": ((0, 0, 0, 1, 0, 0, 0), (0, 2, 2, 0, 2)),
    "11 pool fallback": ((0, 0, 0, 0, 0, 0, 0), (0, 2, 2, 1, 2)),
}


def test_every_call_takes_the_kind_it_took():
    seen = dict(call_kind_sequence())
    for name, what in seen.items():
        print(repr(name) + ":", repr(what) + ",")
    assert seen == EXPECTED
