"""The edge table of test_edges_host.py through the kernels: rows of C exactly on every class limit and table-size switch.

For every probe (rows with the last value on one side of a limit and the first on the other, in different numbers):
  1. test_complete_call: a complete call on a fresh config (reuse = 0), fp64 -- structure and values equal exact_spgemm bit
     for bit (dyadic inputs: one right answer whatever the summation order; no tolerance), and sym_bin_rows / num_bin_rows
     equal the WHOLE expected dict: every class, the counts of both sides of the edge, nothing anywhere else;
  2. test_replayed_over_scribbled_c: a config with reuse on, four calls over a scribbled C, the last one replayed, bit for
     bit again -- with num_verify 1 and 2 (the VERIFY bodies with bounded probing meet a table at its exact limit).  Class
     counts are not compared there: a replay books the register-class rows as nfcopy (esc_fused);
  3. test_complete_call_fp32: step 1 in fp32;
  4. test_the_table_under_canary_zones: step 1 for the whole table once more in a child process whose every device buffer
     carries canary zones (SPECK_GUARD_BYTES): a touched zone fails the call.
Steps 1 and 4 cover every probe; steps 2 and 3 the probes of DEEP_KINDS below.  Nothing is skipped: the one edge
no call can reach is listed with its reason in test_edges_host.UNREACHABLE and shown unreachable there.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import speck_amd as sa
from test_edges_host import PROBES, as_dtype, build, class_counts, expected
from test_gpu_values import _scribble, _to_sa, assert_same_values

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL = [p.name for p in PROBES]
# steps 2 and 3: the register-class edges and everything numeric (tables, sort forms, windows, staging); the probes of kind
# "symbolic" / "analysis" place their edge in the symbolic phase or in the analysis, which steps 1 and 4 run
DEEP_KINDS = ("register", "numeric", "sort", "staging")
DEEP = [p.name for p in PROBES if p.kind in DEEP_KINDS]
PROCESS_WIDE = {"b8k_full_first": 1}      # options that are not the config's own: back to their defaults after a test


def _probe(name):
    return next(p for p in PROBES if p.name == name)


@pytest.fixture
def fresh():
    made = []

    def make(**opts):
        c = sa.spECKConfig.initialize(0)
        made.append(c)
        for k, v in opts.items():
            c.set_option(k, v)
        return c
    yield make
    for c in made:
        for k, v in PROCESS_WIDE.items():
            c.set_option(k, v)
        c.cleanup()


def _upload(name, dtype):
    A, B, _ = build(name)
    return sa.dCSR.from_host(_to_sa(as_dtype(A, dtype))), sa.dCSR.from_host(_to_sa(as_dtype(B, dtype))), sa.dCSR(dtype)


def _complete_call(fresh, name, dtype):
    p = _probe(name)
    cfg = fresh(reuse=0, **p.opts)
    dA, dB, dC = _upload(name, dtype)
    sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    assert not st["replayed"] and not st["eager_through"] and not st["one_walk"] and not st["pool_fallbacks"], st
    assert_same_values(dC.to_host(), expected(name, dtype), f"{name}/{np.dtype(dtype).name}")
    sym, num = class_counts(p)
    print(f"{name}: sym {({k: v for k, v in st['sym_bin_rows'].items() if v})} num {({k: v for k, v in st['num_bin_rows'].items() if v})}")
    assert st["sym_bin_rows"] == sym, (name, "symbolic classes", st["sym_bin_rows"], sym)
    assert st["num_bin_rows"] == num, (name, "numeric classes", st["num_bin_rows"], num)
    _, _, specs = build(name)
    assert st["sum_products"] == sum(r.ops for r in specs) and st["nnz_c"] == sum(r.nnz for r in specs)
    assert st["max_row_ops"] == max(r.ops for r in specs) and st["max_row_nnz_c"] == max(r.nnz for r in specs)


@pytest.mark.parametrize("name", ALL)
def test_complete_call(fresh, name):
    _complete_call(fresh, name, np.float64)


@pytest.mark.parametrize("name", DEEP)
def test_complete_call_fp32(fresh, name):
    _complete_call(fresh, name, np.float32)


@pytest.mark.parametrize("num_verify", [1, 2])
@pytest.mark.parametrize("name", DEEP)
def test_replayed_over_scribbled_c(fresh, name, num_verify):
    p = _probe(name)
    cfg = fresh(num_verify=num_verify, **p.opts)
    dA, dB, dC = _upload(name, np.float64)
    for call in range(4):
        if call:
            _scribble(dC, np.float64, cols=False)     # (the column ids stay: a replay checks them against the fresh ones)
        sa.MultiplyspECK(dA, dB, dC, cfg)
    st = cfg.last_stats()
    assert st["replayed"], st
    assert_same_values(dC.to_host(), expected(name, np.float64), f"replayed {name}")
    assert st["nnz_c"] == expected(name, np.float64).nnz


def test_the_table_under_canary_zones():
    """Step 1 of every probe in a process whose device buffers carry canary zones: a row that overflows its table, its
    window or its scratch slot by one entry touches a zone, the call returns SPECK_ERR_HIP and the child fails.  (The child
    selects test_complete_call only: it cannot start itself again.)"""
    env = dict(os.environ, SPECK_GUARD_BYTES="4096", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-k", "test_complete_call and not fp32",
                        os.path.join(ROOT, "tests", "test_gpu_edges.py")], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"{len(ALL)} passed" in r.stdout and "guard_bytes" not in r.stderr, tail
