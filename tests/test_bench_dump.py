"""bench.py --dump-outputs on the host: the files stay within 64 MB, a larger output is cut to a fixed seeded sample
whose positions are written beside it, and the same output gives the same files."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _csr(rows, nnz, dtype, seed):
    rng = np.random.default_rng(seed)
    ro = np.sort(rng.integers(0, nnz + 1, rows + 1)).astype(np.uint32)
    ro[0], ro[-1] = 0, nnz
    return ro, rng.integers(0, rows, nnz).astype(np.uint32), rng.random(nnz).astype(dtype)


@pytest.mark.parametrize("rows,nnz,dtype", [(3000, 70000, np.float64), (170000, 5300000, np.float64),
                                            (9000000, 6000000, np.float32)])
def test_dump_outputs_is_bounded_and_reproducible(tmp_path, rows, nnz, dtype):
    bench = _bench()
    ro, col, val = _csr(rows, nnz, dtype, 1)
    got = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), rows, rows, ro, col, val)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
        got.append({f[:-len(".npy")]: np.load(d / f) for f in os.listdir(d)})
    g = got[0]
    assert set(g) == set(got[1]) and all((g[n] == got[1][n]).all() for n in g)
    assert g["C_shape"].tolist() == [rows, rows, nnz]
    assert g["C_values"].dtype == dtype and g["C_col_ids"].dtype == np.float64
    sampled = 8 * (rows + 1) + (8 + np.dtype(dtype).itemsize) * nnz > 64_000_000
    assert ("C_entry_index" in g) == sampled
    e = g["C_entry_index"].astype(np.int64) if sampled else slice(None)
    r = g["C_row_offsets_index"].astype(np.int64) if "C_row_offsets_index" in g else slice(None)
    assert (g["C_col_ids"] == col[e]).all() and (g["C_values"] == val[e]).all() and (g["C_row_offsets"] == ro[r]).all()
