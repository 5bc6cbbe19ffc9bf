"""Time speck_sort_rows_f64 against the only device path the library had before it: speck_transpose_f64 twice.

Input: C = A x A of a stand-in (scale 1.0 by default) with every row's entries shuffled on the device, fp64.  Protocol:
warm-up; device events on the config's stream around the call (the call returns with M complete, so the events span its
read-backs as a caller pays them); repeated ALTERNATING rounds (keep, sum, double transpose, early exit) with the median
taken per column; before every timed call the input is restored from a pristine shuffled copy by an untimed
device-to-device copy, since a sorted matrix takes the early exit.  The double transpose is timed with its allocations
inside (two outputs and 5 x 4 x nnz bytes of temporaries each).  Bandwidth column: the algorithmic bytes
8 rows + 2 x 12 nnz (early exit: 4 rows + 4 nnz) over the time, as a fraction of the HBM peak bench.py uses.

    python scripts/sort_rows_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speck_amd as sa  # noqa: E402

HBM_PEAK_GBS = 8000.0  # as bench.py


def shuffled_product(kind, scale, cfg, dev):
    A = sa.gen_matrix(kind, scale, 42, signed=True)
    dA = sa.dCSR.from_host(A)
    dC = sa.dCSR()
    sa.MultiplyspECK(dA, dA, dC, cfg)
    C = dC.to_host()
    dC.reset()
    dA.reset()
    ro = torch.from_numpy(C.row_offsets.view(np.int32).copy()).to(dev)
    col = torch.from_numpy(C.col_ids.view(np.int32).copy()).to(dev)
    val = torch.from_numpy(C.data).to(dev)
    lens = torch.from_numpy(np.diff(C.row_offsets.astype(np.int64))).to(dev)
    row_of = torch.repeat_interleave(torch.arange(C.rows, device=dev, dtype=torch.float64), lens)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    perm = torch.argsort(row_of + torch.rand(C.nnz, device=dev, dtype=torch.float64, generator=g) * 0.999)
    return C, ro, col[perm].contiguous(), val[perm].contiguous(), col, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sort_rows_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        for kind in args.kinds.split(","):
            C, ro, p_col, p_val, sorted_col, sorted_val = shuffled_product(kind, args.scale, cfg, dev)
            w_col, w_val = p_col.clone(), p_val.clone()
            M = sa.dCSR.from_device(C.rows, C.cols, C.nnz, ro.data_ptr(), w_col.data_ptr(), w_val.data_ptr(),
                                    keep=(ro, w_col, w_val), host_row_offsets=C.row_offsets)
            torch.cuda.synchronize()   # (the shuffle ran on torch's current stream: the timed stream does not wait for it)
            s = torch.cuda.Stream(device=dev)
            cfg.set_stream(s.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def restore():
                with torch.cuda.stream(s):
                    w_col.copy_(p_col, non_blocking=True)
                    w_val.copy_(p_val, non_blocking=True)
                s.synchronize()

            def timed(fn):
                with torch.cuda.stream(s):
                    e0.record(s)
                    out = fn()
                    e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1), out

            def double_transpose():
                t1 = sa.transpose(M, cfg)
                t2 = sa.transpose(t1, cfg)
                return t1, t2

            ms = {"keep": [], "sum": [], "transpose2": [], "early_exit": []}
            info = None
            for r in range(args.warmup + args.rounds):
                take = r >= args.warmup
                restore()
                t, info = timed(lambda: sa.sort_rows(M, cfg))
                if take:
                    ms["keep"].append(t)
                # (the matrix is canonical now: the early exit)
                t, again = timed(lambda: sa.sort_rows(M, cfg))
                assert sum(again.rows_sorted) == 0
                if take:
                    ms["early_exit"].append(t)
                restore()
                t, _ = timed(lambda: sa.sort_rows(M, cfg, sum_duplicates=True))
                if take:
                    ms["sum"].append(t)
                restore()
                t, outs = timed(double_transpose)
                if take:
                    ms["transpose2"].append(t)
                if r == 0:   # both paths give the rows of C back
                    got = outs[1].to_host()
                    assert (got.col_ids == C.col_ids).all() and (got.data == C.data).all()
                for o in outs:
                    o.reset()
            restore()
            sa.sort_rows(M, cfg)
            torch.cuda.synchronize()
            assert torch.equal(w_col, sorted_col) and torch.equal(w_val, sorted_val)
            cfg.set_stream(None)
            med = {k: statistics.median(v) for k, v in ms.items()}
            full = 8 * C.rows + 2 * 12 * C.nnz
            early = 4 * C.rows + 4 * C.nnz
            rec = dict(kind=kind, scale=args.scale, rows=C.rows, nnz=C.nnz, rows_in_order=info.rows_in_order,
                       rows_reg=info.rows_sorted[0], rows_lds=info.rows_sorted[1], rows_global=info.rows_sorted[2],
                       keep_ms=med["keep"], sum_ms=med["sum"], transpose2_ms=med["transpose2"], early_exit_ms=med["early_exit"],
                       keep_min_max=(min(ms["keep"]), max(ms["keep"])), sum_min_max=(min(ms["sum"]), max(ms["sum"])),
                       early_exit_min_max=(min(ms["early_exit"]), max(ms["early_exit"])),
                       transpose2_min_max=(min(ms["transpose2"]), max(ms["transpose2"])),
                       keep_hbm_frac=full / (med["keep"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       sum_hbm_frac=full / (med["sum"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       early_exit_hbm_frac=early / (med["early_exit"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       speedup_vs_transpose2=med["transpose2"] / med["keep"], rounds=args.rounds)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del M, w_col, w_val, p_col, p_val, sorted_col, sorted_val, ro
            torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
