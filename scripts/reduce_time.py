"""Time speck_reduce_f64 / _f32 against a copy of the array it reads.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: S and the product S S (made on the device).  Ops: SUM and
ABS_MAX, rows + total.  Yardstick, on the same box in the same rounds: a plain device-to-device copy of A's data array
into a buffer that exists -- it moves the same bytes in and as many out, the reduce moves them in only, so by the byte
count a reduce should not exceed it.  Protocol: warm-up; device events around the whole call (reduce: on the config's
stream, the call returns with its results complete, so the events span its read-back; the copy: on the NULL stream it
runs on); repeated ALTERNATING rounds with the median taken per column.  The row results go to a tensor that exists, so
after the warm-up a reduce allocates nothing.

    python scripts/reduce_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
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
OPS = ("sum", "abs_max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reduce_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        null = torch.cuda.default_stream(dev)
        s = torch.cuda.Stream(device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn, stream):
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        for kind in args.kinds.split(","):
            for dtype in (np.float64, np.float32):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dS, dP = sa.dCSR.from_host(S), sa.dCSR(dtype)
                sa.MultiplyspECK(dS, dS, dP, cfg)
                for name, dA in (("S", dS), ("SS", dP)):
                    H = dA.to_host()
                    src = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                    dst = torch.empty_like(src)
                    out = torch.zeros(max(H.rows, 1), dtype=torch.float64, device=dev)
                    want = {"sum": float(H.data.astype(np.float64).sum()), "abs_max": float(np.abs(H.data).max(initial=0.0))}
                    torch.cuda.synchronize()
                    ms = {k: [] for k in OPS + ("memcpy",)}
                    totals = {}
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        for op in OPS:
                            cfg.set_stream(s.cuda_stream)
                            t, (_, totals[op], info) = timed(lambda: sa.reduce(dA, cfg, op, out_ptr=out.data_ptr()), s)
                            cfg.set_stream(None)
                            if take:
                                ms[op].append(t)
                        t, _ = timed(lambda: dst.copy_(src, non_blocking=True), null)
                        if take:
                            ms["memcpy"].append(t)
                    assert totals["abs_max"] == want["abs_max"], (kind, name, totals, want)
                    assert abs(totals["sum"] - want["sum"]) <= 1e-9 * float(np.abs(H.data).astype(np.float64).sum()), (kind, name)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    nbytes = H.nnz * H.data.itemsize
                    rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, nnz=H.nnz,
                               tiles=info.tiles, rows_split=info.rows_split, rows_empty=info.rows_empty, rounds=args.rounds,
                               memcpy_data_ms=med["memcpy"], memcpy_min_max=(min(ms["memcpy"]), max(ms["memcpy"])),
                               memcpy_hbm_frac=2 * nbytes / (med["memcpy"] * 1e-3) / 1e9 / HBM_PEAK_GBS)
                    for op in OPS:
                        rec[op] = dict(ms=med[op], min_max=(min(ms[op]), max(ms[op])), vs_memcpy_data=med[op] / med["memcpy"])
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                    del src, dst, out
                dS.reset()
                dP.reset()
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
