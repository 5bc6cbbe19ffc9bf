"""Time speck_spmv_f64 / _f32 against the bytes it must read and against the library path a user has today.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: S and the product S S (made on the device).  One call:
y = A x (alpha = 1, beta = 0) into a tensor that exists.  Yardsticks, on the same box in the same rounds:
  copy    a plain device-to-device copy of A's data array plus one of its col_ids into buffers that exist -- the bytes
          the call must read (a copy also writes as many; the product writes 8 rows bytes and gathers from x);
  torch   torch.sparse_csr_tensor(crow, col, values) @ x -- the conversion of the u32 offsets and ids to what torch
          takes stays OUTSIDE the timed region; for fp32 values torch wants x in fp32 too (speck keeps it in double).
Protocol: warm-up; device events around the whole call (spmv: on the config's stream, the call returns with y complete,
so the events span its read-back; the yardsticks: on the NULL stream they run on); repeated ALTERNATING rounds with the
median taken per column.  After the warm-up a spmv allocates nothing.

    python scripts/spmv_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
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
COLUMNS = ("spmv", "copy", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmv.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmv_time.py needs a GPU")
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
                    val = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                    col = torch.from_numpy(H.col_ids.astype(np.int32)).to(dev)
                    val2, col2 = torch.empty_like(val), torch.empty_like(col)
                    x_host = np.random.default_rng(1).uniform(-1.0, 1.0, size=H.cols)
                    x = torch.from_numpy(x_host).to(dev)
                    y = torch.zeros(max(H.rows, 1), dtype=torch.float64, device=dev)
                    # (the index conversion of the torch path: outside the timed region)
                    At = torch.sparse_csr_tensor(torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev),
                                                 torch.from_numpy(H.col_ids.astype(np.int64)).to(dev), val, size=(H.rows, H.cols))
                    xt = x.to(val.dtype)
                    try:  # (a torch build without the sparse CSR product: the column stays empty and the record says why)
                        At @ xt
                        torch_error = None
                    except RuntimeError as err:
                        torch_error = str(err).splitlines()[0][:120]
                    torch.cuda.synchronize()

                    def copies():
                        val2.copy_(val, non_blocking=True)
                        col2.copy_(col, non_blocking=True)

                    ms = {k: [] for k in COLUMNS}
                    yt = None
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        cfg.set_stream(s.cuda_stream)
                        t, (_, info) = timed(lambda: sa.spmv(dA, x, cfg, y=y), s)
                        cfg.set_stream(None)
                        if take:
                            ms["spmv"].append(t)
                        t, _ = timed(copies, null)
                        if take:
                            ms["copy"].append(t)
                        if torch_error is None:
                            t, yt = timed(lambda: At @ xt, null)
                            if take:
                                ms["torch"].append(t)
                    got = y.cpu().numpy()[:H.rows]
                    # (a sanity check of both paths against each other, within the bound of any order: not the test)
                    row = np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))
                    mag = np.bincount(row, weights=np.abs(H.data.astype(np.float64) * x_host[H.col_ids.astype(np.int64)]), minlength=H.rows)
                    tol = 1e-11 if dtype == np.float64 else 1e-3
                    if yt is not None:
                        assert (np.abs(got - yt.cpu().numpy().astype(np.float64)) <= tol * mag + 1e-300).all(), (kind, name)
                    med = {k: statistics.median(v) if v else None for k, v in ms.items()}
                    nbytes = H.nnz * (H.data.itemsize + 4)
                    rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols,
                               nnz=H.nnz, tiles=info.tiles, rows_split=info.rows_split, rows_empty=info.rows_empty,
                               rounds=args.rounds, read_bytes=nbytes,
                               spmv_ms=med["spmv"], spmv_min_max=(min(ms["spmv"]), max(ms["spmv"])),
                               spmv_read_hbm_frac=nbytes / (med["spmv"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               copy_ms=med["copy"], copy_min_max=(min(ms["copy"]), max(ms["copy"])),
                               vs_copy=med["spmv"] / med["copy"])
                    if torch_error is None:
                        rec.update(torch_ms=med["torch"], torch_min_max=(min(ms["torch"]), max(ms["torch"])),
                                   vs_torch=med["spmv"] / med["torch"])
                    else:
                        rec.update(torch_ms=None, torch_error=torch_error)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                    del val, col, val2, col2, x, y, At, xt, yt
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
