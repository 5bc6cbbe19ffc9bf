"""Time speck_spmm_f64 / _f32 with k right-hand sides against k calls of speck_spmv_*, against torch, and against the bytes
that must move.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: S and the product S S (made on the device), and
k in {1, 2, 4, 8, 32}.  One call: Y = A X (alpha = 1, beta = 0) into a contiguous (rows, k) tensor that exists.
Yardsticks, on the same box in the same rounds:
  spmv    k calls of speck_spmv_* on contiguous copies of the k columns, each into a vector that exists -- what a user
          had before: k reads of A, 4 k launches, k read-backs;
  copy    plain device-to-device copies of A's data array, of its col_ids and of a rows x k block of doubles into buffers
          that exist -- the bytes the call must read from A plus those it must write (it also gathers from X);
  torch   torch.sparse_csr_tensor(crow, col, values) @ X -- the conversion of the u32 offsets and ids to what torch takes
          stays OUTSIDE the timed region; for fp32 values torch wants X in fp32 too (speck keeps it in double).
Protocol (that of scripts/spmv_time.py): warm-up; device events around the whole timed item (spmm and spmv: on the
config's stream, a call returns with its result complete, so the events span the read-backs; the yardsticks: on the NULL
stream they run on); repeated ALTERNATING rounds with the median taken per column.  After the warm-up no call allocates.

    python scripts/spmm_time.py [--kinds scircuit,cant,webbase] [--ks 1,2,4,8,32] [--scale 1.0] [--rounds 7] [--out FILE]
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

COLUMNS = ("spmm", "spmv", "copy", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--ks", default="1,2,4,8,32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmm_time.py needs a GPU")
    ks = [int(k) for k in args.ks.split(",")]
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
                    # (the index conversion of the torch path: outside the timed region)
                    At = torch.sparse_csr_tensor(torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev),
                                                 torch.from_numpy(H.col_ids.astype(np.int64)).to(dev), val, size=(H.rows, H.cols))
                    row = np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))
                    for k in ks:
                        X_host = np.random.default_rng(k).uniform(-1.0, 1.0, size=(H.cols, k))
                        X = torch.from_numpy(X_host).to(dev)
                        Y = torch.zeros((max(H.rows, 1), k), dtype=torch.float64, device=dev)
                        Y2 = torch.empty_like(Y)
                        xs = [X[:, c].contiguous() for c in range(k)]
                        ys = [torch.zeros(max(H.rows, 1), dtype=torch.float64, device=dev) for _ in range(k)]
                        Xt = X.to(val.dtype)
                        try:  # (a torch build without the sparse CSR product: the column stays empty and the record says why)
                            At @ Xt
                            torch_error = None
                        except RuntimeError as err:
                            torch_error = str(err).splitlines()[0][:120]
                        torch.cuda.synchronize()

                        def copies():
                            val2.copy_(val, non_blocking=True)
                            col2.copy_(col, non_blocking=True)
                            Y2.copy_(Y, non_blocking=True)

                        def k_spmvs():
                            for c in range(k):
                                sa.spmv(dA, xs[c], cfg, y=ys[c])

                        ms = {n: [] for n in COLUMNS}
                        Yt = None
                        for r in range(args.warmup + args.rounds):
                            take = r >= args.warmup
                            cfg.set_stream(s.cuda_stream)
                            t, (_, info) = timed(lambda: sa.spmm(dA, X, cfg, Y=Y), s)
                            t2, _ = timed(k_spmvs, s)
                            cfg.set_stream(None)
                            if take:
                                ms["spmm"].append(t)
                                ms["spmv"].append(t2)
                            t, _ = timed(copies, null)
                            if take:
                                ms["copy"].append(t)
                            if torch_error is None:
                                t, Yt = timed(lambda: At @ Xt, null)
                                if take:
                                    ms["torch"].append(t)
                        got = Y.cpu().numpy()[:H.rows]
                        # the defining property on the timed data, and torch within the bound of any order in the first and
                        # the last column: a sanity check, not the test
                        for c in range(k):
                            assert got[:, c].tobytes() == ys[c].cpu().numpy()[:H.rows].tobytes(), (kind, name, k, c)
                        tol = 1e-11 if dtype == np.float64 else 1e-3
                        if Yt is not None:
                            yt = Yt.cpu().numpy().astype(np.float64)
                            for c in sorted({0, k - 1}):
                                mag = np.bincount(row, weights=np.abs(H.data.astype(np.float64) * X_host[H.col_ids.astype(np.int64), c]),
                                                  minlength=H.rows)
                                assert (np.abs(got[:, c] - yt[:, c]) <= tol * mag + 1e-300).all(), (kind, name, k, c)
                        med = {n: statistics.median(v) if v else None for n, v in ms.items()}
                        rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols,
                                   nnz=H.nnz, k=k, tiles=info.tiles, rows_split=info.rows_split, terms=info.terms, rounds=args.rounds,
                                   moved_bytes=H.nnz * (H.data.itemsize + 4) + 8 * H.rows * k,
                                   spmm_ms=med["spmm"], spmm_min_max=(min(ms["spmm"]), max(ms["spmm"])),
                                   k_spmv_ms=med["spmv"], k_spmv_min_max=(min(ms["spmv"]), max(ms["spmv"])),
                                   vs_k_spmv=med["spmm"] / med["spmv"],
                                   copy_ms=med["copy"], copy_min_max=(min(ms["copy"]), max(ms["copy"])),
                                   vs_copy=med["spmm"] / med["copy"])
                        if torch_error is None:
                            rec.update(torch_ms=med["torch"], torch_min_max=(min(ms["torch"]), max(ms["torch"])),
                                       vs_torch=med["spmm"] / med["torch"])
                        else:
                            rec.update(torch_ms=None, torch_error=torch_error)
                        line = json.dumps(rec)
                        print(line, flush=True)
                        lines.append(line)
                        del X, Y, Y2, xs, ys, Xt, Yt
                    del val, col, val2, col2, At
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
