"""Time speck_sddmm_f64 / _f32 (in place, alpha = 1, beta = 0) against speck_spmm_* at the same k, against torch, and
record the ratio to spmm plainly.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: S and the product S S (made on the device), and
k in {1, 8, 32, 128}.  U (rows x k) and V (cols x k) are contiguous float64 tensors that exist.
Yardsticks, on the same box in the same rounds:
  spmm    speck_spmm_*(A, V) into a (rows, k) tensor that exists: the same gathers V[id, :] of k doubles per entry (it
          reads A's values beside them and writes rows x k doubles, sddmm reads U[row, :] and writes nnz values);
  gather  (U[row] * V[col]).sum(1) in torch, with the int64 `row` and `col` built OUTSIDE the timed region: it
          materialises nnz x k doubles, so it is skipped, and the record says so, where that exceeds --gather-limit bytes;
  addmm   torch.sparse.sampled_addmm(A_csr, U, V^T, beta = 0) where this torch build serves CSR on the device; where it
          does not, the error text is recorded instead.  The conversion of the u32 offsets and ids stays outside too.
Protocol (that of scripts/spmm_time.py): warm-up; device events around the whole timed item (sddmm and spmm: on the
config's stream, a call returns with its result complete, so the events span the read-back; the yardsticks: on the NULL
stream they run on); repeated ALTERNATING rounds, the median (min - max) per column.  After the warm-up no call allocates.
No threshold: what is found is recorded, the losses included.

--columns sddmm times the call alone: that is how a library built with another L(k) (SPECK_LIB=...)
is compared on the same inputs.

    python scripts/sddmm_time.py [--kinds scircuit,cant,webbase] [--matrices S,SS] [--ks 1,8,32,128] [--scale 1.0]
                                 [--rounds 7] [--columns sddmm,spmm,gather,addmm] [--tag TEXT] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--matrices", default="S,SS")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--ks", default="1,8,32,128")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--columns", default="sddmm,spmm,gather,addmm")
    ap.add_argument("--gather-limit", type=float, default=4e9)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sddmm_time.py needs a GPU")
    ks = [int(k) for k in args.ks.split(",")]
    columns = args.columns.split(",")
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
            for dtype in (np.dtype(d).type for d in args.dtypes.split(",")):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dS, dP = sa.dCSR.from_host(S), sa.dCSR(dtype)
                if "SS" in args.matrices.split(","):
                    sa.MultiplyspECK(dS, dS, dP, cfg)
                for name, dA in (("S", dS), ("SS", dP)):
                    if name not in args.matrices.split(","):
                        continue
                    H = dA.to_host()
                    row_host = np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))
                    want_torch = "gather" in columns or "addmm" in columns
                    if want_torch:      # (the index conversions of the torch paths: outside the timed region)
                        row = torch.from_numpy(row_host).to(dev)
                        col = torch.from_numpy(H.col_ids.astype(np.int64)).to(dev)
                        val = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                        At = torch.sparse_csr_tensor(torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev), col, val,
                                                     size=(H.rows, H.cols))
                    for k in ks:
                        rng = np.random.default_rng(k)
                        U_host = rng.uniform(-1.0, 1.0, size=(H.rows, k))
                        V_host = rng.uniform(-1.0, 1.0, size=(H.cols, k))
                        U, V = torch.from_numpy(U_host).to(dev), torch.from_numpy(V_host).to(dev)
                        Y = torch.zeros((max(H.rows, 1), k), dtype=torch.float64, device=dev)
                        dW = dA.copy()                                  # sddmm works in place on a copy: A stays for spmm
                        gather_note = addmm_error = None
                        if "gather" in columns and H.nnz * k * 8 > args.gather_limit:
                            gather_note = f"skipped: nnz x k doubles = {H.nnz * k * 8 / 1e9:.1f} GB"
                        if "addmm" in columns:
                            Ut, Vt = U.to(val.dtype), V.to(val.dtype).t()
                            try:  # (a torch build without it for CSR on the device: the record says why)
                                torch.sparse.sampled_addmm(At, Ut, Vt, beta=0.0)
                            except (RuntimeError, NotImplementedError) as err:
                                addmm_error = str(err).splitlines()[0][:160]
                        torch.cuda.synchronize()
                        ms = {n: [] for n in columns}
                        info = g = None
                        for r in range(args.warmup + args.rounds):
                            take = r >= args.warmup
                            cfg.set_stream(s.cuda_stream)
                            t, (_, info) = timed(lambda: sa.sddmm(dW, U, V, cfg, inplace=True), s)
                            if take:
                                ms["sddmm"].append(t)
                            if "spmm" in columns:
                                t, _ = timed(lambda: sa.spmm(dA, V, cfg, Y=Y), s)
                                if take:
                                    ms["spmm"].append(t)
                            cfg.set_stream(None)
                            if "gather" in columns and gather_note is None:
                                t, g = timed(lambda: (U[row] * V[col]).sum(1), null)
                                if take:
                                    ms["gather"].append(t)
                            if "addmm" in columns and addmm_error is None:
                                t, _ = timed(lambda: torch.sparse.sampled_addmm(At, Ut, Vt, beta=0.0), null)
                                if take:
                                    ms["addmm"].append(t)
                        # a sanity check on the timed data, not the test: torch's sum within the bound of any order
                        got = dW.to_host().data.astype(np.float64)
                        if g is not None:
                            tol = 1e-11 if dtype == np.float64 else 1e-5
                            mag = (np.abs(U_host[row_host[:100000]]) * np.abs(V_host[H.col_ids[:100000].astype(np.int64)])).sum(1)
                            assert (np.abs(got[:100000] - g.cpu().numpy()[:100000]) <= tol * mag + 1e-300).all(), (kind, name, k)
                        rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols,
                                   nnz=H.nnz, k=k, lanes=info.lanes, tiles=info.tiles, terms=info.terms, rounds=args.rounds,
                                   gathered_bytes=2 * 8 * k * H.nnz)
                        if args.tag:
                            rec["tag"] = args.tag
                        for n in columns:
                            v = ms[n]
                            rec[n + "_ms"] = statistics.median(v) if v else None
                            if v:
                                rec[n + "_min_max"] = (min(v), max(v))
                                if n != "sddmm":
                                    rec["vs_" + n] = rec["sddmm_ms"] / rec[n + "_ms"]
                        if gather_note:
                            rec["gather_note"] = gather_note
                        if addmm_error:
                            rec["addmm_error"] = addmm_error
                        line = json.dumps(rec)
                        print(line, flush=True)
                        lines.append(line)
                        del U, V, Y, dW, g
                        torch.cuda.empty_cache()
                    if want_torch:
                        del row, col, val, At
                dS.reset()
                dP.reset()
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a" if args.tag else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
