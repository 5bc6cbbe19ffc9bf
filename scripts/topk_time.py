"""Time speck_topk_f64 / _f32 (C = the k entries of largest magnitude of every row) against the route that existed before
it, against its floor and against the filter with a threshold that is known in advance.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32: scircuit S, cant S S and webbase S S (the products made
on the device).  Per input and k in 4, 32, 256, by="abs", in the same rounds on the same box:
  a  topk     speck_topk_* into a matrix that exists (the buffers are reused, as in an MCL loop), info included;
  b  route    what a caller could do before: speck_to_coo, then torch -- a stable sort by key, a stable sort by row, the rank
              inside the row, a mask, the kept positions put back in order -- and speck_from_coo_*.  A's values as a torch
              tensor are made outside the timed region; torch's stream is drained in front of speck_from_coo_*;
  c  copies   device-to-device copies of the bytes that must move: A's three arrays read, C's three written;
  d  select   speck_select_* with a magnitude threshold chosen (on the host, outside the timed region) to keep about as
              many entries: the cost of the frame when the predicate is known in advance.
Protocol (that of scripts/extract_time.py): warm-up; device events around the whole timed item -- a and d on the config's
stream, the rest on the NULL stream; every speck call returns with its result complete, so the events span the
read-backs; 7 ALTERNATING rounds, median (min - max) per column.  a and b must agree byte for byte: asserted.
Every record carries the class split: the rows and entries that are copied whole (<= k entries), ranked by a lane group
(<= TOPK_GROUP_MAX), selected in LDS (<= TOPK_LDS_MAX) and selected from global memory.

    python scripts/topk_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--ks 4,32,256] [--scale 1.0] [--rounds 7] [--out FILE]
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


def class_split(lens, k):
    edges = (("copied", lens <= k), ("group", (lens > k) & (lens <= sa.TOPK_GROUP_MAX)),
             ("lds", (lens > k) & (lens > sa.TOPK_GROUP_MAX) & (lens <= sa.TOPK_LDS_MAX)), ("long", (lens > k) & (lens > sa.TOPK_LDS_MAX)))
    return {name: dict(rows=int(m.sum()), entries=int(lens[m].sum())) for name, m in edges}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="scircuit:S,cant:SS,webbase:SS")
    ap.add_argument("--ks", default="4,32,256")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--only-topk", action="store_true", help="time a alone (for a kernel trace of the call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

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

        def stats(v):
            return dict(ms=statistics.median(v), min_max=(min(v), max(v)), rounds=len(v)) if v else None

        for item in args.inputs.split(","):
            kind, name = item.split(":")
            for dtype in (np.dtype(d).type for d in args.dtypes.split(",")):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dA = sa.dCSR.from_host(S)
                if name == "SS":
                    dP = sa.dCSR(dtype)
                    sa.MultiplyspECK(dA, dA, dP, cfg)
                    dA = dP
                H = dA.to_host()
                n, nnz = H.rows, H.nnz
                lens = np.diff(H.row_offsets.astype(np.int64))
                ro_t = torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev)
                val_t = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                mags = np.sort(np.abs(H.data.astype(np.float64)))[::-1]
                base = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=n, cols=H.cols, nnz=nnz,
                            rounds=args.rounds, by="abs", longest_row=int(lens.max()))
                for k in (int(x) for x in args.ks.split(",")):
                    C, R, F = sa.dCSR(dtype), sa.dCSR(dtype), sa.dCSR(dtype)
                    _, info = sa.topk(dA, k, by="abs", cfg=cfg, out=C, return_info=True)
                    threshold = float(mags[info.nnz_out]) if info.nnz_out < nnz else -1.0
                    if threshold >= 0.0:
                        _, sel = sa.select(dA, cfg, abs_gt=threshold, matOut=F)
                    # ---- c: the bytes
                    src = [torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=val_t.dtype, device=dev),
                           torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(info.nnz_out, dtype=torch.int32, device=dev),
                           torch.empty(info.nnz_out, dtype=val_t.dtype, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev)]
                    twins = [torch.empty_like(t) for t in src]

                    def copies():
                        for dst, t in zip(twins, src):
                            dst.copy_(t)

                    # ---- b: the route that existed
                    def route():
                        row, col = sa.to_coo(dA, cfg)
                        first = torch.sort(val_t.abs(), descending=True, stable=True).indices
                        second = torch.sort(row[first], stable=True).indices
                        order = first[second]                                   # by row, inside it by key, inside that by position
                        rank = torch.arange(nnz, device=dev) - ro_t[row[order]]
                        kept = torch.sort(order[rank < k]).values
                        new_row, new_col, new_val = row[kept], col[kept], val_t[kept]
                        torch.cuda.current_stream().synchronize()               # (the config's stream is not torch's)
                        return sa.from_coo(new_row, new_col, new_val, (n, H.cols), cfg, matOut=R)

                    ms = {key: [] for key in "abcd"}
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        cfg.set_stream(s.cuda_stream)
                        ta, _ = timed(lambda: sa.topk(dA, k, by="abs", cfg=cfg, out=C, return_info=True), s)
                        td = timed(lambda: sa.select(dA, cfg, abs_gt=threshold, matOut=F), s)[0] if threshold >= 0.0 and not args.only_topk else None
                        cfg.set_stream(None)
                        if take:
                            ms["a"].append(ta)
                        if args.only_topk:
                            continue
                        tc, _ = timed(copies, null)
                        tb, _ = timed(route, null)
                        if take:
                            ms["b"].append(tb), ms["c"].append(tc)
                            if td is not None:
                                ms["d"].append(td)
                    rec = dict(base, k=k, rows_cut=info.rows_cut, nnz_out=info.nnz_out, ties_cut=info.ties_cut, classes=class_split(lens, k),
                               topk=stats(ms["a"]))
                    if not args.only_topk:
                        G, W = C.to_host(), R.to_host()
                        assert G.row_offsets.tobytes() == W.row_offsets.tobytes(), (kind, name, k)
                        assert G.col_ids.tobytes() == W.col_ids.tobytes(), (kind, name, k)
                        assert G.data.tobytes() == W.data.tobytes(), (kind, name, k)
                        a = statistics.median(ms["a"])
                        rec.update(route=stats(ms["b"]), copies=stats(ms["c"]), select=stats(ms["d"]), select_threshold=threshold,
                                   select_nnz_out=sel.nnz_out if threshold >= 0.0 else None, a_vs_route=a / statistics.median(ms["b"]),
                                   a_vs_copies=a / statistics.median(ms["c"]),
                                   a_vs_select=a / statistics.median(ms["d"]) if ms["d"] else None)
                    emit(rec)
                    C.reset(), R.reset(), F.reset()
                    del src, twins
                    torch.cuda.empty_cache()
                dA.reset()
                del ro_t, val_t
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
