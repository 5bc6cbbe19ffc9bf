"""Time speck_spmm_t_f64 / _f32 (Y = A^T X through a ready transpose plan) against what existed before it, against its floor
and against torch.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32: scircuit S, cant S S and webbase S S (the products made
on the device), and k in {1, 8, 32}.  One call: Y = A^T X (alpha = 1, beta = 0) into a contiguous (cols, k) tensor that
exists.  Per input, in the same rounds on the same box:
  a  spmm_t     speck_spmm_t_* with a plan made outside the timed region;
  b  tr+spmm    what a caller had when the values change every step: speck_transpose_*(A), then speck_spmm_*(At, X), both
                inside the timed region (and the release of At);
  c  spmm(At)   the floor: speck_spmm_*(At, X) alone on a transpose made outside -- a minus c is the indirection and the check
                of the ids;
  d  plan, tr   speck_tplan_create against one speck_transpose_* (once per input, not per k);
  e  torch      torch.sparse_csr_tensor(A).t() @ X, where this torch build serves it (the index conversion outside the timed
                region; for fp32 values torch wants X in fp32 too); otherwise the record says why not.
Protocol (that of scripts/spmm_time.py): warm-up; device events around the whole timed item -- a and c on the config's
stream, the rest on the NULL stream the transpose works on; every speck call returns with its result complete, so the events
span the read-backs; 7 ALTERNATING rounds, median (min - max) per column.  a and b must agree byte for byte: asserted.

    python scripts/spmm_t_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--ks 1,8,32] [--scale 1.0] [--rounds 7] [--out FILE]
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
    ap.add_argument("--inputs", default="scircuit:S,cant:SS,webbase:SS")
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_t.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmm_t_time.py needs a GPU")
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

        def stats(v):
            return dict(ms=statistics.median(v), min_max=(min(v), max(v)))

        for item in args.inputs.split(","):
            kind, name = item.split(":")
            for dtype in (np.float64, np.float32):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dA = sa.dCSR.from_host(S)
                if name == "SS":
                    dP = sa.dCSR(dtype)
                    sa.MultiplyspECK(dA, dA, dP, cfg)
                    dA = dP
                H = dA.to_host()
                plan = sa.transpose_plan(dA, cfg)
                dAt = sa.transpose(dA, cfg)
                tA = torch.sparse_csr_tensor(torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev),
                                             torch.from_numpy(H.col_ids.astype(np.int64)).to(dev),
                                             torch.from_numpy(np.ascontiguousarray(H.data)).to(dev), size=(H.rows, H.cols))
                # d: the plan against one transpose
                ms_plan, ms_tr = [], []
                for r in range(args.warmup + args.rounds):
                    t, p = timed(lambda: sa.transpose_plan(dA, cfg), null)
                    p.free()
                    t2, At = timed(lambda: sa.transpose(dA, cfg), null)
                    At.reset()
                    if r >= args.warmup:
                        ms_plan.append(t)
                        ms_tr.append(t2)
                rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols, nnz=H.nnz,
                           item="plan", rounds=args.rounds, plan_bytes=plan.info.bytes, cols_empty=plan.info.cols_empty,
                           max_col_entries=plan.info.max_col_entries, tplan_create=stats(ms_plan), transpose=stats(ms_tr),
                           plan_vs_transpose=statistics.median(ms_plan) / statistics.median(ms_tr))
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
                for k in ks:
                    X = torch.from_numpy(np.random.default_rng(k).uniform(-1.0, 1.0, size=(H.rows, k))).to(dev)
                    Y = torch.zeros((max(H.cols, 1), k), dtype=torch.float64, device=dev)
                    Yb, Yc = torch.zeros_like(Y), torch.zeros_like(Y)
                    Xt = X.to(tA.dtype)
                    try:  # (a torch build without this product: the column stays empty and the record says why)
                        tA.t() @ Xt
                        torch_error = None
                    except (RuntimeError, NotImplementedError) as err:
                        torch_error = str(err).splitlines()[0][:160]
                    torch.cuda.synchronize()

                    def transpose_then_spmm():
                        At = sa.transpose(dA, cfg)
                        sa.spmm(At, X, cfg, Y=Yb)
                        At.reset()

                    ms = {n: [] for n in "abce"}
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        cfg.set_stream(s.cuda_stream)
                        ta, (_, info) = timed(lambda: sa.spmm_t(dA, X, cfg, plan=plan, Y=Y), s)
                        tc, _ = timed(lambda: sa.spmm(dAt, X, cfg, Y=Yc), s)
                        cfg.set_stream(None)
                        tb, _ = timed(transpose_then_spmm, null)
                        if take:
                            ms["a"].append(ta), ms["b"].append(tb), ms["c"].append(tc)
                        if torch_error is None:
                            te, _ = timed(lambda: tA.t() @ Xt, null)
                            if take:
                                ms["e"].append(te)
                    got = Y.cpu().numpy()
                    assert got.tobytes() == Yb.cpu().numpy().tobytes() == Yc.cpu().numpy().tobytes(), (kind, name, k)
                    a, b, c = (statistics.median(ms[n]) for n in "abc")
                    rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols,
                               nnz=H.nnz, item="product", k=k, tiles=info.tiles, cols_split=info.cols_split, terms=info.terms,
                               rounds=args.rounds, spmm_t=stats(ms["a"]), transpose_then_spmm=stats(ms["b"]),
                               spmm_on_ready_transpose=stats(ms["c"]), a_vs_b=a / b, a_vs_c=a / c)
                    if torch_error is None:
                        rec.update(torch=stats(ms["e"]), a_vs_torch=a / statistics.median(ms["e"]))
                    else:
                        rec.update(torch=None, torch_error=torch_error)
                    print(json.dumps(rec), flush=True)
                    lines.append(json.dumps(rec))
                    del X, Y, Yb, Yc, Xt
                plan.free()
                dAt.reset()
                dA.reset()
                del tA
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
