"""Time speck_spmv_sr_* / speck_spmm_sr_* against speck_spmv_*, against themselves column by column, and against the route
a torch user has today.

Inputs, from the stand-ins at scale 1.0, fp64 and fp32: scircuit S, cant S S, webbase S S (the products made on the device).
  (a) spmv_sr(min_plus) against spmv on the same A and x: the same bytes, the same gathers, the same walk -- spmv.hip is
      not touched by the semiring code, so it is the baseline that is not the code under test;
  (b) spmm_sr(min_plus) with k in {2, 8, 32} against k calls of spmv_sr on contiguous columns;
  (c) both against torch: full(rows, inf).scatter_reduce(0, row, val + x[col], "amin") -- the int64 row index of every
      entry and the int64 column ids are built OUTSIDE the timed region; skipped, and said so, where the terms alone
      would take more than --torch-bytes;
  (d) one whole sssp loop (speck_amd.sssp, 8 sources) on scircuit S with weights |a| + 0.1 against the same loop built
      from (c), both ending with the distances on the host; the two results are compared for equality.
Protocol as scripts/spmv_time.py: warm-up; device events around the whole call (ours: on the config's stream, the call
returns complete, so the events span its read-back; torch: on the NULL stream); ALTERNATING rounds, median (min - max)
per column.  (d) is timed with the host clock around calls that end in a download, --loop-rounds rounds after one warm-up.

    python scripts/semiring_time.py [--rounds 7] [--loop-rounds 7] [--parts a,b,d] [--out FILE]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speck_amd as sa  # noqa: E402

KS = (2, 8, 32)
INPUTS = (("scircuit", "S"), ("cant", "SS"), ("webbase", "SS"))


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v)) if v else None


def torch_sssp(row, col, w, n, sources, dev, max_iters):
    """speck_amd.sssp built from scatter_reduce: the same loop, the same stop"""
    k = len(sources)
    D = torch.full((n, k), float("inf"), dtype=torch.float64, device=dev)
    D[torch.as_tensor(sources, device=dev), torch.arange(k, device=dev)] = 0.0
    rows_k = row[:, None].expand(-1, k)
    iterations = 0
    while iterations < max_iters:
        new = D.scatter_reduce(0, rows_k, w[:, None] + D[col], "amin", include_self=True)
        iterations += 1
        changed = bool((new != D).any().item())
        D = new
        if not changed:
            break
    return D.cpu().numpy(), iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,d", help="which of a (with c), b (with c) and d to run")
    ap.add_argument("--torch-bytes", type=float, default=4e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semiring.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("semiring_time.py needs a GPU")
    parts = set(args.parts.split(","))
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

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

        def ours(fn):
            cfg.set_stream(s.cuda_stream)
            try:
                return timed(fn, s)
            finally:
                cfg.set_stream(None)

        for kind, which in INPUTS:
            if not parts & {"a", "b"} and kind != "scircuit":
                continue
            for dtype in (np.float64, np.float32):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dS = sa.dCSR.from_host(S)
                dA = dS
                if which == "SS":
                    dA = sa.dCSR(dtype)
                    sa.MultiplyspECK(dS, dS, dA, cfg)
                H = dA.to_host()
                rows, cols, nnz = H.rows, H.cols, H.nnz
                rng = np.random.default_rng(1)
                X_host = rng.uniform(-1.0, 1.0, size=(cols, max(KS)))
                X = torch.from_numpy(X_host).to(dev)
                x = X[:, 0].contiguous()
                y = torch.zeros(max(rows, 1), dtype=torch.float64, device=dev)
                # (the torch route's indices: outside the timed region)
                row = torch.from_numpy(np.repeat(np.arange(rows, dtype=np.int64), np.diff(H.row_offsets.astype(np.int64)))).to(dev)
                col = torch.from_numpy(H.col_ids.astype(np.int64)).to(dev)
                val = torch.from_numpy(H.data.astype(np.float64)).to(dev)
                torch.cuda.synchronize()

                def torch_v():
                    return torch.full((rows,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(
                        0, row, val + x[col], "amin", include_self=True)

                ms = {"spmv_sr": [], "spmv": [], "torch": []}
                for r in range(args.warmup + args.rounds if "a" in parts else 0):
                    take = r >= args.warmup
                    for name, fn, mine in (("spmv_sr", lambda: sa.spmv_sr(dA, x, cfg, "min_plus", y=y), True),
                                           ("spmv", lambda: sa.spmv(dA, x, cfg, y=y), True), ("torch", torch_v, False)):
                        t, out = ours(fn) if mine else timed(fn, null)
                        if take:
                            ms[name].append(t)
                sa.spmv_sr(dA, x, cfg, "min_plus", y=y)
                assert np.array_equal(y.cpu().numpy()[:rows], torch_v().cpu().numpy()), (kind, "vector")
                rec = None if "a" not in parts else dict(part="a,c", kind=kind, matrix=which, dtype=np.dtype(dtype).name, rows=rows, cols=cols, nnz=nnz,
                           rounds=args.rounds, spmv_sr_ms=summary(ms["spmv_sr"]), spmv_ms=summary(ms["spmv"]),
                           torch_ms=summary(ms["torch"]))
                if rec:
                    rec["sr_vs_spmv"] = rec["spmv_sr_ms"]["median"] / rec["spmv_ms"]["median"]
                    rec["ranges_overlap"] = rec["spmv_sr_ms"]["min"] <= rec["spmv_ms"]["max"] and rec["spmv_ms"]["min"] <= rec["spmv_sr_ms"]["max"]
                    rec["sr_vs_torch"] = rec["spmv_sr_ms"]["median"] / rec["torch_ms"]["median"]
                    emit(rec)

                for k in KS if "b" in parts else ():
                    Xk = X[:, :k].contiguous()
                    xc = [X[:, c].contiguous() for c in range(k)]
                    Y = torch.zeros((max(rows, 1), k), dtype=torch.float64, device=dev)
                    yc = [torch.zeros(max(rows, 1), dtype=torch.float64, device=dev) for _ in range(k)]
                    with_torch = nnz * k * 8.0 <= args.torch_bytes
                    rows_k = row[:, None].expand(-1, k)

                    def by_column():
                        for c in range(k):
                            sa.spmv_sr(dA, xc[c], cfg, "min_plus", y=yc[c])

                    def torch_b():
                        return torch.full((rows, k), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(
                            0, rows_k, val[:, None] + Xk[col], "amin", include_self=True)

                    ms = {"spmm_sr": [], "k_spmv_sr": [], "torch": []}
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        t, _ = ours(lambda: sa.spmm_sr(dA, Xk, cfg, "min_plus", Y=Y[:rows] if rows else Y))
                        if take:
                            ms["spmm_sr"].append(t)
                        t, _ = ours(by_column)
                        if take:
                            ms["k_spmv_sr"].append(t)
                        if with_torch:
                            t, _ = timed(torch_b, null)
                            if take:
                                ms["torch"].append(t)
                    got = Y.cpu().numpy()[:rows]
                    assert all(np.array_equal(got[:, c], yc[c].cpu().numpy()[:rows]) for c in range(k)), (kind, k)
                    rec = dict(part="b,c", kind=kind, matrix=which, dtype=np.dtype(dtype).name, k=k, nnz=nnz, rounds=args.rounds,
                               spmm_sr_ms=summary(ms["spmm_sr"]), k_spmv_sr_ms=summary(ms["k_spmv_sr"]), torch_ms=summary(ms["torch"]))
                    rec["spmm_vs_k_spmv"] = rec["spmm_sr_ms"]["median"] / rec["k_spmv_sr_ms"]["median"]
                    if with_torch:
                        assert np.array_equal(got, torch_b().cpu().numpy()), (kind, k, "torch")
                        rec["spmm_vs_torch"] = rec["spmm_sr_ms"]["median"] / rec["torch_ms"]["median"]
                    else:
                        rec["torch_skipped"] = f"the terms alone take {nnz * k * 8.0 / 1e9:.1f} GB, more than {args.torch_bytes / 1e9:.1f} GB"
                    emit(rec)
                    del Xk, xc, Y, yc, rows_k

                if kind == "scircuit" and "d" in parts:
                    # (d) the whole loop; row i of the operand holds the in-edges of i: S as it stands, with positive weights
                    W = sa.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, (np.abs(H.data.astype(np.float64)) + 0.1).astype(dtype))
                    dW = sa.dCSR.from_host(W)
                    w = torch.from_numpy(W.data.astype(np.float64)).to(dev)
                    sources = [int(v) for v in np.linspace(0, rows - 1, 8).astype(np.int64)]
                    ms = {"sssp": [], "torch": []}
                    for r in range(1 + args.loop_rounds):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        dist, iterations, converged = sa.sssp(dW, sources, cfg)
                        t1 = time.perf_counter()
                        ref, ref_iterations = torch_sssp(row, col, w, rows, sources, dev, rows)
                        t2 = time.perf_counter()
                        if r:
                            ms["sssp"].append((t1 - t0) * 1e3)
                            ms["torch"].append((t2 - t1) * 1e3)
                    assert converged and iterations == ref_iterations and np.array_equal(dist, ref), "sssp against the torch loop"
                    rec = dict(part="d", kind=kind, matrix=which, dtype=np.dtype(dtype).name, sources=len(sources), iterations=iterations,
                               reached=int(np.isfinite(dist).sum()), rounds=args.loop_rounds, sssp_ms=summary(ms["sssp"]), torch_ms=summary(ms["torch"]))
                    rec["sssp_vs_torch"] = rec["sssp_ms"]["median"] / rec["torch_ms"]["median"]
                    emit(rec)
                    dW.reset()
                del X, x, y, row, col, val
                if dA is not dS:
                    dA.reset()
                dS.reset()
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
