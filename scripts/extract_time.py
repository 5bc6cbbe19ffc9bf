"""Time speck_extract_f64 / _f32 (C = A(p, q): rows gathered by a device index list, columns renumbered or dropped by a
device map) against its floor, against the route that existed before it and against torch.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32, int64 indices: scircuit S, cant S S and webbase S S (the
products made on the device; all square).  Cases, per input:
  row_perm      A[perm]: a row permutation alone, no map;
  sym_perm      A[perm][:, perm]: the map is the inverse permutation;
  induced_10    A[nodes][:, nodes] on a random 10 % of the vertices, renumbered;
  induced_50    ... on 50 %;
  sampled       A[rows], rows drawn with replacement (as many as A has), no map.
Per case, in the same rounds on the same box:
  a  extract    speck_extract_* into a matrix that exists (the buffers are reused, as in a training loop); the index and the
                map are ready (the one scatter that makes the map is timed apart: `map_build`);
  b  copies     device-to-device copies of the bytes the call must move: the gathered ids and values in (gross entries),
                C's three arrays out;
  c  route      what a caller could do before: for a list without repeats speck_to_coo, the inverse row and column maps applied
                with torch, a mask, speck_from_coo_* (which sorts by row: stable, so the bytes are extract's); for the list with
                repeats the gather arithmetic in torch (lengths, cumsum, repeat_interleave) in front of speck_from_coo_* on
                row ids that are in order.  A's arrays as torch tensors are made outside the timed region; torch's stream is
                drained in front of speck_from_coo_*, which runs on the config's;
  d  torch      torch.index_select on a coalesced sparse COO tensor of A, dim 0 and -- where columns are selected -- dim 1, and
                the same on a sparse CSR tensor where this torch build serves it; otherwise the record says why not.  An item
                that takes more than --slow-ms in the warm-up is timed in the warm-up only (`rounds: 1`).
Protocol (that of scripts/from_coo_time.py): warm-up; device events around the whole timed item -- a on the config's stream,
the rest on the NULL stream; every speck call returns with its result complete, so the events span the read-backs; 7
ALTERNATING rounds, median (min - max) per column.  a and c must agree byte for byte: asserted.  Neither side sorts the rows
by column (sort_rows would come on top of both).

    python scripts/extract_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--scale 1.0] [--rounds 7] [--out FILE]
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
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extract_time.py needs a GPU")
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
                assert H.rows == H.cols
                # A as torch tensors (outside every timed region)
                ro_t = torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev)
                col_t = torch.from_numpy(H.col_ids.astype(np.int64)).to(dev)
                val_t = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                row_t = torch.repeat_interleave(torch.arange(n, device=dev), ro_t[1:] - ro_t[:-1])
                coo = torch.sparse_coo_tensor(torch.stack([row_t, col_t]), val_t, size=(n, n)).coalesce()
                try:
                    csr = torch.sparse_csr_tensor(ro_t, col_t, val_t, size=(n, n))
                except (RuntimeError, NotImplementedError):
                    csr = None
                g = torch.Generator(device=dev)
                g.manual_seed(7)
                perm = torch.randperm(n, device=dev, generator=g)
                cases = [("row_perm", perm, None), ("sym_perm", perm, perm), ("induced_10", perm[:n // 10].contiguous(), "nodes"),
                         ("induced_50", perm[:n // 2].contiguous(), "nodes"),
                         ("sampled", torch.randint(0, n, (n,), device=dev, generator=g), None)]
                base = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=n, cols=n, nnz=nnz,
                            rounds=args.rounds, ids="int64")
                for case, rows, colsel in cases:
                    colsel = rows if isinstance(colsel, str) else colsel
                    k = int(rows.shape[0])
                    out_cols = n if colsel is None else int(colsel.shape[0])
                    for _ in range(2):                                      # (the second time: torch's kernels are loaded)
                        t_map, built = timed(lambda: sa.api._inverse_map(colsel, n, "extract_time", "cols") if colsel is not None else None, null)
                    cmap = built[0] if built is not None else None
                    C = sa.dCSR(dtype)
                    _, info = sa.extract(dA, rows=rows, col_map=cmap, out_cols=out_cols, config=cfg, matOut=C)
                    # ---- b: the bytes
                    in_col, in_val = torch.empty(info.gross, dtype=torch.int32, device=dev), torch.empty(info.gross, dtype=val_t.dtype, device=dev)
                    out_col, out_val = torch.empty(info.nnz_out, dtype=torch.int32, device=dev), torch.empty(info.nnz_out, dtype=val_t.dtype, device=dev)
                    out_ro = torch.empty(k + 1, dtype=torch.int32, device=dev)
                    twins = [torch.empty_like(t) for t in (in_col, in_val, out_col, out_val, out_ro)]

                    def copies():
                        for dst, src in zip(twins, (in_col, in_val, out_col, out_val, out_ro)):
                            dst.copy_(src)

                    # ---- c: the route that existed
                    repeats = case == "sampled"
                    R = sa.dCSR(dtype)
                    if not repeats:
                        inv_row = torch.full((n,), -1, dtype=torch.int64, device=dev)
                        inv_row[rows] = torch.arange(k, device=dev)

                    def route():
                        if repeats:
                            glen = ro_t[rows + 1] - ro_t[rows]
                            G = torch.cumsum(glen, 0)
                            src = torch.repeat_interleave(ro_t[rows] - (G - glen), glen) + torch.arange(int(G[-1]), device=dev)
                            new_row = torch.repeat_interleave(torch.arange(k, device=dev), glen)
                            torch.cuda.current_stream().synchronize()   # (the config's stream is not torch's)
                            return sa.from_coo(new_row, col_t[src], val_t[src], (k, out_cols), cfg, matOut=R)
                        row, col = sa.to_coo(dA, cfg)
                        new_row = inv_row[row]
                        new_col = cmap[col] if cmap is not None else col
                        keep = (new_row >= 0) & (new_col >= 0)
                        new_row, new_col, new_val = new_row[keep], new_col[keep], val_t[keep]
                        torch.cuda.current_stream().synchronize()
                        return sa.from_coo(new_row, new_col, new_val, (k, out_cols), cfg, matOut=R)

                    # ---- d: torch
                    def select_on(t):
                        out = torch.index_select(t, 0, rows)
                        return torch.index_select(out, 1, colsel) if colsel is not None else out

                    torch_items, torch_errors = {}, {}
                    for label, t in (("torch_coo", coo), ("torch_csr", csr)):
                        try:
                            if t is None:
                                raise NotImplementedError("torch.sparse_csr_tensor is not served")
                            t_first, _ = timed(lambda: select_on(t), null)
                            t_first, _ = timed(lambda: select_on(t), null)
                            torch_items[label] = (t, t_first)
                        except (RuntimeError, NotImplementedError) as err:
                            torch_errors[label] = str(err).splitlines()[0][:160]
                    torch.cuda.synchronize()
                    ms = {key: [] for key in ("a", "b", "c", "torch_coo", "torch_csr")}
                    for label, (t, t_first) in torch_items.items():
                        if t_first > args.slow_ms:
                            ms[label].append(t_first)
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        cfg.set_stream(s.cuda_stream)
                        ta, _ = timed(lambda: sa.extract(dA, rows=rows, col_map=cmap, out_cols=out_cols, config=cfg, matOut=C), s)
                        cfg.set_stream(None)
                        tb, _ = timed(copies, null)
                        tc, _ = timed(route, null)
                        if take:
                            ms["a"].append(ta), ms["b"].append(tb), ms["c"].append(tc)
                        for label, (t, t_first) in torch_items.items():
                            if t_first <= args.slow_ms:
                                td, _ = timed(lambda: select_on(t), null)
                                if take:
                                    ms[label].append(td)
                    G, W = C.to_host(), R.to_host()
                    assert G.row_offsets.tobytes() == W.row_offsets.tobytes(), (kind, name, case)
                    assert G.col_ids.tobytes() == W.col_ids.tobytes(), (kind, name, case)
                    assert G.data.tobytes() == W.data.tobytes(), (kind, name, case)
                    a, b, c = (statistics.median(ms[key]) for key in "abc")
                    rec = dict(base, case=case, rows_out=info.rows_out, gross=info.gross, nnz_out=info.nnz_out, map_build_ms=t_map if cmap is not None else None,
                               extract=stats(ms["a"]), copies=stats(ms["b"]), route=stats(ms["c"]), a_vs_copies=a / b, a_vs_route=a / c)
                    for label in ("torch_coo", "torch_csr"):
                        if label in torch_errors:
                            rec.update({label: None, label + "_error": torch_errors[label]})
                        else:
                            rec.update({label: stats(ms[label]), "a_vs_" + label: a / statistics.median(ms[label])})
                    emit(rec)
                    C.reset(), R.reset()
                    del in_col, in_val, out_col, out_val, out_ro, twins, torch_items
                    torch.cuda.empty_cache()
                dA.reset()
                del ro_t, col_t, val_t, row_t, coo, csr
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
