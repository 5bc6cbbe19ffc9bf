"""Time speck_from_coo_f64 / _f32 (device COO triplets -> device CSR) and speck_to_coo against their floor, against the same
sort in this tree and against torch.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32, int64 and int32 ids: scircuit S, cant S S and webbase S S
(the products made on the device), each as COO in three orders: row-sorted (what speck_to_coo gives), sorted by column, and
randomly permuted.  Per input and order, in the same rounds on the same box:
  a  from_coo   speck_from_coo_* into a matrix that exists (the buffers are reused, as in a training loop);
  b  copies     the floor: device-to-device copies of the three arrays;
  c  transpose  speck_transpose_* of the same matrix: the same radix sort in this tree, on column keys, with its own
                temporaries allocated and released inside;
  d  torch sort torch.sort(row, stable=True), two gathers, torch._convert_indices_from_coo_to_csr, and the casts to the
                32-bit offsets and ids this ABI takes -- inside the timed region, because that is what a caller pays;
  e  coalesce   torch.sparse_coo_tensor(...).coalesce().to_sparse_csr() where this torch build serves it (it also sorts the
                columns and sums duplicates: more work; the stand-ins have no duplicates); otherwise the record says why not.
And once per input:  f  to_coo  speck_to_coo (rows only, and rows with columns) against  g  torch.repeat_interleave of
arange(rows) on the row lengths (made outside the timed region).
Protocol (that of scripts/spmm_t_time.py): warm-up; device events around the whole timed item -- a and f on the config's
stream, the rest on the NULL stream; every speck call returns with its result complete, so the events span the read-backs;
7 ALTERNATING rounds, median (min - max) per column.  a and d must agree byte for byte: asserted.

    python scripts/from_coo_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--scale 1.0] [--rounds 7] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "from_coo.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("from_coo_time.py needs a GPU")
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
                n, shape = H.nnz, (H.rows, H.cols)
                val_sorted = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                lens = torch.from_numpy(np.diff(H.row_offsets.astype(np.int64))).to(dev)
                base = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols, nnz=n,
                            rounds=args.rounds)
                for index_dtype in (torch.int64, torch.int32):
                    ids = "int64" if index_dtype is torch.int64 else "int32"
                    row_sorted, col_sorted = sa.to_coo(dA, cfg, index_dtype=index_dtype)
                    # ---- f, g: the way out
                    ms = {k: [] for k in "fFg"}
                    arange = torch.arange(H.rows, device=dev, dtype=index_dtype)
                    for r in range(args.warmup + args.rounds):
                        cfg.set_stream(s.cuda_stream)
                        tf, _ = timed(lambda: sa.to_coo(dA, cfg, index_dtype=index_dtype, cols=False), s)
                        tF, _ = timed(lambda: sa.to_coo(dA, cfg, index_dtype=index_dtype), s)
                        cfg.set_stream(None)
                        tg, rep = timed(lambda: torch.repeat_interleave(arange, lens), null)
                        if r >= args.warmup:
                            ms["f"].append(tf), ms["F"].append(tF), ms["g"].append(tg)
                    assert torch.equal(rep, row_sorted)
                    emit(dict(base, item="to_coo", ids=ids, to_coo_rows=stats(ms["f"]), to_coo_rows_and_cols=stats(ms["F"]),
                              torch_repeat_interleave=stats(ms["g"]),
                              f_vs_g=statistics.median(ms["f"]) / statistics.median(ms["g"])))
                    # ---- a .. e: the way in
                    for order in ("row_sorted", "col_sorted", "random"):
                        if order == "row_sorted":
                            row, col, val = row_sorted, col_sorted, val_sorted
                        else:
                            g = torch.Generator(device=dev)
                            g.manual_seed(7)
                            p = torch.sort(col_sorted, stable=True).indices if order == "col_sorted" else torch.randperm(n, device=dev, generator=g)
                            row, col, val = row_sorted[p].contiguous(), col_sorted[p].contiguous(), val_sorted[p].contiguous()
                        C = sa.dCSR(dtype)
                        row2, col2, val2 = torch.empty_like(row), torch.empty_like(col), torch.empty_like(val)

                        def copies():
                            row2.copy_(row), col2.copy_(col), val2.copy_(val)

                        def torch_sort():
                            rs, p = torch.sort(row, stable=True)
                            crow = torch._convert_indices_from_coo_to_csr(rs.to(torch.int64), H.rows, out_int32=True)
                            return crow, col[p].to(torch.int32), val[p]

                        def torch_coalesce():
                            t = torch.sparse_coo_tensor(torch.stack([row, col]).to(torch.int64), val, size=shape)
                            return t.coalesce().to_sparse_csr()

                        try:
                            torch_coalesce()
                            coalesce_error = None
                        except (RuntimeError, NotImplementedError) as err:
                            coalesce_error = str(err).splitlines()[0][:160]
                        torch.cuda.synchronize()
                        ms = {k: [] for k in "abcde"}
                        for r in range(args.warmup + args.rounds):
                            take = r >= args.warmup
                            cfg.set_stream(s.cuda_stream)
                            ta, (_, info) = timed(lambda: sa.from_coo(row, col, val, shape, cfg, matOut=C), s)
                            cfg.set_stream(None)
                            tb, _ = timed(copies, null)
                            tc, At = timed(lambda: sa.transpose(dA, cfg), null)
                            At.reset()
                            td, ours = timed(torch_sort, null)
                            if take:
                                ms["a"].append(ta), ms["b"].append(tb), ms["c"].append(tc), ms["d"].append(td)
                            if coalesce_error is None:
                                te, _ = timed(torch_coalesce, null)
                                if take:
                                    ms["e"].append(te)
                        G = C.to_host()
                        assert G.row_offsets.tobytes() == ours[0].cpu().numpy().tobytes(), (kind, name, order)
                        assert G.col_ids.tobytes() == ours[1].cpu().numpy().tobytes(), (kind, name, order)
                        assert G.data.tobytes() == ours[2].cpu().numpy().tobytes(), (kind, name, order)
                        a, b, c, d = (statistics.median(ms[k]) for k in "abcd")
                        rec = dict(base, item="from_coo", ids=ids, order=order, sorted_input=info.sorted_input,
                                   sort_passes=info.sort_passes, from_coo=stats(ms["a"]), copies=stats(ms["b"]),
                                   transpose=stats(ms["c"]), torch_sort=stats(ms["d"]), a_vs_copies=a / b, a_vs_transpose=a / c,
                                   a_vs_torch_sort=a / d)
                        if coalesce_error is None:
                            rec.update(torch_coalesce=stats(ms["e"]), a_vs_torch_coalesce=a / statistics.median(ms["e"]))
                        else:
                            rec.update(torch_coalesce=None, torch_coalesce_error=coalesce_error)
                        emit(rec)
                        C.reset()
                        del row2, col2, val2, ours
                    del row_sorted, col_sorted
                dA.reset()
                del val_sorted, lens
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
