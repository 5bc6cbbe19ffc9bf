"""Time speck_sample_f64 / _f32 (k random neighbours per row, without replacement) against the route that existed before it,
against a torch-only route and against its floor.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32: scircuit S, cant S S and webbase S S (the products made
on the device).  Per input, k in 4, 32, all rows and a list of 10 % of the rows (a random permutation's head, int64), in the
same rounds on the same box:
  a  sample   speck_sample_* into a matrix that exists (the buffers are reused, as from step to step), info included;
  b  route    what a caller could do before: speck_extract_* of the rows (into torch buffers; all rows: the matrix itself,
              nothing is extracted), a twin of it whose values are random keys -- 20 random bits above the entry's position
              in the mantissa of a double in [1, 2), made with torch --, speck_topk_* of the twin, the original values
              gathered back through the positions the kept keys carry.  Result: offsets and ids in a matrix, values in a
              tensor;
  c  torch    torch alone, then speck_from_coo_*: the gathered entries' rows and sources from the offsets, torch.rand keys, a
              stable sort by key and one by row, the rank inside the row, a mask, the kept entries put back in order;
  d  copies   device-to-device copies of the bytes the OUTPUT holds: C's three arrays.
  e  draws    speck_sample_* with replacement, alone (no route is compared).
Protocol (that of scripts/topk_time.py): warm-up; device events around the whole timed item -- a and e on the config's stream,
the rest on the NULL stream; every speck call returns with its result complete, so the events span the read-backs; 7
ALTERNATING rounds, median (min - max) per column.  The three samples differ (other keys); what is asserted: a is the numpy
statement's sample where the input is small enough to restate, and b and c give a's row lengths.
Every record carries the class split of the gathered rows: copied whole (<= k entries), ranked by a lane group
(<= SAMPLE_GROUP_MAX), selected in LDS (<= SAMPLE_LDS_MAX) and selected with recomputed keys.

    python scripts/sample_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--ks 4,32] [--row-lists all,tenth] [--scale 1.0] [--rounds 7]\
        [--only-sample] [--out FILE]
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
from speck_amd import _lib  # noqa: E402


def class_split(lens, k):
    edges = (("copied", lens <= k), ("group", (lens > k) & (lens <= sa.SAMPLE_GROUP_MAX)),
             ("lds", (lens > k) & (lens > sa.SAMPLE_GROUP_MAX) & (lens <= sa.SAMPLE_LDS_MAX)), ("long", (lens > k) & (lens > sa.SAMPLE_LDS_MAX)))
    return {name: dict(rows=int(m.sum()), entries=int(lens[m].sum())) for name, m in edges}


def torch_matrix(rows, cols, nnz, dtype, dev, values=None):
    """a dCSR over torch buffers (a call whose result has these rows and entries reuses them): (matrix, offsets, ids, values)"""
    ro = torch.zeros(rows + 1, dtype=torch.int32, device=dev)
    ci = torch.zeros(max(nnz, 1), dtype=torch.int32, device=dev)
    va = torch.zeros(max(nnz, 1), dtype=torch.float64 if dtype == np.float64 else torch.float32, device=dev) if values is None else values
    return sa.dCSR.from_device(rows, cols, nnz, ro.data_ptr(), ci.data_ptr(), va.data_ptr(), dtype=dtype, keep=(ro, ci, va)), ro, ci, va


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="scircuit:S,cant:SS,webbase:SS")
    ap.add_argument("--ks", default="4,32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--row-lists", default="all,tenth", help="all: every row; tenth: a list of 10 % of the rows")
    ap.add_argument("--only-sample", action="store_true", help="time a alone (for a kernel trace of the call)")
    ap.add_argument("--restate-below", type=int, default=3_000_000, help="gathered entries up to which a is compared with numpy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_time.py needs a GPU")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_sample_host import numpy_sample
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
                all_lens = np.diff(H.row_offsets.astype(np.int64))
                ro_t = torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev)
                col_t = torch.from_numpy(H.col_ids.astype(np.int64)).to(dev)
                val_t = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                tenth = torch.randperm(n, generator=torch.Generator().manual_seed(7))[:max(n // 10, 1)].to(dev)
                base = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=n, cols=H.cols, nnz=nnz,
                            rounds=args.rounds, longest_row=int(all_lens.max()))
                for rows_name, rows_t in (("all", None), ("tenth", tenth)):
                    if rows_name not in args.row_lists.split(","):
                        continue
                    idx = np.arange(n) if rows_t is None else rows_t.cpu().numpy()
                    m = len(idx)
                    lens = all_lens[idx]
                    gross = int(lens.sum())
                    for k in (int(x) for x in args.ks.split(",")):
                        seed = 1000 + k
                        C, info = sa.sample_neighbors(dA, k, seed, rows=rows_t, cfg=cfg)
                        C_t = torch_matrix(m, H.cols, info.nnz_out, dtype, dev)        # a and e write into matrices that exist
                        D, dinfo = sa.sample_neighbors(dA, k, seed, rows=rows_t, replace=True, cfg=cfg)
                        D_t = torch_matrix(m, H.cols, dinfo.nnz_out, dtype, dev)
                        if gross <= args.restate_below:
                            want = numpy_sample(H.row_offsets, H.col_ids, H.data, k, seed, None if rows_t is None else idx)
                            G = C.to_host()
                            assert G.row_offsets.tobytes() == want[0].tobytes() and G.col_ids.tobytes() == want[1].tobytes(), (kind, name, k)
                            assert G.data.view(want[2].dtype).tobytes() == want[2].tobytes(), (kind, name, k)
                        want_lens = np.minimum(lens, k)

                        prm = _lib.CSampleParams()
                        prm.k, prm.seed, prm.n_rows, prm.index_bytes = k, seed, m, 8
                        prm.d_row_index = rows_t.data_ptr() if rows_t is not None else None
                        fn = _lib.load().speck_sample_f32 if dtype == np.float32 else _lib.load().speck_sample_f64
                        cinfo = _lib.CSampleInfo()

                        def sample(mode, out):
                            import ctypes
                            prm.mode = mode
                            rc = fn(cfg._h, ctypes.byref(dA._c), ctypes.byref(prm), ctypes.byref(out._c), ctypes.byref(cinfo))
                            assert rc == 0, rc

                        # ---- d: the bytes of the output
                        src = [torch.empty(info.nnz_out, dtype=torch.int32, device=dev), torch.empty(info.nnz_out, dtype=val_t.dtype, device=dev),
                               torch.empty(m + 1, dtype=torch.int32, device=dev)]
                        twins = [torch.empty_like(t) for t in src]

                        def copies():
                            for dst, t in zip(twins, src):
                                dst.copy_(t)

                        # ---- b: extract -> random keys that carry the position -> topk -> the values gathered back
                        if rows_t is None:
                            E, e_ro, e_ci, e_val = dA, None, None, val_t
                        else:
                            E, e_ro, e_ci, e_val = torch_matrix(m, H.cols, gross, dtype, dev)
                        keys = torch.empty(max(gross, 1), dtype=torch.float64, device=dev)
                        T, t_ro, t_ci, t_val = torch_matrix(m, H.cols, info.nnz_out, np.float64, dev)
                        at = torch.arange(max(gross, 1), dtype=torch.int64, device=dev)

                        def route():
                            if rows_t is not None:
                                sa.gather_rows(dA, rows_t, config=cfg, matOut=E)
                            rnd = torch.randint(0, 1 << 20, (max(gross, 1),), dtype=torch.int64, device=dev)
                            keys.view(torch.int64).copy_((rnd << 32) | at | 0x3FF0000000000000)
                            torch.cuda.current_stream().synchronize()               # (the config's stream is not torch's)
                            K = sa.dCSR.from_device(m, H.cols, gross, E._c.row_offsets, E._c.col_ids, keys.data_ptr(), dtype=np.float64)
                            sa.topk(K, k, by="largest", cfg=cfg, out=T)
                            pos = t_val.view(torch.int64)[:info.nnz_out] & 0xFFFFFFFF
                            return e_val[pos]

                        # ---- c: torch alone, then from_coo
                        R = sa.dCSR(dtype)
                        picks = torch.arange(n, device=dev) if rows_t is None else rows_t
                        span = torch.arange(m, device=dev)

                        def torch_route():
                            first = ro_t[picks]
                            glen = ro_t[picks + 1] - first
                            G0 = torch.cumsum(glen, 0) - glen
                            row = torch.repeat_interleave(span, glen)
                            src_at = (first - G0)[row] + torch.arange(gross, device=dev)
                            key = torch.rand(gross, device=dev, dtype=torch.float64)
                            a1 = torch.sort(key, stable=True).indices
                            a2 = torch.sort(row[a1], stable=True).indices
                            order = a1[a2]                                          # by row, inside it by key, inside that by position
                            rank = torch.arange(gross, device=dev) - G0[row[order]]
                            kept = torch.sort(order[rank < k]).values
                            new_row, new_col, new_val = row[kept], col_t[src_at[kept]], val_t[src_at[kept]]
                            torch.cuda.current_stream().synchronize()               # (the config's stream is not torch's)
                            return sa.from_coo(new_row, new_col, new_val, (m, H.cols), cfg, matOut=R)

                        ms = {key: [] for key in "abcde"}
                        for r in range(args.warmup + args.rounds):
                            take = r >= args.warmup
                            cfg.set_stream(s.cuda_stream)
                            ta, _ = timed(lambda: sample(0, C_t[0]), s)
                            te, _ = timed(lambda: sample(1, D_t[0]), s)
                            cfg.set_stream(None)
                            if take:
                                ms["a"].append(ta), ms["e"].append(te)
                            if args.only_sample:
                                continue
                            td, _ = timed(copies, null)
                            tb, _ = timed(route, null)
                            tc, _ = timed(torch_route, null)
                            if take:
                                ms["b"].append(tb), ms["c"].append(tc), ms["d"].append(td)
                        assert C_t[1].cpu().numpy().view(np.uint32).tobytes() == C.to_host().row_offsets.tobytes()   # the timed call is the checked one
                        assert C_t[2][:info.nnz_out].cpu().numpy().view(np.uint32).tobytes() == C.to_host().col_ids.tobytes()
                        rec = dict(base, row_list=rows_name, rows_out=m, k=k, gross=gross, rows_cut=info.rows_cut, nnz_out=info.nnz_out,
                                   nnz_out_draws=dinfo.nnz_out, classes=class_split(lens, k), sample=stats(ms["a"]), draws=stats(ms["e"]))
                        if not args.only_sample:
                            assert np.array_equal(np.diff(t_ro.cpu().numpy().astype(np.int64)), want_lens), (kind, name, k, "route")
                            assert np.array_equal(np.diff(R.to_host().row_offsets.astype(np.int64)), want_lens), (kind, name, k, "torch")
                            a = statistics.median(ms["a"])
                            rec.update(route=stats(ms["b"]), torch=stats(ms["c"]), copies=stats(ms["d"]), a_vs_route=a / statistics.median(ms["b"]),
                                       a_vs_torch=a / statistics.median(ms["c"]), a_vs_copies=a / statistics.median(ms["d"]))
                        emit(rec)
                        C.reset(), D.reset(), R.reset()
                        del src, twins, keys, at, C_t, D_t, T, t_ro, t_ci, t_val, E, e_ro, e_ci, e_val
                        torch.cuda.empty_cache()
                dA.reset()
                del ro_t, col_t, val_t
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
