"""Time speck_bmat_f64 / _f32 (C = bmat(grid): a device CSR assembled from a grid of device CSR blocks) against its floor,
against the route that existed before it and against torch.

Inputs, from the stand-ins at scale 1.0 by default, fp64 and fp32:
  vstack8       vstack of the 8 row-range views (equal row counts) of webbase S S and of cant S S: the views share one set of
                buffers, every block row holds one block (the tile kernel takes whole blocks for its units);
  vstack8_pieces  the same bytes through the piece machinery: every block row also holds a block of 0 columns and no entry,
                so no tile may take the single-block path -- what that path saves;
  block_diag512 block_diag of 512 small scircuit-like graphs (64 generated at --small-scale with different seeds, each
                uploaded 8 times into buffers of its own);
  saddle        the 2 x 2 grid [[H, A^T], [A, 0]] on cant: H = S, A = the first quarter of S's rows.
Per case, in the same rounds on the same box:
  a  bmat       speck_bmat_* into a matrix that exists (the buffers are reused, as in a training loop), on descriptors that
                exist; `wrapper`: the same through speck_amd's Python wrapper, which builds the descriptors in every call;
  b  floor      speck_dcsr_copy of the finished matrix (`copy`), and device-to-device copies of the bytes the call must move:
                every block's ids and values in, C's three arrays out (`copies`);
  c  route      what a caller could do before: speck_to_coo per block (row_base = the block row's origin; a view as its copy,
                made outside the timed region), the column
                origin added with torch, torch.cat in (block row, block column) order, speck_from_coo_* (which sorts by row:
                stable, so the bytes are bmat's).  The blocks' values as torch tensors are made outside the timed region;
                torch's stream is drained in front of speck_from_coo_*, which runs on the config's;
  d  torch      torch.cat of sparse COO tensors (dim 0 for vstack, dim 1 inside a block row and dim 0 over the block rows
                otherwise, an absent cell an empty tensor) followed by .to_sparse_csr().  An item that takes more than
                --slow-ms in the warm-up is timed in the warm-up only (`rounds: 1`).
Protocol (that of scripts/extract_time.py): warm-up; device events around the whole timed item -- a on the config's stream,
the rest on the NULL stream; every speck call returns with its result complete, so the events span the read-backs; 7
ALTERNATING rounds, median (min - max) per column.  a and c must agree byte for byte: asserted.

    python scripts/bmat_time.py [--cases vstack8:webbase,vstack8:cant,block_diag512:scircuit,saddle:cant] [--rounds 7] [--out FILE]
Needs a GPU: there is no fallback."""
import argparse
import ctypes
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
    ap.add_argument("--cases", default="vstack8:webbase,vstack8:cant,block_diag512:scircuit,saddle:cant")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--small-scale", type=float, default=0.004)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bmat.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bmat_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    def with_host_offsets(d):
        """the same matrix with its row offsets known on the host (row_view needs them)"""
        return sa.dCSR.from_host(d.to_host())

    def stand_in(kind, dtype, scale, seed=42):
        S = sa.gen_matrix(kind, scale, seed, signed=True)
        return sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))

    def grids(case, kind, dtype):
        """name -> (cells [(block row, block column, dCSR)], block_rows, block_cols); the device matrices stay alive in `keep`"""
        keep = []
        if case == "vstack8":
            dS = sa.dCSR.from_host(stand_in(kind, dtype, args.scale))
            dP = sa.dCSR(dtype)
            sa.MultiplyspECK(dS, dS, dP, cfg)
            dA = with_host_offsets(dP)
            dP.reset(), dS.reset()
            cuts = [dA.rows * k // 8 for k in range(9)]
            views = [dA.row_view(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
            empty = [sa.dCSR.from_host(sa.HostCSR(v.rows, 0, np.zeros(v.rows + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype))) for v in views]
            keep += [dA, views, empty]
            out = {"vstack8": ([(g, 0, v) for g, v in enumerate(views)], 8, 1),
                   "vstack8_pieces": ([(g, 0, v) for g, v in enumerate(views)] + [(g, 1, e) for g, e in enumerate(empty)], 8, 2)}
        elif case == "block_diag512":
            mats = []
            for seed in range(64):
                H = stand_in(kind, dtype, args.small_scale, seed)
                mats += [sa.dCSR.from_host(H) for _ in range(8)]
            keep.append(mats)
            out = {"block_diag512": ([(i, i, m) for i, m in enumerate(mats)], 512, 512)}
        elif case == "saddle":
            S = stand_in(kind, dtype, args.scale)
            dH = sa.dCSR.from_host(S)
            dA = dH.row_view(0, S.rows // 4).copy()
            dAt = sa.transpose(dA, cfg)
            keep += [dH, dA, dAt]
            out = {"saddle": ([(0, 0, dH), (0, 1, dAt), (1, 0, dA)], 2, 2)}
        else:
            sys.exit(f"unknown case {case}")
        return out, keep

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

        for item in args.cases.split(","):
            case, kind = item.split(":")
            for dtype in (np.dtype(d).type for d in args.dtypes.split(",")):
                found, keep = grids(case, kind, dtype)
                tdt = torch.float64 if dtype == np.float64 else torch.float32
                for name, (cells, br, bc) in found.items():
                    cells = sorted(cells, key=lambda c: (c[0], c[1]))
                    p_lay, keep_lay, _ = sa.api._bmat_params(cells, br, bc, None, None, "bmat_time")
                    lay = sa.api._bmat_layout(p_lay, "bmat_time")
                    del p_lay, keep_lay
                    C = sa.dCSR(dtype)
                    wrapped = lambda: sa.api._bmat_call(cells, br, bc, cfg, None, None, C, True, "bmat_time")  # noqa: E731
                    _, info = wrapped()
                    # a: the C call on descriptors that exist (a caller in C++ has them; the Python wrapper's own time, which
                    # grows with the number of cells, is the column `wrapper`)
                    p_call, keep_call, _ = sa.api._bmat_params(cells, br, bc, None, None, "bmat_time")
                    c_info = sa._lib.CBmatInfo()
                    fn = sa._lib.load().speck_bmat_f32 if dtype == np.float32 else sa._lib.load().speck_bmat_f64

                    def call():
                        rc = fn(cfg._h, ctypes.byref(p_call), ctypes.byref(C._c), ctypes.byref(c_info))
                        assert rc == 0, rc
                    # ---- the blocks as torch tensors (outside every timed region)
                    hosts = [m.copy().to_host() for _, _, m in cells]              # (a view's copy counts from 0)
                    vals = [torch.from_numpy(np.ascontiguousarray(H.data)).to(dev) for H in hosts]
                    def no_entry(h, w):
                        return torch.sparse_coo_tensor(torch.empty((2, 0), dtype=torch.int64, device=dev), torch.empty(0, dtype=tdt, device=dev), size=(h, w))

                    coos = []
                    for (g, q, m), H in zip(cells, hosts):
                        if H.nnz == 0:
                            coos.append(no_entry(H.rows, H.cols))
                            continue
                        rows_t = torch.repeat_interleave(torch.arange(H.rows, device=dev), torch.from_numpy(np.diff(H.row_offsets.astype(np.int64))).to(dev))
                        idx = torch.stack([rows_t, torch.from_numpy(H.col_ids.astype(np.int64)).to(dev)])
                        coos.append(torch.sparse_coo_tensor(idx, torch.from_numpy(np.ascontiguousarray(H.data)).to(dev), size=(H.rows, H.cols)).coalesce())
                    del hosts
                    # ---- b: the floor
                    n_in = sum(m.nnz for _, _, m in cells)
                    in_col, in_val = torch.empty(n_in, dtype=torch.int32, device=dev), torch.empty(n_in, dtype=tdt, device=dev)
                    out_col, out_val = torch.empty(C.nnz, dtype=torch.int32, device=dev), torch.empty(C.nnz, dtype=tdt, device=dev)
                    out_ro = torch.empty(C.rows + 1, dtype=torch.int32, device=dev)
                    twins = [torch.empty_like(t) for t in (in_col, in_val, out_col, out_val, out_ro)]

                    def copies():
                        for dst, src in zip(twins, (in_col, in_val, out_col, out_val, out_ro)):
                            dst.copy_(src)

                    def dcsr_copy():
                        C.copy().reset()

                    # ---- c: the route that existed.  (A view goes in as its copy, made here: speck_to_coo does not know the value
                    # type and refuses an output anywhere in the span a view's 8-byte values could take behind A->data, and
                    # that is where torch's allocator puts the outputs when the values are floats.)
                    R = sa.dCSR(dtype)
                    route_cells = [(g, q, m.copy() if not m._owner and isinstance(m._keep, sa.dCSR) else m) for g, q, m in cells]

                    def route():
                        rows_l, cols_l = [], []
                        for g, q, m in route_cells:
                            if m.nnz == 0:
                                continue
                            row, col = sa.to_coo(m, cfg, row_base=lay.row_origins[g])
                            rows_l.append(row)
                            cols_l.append(col + lay.col_origins[q])
                        row, col, val = torch.cat(rows_l), torch.cat(cols_l), torch.cat(vals)
                        torch.cuda.current_stream().synchronize()   # (the config's stream is not torch's)
                        return sa.from_coo(row, col, val, (lay.rows, lay.cols), cfg, matOut=R)

                    # ---- d: torch
                    def torch_cat():
                        if bc == 1:
                            return torch.cat(coos, dim=0).to_sparse_csr()
                        at, lines_t = 0, []
                        for g in range(br):
                            parts, h = [], lay.row_origins[g + 1] - lay.row_origins[g]
                            q0 = 0
                            while at < len(cells) and cells[at][0] == g:
                                q = cells[at][1]
                                if q > q0:      # the absent cells in front as one empty tensor
                                    parts.append(no_entry(h, lay.col_origins[q] - lay.col_origins[q0]))
                                parts.append(coos[at])
                                q0, at = q + 1, at + 1
                            if q0 < bc:
                                parts.append(no_entry(h, lay.col_origins[bc] - lay.col_origins[q0]))
                            lines_t.append(torch.cat(parts, dim=1))
                        return torch.cat(lines_t, dim=0).to_sparse_csr()

                    torch_first, torch_error = None, None
                    try:
                        torch_first, _ = timed(torch_cat, null)
                        torch_first, _ = timed(torch_cat, null)
                    except (RuntimeError, NotImplementedError) as err:
                        torch_error = str(err).splitlines()[0][:160]
                    torch.cuda.synchronize()
                    ms = {key: [] for key in ("a", "w", "copy", "copies", "c", "d")}
                    if torch_first is not None and torch_first > args.slow_ms:
                        ms["d"].append(torch_first)
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        cfg.set_stream(s.cuda_stream)
                        ta, _ = timed(call, s)
                        tw, _ = timed(wrapped, s)
                        cfg.set_stream(None)
                        t1, _ = timed(dcsr_copy, null)
                        t2, _ = timed(copies, null)
                        tc, _ = timed(route, null)
                        if take:
                            ms["a"].append(ta), ms["w"].append(tw), ms["copy"].append(t1), ms["copies"].append(t2), ms["c"].append(tc)
                        if torch_first is not None and torch_first <= args.slow_ms:
                            td, _ = timed(torch_cat, null)
                            if take:
                                ms["d"].append(td)
                    G, W = C.to_host(), R.to_host()
                    assert G.row_offsets.tobytes() == W.row_offsets.tobytes(), (case, kind, name)
                    assert G.col_ids.tobytes() == W.col_ids.tobytes(), (case, kind, name)
                    assert G.data.tobytes() == W.data.tobytes(), (case, kind, name)
                    a = statistics.median(ms["a"])
                    rec = dict(case=name, kind=kind, dtype=np.dtype(dtype).name, blocks=info.blocks, rows=info.rows_out, cols=info.cols_out,
                               nnz=info.nnz_out, pieces=info.pieces, rounds=args.rounds, bmat=stats(ms["a"]), wrapper=stats(ms["w"]), dcsr_copy=stats(ms["copy"]),
                               copies=stats(ms["copies"]), route=stats(ms["c"]), a_vs_dcsr_copy=a / statistics.median(ms["copy"]),
                               a_vs_copies=a / statistics.median(ms["copies"]), a_vs_route=a / statistics.median(ms["c"]))
                    if torch_error is not None:
                        rec.update(torch_cat=None, torch_cat_error=torch_error)
                    else:
                        rec.update(torch_cat=stats(ms["d"]), a_vs_torch_cat=a / statistics.median(ms["d"]))
                    emit(rec)
                    C.reset(), R.reset()
                    del in_col, in_val, out_col, out_val, out_ro, twins, vals, coos, route_cells, p_call, keep_call
                    torch.cuda.empty_cache()
                del found, keep
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
