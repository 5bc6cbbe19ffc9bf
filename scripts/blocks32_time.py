"""Time the float-block calls speck_spmm_*_b32, speck_spmm_t_*_b32 and speck_sddmm_*_b32 against what a caller had before
them and against that route's floor.

Inputs, from the stand-ins at scale 1.0 by default, both value types of A: scircuit S, cant S S and webbase S S (the
products made on the device), and k in {1, 8, 32, 128}.  Per input, k and call (spmm: Y = A X; spmm_t: Y = A^T X through a
plan made outside; sddmm: C = U V^T on A's pattern into a C that exists), in the same rounds on the same box:
  a  b32        the new call on float32 blocks;
  b  widen      what a caller had: .double() of the blocks, the double-block call, .float() of the result (spmm, spmm_t; the
                result of sddmm is a matrix and needs no narrowing) -- all inside the timed region;
  c  f64        the double-block call alone on blocks widened beforehand: the floor of b, and the yardstick of whether
                halving the gathered bytes shows at all;
  t  torch      spmm with fp32 values only: torch.sparse_csr @ X in fp32, where this torch build serves it.
Protocol (that of scripts/spmm_t_time.py): warm-up; device events around the whole timed item on the config's stream (torch
works on it too: the conversions of b are ordered with the call); every speck call returns with its result complete, so
the events span the read-backs; 7 ALTERNATING rounds, median (min - max) per column.  a must equal b and float(c) byte
for byte: asserted before anything is timed.

--label names the build in every record: the committed library is `cb4` (SPECK_SPMM_COLUMN_BLOCK_B32 columns per block); a
measurement build of the other column-block form (-DSPECK_SPMM_B32_FORCE_BLOCK=8) is loaded with SPECK_LIB=<path> and
timed with --label cb8 --calls spmm,spmm_t --append.

    python scripts/blocks32_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--ks 1,8,32,128] [--calls spmm,spmm_t,sddmm]
                                    [--scale 1.0] [--rounds 7] [--label cb4] [--out FILE] [--append]
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
    ap.add_argument("--ks", default="1,8,32,128")
    ap.add_argument("--calls", default="spmm,spmm_t,sddmm")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="cb%d" % sa.SPMM_COLUMN_BLOCK_B32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks32.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("blocks32_time.py needs a GPU")
    ks = [int(k) for k in args.ks.split(",")]
    calls = args.calls.split(",")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        s = torch.cuda.Stream(device=dev)
        cfg.set_stream(s.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):
            e0.record(s)
            out = fn()
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        def stats(v):
            return dict(ms=statistics.median(v), min_max=(min(v), max(v)))

        def block(n, k, seed):
            return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(max(n, 1), k)).astype(np.float32)).to(dev)

        with torch.cuda.stream(s):
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
                    plan = sa.transpose_plan(dA, cfg) if "spmm_t" in calls else None
                    tA = None
                    if dtype == np.float32 and "spmm" in calls:
                        tA = torch.sparse_csr_tensor(torch.from_numpy(H.row_offsets.astype(np.int64)).to(dev),
                                                     torch.from_numpy(H.col_ids.astype(np.int64)).to(dev),
                                                     torch.from_numpy(np.ascontiguousarray(H.data)).to(dev), size=(H.rows, H.cols))
                    C32, C64, C64b = sa.dCSR(dtype), sa.dCSR(dtype), sa.dCSR(dtype)
                    for call in calls:
                        for k in ks:
                            # the blocks of the call: what it reads (one or two), what it writes (spmm, spmm_t)
                            if call == "spmm":
                                ins, n_out = [block(H.cols, k, k)], H.rows
                            elif call == "spmm_t":
                                ins, n_out = [block(H.rows, k, k)], H.cols
                            else:
                                ins, n_out = [block(H.rows, k, k), block(H.cols, k, k + 1)], 0
                            wide = [x.double() for x in ins]
                            Y32 = torch.zeros((max(n_out, 1), k), dtype=torch.float32, device=dev)
                            Y64 = torch.zeros((max(n_out, 1), k), dtype=torch.float64, device=dev)
                            Y64b = torch.zeros_like(Y64)

                            def run(blocks, Y, C, kw):
                                if call == "spmm":
                                    return sa.spmm(dA, blocks[0], cfg, Y=Y, **kw)[1]
                                if call == "spmm_t":
                                    return sa.spmm_t(dA, blocks[0], cfg, plan=plan, Y=Y, **kw)[1]
                                return sa.sddmm(dA, blocks[0], blocks[1], cfg, matOut=C, **kw)[1]

                            def route_a():
                                return run(ins, Y32, C32, dict(blocks="float32"))

                            def route_b():
                                run([x.double() for x in ins], Y64b, C64b, {})
                                return Y64b.float() if n_out else None

                            def route_c():
                                return run(wide, Y64, C64, {})

                            # the routes agree byte for byte before anything is timed
                            info = route_a()
                            narrowed = route_b()
                            route_c()
                            torch.cuda.synchronize()
                            if n_out:
                                got = Y32.cpu().numpy().tobytes()
                                assert got == narrowed.cpu().numpy().tobytes() == Y64.float().cpu().numpy().tobytes(), (kind, name, call, k)
                            else:
                                got = C32.to_host().data.tobytes()
                                assert got == C64b.to_host().data.tobytes() == C64.to_host().data.tobytes(), (kind, name, call, k)
                            torch_error = "not timed"
                            if tA is not None and call == "spmm":
                                try:  # (a torch build without this product: the column stays empty and the record says why)
                                    tA @ ins[0]
                                    torch_error = None
                                except (RuntimeError, NotImplementedError) as err:
                                    torch_error = str(err).splitlines()[0][:160]
                            torch.cuda.synchronize()
                            ms = {n: [] for n in "abct"}
                            for r in range(args.warmup + args.rounds):
                                take = r >= args.warmup
                                ta, _ = timed(route_a)
                                tb, _ = timed(route_b)
                                tc, _ = timed(route_c)
                                if take:
                                    ms["a"].append(ta), ms["b"].append(tb), ms["c"].append(tc)
                                if torch_error is None:
                                    tt, _ = timed(lambda: tA @ ins[0])
                                    if take:
                                        ms["t"].append(tt)
                            a, b, c = (statistics.median(ms[n]) for n in "abc")
                            rec = dict(label=args.label, kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale,
                                       rows=H.rows, cols=H.cols, nnz=H.nnz, call=call, k=k, terms=info.terms, rounds=args.rounds,
                                       b32=stats(ms["a"]), widen_call_narrow=stats(ms["b"]), f64_on_widened=stats(ms["c"]),
                                       a_vs_b=a / b, a_vs_c=a / c)
                            if torch_error is None:
                                rec.update(torch_f32=stats(ms["t"]), a_vs_torch=a / statistics.median(ms["t"]))
                            elif tA is not None and call == "spmm":
                                rec.update(torch_f32=None, torch_error=torch_error)
                            print(json.dumps(rec), flush=True)
                            lines.append(json.dumps(rec))
                            del ins, wide, Y32, Y64, Y64b
                    if plan is not None:
                        plan.free()
                    for m in (C32, C64, C64b, dA):
                        m.reset()
                    del tA
                    torch.cuda.empty_cache()
    finally:
        cfg.set_stream(None)
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
