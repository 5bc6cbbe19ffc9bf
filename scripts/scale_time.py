"""Time speck_scale_f64 / _f32 against a copy of the arrays it moves.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: S and the product S S (made on the device).  Forms:
    a  in place, alpha only                                 (the stream: data in, data out)
    b  in place, rows divided by a vector                   (the tiles: + row_offsets, the vector once per row)
    c  in place, one vector times rows and columns          (+ col_ids in, a gather per entry)
    d  into a new matrix, rows divided by a vector          (+ col_ids in and out, row_offsets out)
Yardsticks, on the same box in the same rounds: a plain device-to-device copy of A's data array into a buffer that exists
-- exactly the bytes form a has to move -- and, for d, the copies of data, col_ids and row_offsets together.  Protocol:
warm-up; device events around the whole call (scale: on the config's stream, the call returns complete, so the events
span its read-back; the copies: on the NULL stream they run on); repeated ALTERNATING rounds with the median taken per
column.  Form d writes into a matrix that exists, so after the warm-up no call allocates.  The in-place forms keep
scaling the same values: alpha is 1 and the vectors hold +-1, so nothing drifts and every result is checked at the end
(and only there: a round is nothing but its calls).

    python scripts/scale_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
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

HBM_PEAK_GBS = 8000.0  # as bench.py
FORMS = ("a", "b", "c", "d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scale_time.py needs a GPU")
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
                    src = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                    dst = torch.empty_like(src)
                    src_ci = torch.from_numpy(H.col_ids.view(np.int32)).to(dev)
                    dst_ci = torch.empty_like(src_ci)
                    src_ro = torch.from_numpy(H.row_offsets.view(np.int32)).to(dev)
                    dst_ro = torch.empty_like(src_ro)
                    # (+-1: dividing and multiplying by them any number of times keeps every magnitude)
                    signs = np.where(np.random.default_rng(1).random(max(H.rows, H.cols)) < 0.5, -1.0, 1.0)
                    vec = torch.from_numpy(signs).to(dev)
                    row, col = vec[:H.rows], vec[:H.cols]
                    dC = sa.dCSR(dtype)
                    calls = {
                        "a": lambda: sa.scale(dA, cfg, inplace=True),
                        "b": lambda: sa.scale(dA, cfg, row=row, row_div=True, inplace=True),
                        "c": lambda: sa.scale(dA, cfg, row=row, col=col, inplace=True),
                        "d": lambda: sa.scale(dA, cfg, row=row, row_div=True, matOut=dC),
                    }

                    def copy3():
                        dst.copy_(src, non_blocking=True)
                        dst_ci.copy_(src_ci, non_blocking=True)
                        dst_ro.copy_(src_ro, non_blocking=True)

                    torch.cuda.synchronize()
                    ms = {k: [] for k in FORMS + ("memcpy", "memcpy3")}
                    infos = {}
                    # (nothing but the calls between the events of a round: host work in between cools the launch path)
                    for r in range(args.warmup + args.rounds):
                        take = r >= args.warmup
                        for form in FORMS:
                            cfg.set_stream(s.cuda_stream)
                            t, (_, infos[form]) = timed(calls[form], s)
                            cfg.set_stream(None)
                            if take:
                                ms[form].append(t)
                        t, _ = timed(lambda: dst.copy_(src, non_blocking=True), null)
                        if take:
                            ms["memcpy"].append(t)
                        t, _ = timed(copy3, null)
                        if take:
                            ms["memcpy3"].append(t)
                    got, new = dA.to_host(), dC.to_host()
                    rows_of = np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))
                    calls_made = args.warmup + args.rounds       # b: rows once per call; c: rows and columns once per call
                    applied = (signs[rows_of] ** (2 * calls_made)) * (signs[H.col_ids] ** calls_made)
                    want = (H.data.astype(np.float64) * applied).astype(dtype)
                    assert got.data.tobytes() == want.tobytes(), (kind, name, "in place")
                    assert new.data.tobytes() == (want.astype(np.float64) / signs[rows_of]).astype(dtype).tobytes(), (kind, name, "new")
                    assert new.col_ids.tobytes() == H.col_ids.tobytes() and new.row_offsets.tobytes() == H.row_offsets.tobytes()
                    assert all(i.nonfinite == 0 and i.entries == H.nnz for i in infos.values())
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    nbytes = H.nnz * H.data.itemsize
                    rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, nnz=H.nnz,
                               tiles=infos["b"].tiles, rounds=args.rounds,
                               memcpy_data_ms=med["memcpy"], memcpy_min_max=(min(ms["memcpy"]), max(ms["memcpy"])),
                               memcpy_hbm_frac=2 * nbytes / (med["memcpy"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               memcpy_all_ms=med["memcpy3"], memcpy_all_min_max=(min(ms["memcpy3"]), max(ms["memcpy3"])))
                    for form in FORMS:
                        yard = "memcpy3" if form == "d" else "memcpy"
                        rec[form] = dict(ms=med[form], min_max=(min(ms[form]), max(ms[form])),
                                         **{"vs_memcpy_all" if form == "d" else "vs_memcpy_data": med[form] / med[yard]})
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                    dC.reset()
                    del src, dst, src_ci, dst_ci, src_ro, dst_ro, vec, row, col
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
