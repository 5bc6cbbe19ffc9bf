"""Time speck_select_f64 against a copy of the same matrix: a filter that keeps everything is a copy plus a byte per entry.

Input: C = S x S of a stand-in (scale 1.0 by default), fp64.  Predicates: BAND (the strict lower triangle), ABS (threshold =
the median |v|, computed on the host) and PATTERN (M = the pattern of S), plus the call without a predicate.  Yardsticks, on
the same box in the same rounds: speck_dcsr_copy of C (with the allocation of its result inside, as a caller pays it) and
three plain device-to-device copies of C's arrays into buffers that exist (the floor: no allocation, no kernel of ours).
Protocol: warm-up; device events around the whole call (select: on the config's stream, the call returns with its result
complete, so the events span its read-back; the copies: on the NULL stream they run on); repeated ALTERNATING rounds with
the median taken per column.  The result matrix of a predicate is reused from round to round, so after the warm-up a select
allocates nothing.

    python scripts/select_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("select_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        for kind in args.kinds.split(","):
            S = sa.gen_matrix(kind, args.scale, 42, signed=True)
            dS = sa.dCSR.from_host(S)
            dC = sa.dCSR()
            sa.MultiplyspECK(dS, dS, dC, cfg)
            C = dC.to_host()
            dC.reset()
            # (the matrix lives in torch tensors: the plain copies below are tensor copies)
            src = [torch.from_numpy(C.row_offsets.view(np.int32).copy()).to(dev), torch.from_numpy(C.col_ids.view(np.int32).copy()).to(dev),
                   torch.from_numpy(C.data).to(dev)]
            dC = sa.dCSR.from_device(C.rows, C.cols, C.nnz, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), keep=src,
                                     host_row_offsets=C.row_offsets)
            t_abs = float(np.median(np.abs(C.data)))
            preds = {"none": {}, "band": dict(band=(None, -1)), "abs": dict(abs_gt=t_abs), "pattern": dict(pattern=dS)}
            # what the predicates have to keep, on the host
            row = np.repeat(np.arange(C.rows, dtype=np.int64), np.diff(C.row_offsets.astype(np.int64)))
            s_row = np.repeat(np.arange(S.rows, dtype=np.int64), np.diff(S.row_offsets.astype(np.int64)))
            want = {"none": C.nnz, "band": int((C.col_ids.astype(np.int64) < row).sum()),
                    "abs": int((~(np.abs(C.data) <= t_abs)).sum()),
                    "pattern": int(np.isin(row * C.cols + C.col_ids, s_row * S.cols + S.col_ids).sum())}
            del row, s_row
            dst = [torch.empty_like(t) for t in src]   # targets of the plain copies
            torch.cuda.synchronize()
            s = torch.cuda.Stream(device=dev)
            null = torch.cuda.default_stream(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn, stream):
                e0.record(stream)
                out = fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), out

            def plain_copies():   # (torch's current stream is the NULL stream here)
                for a, d in zip(src, dst):
                    d.copy_(a, non_blocking=True)

            outs = {k: sa.dCSR() for k in preds}
            ms = {k: [] for k in list(preds) + ["copy", "memcpy"]}
            infos = {}
            for r in range(args.warmup + args.rounds):
                take = r >= args.warmup
                for k, pred in preds.items():
                    cfg.set_stream(s.cuda_stream)
                    t, (_, infos[k]) = timed(lambda: sa.select(dC, cfg, matOut=outs[k], **pred), s)
                    cfg.set_stream(None)
                    if take:
                        ms[k].append(t)
                t, cp = timed(lambda: dC.copy(), null)
                cp.reset()
                if take:
                    ms["copy"].append(t)
                t, _ = timed(plain_copies, null)
                if take:
                    ms["memcpy"].append(t)
            for k in preds:
                assert infos[k].nnz_out == want[k] == outs[k].nnz, (k, infos[k], want[k])
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = dict(kind=kind, scale=args.scale, rows=C.rows, nnz=C.nnz, nnz_pattern=S.nnz, abs_threshold=t_abs,
                       rounds=args.rounds, copy_ms=med["copy"], memcpy_ms=med["memcpy"],
                       copy_min_max=(min(ms["copy"]), max(ms["copy"])), memcpy_min_max=(min(ms["memcpy"]), max(ms["memcpy"])),
                       memcpy_hbm_frac=2 * (12 * C.nnz + 4 * C.rows) / (med["memcpy"] * 1e-3) / 1e9 / HBM_PEAK_GBS)
            for k in preds:
                rec[k] = dict(ms=med[k], min_max=(min(ms[k]), max(ms[k])), kept=infos[k].kept,
                              rows_unchanged=infos[k].rows_unchanged, vs_copy=med[k] / med["copy"],
                              vs_memcpy=med[k] / med["memcpy"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            for o in outs.values():
                o.reset()
            dC.reset()
            dS.reset()
            del dst, src
            torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
