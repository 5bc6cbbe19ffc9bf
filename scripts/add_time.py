"""Time speck_add_f64 against copies of the matrices it reads and writes.

Inputs, from a stand-in S (scale 1.0 by default), fp64: S + S^T (the transpose made on the device), S S + S (the product made
on the device) and S + S (two copies of S).  Yardsticks, on the same box in the same rounds: plain device-to-device copies
of the arrays of A, of B and of C into buffers that exist (the traffic floor of reading both and writing the result: no
allocation, no kernel of ours) and speck_dcsr_copy of C (with the allocation of its result inside, as a caller pays it).
Protocol: warm-up; device events around the whole call (add: on the config's stream, the call returns with its result
complete, so the events span its read-back; the copies: on the NULL stream they run on); repeated ALTERNATING rounds with
the median taken per column.  The result matrix of a sum is reused from round to round, so after the warm-up an add
allocates nothing.

    python scripts/add_time.py [--kinds scircuit,cant,webbase] [--scale 1.0] [--rounds 7] [--out FILE]
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


def keys(H):
    row = np.repeat(np.arange(H.rows, dtype=np.int64), np.diff(H.row_offsets.astype(np.int64)))
    return row * H.cols + H.col_ids.astype(np.int64)


def on_device(H, dev):
    """the matrix in torch tensors (the plain copies are tensor copies) and the dCSR over them"""
    t = [torch.from_numpy(H.row_offsets.view(np.int32).copy()).to(dev), torch.from_numpy(H.col_ids.view(np.int32).copy()).to(dev),
         torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)]
    d = sa.dCSR.from_device(H.rows, H.cols, H.nnz, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), keep=t,
                            host_row_offsets=H.row_offsets)
    return t, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="scircuit,cant,webbase")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("add_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfgs = {"add": sa.spECKConfig.initialize(0)}
    lines = []
    try:
        for kind in args.kinds.split(","):
            S = sa.gen_matrix(kind, args.scale, 42, signed=True)
            dS = sa.dCSR.from_host(S)
            hosts = {"S": S}
            if S.rows == S.cols:
                hosts["St"] = sa.transpose(dS, cfgs["add"]).to_host()
            dP = sa.dCSR()
            sa.MultiplyspECK(dS, dS, dP, cfgs["add"])
            hosts["SS"] = dP.to_host()
            dP.reset()
            dS.reset()
            sums = {"S+S": ("S", "S"), "SS+S": ("SS", "S")}
            if "St" in hosts:
                sums["S+St"] = ("S", "St")
            null = torch.cuda.default_stream(dev)
            s = torch.cuda.Stream(device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn, stream):
                e0.record(stream)
                out = fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), out

            for name, (ka, kb) in sums.items():
                HA, HB = hosts[ka], hosts[kb]
                ta, dA = on_device(HA, dev)
                tb, dB = on_device(HB, dev)     # (a second copy where the operands are the same matrix)
                want = len(np.union1d(keys(HA), keys(HB)))
                outs = {k: sa.dCSR() for k in cfgs}
                # a first call: the result the copies are measured on
                first, _ = sa.add(dA, dB, cfgs["add"], alpha=2.5, beta=-0.5)
                tc, dC = on_device(first.to_host(), dev)
                first.reset()
                src = ta + tb + tc
                dst = [torch.empty_like(t) for t in src]   # targets of the plain copies
                torch.cuda.synchronize()

                def plain_copies():   # (torch's current stream is the NULL stream here)
                    for a, d in zip(src, dst):
                        d.copy_(a, non_blocking=True)

                ms = {k: [] for k in list(cfgs) + ["copy", "memcpy"]}
                infos = {}
                for r in range(args.warmup + args.rounds):
                    take = r >= args.warmup
                    for k, cfg in cfgs.items():
                        cfg.set_stream(s.cuda_stream)
                        t, (_, infos[k]) = timed(lambda: sa.add(dA, dB, cfg, alpha=2.5, beta=-0.5, matOut=outs[k]), s)
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
                for k in cfgs:
                    assert infos[k].nnz_out == want == outs[k].nnz == dC.nnz, (name, k, infos[k], want)
                med = {k: statistics.median(v) for k, v in ms.items()}
                nnz_all, rows = HA.nnz + HB.nnz + dC.nnz, HA.rows
                rec = dict(kind=kind, sum=name, scale=args.scale, rows=rows, nnz_a=HA.nnz, nnz_b=HB.nnz, nnz_c=dC.nnz,
                           both=infos["add"].both, rounds=args.rounds, copy_c_ms=med["copy"], memcpy_abc_ms=med["memcpy"],
                           copy_c_min_max=(min(ms["copy"]), max(ms["copy"])), memcpy_abc_min_max=(min(ms["memcpy"]), max(ms["memcpy"])),
                           memcpy_hbm_frac=2 * (12 * nnz_all + 12 * rows) / (med["memcpy"] * 1e-3) / 1e9 / HBM_PEAK_GBS)
                for k in cfgs:
                    rec[k] = dict(ms=med[k], min_max=(min(ms[k]), max(ms[k])), vs_memcpy_abc=med[k] / med["memcpy"],
                                  vs_copy_c=med[k] / med["copy"])
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                for o in outs.values():
                    o.reset()
                del dst, src, ta, tb, tc, dA, dB, dC
                torch.cuda.empty_cache()
    finally:
        for cfg in cfgs.values():
            cfg.cleanup()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
