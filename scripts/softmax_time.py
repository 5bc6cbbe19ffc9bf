"""Time speck_softmax_f64 / _f32 (in place, mode NORMALIZED, alpha = 1) against what bounds it and against what a user
writes today, and record the ratios plainly.

Inputs, from a stand-in S (scale 1.0 by default), fp64 and fp32: scircuit S, cant S S and webbase S S (the products made
on the device).  Yardsticks, on the same box in the same rounds:
  copy    a device-to-device copy of `data` (torch copy_ between two tensors of nnz values);
  scale   speck_scale_*(A, row = l) in place: the same tile frame with one read and one write and no exp -- the floor the
          call can approach;
  torch   the composition a user writes today: scatter_reduce(amax), exp, index_add_, a division, with the int64 row
          index built OUTSIDE the timed region; it materialises three arrays of nnz doubles.
Protocol (that of scripts/sddmm_time.py): warm-up; device events around the whole timed item (the library's calls: on the
config's stream, a call returns with its result complete, so the events span the read-back; the yardsticks: on the NULL
stream they run on); repeated ALTERNATING rounds, the median (min - max) per column.  No threshold: what is found is
recorded, the losses included.

--exp-ulp measures the device's double exp instead: mode "exp" on rows (0, v), v <= 0, gives exp(v) itself; v runs over
the arguments x - m of the accuracy inputs of tests/test_gpu_softmax.py and over a uniform sweep of [-745, 0]; the
reference is np.exp in np.longdouble; the record holds the worst error in ULPs of the double result.

--tag TEXT appends the records under that tag: how a library built another way (SPECK_LIB=...) is compared on the same
inputs (profiles/softmax.txt holds the first form of the tile kernel so: an LDS array of its own for m and s).

    python scripts/softmax_time.py [--inputs scircuit:S,cant:SS,webbase:SS] [--scale 1.0] [--rounds 7] [--exp-ulp]
                                   [--tag TEXT] [--out FILE]
Needs a GPU: there is no fallback."""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speck_amd as sa  # noqa: E402


def exp_ulp(cfg):
    """the records of --exp-ulp"""
    spec = importlib.util.spec_from_file_location("test_gpu_softmax", os.path.join(ROOT, "tests", "test_gpu_softmax.py"))
    tests = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tests)
    args = {}
    for kind in ("uniform", "decades"):
        for dtype in tests.DTYPES:
            H = tests.edge_matrix(dtype, kind)
            for alpha in tests.ALPHAS:
                x = alpha * H.data.astype(np.float64)
                _, m, _ = tests.numpy_forward(H, alpha)
                args[f"tests {kind} {np.dtype(dtype).name} alpha={alpha}"] = x - m[tests.rows_of(H.row_offsets)]
    args["uniform sweep of [-745, 0]"] = np.random.default_rng(1).uniform(-745.0, 0.0, size=1 << 20)
    lines = []
    for name, v in args.items():
        assert (v <= 0).all()
        n = len(v)
        data = np.zeros(2 * n)
        data[1::2] = v
        H = sa.HostCSR(n, 2, (2 * np.arange(n + 1)).astype(np.uint32), np.tile(np.array([0, 1], dtype=np.uint32), n), data)
        E, _ = sa.softmax(sa.dCSR.from_host(H), cfg, mode="exp")
        got = E.to_host().data
        assert (got[0::2] == 1.0).all()
        ref = np.exp(v.astype(np.longdouble))
        normal = ref >= np.finfo(np.float64).tiny                     # (a ULP of a subnormal is not relative)
        ulps = np.abs(got[1::2].astype(np.longdouble) - ref)[normal] / np.spacing(ref[normal].astype(np.float64))
        rec = dict(exp_ulp=name, arguments=int(normal.sum()), worst_ulps=float(ulps.max()), at=float(v[normal][int(ulps.argmax())]))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    # what tests/test_gpu_softmax.py takes for U_EXP: twice the worst over ITS arguments, rounded up to an integer
    worst = max(json.loads(line)["worst_ulps"] for line in lines if json.loads(line)["exp_ulp"].startswith("tests"))
    lines.append(json.dumps(dict(exp_ulp="choice", worst_ulps_on_the_test_inputs=worst, u_exp=math.ceil(2 * worst),
                                 rule="twice the worst observed, rounded up to an integer")))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="scircuit:S,cant:SS,webbase:SS")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exp-ulp", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmax_time.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        if args.exp_ulp:
            lines = exp_ulp(cfg)
        null = torch.cuda.default_stream(dev)
        s = torch.cuda.Stream(device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn, stream):
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        for item in ([] if args.exp_ulp else args.inputs.split(",")):
            kind, name = item.split(":")
            for dtype in (np.dtype(d).type for d in args.dtypes.split(",")):
                S = sa.gen_matrix(kind, args.scale, 42, signed=True)
                S = sa.HostCSR(S.rows, S.cols, S.row_offsets, S.col_ids, S.data.astype(dtype))
                dS = sa.dCSR.from_host(S)
                dA = dS
                if name == "SS":
                    dA = sa.dCSR(dtype)
                    sa.MultiplyspECK(dS, dS, dA, cfg)
                H = dA.to_host()
                row_host = np.repeat(np.arange(H.rows), np.diff(H.row_offsets.astype(np.int64)))
                row = torch.from_numpy(row_host).to(dev)           # (the index of the torch path: outside the timed region)
                val = torch.from_numpy(H.data.astype(np.float64)).to(dev)
                src = torch.from_numpy(np.ascontiguousarray(H.data)).to(dev)
                dst = torch.empty_like(src)
                ones = torch.full((max(H.rows, 1),), 1.5, dtype=torch.float64, device=dev)
                dW, dX = dA.copy(), dA.copy()                      # softmax and scale work in place on copies

                def composition():
                    m = torch.full((H.rows,), -np.inf, dtype=torch.float64, device=dev)
                    m.scatter_reduce_(0, row, val, "amax")
                    e = torch.exp(val - m[row])
                    t = torch.zeros(H.rows, dtype=torch.float64, device=dev).index_add_(0, row, e)
                    return e / t[row]

                columns = ("softmax", "copy", "scale", "torch")
                ms = {n: [] for n in columns}
                info = want = None
                for r in range(args.warmup + args.rounds):
                    take = r >= args.warmup
                    cfg.set_stream(s.cuda_stream)
                    if r == 0:
                        first, info = sa.softmax(dA.copy(), cfg, inplace=True)
                        first = first.to_host().data
                    t_soft, _ = timed(lambda: sa.softmax(dW, cfg, inplace=True), s)
                    t_scale, _ = timed(lambda: sa.scale(dX, cfg, row=ones, inplace=True), s)
                    cfg.set_stream(None)
                    t_copy, _ = timed(lambda: dst.copy_(src), null)
                    t_torch, want = timed(composition, null)
                    if take:
                        for n, t in zip(columns, (t_soft, t_copy, t_scale, t_torch)):
                            ms[n].append(t)
                # a sanity check on the timed data, not the test
                tol = 1e-11 if dtype == np.float64 else 1e-5
                assert np.allclose(first.astype(np.float64), want.cpu().numpy(), rtol=tol, atol=1e-300), (kind, name)
                rec = dict(kind=kind, matrix=name, dtype=np.dtype(dtype).name, scale=args.scale, rows=H.rows, cols=H.cols, nnz=H.nnz,
                           tiles=info.tiles, rows_split=info.rows_split, rows_empty=info.rows_empty, rounds=args.rounds,
                           data_bytes=2 * H.nnz * np.dtype(dtype).itemsize)
                for n in columns:
                    rec[n + "_ms"] = statistics.median(ms[n])
                    rec[n + "_min_max"] = (min(ms[n]), max(ms[n]))
                    if n != "softmax":
                        rec["vs_" + n] = rec["softmax_ms"] / rec[n + "_ms"]
                if args.tag:
                    rec["tag"] = args.tag
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                del row, val, src, dst, ones, dW, dX, want
                dS.reset()
                if dA is not dS:
                    dA.reset()
                torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a" if args.exp_ulp or args.tag else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
