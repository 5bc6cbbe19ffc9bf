"""Time speck_multiply_masked_f64 against the complete speck_multiply_f64 call on the same A and B.

Inputs (stand-ins at scale 1.0, seed 7, fp64): scircuit, cant, webbase with A = B = S, M = pattern(S), and the triangle
case of webbase, A = B = M = L, L the strictly lower triangle of pattern(S + S^T) with unit values.  The baseline is the
complete multiply of ANOTHER build of the library (--baseline-lib: a build of the parent commit), run in a child process
that loads it through SPECK_LIB: its complete call (option reuse = 0, output matrix reused -- what bench.py reports as
`value`) and its reuse sequence (`value_reuse`).  That is a lower bound of any multiply-then-filter path: the filter comes
on top.  Without --baseline-lib the child loads the library of this tree.

Protocol: warm-up rounds, then ALTERNATING rounds -- masked STRUCTURE, masked FULL_PATTERN here, then one round of the child
(complete, reuse) -- with device events on the config's stream around the whole call (read-backs included); median, min
and max per column.  One process touches the GPU at a time: the child works only when it is told to.

    python scripts/masked_time.py [--inputs scircuit,cant,webbase,webbase_tri] [--scale 1.0] [--rounds 7] [--out FILE]
                                  [--baseline-lib PATH] [--no-baseline]
--no-baseline: the masked legs alone, no child process (what a kernel trace of them is taken from).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speck_amd as sa  # noqa: E402


def make_inputs(name, scale):
    """(A = B, M) as speck_amd.HostCSR"""
    kind = name[:-4] if name.endswith("_tri") else name
    S = sa.gen_matrix(kind, scale, 7, signed=True)
    if not name.endswith("_tri"):
        return S, S
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(S.nnz), S.col_ids, S.row_offsets.astype(np.int64)), shape=(S.rows, S.cols))
    L = sp.tril(((P + P.T) > 0).astype(np.float64), k=-1).tocsr()
    L.sort_indices()
    H = sa.HostCSR(L.shape[0], L.shape[1], L.indptr.astype(np.uint32), L.indices.astype(np.uint32), L.data)
    return H, H


class Timer:
    def __init__(self, cfg, dev):
        self.s = torch.cuda.Stream(device=dev)
        cfg.set_stream(self.s.cuda_stream)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __call__(self, fn):
        with torch.cuda.stream(self.s):
            self.e0.record(self.s)
            out = fn()
            self.e1.record(self.s)
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1), out


def child(name, scale):
    """the baseline: one line per command on stdin -- `round` -> {"complete": ms, "reuse": ms}, `quit`"""
    import ctypes
    from speck_amd import _lib
    older = ctypes.CDLL(_lib.LIB_PATH)   # (a build of an earlier commit does not export what was added since: the loader
    for sym in [n for n in _lib._SIGS if not hasattr(older, n)]:   #  binds every declared symbol, the multiply is all we need)
        del _lib._SIGS[sym]
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    A, _ = make_inputs(name, scale)
    dA = sa.dCSR.from_host(A)
    dC_eager, dC_reuse = sa.dCSR(), sa.dCSR()
    timed = Timer(cfg, dev)
    cfg.set_option("reuse", 1)
    for _ in range(3):   # (the reuse sequence is planned by the repeated identical call)
        sa.MultiplyspECK(dA, dA, dC_reuse, cfg)
    print(json.dumps(dict(ready=True, lib=sa.lib_path(), nnz_c=dC_reuse.nnz,
                          products=cfg.last_stats()["sum_products"])), flush=True)
    for line in sys.stdin:
        if line.strip() != "round":
            break
        cfg.set_option("reuse", 0)
        t_complete, _ = timed(lambda: sa.MultiplyspECK(dA, dA, dC_eager, cfg))
        cfg.set_option("reuse", 1)
        sa.MultiplyspECK(dA, dA, dC_reuse, cfg)      # (untimed: the option change dropped the sequence)
        sa.MultiplyspECK(dA, dA, dC_reuse, cfg)
        t_reuse, _ = timed(lambda: sa.MultiplyspECK(dA, dA, dC_reuse, cfg))
        print(json.dumps(dict(complete=t_complete, reuse=t_reuse, replayed=bool(cfg.last_stats()["replayed"]))), flush=True)
    cfg.set_stream(None)
    cfg.cleanup()


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="scircuit,cant,webbase,webbase_tri")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--no-baseline", action="store_true", help="the masked legs alone (a kernel trace of them)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masked_time.py needs a GPU")
    if args.child:
        return child(args.child, args.scale)
    dev = torch.device("cuda:0")
    cfg = sa.spECKConfig.initialize(0)
    lines = []
    try:
        for name in args.inputs.split(","):
            A, M = make_inputs(name, args.scale)
            dA = sa.dCSR.from_host(A)
            dM = dA if M is A else sa.dCSR.from_host(M)
            outs = {False: sa.dCSR(), True: sa.dCSR()}
            env = dict(os.environ)
            if args.baseline_lib:
                env["SPECK_LIB"] = os.path.abspath(args.baseline_lib)
            base, ready = None, dict(lib=None, nnz_c=None, products=None)
            if not args.no_baseline:
                base = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", name, "--scale", str(args.scale)],
                                        stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
                ready = json.loads(base.stdout.readline())
            timed = Timer(cfg, dev)
            ms = {"structure": [], "full": [], "complete": [], "reuse": []}
            info = {}
            for r in range(args.warmup + args.rounds):
                take = r >= args.warmup
                for full in (False, True):
                    t, (_, info[full]) = timed(lambda: sa.multiply_masked(dA, dA, dM, cfg, matOut=outs[full], full_pattern=full))
                    if take:
                        ms["full" if full else "structure"].append(t)
                if base is None:
                    continue
                base.stdin.write("round\n")
                base.stdin.flush()
                b = json.loads(base.stdout.readline())
                assert b["replayed"], "the baseline's reuse leg did not replay"
                if take:
                    ms["complete"].append(b["complete"])
                    ms["reuse"].append(b["reuse"])
            if base is not None:
                base.stdin.write("quit\n")
                base.stdin.flush()
                base.wait(timeout=120)
            cfg.set_stream(None)
            i = info[False]
            assert base is None or i.products == ready["products"], "the masked call walks the products of the multiply"
            rec = dict(input=name, scale=args.scale, rows=A.rows, nnz_a=A.nnz, nnz_m=M.nnz, rows_idle=i.rows_idle,
                       rows_group=i.rows_class[0], rows_lds=i.rows_class[1], rows_global=i.rows_class[2],
                       products=i.products, hits=i.hits, nnz_out=i.nnz_out, nnz_full_product=ready["nnz_c"],
                       structure_ms=spread(ms["structure"]), full_pattern_ms=spread(ms["full"]),
                       baseline_complete_ms=spread(ms["complete"]) if base else None,
                       baseline_reuse_ms=spread(ms["reuse"]) if base else None,
                       baseline_lib=ready["lib"], rounds=args.rounds)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            for d in outs.values():
                d.reset()
            del dM, dA
            torch.cuda.empty_cache()
    finally:
        cfg.cleanup()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
