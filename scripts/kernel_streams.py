#!/usr/bin/env python3
"""Compare the kernels of two device-only assembly listings of one source file:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ispeck_amd/csrc --cuda-device-only -S speck_amd/csrc/X.hip -o X.s
Kernel names come from the .amdhsa_kernel lines.  A kernel's instruction stream is what stands between its label and its
.Lfunc_end, with comments and runs of whitespace removed and the function index taken out of the BB<n>_ / func_end<n>
labels (the index counts the functions of the listing in front of it); the streams are compared by their sha1.
usage: kernel_streams.py before.s after.s     (exit status 1: a kernel both listings have differs)"""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")]
    out = {}
    for n in names:
        i = next(k for k, l in enumerate(lines) if l.startswith(n + ":"))
        body = []
        for l in lines[i + 1:]:
            l = re.sub(r"\s+", " ", l.split(";")[0]).strip()
            l = re.sub(r"BB\d+_", "BB_", re.sub(r"func_end\d+", "func_end", l))
            if l.startswith(".Lfunc_end"):
                break
            if l:
                body.append(l)
        out[n] = (hashlib.sha1("\n".join(body).encode()).hexdigest()[:12], len(body))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    short = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout.split("\n")))
    diff = 0
    for n in names:
        if n in a and n in b:
            same = a[n] == b[n]
            diff += not same
            print(f"{'same' if same else 'DIFF'}  {a[n][0]} {a[n][1]:6d} lines  {short[n]}")
    for n in names:
        if n not in b:
            print(f"gone  {a[n][0]} {a[n][1]:6d} lines  {short[n]}")
    for n in names:
        if n not in a:
            print(f"NEW   {b[n][0]} {b[n][1]:6d} lines  {short[n]}")
    print(f"# {len(a)} kernels before, {len(b)} after: {sum(n in b for n in a)} in both, {diff} of them differ, "
          f"{sum(n not in b for n in a)} gone, {sum(n not in a for n in b)} new")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
