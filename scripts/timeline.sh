#!/bin/bash
# start / duration / end of the last kernels of a bench run (one replayed multiply = the tail): where the time between
# the launches of a replayed sequence goes.  usage (GPU box): bash scripts/timeline.sh tag workload [n] [bench opts...]
TAG=$1; W=$2; N=${3:-24}; shift 3
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_ROOT=${OUT_ROOT:-build/out}  # everything the script writes goes under here
export PYTHONPATH=$PWD
mkdir -p $OUT_ROOT/timeline
rm -rf $OUT_ROOT/_tl_tmp
rocprofv3 --kernel-trace -d $OUT_ROOT/_tl_tmp -o r -- python bench.py --full --workload $W --steps 5 --warmup 3 --no-cpu-baseline --no-config5 --no-configs --no-verify "$@" > $OUT_ROOT/timeline/${TAG}.log 2>&1
db=$(find $OUT_ROOT/_tl_tmp -name "*.db" | head -n 1)
python scripts/rocpd_timeline.py $db $N > $OUT_ROOT/timeline/${TAG}.txt
rm -rf $OUT_ROOT/_tl_tmp
cat $OUT_ROOT/timeline/${TAG}.txt
