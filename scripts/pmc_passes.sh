#!/bin/bash
# usage (GPU box): bash scripts/pmc_passes.sh <tag> <workload> [bench opts...]   -> $OUT_ROOT/pmc/<tag>_passN.csv
# separate rocprofv3 --pmc passes (kernel-trace only, counters in runs of their own) of a short bench run
TAG=$1; W=$2; shift 2
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT_ROOT=${OUT_ROOT:-build/out}  # everything the script writes goes under here
export PYTHONPATH=$PWD
mkdir -p $OUT_ROOT/pmc
PASSES=(
 "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM"
 "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM_RD SQ_INST_CYCLES_VMEM_WR SQ_WAIT_INST_LDS SQ_INSTS_SALU"
 "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS_ATOMIC SQ_WAVES SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS SQ_LEVEL_WAVES GRBM_GUI_ACTIVE"
 "TA_TA_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum"
 "TCP_TCP_TA_DATA_STALL_CYCLES_sum TCP_PENDING_STALL_CYCLES_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_DATA_STALLED_BY_TC_CYCLES_sum"
 "TA_FLAT_READ_WAVEFRONTS_sum TA_FLAT_WRITE_WAVEFRONTS_sum TCP_GATE_EN1_sum TCP_TCC_READ_REQ_LATENCY_sum"
)
i=0
for p in "${PASSES[@]}"; do
  i=$((i+1))
  rm -rf $OUT_ROOT/_pmc_tmp
  timeout 600 rocprofv3 --kernel-trace --pmc $p -d $OUT_ROOT/_pmc_tmp -o r -- python bench.py --full --workload $W --steps 3 --warmup 2 --no-cpu-baseline --no-config5 --no-configs --no-verify "$@" > $OUT_ROOT/pmc/${TAG}_pass$i.log 2>&1
  db=$(find $OUT_ROOT/_pmc_tmp -name "*.db" | head -n 1)
  if [ -n "$db" ]; then python scripts/rocpd_pmc.py $db $OUT_ROOT/pmc/${TAG}_pass$i.csv > /dev/null; else echo "pass $i: no db"; tail -n 3 $OUT_ROOT/pmc/${TAG}_pass$i.log; fi
done
rm -rf $OUT_ROOT/_pmc_tmp
