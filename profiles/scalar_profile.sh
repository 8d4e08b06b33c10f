#!/bin/bash
# Scalar / vector instruction counters of the headline's trace kernel, and its kernel time:  bash profiles/scalar_profile.sh <outdir>
#   (RT_HIP_LIB=<library> RT_HIP_LIB_OLDER=1: an A/B library instead of the tree's own; TRACE=0: the counter passes alone)
# Three rocprofv3 counter passes, each a run of its own with no tracing beside it, over the short child form of the default bench.py
# command (as profiles/smem_profile.sh takes its passes), then one --kernel-trace --stats run of the default command (--no-cold).
# A counter pass that the profiler refuses is reported and skipped; a run that is killed, aborts or times out ends the script.
#   -> <outdir>/pmc_<name>/ (profiles/pmc_medians.py <outdir> prints the per-launch medians), <outdir>/trace/, <outdir>/summary.txt
set -uo pipefail
OUT=$1; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
REPO=$(cd "$(dirname "$0")/.." && pwd)
cd "$REPO"
fatal() { case $1 in 124|137|134|139) echo "run ended with status $1: stopping" | tee -a "$OUT/summary.txt"; exit $1 ;; esac; }
pass() {                    # pass <name> <counters...>
  local name=$1; shift
  RT_BENCH_CHILD=1 RT_BENCH_NO_SETTLE=1 timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d "$OUT/pmc_$name" -- \
    python3 bench.py --steps 12 --warmup 2 --no-pmc --no-cpu-baseline > "$OUT/pmc_$name.log" 2>&1
  local rc=$?
  fatal $rc
  [ $rc -ne 0 ] && echo "pass $name ($*) failed with status $rc: $(tail -n 2 "$OUT/pmc_$name.log" | tr '\n' ' ')" | tee -a "$OUT/summary.txt"
  return 0
}
: > "$OUT/summary.txt"
pass insts SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VALU SQ_WAVES
pass active SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES
pass fp64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_TRANS_F64
python3 profiles/pmc_medians.py "$OUT" | tee -a "$OUT/summary.txt"
find "$OUT" -name '*counter_collection.csv' -delete     # (the per-launch rows: the medians above are kept)
[ "${TRACE:-1}" = 1 ] || exit 0
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
  python3 bench.py --steps 500 --warmup 10 --no-pmc --no-cpu-baseline --no-cold > "$OUT/trace.log" 2>&1
rc=$?; fatal $rc
[ $rc -ne 0 ] && { echo "kernel trace failed with status $rc" | tee -a "$OUT/summary.txt"; exit $rc; }
for f in $(find "$OUT/trace" -name '*kernel_stats.csv'); do head -n 3 "$f" | tee -a "$OUT/summary.txt"; done
find "$OUT/trace" -name '*kernel_trace.csv' -delete          # (the per-launch rows: megabytes; the statistics are kept)
