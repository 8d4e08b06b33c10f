#!/bin/bash
# On the GPU box: bench each named A/B build (build/ab/librt_hip_<name>.so), interleaved, 2 rounds.
#   bash profiles/ab_run.sh w2 w4 ...      prints: name Mpixel/s ms_per_step kernel_ms max_lsb [new_camera_every_step ms]
#   ROUNDS=3 STEPS=2000 WARMUP=20 ...      more rounds, the default command's steps;  COLD=1: with the cold-frame / moving-camera legs of --full
#   Every bench run under its own time limit (STEP_LIMIT seconds); a run that fails ends the script.
STEPS=${STEPS:-100}
STEP_LIMIT=${STEP_LIMIT:-300}
NOCOLD=--no-cold; [ "${COLD:-0}" = 1 ] && NOCOLD=
ERR=$(mktemp)
for round in $(seq 1 ${ROUNDS:-2}); do
for v in "$@"; do
  LIB=$PWD/build/ab/librt_hip_$v.so
  [ "$v" = "product" ] && LIB=$PWD/html5-canvas-raytracer_amd/csrc/librt_hip.so
  RT_HIP_LIB_OLDER=1 RT_HIP_LIB=$LIB timeout -k 10 $STEP_LIMIT python3 bench.py --steps $STEPS --warmup ${WARMUP:-10} --full --no-cpu-baseline --no-pmc $NOCOLD ${BENCH_ARGS:-} 2>$ERR | python3 -c "
import json,sys
l=sys.stdin.readline()
try:
    d=json.loads(l); print('$v', d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['max_lsb_vs_reference_rows'], (d.get('new_camera_every_step') or {}).get('ms_per_step', ''))
except Exception as e: print('$v FAILED', l[:200]); print(open('$ERR').read()[-1500:]); sys.exit(1)
" || { rm -f $ERR; exit 1; }
done; done
rm -f $ERR
