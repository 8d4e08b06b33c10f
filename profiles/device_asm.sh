#!/bin/bash
# The device-assembly gate of a source-only change to the trace kernels:  profiles/device_asm.sh <tree> <outdir>
# Compiles <tree>/html5-canvas-raytracer_amd/csrc/rt_kernel.hip device-only to assembly with the Makefile's own COMMON / KFLAGS plus
# -cuid=compare (without it the unit's id, a hash of the source, is the one symbol that differs) for
#   fast, strict, test_fast, test_strict      RT_STRICT 0 / 1, as the product build and with -DRT_TESTING
#   ablate_<NAME>                             one test build (RT_STRICT=0) per RT_ABLATE_<NAME> named in rt_kernel*.hip / .h or rt_device.h
#   wave_log                                  the product build with -DRT_WAVE_LOG - as LLVM IR (wave_log.ll): the backend refuses this build
#                                             ("illegal VGPR to SGPR copy" in rt_trace), so the last form that exists is compared, with
#                                             the inline asm statements' !srcloc cookies - positions in the source text - set to 0
# -> <outdir>/<build>.s and <outdir>/sha256.txt (one line per build).  It compiles and hashes, nothing else; two trees are compared with
#   for f in A/*.s A/*.ll; do cmp $f B/$(basename $f); done        (JOBS=<n>: compilations at a time, default 4)
set -euo pipefail
TREE=$(cd "$1" && pwd); mkdir -p "$2"; OUT=$(cd "$2" && pwd)
SRC=$TREE/html5-canvas-raytracer_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON=$(make -s --no-print-directory -C "$SRC" print-COMMON); KFLAGS=$(make -s --no-print-directory -C "$SRC" print-KFLAGS)
FAST="-DRT_STRICT=0 -ffp-contract=fast"; STRICT="-DRT_STRICT=1 -ffp-contract=off"
BUILDS=("fast $FAST" "strict $STRICT" "test_fast -DRT_TESTING $FAST" "test_strict -DRT_TESTING $STRICT" "wave_log -emit-llvm -DRT_WAVE_LOG $FAST")
for a in $(cat "$SRC"/rt_kernel*.hip "$SRC"/rt_kernel*.h "$SRC"/rt_device.h 2>/dev/null | grep -o 'RT_ABLATE_[A-Z0-9_]*' | sort -u); do
  BUILDS+=("ablate_${a#RT_ABLATE_} -DRT_TESTING -D$a $FAST")
done
cd "$SRC"                                            # (the Makefile's own working directory: no path of the tree in the output)
rm -f "$OUT"/*.s "$OUT"/*.ll "$OUT"/sha256.txt "$OUT"/failed
for b in "${BUILDS[@]}"; do
  while [ "$(jobs -rp | wc -l)" -ge "${JOBS:-4}" ]; do wait -n || true; done
  case "$b" in *-emit-llvm*) e=ll ;; *) e=s ;; esac
  ($HIPCC $COMMON $KFLAGS ${b#* } -cuid=compare --offload-device-only -S rt_kernel.hip -o "$OUT/${b%% *}.$e" || echo "${b%% *}" >> "$OUT/failed") &
done
wait
sed -i -E 's/^(![0-9]+ = !\{i64 )[0-9]+\}$/\10}/' "$OUT"/*.ll
if [ -e "$OUT/failed" ]; then echo "failed to compile: $(tr '\n' ' ' < "$OUT/failed")" >&2; exit 1; fi
(cd "$OUT" && sha256sum *.s *.ll > sha256.txt && cat sha256.txt)
