#!/bin/bash
# Build A/B variants of librt_hip.so with extra kernel flags:  profiles/ab_build.sh <name> "<KFLAGS>" [product]
# -> build/ab/librt_hip_<name>.so   (bench with RT_HIP_LIB=<that path>); a test build (-DRT_TESTING) unless "product" is given
set -e
#    "hybrid": product kernels (96 VGPRs) under a test-build host layer, so that the host's environment switches exist (the probe fields
#    the test build appends to rt_launch are its LAST members: the product kernels read the prefix they know)
NAME=$1; FLAGS=$2; TESTING=-DRT_TESTING; APITESTING=-DRT_TESTING
[ "${3:-}" = product ] && { TESTING=; APITESTING=; }
[ "${3:-}" = hybrid ] && { TESTING=; APITESTING=-DRT_TESTING; }
REPO=$(cd "$(dirname "$0")/.." && pwd)
SRC=$REPO/html5-canvas-raytracer_amd/csrc
OUT=$REPO/build/ab; mkdir -p $OUT
T=$(mktemp -d)
COMMON="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-fast-math -I$SRC"
KERNEL="$COMMON -mllvm -disable-machine-licm $TESTING $FLAGS"
# the objects librt_hip.so links, from the Makefile; each is compiled as the Makefile does, with FLAGS added
OBJS=$(make -s --no-print-directory -C $SRC print-LIB_OBJS); HOST=" $(make -s --no-print-directory -C $SRC print-HOST) "
for o in $OBJS; do
  u=${o%.o}
  case "$u" in
    rt_kernel_fast)   /opt/rocm/bin/hipcc $KERNEL -DRT_STRICT=0 -ffp-contract=fast -c $SRC/rt_kernel.hip -o $T/$o & ;;
    rt_kernel_strict) /opt/rocm/bin/hipcc $KERNEL -DRT_STRICT=1 -ffp-contract=off -c $SRC/rt_kernel.hip -o $T/$o & ;;
    rt_tables)        /opt/rocm/bin/hipcc -O2 -std=c++17 -fPIC -Wall -I$SRC $FLAGS -x c++ -c $SRC/rt_tables.cpp -o $T/$o & ;;
    *) if [ "${HOST#* $u }" != "$HOST" ]; then /opt/rocm/bin/hipcc $COMMON $APITESTING $FLAGS -c $SRC/$u.hip -o $T/$o &     # the host layer
       else /opt/rocm/bin/hipcc $COMMON $FLAGS -ffp-contract=off -c $SRC/$u.hip -o $T/$o &                                     # the tables / objects / hits builders
       fi ;;
  esac
done
wait
(cd $T && /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $OUT/librt_hip_$NAME.so $OBJS -ldl)
cp $T/rt_kernel_fast.o $OUT/rt_kernel_fast_$NAME.o      # for profiles/kernel_resources.sh / isa_histogram.sh
rm -rf $T
echo built $OUT/librt_hip_$NAME.so
