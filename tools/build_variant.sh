#!/bin/bash
# Build a variant of libimsegm_hip.so with extra compile flags for ONE source file, for A/B runs on the same GPU box:
#   tools/build_variant.sh volprof volume.hip -DIMSEGM_VOL_PHASE_PROF
#   tools/build_variant.sh base                       (a copy of the current library)
# -> pyimsegm_amd/build/variants/<name>.so ; select it with IMSEGM_HIP_LIBRARY (tools/ab/run.py alternates two libraries on one box).
# The kernels take no -D tuning switch: their tile shapes, wave counts and phase lengths are constants in csrc/ with the measurements
# next to them (to try another value, edit the constant in a copy of the tree and build `base` there).  The one compile-time
# option is the instrumentation IMSEGM_VOL_PHASE_PROF (tools/vol_phase_probe.py).
set -e
REPO=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
python -m pyimsegm_amd.build > /dev/null
mkdir -p $REPO/pyimsegm_amd/build/variants
if [ $# -eq 0 ]; then cp $REPO/pyimsegm_amd/libimsegm_hip.so $REPO/pyimsegm_amd/build/variants/$NAME.so; echo "$NAME = current library"; exit 0; fi
SRC=$1; shift
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wno-unused-function"
OBJ=/tmp/variant_${NAME}_${SRC%.hip}.o
/opt/rocm/bin/hipcc $FLAGS "$@" -c $REPO/pyimsegm_amd/csrc/$SRC -o $OBJ
OBJS=$(ls $REPO/pyimsegm_amd/build/*.o | grep -v "/${SRC%.hip}.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $REPO/pyimsegm_amd/build/variants/$NAME.so $OBJS $OBJ
echo "built pyimsegm_amd/build/variants/$NAME.so ($SRC $*)"
