#!/bin/bash
# build_variant.sh <suffix> <source under quantized-cnn_amd/csrc> <extra hipcc flags...>: libqcnn_hip<suffix>.so = the
# current objects with ONE source recompiled under extra flags (timing experiments; select with QCNN_HIP_LIB)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
sfx=$1; src=$2; shift 2
C=$R/quantized-cnn_amd/csrc
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $C/$src -o /tmp/variant$sfx.o
objs=""
# the object list of the default build (build.py's HIP_SOURCES), so that a variant exports every entry point
for o in $(cd $R/quantized-cnn_amd && python -c "import build; print(' '.join(build.HIP_SOURCES))"); do
  if [ "$o" == "$src" ]; then objs="$objs /tmp/variant$sfx.o"; else objs="$objs $C/$o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/quantized-cnn_amd/libqcnn_hip$sfx.so $objs -L/opt/rocm/lib -lrccl -lpthread
echo built libqcnn_hip$sfx.so
