#!/bin/bash
# A/B builds of one kernel file with extra -D flags: tools/build_variant.sh NAME FILE.hip -DX ... -> ceracoder_amd/variants/libmi355enc_NAME.so
set -e
cd "$(dirname "$0")/../ceracoder_amd/csrc"
name=$1; file=$2; shift; shift
mkdir -p ../variants
extra=""; case $file in k_deblock.hip|k_intra.hip) extra="-mllvm -amdgpu-sched-strategy=max-ilp";; esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical $extra "$@" -c $file -o ../variants/${file%.hip}_$name.o
objs=""; for o in $(make -s --no-print-directory objs); do # (the library's objects are the Makefile's to name)
  if [ "$o" = "${file%.hip}.o" ]; then objs="$objs ../variants/${file%.hip}_$name.o"; else objs="$objs $o"; fi; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../variants/libmi355enc_$name.so $objs -lm -lpthread
echo built ../variants/libmi355enc_$name.so
