#!/bin/bash
# A/B builds of one kernel file with extra -D flags: tools/build_variant.sh NAME FILE.hip -DX ... -> ceracoder_amd/variants/libmi355enc_NAME.so
set -e
cd "$(dirname "$0")/../ceracoder_amd/csrc"
name=$1; file=$2; shift; shift
mkdir -p ../variants
extra=""; case $file in k_deblock.hip|k_intra.hip) extra="-mllvm -amdgpu-sched-strategy=max-ilp";; esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical $extra "$@" -c $file -o ../variants/${file%.hip}_$name.o
objs=""; for o in enc_handle.o enc_input.o enc_schedule.o enc_stages.o enc_scale.o enc_csc.o enc_quality.o enc_overlay.o enc_jpeg.o enc_orient.o enc_image.o enc_snapshot.o enc_rate.o enc_hdr.o enc_adjust.o enc_denoise.o enc_stab.o enc_warp.o enc_autolevel.o enc_dspatial.o enc_lut3d.o enc_roi.o enc_mask.o enc_sync.o k_motion.o k_inter.o k_intra.o k_deblock.o k_handover.o k_scale.o k_csc.o k_quality.o k_overlay.o k_jpeg.o k_orient.o k_image.o k_snapshot.o k_rate.o k_hdr.o k_adjust.o k_denoise.o k_stab.o k_warp.o k_autolevel.o k_dspatial.o k_lut3d.o k_roi.o k_mask.o h264_host.o ratecontrol.o tsmux.o jpeg_host.o image_host.o snapshot_host.o rate_host.o hdr_host.o adjust_host.o denoise_host.o stab_host.o warp_host.o autolevel_host.o dspatial_host.o lut3d_host.o roi_host.o mask_host.o; do
  if [ "$o" = "${file%.hip}.o" ]; then objs="$objs ../variants/${file%.hip}_$name.o"; else objs="$objs $o"; fi; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../variants/libmi355enc_$name.so $objs -lm -lpthread
echo built ../variants/libmi355enc_$name.so
