#!/bin/bash
# Diagnostic builds of libsvo_hip into build_ab/ (git-ignored; travels to the GPU box):
#   build_variants.sh stamps            -> build_ab/libsvo_hip_stamps.so  (-DSVO_SIA_STAMPS)
#   build_variants.sh stamps_chain -DSVO_SIA_STAMPS -DSVO_SIA_PRELOAD=0 -> the same stamps on the loads as they were before round 7
#   build_variants.sh <tag> <flags...>  -> build_ab/libsvo_hip_<tag>.so   (extra hipcc flags)
# sia_gn_kernel<1,2> (sia.hip): -DSVO_SIA_STG1=64 stages 64 keypoints at a time (36 KB of LDS),
#   -DSVO_SIA_ACC_U=4 adds four keypoints per trip (over 256 registers), -DSVO_SIA_OCC=n caps the registers,
#   -DSVO_SIA_PRELOAD=0 loads MODE 2's operands where they are used, one behind the other (the kernels of round 6, instruction
#   for instruction), -DSVO_SIA_QREG=0 hands the projections from cost() to get_gradient through kp_ws.
# ssd_disparity_kernel (depth.hip): build_variants.sh ssd4 -DSVO_SSD_FOUR_WAVES launches the four-wave kernel that the one-wave
#   kernel replaced (kept in svo_capi_check.hip) on the product path: the parent's SSD shape without a parent checkout.
# Run it in a checkout of the commit to compare against for that commit's library; never while a source is being edited.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/stereo-svo-slam_amd/csrc
TAG=$1; shift
FLAGS="$@"
[ "$TAG" = stamps ] && FLAGS="-DSVO_SIA_STAMPS $FLAGS"
mkdir -p $ROOT/build_ab/$TAG
# (the sources of libsvo_hip.so, as the Makefile lists them)
SRC=$(sed -n 's/^SRC *:= *//p' $CSRC/Makefile)
for f in ${SRC//.hip/}; do
  /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 $FLAGS -c $CSRC/$f.hip -o $ROOT/build_ab/$TAG/$f.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $ROOT/build_ab/libsvo_hip_$TAG.so $ROOT/build_ab/$TAG/*.o
ls -la $ROOT/build_ab/libsvo_hip_$TAG.so
