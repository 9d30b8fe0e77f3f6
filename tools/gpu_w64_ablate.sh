#!/bin/bash
# Per-launch times of the 64-channel Winograd layers, shipped library against the no-stores build of that kernel
# (make -C gance_amd/csrc w64ablate: GANCE_W64_ABLATE=1, wrong results by design). GANCE_TUNE_WINO43=0: the default plan
# runs these layers in F(4x4,3x3) form, and this kernel only without it.
steps=$(mktemp)
for lib in "" _w64ab1; do
  GANCE_TUNE_WINO43=0 GANCE_HIP_LIBRARY=$PWD/gance_amd/libgance_hip$lib.so timeout -k 10 200 python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras --print-steps \
    > /dev/null 2> $steps || exit 1
  echo "libgance_hip$lib: $(grep convW $steps | awk '{printf "%s ", $2}')"
done
