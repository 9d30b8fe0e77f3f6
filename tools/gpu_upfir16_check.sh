#!/bin/bash
# Parity subset of the 16-channel fused up kernel (upfir16_fused.hip):
#   bash tools/gpu_upfir16_check.sh tag
# writes upfir16_<tag>_tests.log into the run's output directory
tag=${1:-a}
mkdir -p gpurun_out
timeout -k 10 420 python -m pytest tests/test_synthesis_gpu.py -m gpu -x -q -s \
  -k "fused_upsampling or 512_both or every_term_on_default or noise_draws" > gpurun_out/upfir16_${tag}_tests.log 2>&1
echo "pytest rc=$?" >> gpurun_out/upfir16_${tag}_tests.log
tail -4 gpurun_out/upfir16_${tag}_tests.log
