#!/bin/bash
# The top-K consumer (topk_score.hip: topk_f32_kernel, topk_bf16_kernel<KS>) keeps its accumulators, the requested rows'
# fragments and the per-row thresholds in registers: an instantiation that spills runs slowly without failing any test.
# Fail the build if one of them uses scratch or spills.
#   usage: check_topk_scratch.sh <kernel-resource-usage remarks>
R=$1
N=$(grep -c 'Function Name: _ZN2gg12_GLOBAL__N_1[0-9]*topk_\(f32\|bf16\)_kernel' "$R")
BAD=$(awk '/Function Name:/{k = ($0 ~ /topk_(f32|bf16)_kernel/) ? $5 : ""}
           /ScratchSize \[bytes\/lane\]:|VGPRs Spill:/{ v = $(NF-1); if (k != "" && v != 0) print k, $0 }' "$R")
if [ "$N" -lt 5 ]; then echo "check_topk_scratch: expected 5 instantiations of the top-K tile-stream kernels, found $N" >&2; exit 1; fi
if [ -n "$BAD" ]; then echo "check_topk_scratch: a top-K tile-stream kernel spills: $BAD" >&2; exit 1; fi
echo "check_topk_scratch: $N instantiations of the top-K tile-stream kernels, no scratch, no spill"
