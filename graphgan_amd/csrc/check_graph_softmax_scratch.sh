#!/bin/bash
# The graph-softmax kernels (graph_softmax.hip: gs_fill_kernel<NCH>, the level / long-list / abort / gather kernels) keep their
# rows, candidates and partial sums in registers: an instantiation that spills runs slowly without failing any test.
# Fail the build if one of them uses scratch or spills.
#   usage: check_graph_softmax_scratch.sh <kernel-resource-usage remarks>
R=$1
N=$(grep -c 'Function Name: _ZN2gg12_GLOBAL__N_1[0-9]*gs_[a-z_]*kernel' "$R")
BAD=$(awk '/Function Name:/{k = ($0 ~ /gs_[a-z_]*kernel/) ? $5 : ""}
           /ScratchSize \[bytes\/lane\]:|VGPRs Spill:/{ v = $(NF-1); if (k != "" && v != 0) print k, $0 }' "$R")
if [ "$N" -lt 10 ]; then echo "check_graph_softmax_scratch: expected 10 graph-softmax kernels, found $N" >&2; exit 1; fi
if [ -n "$BAD" ]; then echo "check_graph_softmax_scratch: a graph-softmax kernel spills: $BAD" >&2; exit 1; fi
echo "check_graph_softmax_scratch: $N graph-softmax kernels, no scratch, no spill"
