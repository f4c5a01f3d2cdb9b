#!/bin/bash
# The kernels that keep their operands, accumulators and running state in registers (the wide all-pairs kernel, the tile-stream
# kernels of all_score.hip and topk_score.hip, the graph-softmax kernels): an instantiation that does not fit moves whole arrays
# to scratch and runs at a fraction of its speed without failing any test.  Fail the build if one uses scratch or spills.
#   usage: check_no_scratch.sh <kernel-resource-usage remarks> [<kernel-name regex> <min count> <label>] ...
# The regex is matched against the (mangled) function name, so it names the kernel, not its namespace.  Without one, every
# kernel of the file is audited.
R=$1
shift
[ $# -ge 3 ] || set -- '.' 1 'kernels'
while [ $# -ge 3 ]; do
    PAT=$1 MIN=$2 LABEL=$3
    shift 3
    N=$(awk -v pat="$PAT" '/Function Name:/ && $5 ~ pat { n++ } END { print n + 0 }' "$R")
    BAD=$(awk -v pat="$PAT" '/Function Name:/{k = ($5 ~ pat) ? $5 : ""}
               /ScratchSize \[bytes\/lane\]:|VGPRs Spill:/{ v = $(NF-1); if (k != "" && v != 0) print k, $0 }' "$R")
    if [ "$N" -lt "$MIN" ]; then echo "check_no_scratch: expected at least $MIN $LABEL, found $N" >&2; exit 1; fi
    if [ -n "$BAD" ]; then echo "check_no_scratch: $LABEL spills: $BAD" >&2; exit 1; fi
    echo "check_no_scratch: $N $LABEL, no scratch, no spill"
done
