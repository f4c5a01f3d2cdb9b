#!/bin/bash
# Second GPU session of a round's profiles (bash tools/profile_extra.sh r5; output under $PROFILE_OUT, default profile_out/): the all-roots
# epoch at 1M nodes, BASELINE configs[2] and the configs[4] size on one GPU, and the per-seed accuracies of the end-to-end float-parity tests.
T=${1:-r5}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${PROFILE_OUT:-$R/profile_out}
mkdir -p $O
cd $R
python -m pytest tests/test_gpu_e2e.py -m gpu -q -s -k "schedule" 2>&1 | grep -E "^seed|^\.seed|schedule:|passed|failed" | sed 's/^\.//' | cut -c1-1200 > $O/${T}_e2e_parity.txt
python tools/epoch_1m.py 1000000 $O/${T}_epoch_1m.json > $O/${T}_epoch_1m.log 2>&1
python bench.py --full --nodes 100000 --roots 8192 --no-cpu-baseline --no-strict --fresh-batches 12 > $O/${T}_bench_100k.json 2> $O/${T}_bench_100k.err
python bench.py --full --nodes 10000000 --emb 256 --roots 512 --steps 5 --warmup 2 --no-cpu-baseline --no-strict --fresh-batches 1 --overlap-steps 0 > $O/${T}_bench_10m.json 2> $O/${T}_bench_10m.err
tail -3 $O/${T}_e2e_parity.txt | cut -c1-300; tail -2 $O/${T}_epoch_1m.log | cut -c1-300; cut -c1-160 $O/${T}_bench_100k.json; cut -c1-160 $O/${T}_bench_10m.json
