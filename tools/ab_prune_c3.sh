#!/bin/bash
# Alternating A/B of the decode pruning on config 3 only (no other workload between runs)
#   bash tools/ab_prune_c3.sh [out-dir]
set -euo pipefail
O=${1:-ab_out/ab3}; mkdir -p $O
for i in 1 2 3; do
  for m in 0 1; do
    RS_MI355X_DECODE_PRUNE=$m timeout -k 10 100 python -u bench.py --full --no-cpu --no-host --no-copy --batch 1 --config 32768x32768x1k --steps 400 --warmup 20 > $O/c3_m${m}_$i.json
  done
done
