#!/bin/bash
# Level size A/B (RS_MI355X_MAX_K: caps encode and decode pass levels) on configs 3 and 4
#   bash tools/ab_maxk.sh [out-dir]
set -euo pipefail
O=${1:-ab_out/abk}; mkdir -p $O
for i in 1 2; do
  for k in 5 6 7 8; do
    RS_MI355X_MAX_K=$k timeout -k 10 100 python -u bench.py --full --no-cpu --no-host --no-copy --batch 1 --config 32768x32768x1k --steps 200 --warmup 10 > $O/c3_k${k}_$i.json
    RS_MI355X_MAX_K=$k timeout -k 10 100 python -u bench.py --full --no-cpu --no-host --no-copy --batch 1 --config 8192x8192x64k --steps 10 --warmup 2 > $O/c4_k${k}_$i.json
  done
done
