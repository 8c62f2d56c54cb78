#!/bin/bash
# setup phase timing (AMG_TIMING=1) for the three single-GPU bench configs
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
for cfg in 7pt sa27 g3sub; do
  AMG_TIMING=1 timeout -k 10 400 python bench.py --full --config $cfg --steps 5 --warmup 1 --no-cpu-baseline --spmv-reps 5 > $OUT/setup_$cfg.json 2> $OUT/setup_$cfg.err || { tail $OUT/setup_$cfg.err; exit 1; }
  echo "== $cfg"; grep -E "\[amg\]|setup|built" $OUT/setup_$cfg.err
done
