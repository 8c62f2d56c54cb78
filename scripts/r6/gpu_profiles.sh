#!/bin/bash
# Round-6 profiles on one MI355X (outputs under $OUT/, copied to profiles/r6 by hand):
#  1. PMC FETCH_SIZE / WRITE_SIZE passes (separate runs) over every cycle operation of the sa27
#     and g3sub hierarchies (the SA definition changed: new formats) and of 7-pt -> the
#     pmc_vcycle_kernels*.json files bench.py reads for its traffic column;
#  2. rocprofv3 --kernel-trace --stats of the default bench command (7-pt), its summary.
set -o pipefail
cd "$(dirname "$0")/../.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
R=${R:-s6p}
for CFG in ${PMC_CONFIGS:-sa27 g3sub 7pt}; do
  for pass in FETCH_SIZE WRITE_SIZE; do
    AMG_PMC_OPS=$OUT/${R}_${CFG}_pmc_ops.json timeout -k 10 -s KILL 300 rocprofv3 --pmc $pass --output-format csv \
      -d $OUT/${R}_${CFG}_vpmc_$pass -o run -- python scripts/pmc_vcycle.py 256 $CFG \
      > $OUT/${R}_${CFG}_vpmc_$pass.log 2>&1 || { tail -5 $OUT/${R}_${CFG}_vpmc_$pass.log; exit 1; }
  done
  python scripts/pmc_vcycle_traffic.py $OUT/${R}_${CFG}_vpmc $OUT/${R}_${CFG}_pmc_ops.json \
    $OUT/${R}_pmc_vcycle_kernels_${CFG}.json || exit 1
  echo "pmc $CFG done"
done
if [ -z "$NO_TRACE" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_prof -o run -- \
    python bench.py --full --no-cpu-baseline > $OUT/${R}_prof_bench.json 2> $OUT/${R}_prof_bench.err || { tail $OUT/${R}_prof_bench.err; exit 1; }
  python scripts/trace_summary.py $OUT/${R}_prof/run_kernel_trace.csv > $OUT/${R}_trace_summary.txt
  cp $OUT/${R}_prof/run_kernel_stats.csv $OUT/${R}_kernel_stats.csv
  head -14 $OUT/${R}_trace_summary.txt
fi
echo profiles-done
