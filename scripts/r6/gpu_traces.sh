#!/bin/bash
# rocprofv3 --kernel-trace --stats of the bench command per config (round 6, final tree): the
# summaries the bench lines' in-graph roofline is cross-checked against (outputs under $OUT/)
set -o pipefail
cd "$(dirname "$0")/../.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
R=${R:-s6r}
for cfg in ${CONFIGS:-sa27 g3sub}; do
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_prof_$cfg -o run -- \
    python bench.py --full --config $cfg --no-cpu-baseline $EXTRA > $OUT/${R}_prof_bench_$cfg.json 2> $OUT/${R}_prof_bench_$cfg.err || { tail $OUT/${R}_prof_bench_$cfg.err; exit 1; }
  python scripts/trace_summary.py $OUT/${R}_prof_$cfg/run_kernel_trace.csv > $OUT/${R}_trace_summary_$cfg.txt
  cp $OUT/${R}_prof_$cfg/run_kernel_stats.csv $OUT/${R}_kernel_stats_$cfg.csv
  head -8 $OUT/${R}_trace_summary_$cfg.txt
done
echo traces-done
