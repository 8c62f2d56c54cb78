#!/bin/bash
# Round-2 check on one MI355X: gpu tests (verbose, per-test timeout), smoke, the default bench
# line.  ROUND names the output files under $OUT/.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
R=${ROUND:-r2}
TESTS=${TESTS:-tests}
timeout -k 10 900 python -u -m pytest $TESTS -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${R}_tests.log 2>&1 || { tail -40 $OUT/${R}_tests.log; exit 1; }
tail -1 $OUT/${R}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${R}_smoke.log 2>&1 || { tail $OUT/${R}_smoke.log; exit 1; }
tail -1 $OUT/${R}_smoke.log
timeout -k 10 600 python bench.py --full $BENCH_ARGS > $OUT/${R}_bench.json 2> $OUT/${R}_bench.err || { tail $OUT/${R}_bench.err; exit 1; }
cat $OUT/${R}_bench.json
