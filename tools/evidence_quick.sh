#!/bin/bash
# Usage (GPU box): tools/evidence_quick.sh <tag>  - the short evidence run: GPU suite, smoke, the default bench line, rocprofv3 kernel stats of the
# headline variant, rank 0 of an emulated 8-way partition. (tools/evidence.sh adds the PMC passes, config B, N = 2 / 4 and the soak.)
export TMPDIR=/tmp; cd "$(dirname "$0")/.."  # the repository root
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
T=${1:-r4quick}
mkdir -p $RUNS/$T
( time python -m pytest tests -m gpu -q -s -p no:cacheprovider ) > $RUNS/$T/tests.log 2>&1; tail -4 $RUNS/$T/tests.log
grep -a -o "REPORT.*" $RUNS/$T/tests.log > $RUNS/$T/parity_levels.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
python bench.py --full > $RUNS/$T/bench_line_default.json 2> $RUNS/$T/bench_default.err; cut -c1-400 $RUNS/$T/bench_line_default.json
mkdir -p $RUNS/$T/prof
rocprofv3 --kernel-trace --stats --output-format csv -d $RUNS/$T/prof/trace_init -o t -- python bench.py --full --steps 100 --warmup 300 --prewarm-seconds 3 --no-cpu-baseline --no-second-variant --primary-steps 0 --variant init > $RUNS/$T/prof/bench_under_rocprof_init.log 2>&1
grep -a "^{" $RUNS/$T/prof/bench_under_rocprof_init.log | tail -1 > $RUNS/$T/prof/bench_line_under_rocprof_init.json
find $RUNS/$T/prof/trace_init -name "*kernel_stats.csv" -exec cp {} $RUNS/$T/rocprofv3_kernel_stats_init.csv \;
rm -rf $RUNS/$T/prof/trace_init
head -8 $RUNS/$T/rocprofv3_kernel_stats_init.csv
bash tools/emu.sh $T 8
