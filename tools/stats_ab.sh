#!/bin/bash
# Usage (GPU box): tools/stats_ab.sh <tag> "ENV1=a" "ENV1=b" ... - build the EGR_TRAVERSAL_STATS=1 variant of each build-time setting, print the per-phase
# cycle sums and visit counters of one full-size grad launch per cloud variant (VARIANTS, default "init trained")
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; shift
mkdir -p $RUNS/$TAG
for CFG in "$@"; do
  NAME=$(echo "$CFG" | tr ' =' '__')
  env EGR_TRAVERSAL_STATS=1 $CFG tools/build_variant.sh > $RUNS/$TAG/build_$NAME.log 2>&1 || { echo "$CFG: BUILD FAILED"; tail -5 $RUNS/$TAG/build_$NAME.log; continue; }
  for V in ${VARIANTS:-init trained}; do
    echo "== $CFG $V"
    env EGR_TRAVERSAL_STATS=1 $CFG GRADS=1 VARIANT=$V EGR_PRINT_TRAVERSAL_STATS=1 python tools/stats_run.py 2>&1 | grep -a "egr stats\|rays" | tee $RUNS/$TAG/stats_${NAME}_$V.txt
  done
done
