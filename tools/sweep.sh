#!/bin/bash
# Usage (GPU box): tools/sweep.sh <tag> "ENV1=a ENV2=b" "ENV1=c" ...   - build the variant of each build-time setting and bench it
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; shift
mkdir -p $RUNS/$TAG
for CFG in "$@"; do
  NAME=$(echo "$CFG" | tr ' =' '__')
  env $CFG tools/build_variant.sh > $RUNS/$TAG/build_$NAME.log 2>&1 || { echo "$CFG: BUILD FAILED"; tail -5 $RUNS/$TAG/build_$NAME.log; continue; }
  env $CFG python bench.py --full --no-cpu-baseline --steps 60 --warmup 40 ${SWEEP_ARGS:---no-second-variant} > $RUNS/$TAG/bench_$NAME.json 2> $RUNS/$TAG/bench_$NAME.err
  python - <<PY
import json
try:
    d=json.load(open("$RUNS/$TAG/bench_$NAME.json")); o=d.get("other_variant") or {}
    print("$CFG:", d["value"], d["ms_per_step"], {k:d["kernel_ms"][k] for k in ("forward_chain","backward_chain")}, "status", d["status"], "| other", o.get("value"), (o.get("kernel_ms") or {}).get("forward_chain"), (o.get("kernel_ms") or {}).get("backward_chain"))
except Exception as e:
    print("$CFG: FAILED", e)
PY
done
