#!/bin/bash
# Usage (GPU box): tools/sweep2.sh <tag> "ENV1=a ENV2=b" ...  - like sweep.sh, with the primary-only leg and the per-kernel times of both variants on one line each
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; shift
mkdir -p $RUNS/$TAG
for CFG in "$@"; do
  NAME=$(echo "$CFG" | tr ' =' '__')
  env $CFG tools/build_variant.sh > $RUNS/$TAG/build_$NAME.log 2>&1 || { echo "$CFG: BUILD FAILED"; tail -5 $RUNS/$TAG/build_$NAME.log; continue; }
  env $CFG python bench.py --full --no-cpu-baseline --steps 60 --warmup 40 ${SWEEP_ARGS} > $RUNS/$TAG/bench_$NAME.json 2> $RUNS/$TAG/bench_$NAME.err
  python - <<PY
import json
try:
    d=json.load(open("$RUNS/$TAG/bench_$NAME.json")); o=d.get("other_variant") or {}
    km=lambda k: {x:k[x] for x in ("forward_chain","backward_chain") if x in k}
    print("$CFG: init", d["value"], d["ms_per_step"], km(d["kernel_ms"]), "primary-only", (d.get("primary_only") or {}).get("ms_per_step"), "| trained", o.get("value"), o.get("ms_per_step"), km(o.get("kernel_ms") or {}), "primary-only", (o.get("primary_only") or {}).get("ms_per_step"), "status", d["status"])
except Exception as e:
    print("$CFG: FAILED", e)
PY
done
