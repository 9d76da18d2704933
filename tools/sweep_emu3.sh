#!/bin/bash
# Usage (GPU box): tools/sweep_emu3.sh <tag> <world> "BUILDENV1" "BUILDENV2" ... - rank 0 of an emulated partition (team help on) per build-time setting, both clouds, two runs each
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; W=$2; shift 2
mkdir -p $RUNS/$TAG
for B in "$@"; do
  env $B tools/build_variant.sh > $RUNS/$TAG/build.log 2>&1 || { echo "$B: BUILD FAILED"; tail -5 $RUNS/$TAG/build.log; continue; }
  for V in init trained; do for rep in 1 2; do
    env $B python bench.py --full --no-cpu-baseline --no-second-variant --steps 60 --warmup 40 --primary-steps 0 --emulate-world $W --variant $V 2>/dev/null | tail -1 > $RUNS/$TAG/emu.json
    python - <<PY
import json
d = json.load(open("$RUNS/$TAG/emu.json"))
print("$B | world $W $V:", d["ms_per_step"], {k: d["kernel_ms"][k] for k in ("forward_chain", "backward_chain")}, "status", d["status"])
PY
  done; done
done
