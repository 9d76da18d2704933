#!/bin/bash
# Usage (GPU box): tools/sweep_emu.sh <tag> "ENV1=a ENV2=b" "ENV1=c" ...  - build the variant of each build-time setting; bench the whole image (both clouds) and rank 0 of an emulated 8-way partition
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; shift
mkdir -p $RUNS/$TAG
for CFG in "$@"; do
  NAME=$(echo "$CFG" | tr ' =' '__')
  env $CFG tools/build_variant.sh > $RUNS/$TAG/build_$NAME.log 2>&1 || { echo "$CFG: BUILD FAILED"; tail -5 $RUNS/$TAG/build_$NAME.log; continue; }
  env $CFG python bench.py --full --no-cpu-baseline --steps 60 --warmup 40 --primary-steps 0 > $RUNS/$TAG/bench_$NAME.json 2> $RUNS/$TAG/bench_$NAME.err
  python - <<PY
import json
try:
    d=json.load(open("$RUNS/$TAG/bench_$NAME.json")); o=d.get("other_variant") or {}
    print("$CFG: whole image init/trained", d["value"], o.get("value"), "fwd", d["kernel_ms"]["forward_chain"], (o.get("kernel_ms") or {}).get("forward_chain"), "bwd", d["kernel_ms"]["backward_chain"], (o.get("kernel_ms") or {}).get("backward_chain"), "status", d["status"], o.get("status"))
except Exception as e:
    print("$CFG: FAILED", e)
PY
  for V in init trained; do
    env $CFG python bench.py --full --no-cpu-baseline --no-second-variant --steps 60 --warmup 40 --primary-steps 0 --emulate-world 8 --variant $V ${EMU_ARGS} 2>/dev/null | tail -1 > $RUNS/$TAG/emu_$NAME_$V.json
    python - <<PY
import json
d = json.load(open("$RUNS/$TAG/emu_$NAME_$V.json"))
print("   emu8 $V:", d["ms_per_step"], d["kernel_ms"])
PY
  done
done
