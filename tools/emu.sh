#!/bin/bash
# Usage (GPU box): tools/emu.sh <tag> [world...]  - rank 0 of an emulated N-way tile partition on this one GPU (no collective), both clouds
RUNS=${EGR_RUNS_DIR:-runs}  # results go to $RUNS/<tag> (runs/ is kept out of git)
TAG=$1; shift; mkdir -p $RUNS/$TAG
for N in "${@:-8}"; do for V in init trained; do
  python bench.py --full --no-cpu-baseline --no-second-variant --steps 60 --warmup 40 --primary-steps 0 --emulate-world $N --variant $V ${EMU_ARGS} 2>/dev/null | tail -1 > $RUNS/$TAG/emu.json
  python - <<PY | tee -a $RUNS/$TAG/emulated_partition_rank0.jsonl
import json
d = json.load(open("$RUNS/$TAG/emu.json"))
print(json.dumps({"world": $N, "variant": "$V", "ms_per_iteration": d["ms_per_step"], "kernel_ms": d["kernel_ms"], "env": "${EMU_ENV}"}))
PY
done; done
