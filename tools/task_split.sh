#!/bin/bash
# Usage (GPU box): tools/task_split.sh <step> [variant] - per-task stamps of ONE forward step (EGR_TASK_TIMES=<step> build): walk vs selection + compositing of the heaviest tasks
STEP=${1:-1}; V=${2:-init}
EGR_TASK_TIMES=$STEP tools/build_variant.sh > /dev/null 2>&1
EGR_TASK_TIMES=$STEP VARIANT=$V TT_STEP=$STEP CALL=10 python tools/task_times.py 2>&1 | grep -a "heaviest\|longest list\|walk share\|tasks "
