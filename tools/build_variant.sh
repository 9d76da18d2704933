#!/bin/bash
# Usage: [EGR_TRAVERSAL_STATS=1 | EGR_TASK_TIMES=<n> | EGR_EXTRA_FLAGS="-DEGR_GPOP=4" ...] tools/build_variant.sh - build what the environment's build-time settings select (build.py:
# the product in build/, a variant in build/variants/<name>/) and print its directory as the last line. A run with the same settings loads that build; build/ always holds the product.
exec python "$(dirname "$0")/../editable-gaussian-reflections_amd/build.py" "$@"
