#!/bin/bash
# GPU-box helper: rocprofv3 kernel-trace + stats of a short eager bench run (no CPU baseline).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}   # where this script leaves its results
mkdir -p $OUT/prof
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- \
  python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --sampler-steps 5 ${PROF_ARGS} > $OUT/prof/bench.json 2> $OUT/prof/bench.err
echo "prof rc=$?"
find $OUT/prof -name "*stats*" | head
