#!/bin/bash
# GPU-box helper: bench (1 GPU) then a rocprofv3 kernel-trace summary of a short bench run.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}   # where this script leaves its results
mkdir -p $OUT
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 10 --warmup 3} > $OUT/bench.json 2> $OUT/bench.err
echo "bench rc=$?"
