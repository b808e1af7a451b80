#!/bin/bash
# usage (on the GPU box, from the repo root): [PROF_OUT=dir] scripts/rocprof_bench.sh <tag> [bench args]
# kernel-trace + stats of the default bench workload (`bench.py --full`: timed window, its profiled replays and steady_state); summary
# copied to $PROF_OUT/<tag>_kernel_stats.csv (default prof_out/)
set -e
TAG=${1:-prof}; shift || true
export TMPDIR=/tmp
RES=${PROF_OUT:-prof_out}
OUT=$PWD/$RES/prof_$TAG
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -o $TAG -- python bench.py --full --no-cpu-baseline "$@" > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
grep "\"metric\"" $OUT/bench.log | tail -1 > "$RES/${TAG}_bench.json"
f=$(find $OUT -name "*kernel_stats.csv" | head -1)
cp "$f" "$RES/${TAG}_kernel_stats.csv"
head -20 "$RES/${TAG}_kernel_stats.csv"
