#!/bin/bash
# kernel-trace profile of the full bench run (bench.py --full) on the default workload; writes $PROF_OUT/<tag>/*kernel_stats.csv (PROF_OUT defaults to prof_out)
tag=${1:-prof}
shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
out=${PROF_OUT:-prof_out}; mkdir -p "$out" || exit 1
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/$tag" -o k -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline "$@" > "$out/$tag.log" 2>&1
