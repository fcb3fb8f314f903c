#!/bin/bash
# Kernel trace of a short bench.py run -> gpurun_out/prof_bench (timeline gaps: scripts/timeline.py)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
rm -rf gpurun_out/prof_bench
set -- --full "$@"   # every leg of the benchmark in the trace, not the headline steps alone
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof_bench -o bench -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline "$@" > gpurun_out/prof_bench.log 2>&1
