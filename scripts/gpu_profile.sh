#!/bin/bash
# rocprofv3 kernel-trace stats of the bench command (no PMC here; counters get their own pass).  Output under $PROF_DIR
# (default build/prof); --full keeps the instrumented per-kernel pass in the profiled run.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
REPO=$PWD
P=${PROF_DIR:-$REPO/build/prof}
rm -rf "$P"; mkdir -p "$P"
export TMPDIR=/tmp
cd /tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$P" -o bench -- python "$REPO/bench.py" --full --steps 20 --warmup 5 --no-graph --no-cpu-baseline --no-coherent --no-overlap --no-train --no-other-configs --no-stream-inputs > "$P/bench_under_rocprof.json" 2> "$P/rocprof.err"
echo "rocprof exit $?"
cd "$REPO"
ls "$P" | head
f=$(find "$P" -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -40 "$f" | cut -c1-200
# keep the merge small: the per-dispatch trace can be tens of MB
find "$P" -name "*kernel_trace.csv" -size +20M -delete
