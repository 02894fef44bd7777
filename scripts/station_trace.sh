#!/bin/bash
# rocprofv3 kernel trace of bench.py's config-5 station leg (--full with every other optional leg off): five
# closed-loop steps after one warmup step.  Its kernel trace is what scripts/trace_loop.py reads and its
# stats are the station_kernel_stats.csv records under profiles/.
# usage: bash scripts/station_trace.sh OUTDIR   (trace under OUTDIR/sprofk, the run's own output in OUTDIR/sprofk.log)
[ -n "$1" ] || { echo "usage: bash $0 OUTDIR" >&2; exit 2; }
mkdir -p "$1" && OUT=$(cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/.." || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/sprofk" -o run --output-format csv -- \
  python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-direct --no-contracts \
  --station-steps 5 --station-warmup 1 --station-prof-steps 0 > "$OUT/sprofk.log" 2>&1
rc=$?; echo "sprofk rc=$rc"; exit $rc
