#!/bin/bash
# Measurement of the device-side error statistics at config 4 (run from the repository root, after python lvi-exc_amd/build.py):
#   1. tools/error_stats_bench.py: lvx_error_statistics_d against lvx_evaluate(COST | RESIDUALS) + copy + numpy -> profiles/error_stats_config4.json
#   2. the same under rocprofv3 --kernel-trace --stats -> profiles/error_stats_trace/ (kernel statistics only)
# Every GPU step has its own time limit and the steps are chained: a step that fails or hangs ends the script.
set -o pipefail
OUT=${1:-profiles}
TMP=${2:-profile_out/error_stats}
mkdir -p "$OUT/error_stats_trace" "$TMP"
timeout -k 10 420 python tools/error_stats_bench.py --steps 50 --warmup 5 --out "$OUT/error_stats_config4.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -o stats -- python tools/error_stats_bench.py --steps 20 --warmup 3 > "$TMP/run.log" 2>&1 &&
f=$(find "$TMP" -name "*kernel_stats.csv" | head -1) && test -n "$f" && cp "$f" "$OUT/error_stats_trace/stats_kernel_stats.csv"
