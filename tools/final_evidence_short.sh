#!/usr/bin/env bash
# The reduced form of tools/final_evidence.sh for a change confined to the bf > 255 compare: its parity cases, the profile
# passes (kernel stats + FETCH_SIZE / WRITE_SIZE) and the full bench line on the same sources; the whole GPU suite is NOT
# re-run.  Outputs under $BB_OUT (default evidence/ in the repository).
set -u
TAG="${1:-r05}"
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
export BB_OUT="${BB_OUT:-$ROOT/evidence}"
mkdir -p "$BB_OUT"
BB_OUT="$(cd "$BB_OUT" && pwd)"
timeout 100 python -m pytest tests/test_hip_tree.py -m gpu -q -x -k "block_compare" > "$BB_OUT/block_tests_final.txt" 2>&1
timeout 120 bash tools/profile_bench.sh "$TAG" 1000000 > "$BB_OUT/profile_$TAG.log" 2>&1
if [ -f "$BB_OUT/prof_$TAG/pmc_latest.json" ]; then cp "$BB_OUT/prof_$TAG/pmc_latest.json" profiles/pmc_latest.json; fi
cd "$ROOT"
( time timeout 270 python bench.py --full > "$BB_OUT/bench_line_final.json" 2> "$BB_OUT/bench_final.err" ) 2> "$BB_OUT/bench_final.time"
tail -n 2 "$BB_OUT/block_tests_final.txt" "$BB_OUT/bench_final.time"
head -c 300 "$BB_OUT/bench_line_final.json"
