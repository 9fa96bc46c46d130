#!/usr/bin/env bash
# Round-end evidence on the GPU machine in one go (outputs under $BB_OUT, default evidence/ in the repository; copy what
# should be judged into profiles/):
#   1. rocprofv3 kernel stats + FETCH_SIZE / WRITE_SIZE passes of the bench command (tools/profile_bench.sh)
#   2. the full bench line (`bench.py --full`), quoting those counters (profiles/pmc_latest.json must describe THIS kernel source)
#   3. smoke(), 4. the GPU test suite
# usage: [BB_OUT=dir] bash tools/final_evidence.sh <tag, e.g. r05>
set -u
TAG="${1:-r05}"
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
export BB_OUT="${BB_OUT:-$ROOT/evidence}"
mkdir -p "$BB_OUT"
BB_OUT="$(cd "$BB_OUT" && pwd)"
bash tools/profile_bench.sh "$TAG" 1000000 > "$BB_OUT/profile_$TAG.log" 2>&1
if [ -f "$BB_OUT/prof_$TAG/pmc_latest.json" ]; then cp "$BB_OUT/prof_$TAG/pmc_latest.json" profiles/pmc_latest.json; fi
cd "$ROOT"
( time python bench.py --full > "$BB_OUT/bench_line_final.json" 2> "$BB_OUT/bench_final.err" ) 2> "$BB_OUT/bench_final.time"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$BB_OUT/smoke.log" 2>&1
python -m pytest tests -m gpu -q -x > "$BB_OUT/gputest_final.log" 2>&1
tail -n 2 "$BB_OUT/gputest_final.log" "$BB_OUT/smoke.log" "$BB_OUT/bench_final.time"
head -c 400 "$BB_OUT/bench_line_final.json"
