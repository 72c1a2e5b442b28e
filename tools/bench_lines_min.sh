#!/bin/bash
# the two headline lines only (tools/bench_lines.sh: every mode), under $OUT (default bench_out/lines)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out/lines}
mkdir -p "$OUT"
python bench.py --full > "$OUT/r06_bench_line.json" 2> "$OUT/err0"
python bench.py --full --steps 20 --warmup 5 --no-extra --no-cpu-baseline > "$OUT/r06_bench_line_driver_command.json" 2>> "$OUT/err0"
tail -2 "$OUT/err0"
