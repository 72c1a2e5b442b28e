#!/bin/bash
# every bench mode, one JSON line per file under $OUT (default bench_out/lines)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out/lines}
mkdir -p "$OUT"
python bench.py --full > "$OUT/r06_bench_line.json" 2> "$OUT/err0"
(time python bench.py --gpus 1 --steps 20 --warmup 5 > "$OUT/r06_bench_line_driver_command.json") 2>> "$OUT/err0"   # the driver's exact command, timed
python bench.py --full --dtype bf16 --no-cpu-baseline > "$OUT/r06_bench_line_bf16.json" 2>> "$OUT/err0"
python bench.py --full --dtype f16 --width 2048 --height 1024 --no-cpu-baseline > "$OUT/r06_bench_line_config5_f16_2048x1024.json" 2>> "$OUT/err0"
python bench.py --step head > "$OUT/r06_bench_line_step_head.json" 2>> "$OUT/err0"
python bench.py --step model > "$OUT/r06_bench_line_step_model.json" 2>> "$OUT/err0"
python bench.py --step model --dtype bf16 > "$OUT/r06_bench_line_step_model_bf16.json" 2>> "$OUT/err0"
python bench.py --step model --model-table --steps 6 --warmup 2 > "$OUT/r06_bench_line_step_model_table.json" 2>> "$OUT/err0"
python bench.py --gpus 2 > "$OUT/r06_bench_line_gpus2_on_a_1gpu_box.json" 2>> "$OUT/err0"
tail -3 "$OUT/err0"
for f in "$OUT"/*.json; do echo "$f: $(head -c 300 $f)"; done
