#!/bin/bash
# the round's bench line: default command with every leg (--full); files go to $OUT (default bench_out/)
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
S=$(date +%s)
timeout -k 10 1000 python bench.py --full --repeats 3 > "$OUT/r02_bench_default.json" 2> "$OUT/r02_bench_default.err"; tail -2 "$OUT/r02_bench_default.err"
echo "wall seconds: $(( $(date +%s) - S ))" | tee "$OUT/r02_bench_default.time"
cut -c1-300 "$OUT/r02_bench_default.json"; echo
