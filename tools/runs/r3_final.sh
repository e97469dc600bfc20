#!/bin/bash
# the round's committed numbers: default bench line (every leg: --full), profile set, C3 run;
# the bench line and the logs go to $OUT (default bench_out/)
OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export OUT
S=$(date +%s)
timeout -k 10 400 python bench.py --full --repeats 3 > "$OUT/r03_bench_default.json" 2> "$OUT/r03_bench_default.err"; echo "bench rc=$? $(( $(date +%s) - S )) s"
cut -c1-400 "$OUT/r03_bench_default.json"; echo
bash tools/profile_r03.sh r03 --steps 40 > "$OUT/r03_profile.log" 2>&1; echo "profile rc=$?"
bash tools/runs/r3_hd.sh 2>&1 | tail -12 | cut -c1-200
