# Default bench at 100M and 12.5M rows (GBM + companion GLM).
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python bench.py --full > $OUT/bench_default.log 2>&1
tail -1 $OUT/bench_default.log | cut -c1-700
timeout -k 10 300 python bench.py --full --rows 12500000 --steps 20 --warmup 3 > $OUT/bench_12m5.log 2>&1
grep -o '"ms_per_step": [0-9.]*\|"glm_ms_per_iter": [0-9.]*' $OUT/bench_12m5.log
