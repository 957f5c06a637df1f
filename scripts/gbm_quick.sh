set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests/test_tree_kernels_gpu.py tests/test_gpu_algos.py -x -q --timeout 120 --timeout-method thread > $OUT/pytest_tree.log 2>&1 || { tail -40 $OUT/pytest_tree.log; exit 1; }
tail -n 1 $OUT/pytest_tree.log
for R in 12500000 100000000; do
  timeout -k 10 300 python bench.py --full --rows $R --steps 20 --warmup 3 > $OUT/gbm_$R.log 2>&1
  echo "rows=$R $(grep -o '"ms_per_step": [0-9.]*' $OUT/gbm_$R.log) $(grep -o '"train_logloss_after": [0-9.]*' $OUT/gbm_$R.log)"
done
