# One-pass GBM residual kernel: tree tests, then bench A/B at 12.5M and 100M rows.
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_tree_kernels_gpu.py \
  tests/test_gpu_algos.py > $OUT/pytest_grad.log 2>&1
tail -2 $OUT/pytest_grad.log
for R in 12500000 100000000; do
  for G in 0 1; do
    H2O3_GBM_GRAD=$G timeout -k 10 300 python bench.py --full --rows $R --steps 10 --warmup 2 > $OUT/grad_ab.log 2>&1
    echo "rows=$R grad=$G: $(grep -o '"ms_per_step": [0-9.]*' $OUT/grad_ab.log) $(grep -o '"train_logloss_after": [0-9.]*' $OUT/grad_ab.log)"
  done
done
