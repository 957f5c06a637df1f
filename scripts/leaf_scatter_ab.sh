# A/B: write-only leaf scatter + fused add in the residual pass vs in-place RMW leaf update.
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_tree_kernels_gpu.py \
  -k "scatter or fill_nid" > $OUT/pytest_scatter.log 2>&1 || { tail -30 $OUT/pytest_scatter.log; exit 1; }
tail -1 $OUT/pytest_scatter.log
for R in 100000000 12500000; do
  for S in 0 1 0 1; do
    H2O3_LEAF_SCATTER=$S timeout -k 10 300 python bench.py --full --rows $R --steps 20 --warmup 3 --no-glm > $OUT/ls.log 2>&1
    echo "rows=$R scatter=$S $(grep -o '"ms_per_step": [0-9.]*' $OUT/ls.log) $(grep -o '"train_logloss_after": [0-9.]*' $OUT/ls.log)"
  done
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/rocprof_ls -o run --output-format csv -- python3 bench.py --steps 10 --warmup 2 --no-glm > $OUT/rocprof_ls.log 2>&1
grep -E "leaf_scatter|leaf_update|gbm_grad" $OUT/rocprof_ls/run_kernel_stats.csv | cut -d, -f1-4 | cut -c1-150
rm -f $OUT/rocprof_ls/run_kernel_trace.csv
