# A/B: leaf gather + uncompacted last level (default) vs leaf scatter + compacted last level
# (H2O3_LEAF_GATHER=0 H2O3_DEV_LAST_LEVEL=0), same build, alternating runs of plain bench.py.
# PARENT=<checkout of the parent commit, built> adds one run of it per size (switches-off must equal it).
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
RUNS=${RUNS:-3}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest -x -q tests/test_leaf_gather_gpu.py > $OUT/pytest_gather.log 2>&1 \
  || { tail -30 $OUT/pytest_gather.log; exit 1; }
tail -1 $OUT/pytest_gather.log
for R in ${ROWS:-100000000 12500000}; do
  if [ -n "$PARENT" ]; then
    (cd "$PARENT" && timeout -k 10 300 python bench.py --rows $R) > $OUT/lg.log 2>&1
    echo "rows=$R parent   $(grep -o '"value": [0-9.]*' $OUT/lg.log) $(grep -o '"ms_per_step": [0-9.]*' $OUT/lg.log)"
  fi
  for i in $(seq $RUNS); do
    for S in 0 1; do
      H2O3_LEAF_GATHER=$S H2O3_DEV_LAST_LEVEL=$S timeout -k 10 300 python bench.py --rows $R > $OUT/lg.log 2>&1
      echo "rows=$R switches=$S $(grep -o '"value": [0-9.]*' $OUT/lg.log) $(grep -o '"ms_per_step": [0-9.]*' $OUT/lg.log)"
    done
  done
done
