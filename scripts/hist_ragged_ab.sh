# A/B of the id-free root (H2O3_DEV_ROOT_IDENT) and of the ragged last histogram group
# (H2O3_HIST_BM_RAGGED), each on its own against both switches off, same build, alternating
# runs of plain bench.py.  PARENT=<checkout of the parent commit, built> adds one run of it
# per size (both switches off must equal it).  CONFIGS="ident:ragged ..." picks the pairs.
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
RUNS=${RUNS:-3}
CONFIGS=${CONFIGS:-"0:0 1:0 0:1"}
mkdir -p "$OUT"
for R in ${ROWS:-100000000 12500000}; do
  if [ -n "$PARENT" ]; then
    (cd "$PARENT" && timeout -k 10 300 python bench.py --rows $R) > $OUT/hr.log 2>&1
    echo "rows=$R parent            $(grep -o '"value": [0-9.]*' $OUT/hr.log) $(grep -o '"ms_per_step": [0-9.]*' $OUT/hr.log)"
  fi
  for i in $(seq $RUNS); do
    for C in $CONFIGS; do
      H2O3_DEV_ROOT_IDENT=${C%:*} H2O3_HIST_BM_RAGGED=${C#*:} timeout -k 10 300 python bench.py --rows $R > $OUT/hr.log 2>&1
      echo "rows=$R ident=${C%:*} ragged=${C#*:} $(grep -o '"value": [0-9.]*' $OUT/hr.log) $(grep -o '"ms_per_step": [0-9.]*' $OUT/hr.log)"
    done
  done
done
