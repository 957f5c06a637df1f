# GLM bf16x3 kernel with the swizzled LDS image: GPU tests + bench.
set -e
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_linalg_gpu.py tests/test_glm.py -m gpu > $OUT/pytest_glm.log 2>&1 || { tail -40 $OUT/pytest_glm.log; exit 1; }
tail -n 2 $OUT/pytest_glm.log
timeout -k 10 300 python bench.py --full --algo glm --steps 20 --warmup 3 > $OUT/glm_swz.log 2>&1
grep -o '"ms_per_step": [0-9.]*\|"train_deviance_per_row": [0-9.]*' $OUT/glm_swz.log
timeout -k 10 300 python bench.py --algo glm --rows 12500000 --steps 20 --warmup 3 > $OUT/glm_swz_12m5.log 2>&1
grep -o '"ms_per_step": [0-9.]*' $OUT/glm_swz_12m5.log
