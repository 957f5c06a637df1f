#!/bin/bash
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest tests/test_linalg_gpu.py -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/r5_tests27.log 2>&1
rc=$?
tail -3 $OUT/r5_tests27.log
if [ $rc -ne 0 ]; then grep -E "FAILED|Error|assert" $OUT/r5_tests27.log | head -20; exit 1; fi
timeout -k 10 300 python -u bench.py --full --algo glm --steps 10 --warmup 3 > $OUT/r5_glm_narrow_bf16.json 2> $OUT/r5_glm_narrow_bf16.err || { tail -20 $OUT/r5_glm_narrow_bf16.err; exit 1; }
cut -c1-220 $OUT/r5_glm_narrow_bf16.json
grep -o '"iters": [0-9]*, "hessian_tier": "[a-z0-9]*", "hessian_kappa": [0-9.]*' $OUT/r5_glm_narrow_bf16.json
timeout -k 10 600 python -u scripts/glm_precision.py --out $OUT/glm_precision_bf16_r5.json > $OUT/r5_prec.log 2>&1 || { tail -20 $OUT/r5_prec.log; exit 1; }
tail -45 $OUT/r5_prec.log
