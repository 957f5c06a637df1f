set -e
export TMPDIR=/tmp
export PYTHONPATH=$PWD
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_linalg_gpu.py -x -q --timeout 120 --timeout-method thread > $OUT/pytest_lin.log 2>&1 || { tail -30 $OUT/pytest_lin.log; exit 1; }
tail -n 1 $OUT/pytest_lin.log
for cfg in ${CFGS:-1:0 1:7 1:15 0:0 0:15}; do
  MB_BF3=${cfg%%:*} MB_DBG=${cfg##*:} timeout -k 10 120 python scripts/glm_ws_mb.py 2>&1 | grep bf3 >> $OUT/glm_ws_mb.txt
done
cat $OUT/glm_ws_mb.txt
