"""Worker for tests/test_forest_predict_gpu.py: a fresh process, so that
H2O3_PREDICT_TW (trees walked together per thread; read once per process by
h2o_forest_predict) takes effect.

Scores the lane, class and edge cases of forest_predict_common with
Forest.predict on the GPU and writes `<case>/sums` and `<case>/leaf` to the
.npz path given on the command line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(out_path):
    import numpy as np
    import torch
    import h2o3_amd as h2o
    from forest_predict_common import WORKER_CASE_NAMES, inputs
    h2o.init(device="cuda:0", verbose=False)
    res = {}
    for name in WORKER_CASE_NAMES:
        fo, X, K = inputs(name)
        Xd = torch.tensor(X, device="cuda")
        res[name + "/sums"] = fo.predict(Xd, K).cpu().numpy()
        res[name + "/leaf"] = fo.predict(Xd, K, leaf=True).cpu().numpy()
    with open(out_path, "wb") as f:
        np.savez(f, **res)


if __name__ == "__main__":
    run(sys.argv[1])
