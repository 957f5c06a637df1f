"""Worker for tests/test_shap_baseline.py: one rank of a gloo (CPU) cloud.

Builds a GLM and a Deep Learning model, sets their coefficients / weights to
seeded values (so the model does not depend on the sharding), computes
baseline SHAP with both frames row-sharded and dumps the global result to
JSON (rank 0 writes)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(out_path):
    import numpy as np
    import torch
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2ODeepLearningEstimator, H2OGeneralizedLinearEstimator
    from h2o3_amd.parallel import cloud
    from shap_baseline_common import X_COLS, make_df
    h2o.init(verbose=False)
    fr = h2o.H2OFrame(make_df(200, 0))
    bg = h2o.H2OFrame(make_df(10, 5))
    te = h2o.H2OFrame(make_df(21, 9))
    glm = H2OGeneralizedLinearEstimator(family="binomial", lambda_=0.0)
    glm.train(x=X_COLS, y="yb", training_frame=fr)
    rng = np.random.default_rng(1)
    glm._beta_std = rng.normal(size=len(glm._beta_std))
    dl = H2ODeepLearningEstimator(hidden=[6, 4], activation="Tanh", epochs=1, seed=3)
    dl.train(x=X_COLS, y="y", training_frame=fr)
    g = torch.Generator().manual_seed(2)
    for L in dl._layers:
        L.W.copy_(torch.randn(L.W.shape, generator=g))
        L.b.copy_(torch.randn(L.b.shape, generator=g) * 0.3)
    dl._ymu, dl._ysd = 0.5, 2.0
    res = {"bg_local_rows": bg.nlocal}
    for name, m in (("glm", glm), ("dl", dl)):
        avg = m.predict_contributions(te, background_frame=bg, output_space=name == "glm").as_data_frame()
        per = m.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
        res[name + "_avg"] = avg.values.tolist()
        res[name + "_per_ref"] = per.values.tolist()
        res.setdefault("cols", []).append(list(per.columns))
    if cloud.rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    cloud.barrier()


if __name__ == "__main__":
    run(sys.argv[1])
