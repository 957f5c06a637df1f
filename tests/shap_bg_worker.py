"""Worker for tests/test_shap_background.py: one rank of a gloo (CPU) cloud.

Trains a small forest, computes baseline SHAP with both frames row-sharded
and dumps the global result to JSON (rank 0 writes)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_df(n, seed):
    import numpy as np
    import pandas as pd
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 4))
    X[rng.random(n) < 0.05, 2] = np.nan
    df = pd.DataFrame(X, columns=list("abcd"))
    df["k"] = rng.choice(["u", "v", "w"], n)
    df["y"] = 2 * X[:, 0] - X[:, 1] * (df["k"] == "u") + np.nan_to_num(X[:, 2]) + rng.normal(scale=0.2, size=n)
    return df


def run(out_path):
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2ORandomForestEstimator
    from h2o3_amd.parallel import cloud
    h2o.init(verbose=False)
    fr = h2o.H2OFrame(make_df(400, 0))
    bg = h2o.H2OFrame(make_df(30, 5))
    te = h2o.H2OFrame(make_df(50, 9))
    x = list("abcd") + ["k"]
    # every row and column in every tree: the trees do not depend on the sharding
    m = H2ORandomForestEstimator(ntrees=3, max_depth=4, seed=3, sample_rate=1.0, mtries=-2)
    m.train(x=x, y="y", training_frame=fr)
    res = {"trees": [[list(map(int, t.feat)), list(map(int, t.left)), [float(v) for v in t.value]]
                     for t in m._forest.trees],
           "bg_local_rows": bg.nlocal}
    avg = m.predict_contributions(te, background_frame=bg).as_data_frame()
    per = m.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    res["avg"] = avg.values.tolist()
    res["per_ref"] = per.values.tolist()
    res["per_ref_cols"] = list(per.columns)
    if cloud.rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    cloud.barrier()


if __name__ == "__main__":
    run(sys.argv[1])
