"""Worker for tests/test_fairness.py: one rank of a gloo (CPU) cloud.

Builds the hand-made frame row-sharded over the ranks, computes the fairness
overview of a model that scores with a column of the frame (so nothing
depends on the sharding but the sketch's all-reduce) and dumps the table to
JSON (rank 0 writes)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(out_path):
    import h2o3_amd as h2o
    from fairness_common import ScoredModel, make_df, to_frame
    from h2o3_amd.models.fairness import fairness_metrics
    from h2o3_amd.parallel import cloud
    h2o.init(verbose=False)
    fr = to_frame(make_df())
    out = fairness_metrics(ScoredModel("score"), fr, ["sex", "race"], ["M", "a"], "yes")
    ov = out["overview"].as_data_frame()
    rows = [[None if isinstance(v, float) and v != v else (v if isinstance(v, str) else float(v)) for v in r]
            for r in ov.values.tolist()]
    res = {"columns": list(ov.columns), "overview": rows, "tables": sorted(k for k in out if k != "overview"),
           "local_rows": fr.nlocal}
    if cloud.rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    cloud.barrier()


if __name__ == "__main__":
    run(sys.argv[1])
