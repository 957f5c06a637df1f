"""Fairness tables (models/fairness.py), on the torch path of the grouped
score sketch when the cloud has no GPU: the overview against a pure-numpy
brute force, a group that counts no row, the p.value rule against exact
enumeration and the G-test's closed form, disparate_analysis, fair_shap,
fair_pd, the argument errors, the compat import and 2 gloo ranks against 1."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from fairness_common import RACE, SEX, ScoredModel, brute_overview, fisher_exact, make_df, to_frame

HERE = os.path.dirname(os.path.abspath(__file__))
PROT = ["sex", "race"]
REF = ["M", "a"]


@pytest.fixture(scope="module")
def data():
    df = make_df()
    return df, to_frame(df)


@pytest.fixture(scope="module")
def gbm(data):
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    m = H2OGradientBoostingEstimator(ntrees=4, max_depth=3, seed=2, min_rows=5)
    m.train(x=["x", "score", "score2", "sex", "race"], y="y", training_frame=data[1])
    return m


def _same(a, b, tol):
    return (a != a and b != b) or abs(a - b) <= tol


def _check_overview(ov, ref_rows, tol=1e-12):
    assert len(ov) == len(ref_rows)
    assert list(ov.columns) == list(ref_rows[0].keys())
    for i, r in enumerate(ref_rows):
        for k, v in r.items():
            got = ov[k].iloc[i]
            if isinstance(v, str):
                assert got == v, (i, k, got, v)
            elif k in ("tp", "fp", "tn", "fn", "total", "selected"):
                assert int(got) == v, (i, k, got, v)
            else:
                # p.value: lgamma against exact rationals; the rest: the same sums in another order
                assert _same(float(got), float(v), 1e-9 if k == "p.value" else tol), (i, k, got, v)


@pytest.mark.parametrize("favorable", ["yes", "no"])
def test_overview_matches_brute_force(data, favorable):
    from h2o3_amd.models.fairness import fairness_metrics
    df, fr = data
    m = ScoredModel("score")
    out = fairness_metrics(m, fr, PROT, REF, favorable)
    # the torch path on a CPU cloud, the kernel where the frame lives on a GPU
    assert m._fairness_why == (None if fr.vec("score").data.is_cuda else "CPU tensors")
    ov = out["overview"].as_data_frame()
    ref_rows = brute_overview(df, "score", PROT, [SEX, RACE], REF, favorable)
    _check_overview(ov, ref_rows)
    # the NA level is a group of its own, after the column's levels
    assert "NA" in set(ov["sex"]) and "NA" in set(ov["race"])
    assert len(ov) == 12 and list(ov["sex"].iloc[:4]) == ["F"] * 4 and list(ov["race"].iloc[:4]) == RACE + ["NA"]
    # the reference group selects every favourable row and no other: fn = fp = 0, so their AIR is NaN everywhere
    r = ov[(ov["sex"] == "M") & (ov["race"] == "a")].iloc[0]
    assert r["fn"] == 0 and r["fp"] == 0 and r["AIR_tp"] == 1.0 and math.isnan(r["p.value"])
    assert ov["AIR_fn"].isna().all() and ov["AIR_fp"].isna().all()
    assert not ov["AIR_selectedRatio"].isna().any()
    assert ov["relativeSize"].sum() == pytest.approx(1.0, abs=1e-12)
    # one threshold table per group
    tabs = [k for k in out if k.startswith("thresholds_and_metrics_")]
    assert len(tabs) == 12 and "thresholds_and_metrics_F,NA" in out
    t = out["thresholds_and_metrics_M,a"].as_data_frame()
    assert {"threshold", "tps", "fps", "tpr", "fpr", "f1"} <= set(t.columns) and len(t) <= 7


def test_unoccupied_reference_gives_nan(data):
    from h2o3_amd.models.fairness import fairness_metrics
    df, _ = data
    sub = df[~((df["sex"] == "M") & (df["race"] == "a"))].reset_index(drop=True)
    sub = pd.concat([sub, df[(df["sex"] == "M") & (df["race"] == "b")].head(1)], ignore_index=True)
    fr = to_frame(sub)
    ov = fairness_metrics(ScoredModel("score"), fr, PROT, REF, "yes")["overview"].as_data_frame()
    assert len(ov) == 11
    assert ov[[c for c in ov.columns if c.startswith("AIR_")]].isna().all().all() and ov["p.value"].isna().all()
    _check_overview(ov, brute_overview(sub, "score", PROT, [SEX, RACE], REF, "yes"))


def test_group_with_no_counted_row(data):
    """Every row of (F, c) has an NA response: the group is occupied but
    counts nothing."""
    from h2o3_amd.models.fairness import disparate_analysis, fairness_metrics
    df, fr = data
    holed = df.copy()
    hole = ((holed["sex"] == "F") & (holed["race"] == "c")).to_numpy()
    assert hole.sum() > 5
    holed.loc[hole, "y"] = None
    for favorable in ("yes", "no"):
        out = fairness_metrics(ScoredModel("score"), to_frame(holed), PROT, REF, favorable)
        ov = out["overview"].as_data_frame()
        _check_overview(ov, brute_overview(holed, "score", PROT, [SEX, RACE], REF, favorable))
        r = ov.iloc[2]
        assert (r["sex"], r["race"], r["total"], r["selected"], r["relativeSize"]) == ("F", "c", 0, 0, 0.0)
        for k in ("accuracy", "precision", "f1", "tpr", "tnr", "fpr", "fnr", "auc", "aucpr", "gini", "selectedRatio",
                  "logloss", "AIR_accuracy", "AIR_auc", "AIR_selectedRatio", "AIR_logloss", "p.value"):
            assert math.isnan(r[k]), k
        assert r["AIR_tp"] == 0.0 and r["AIR_total"] == 0.0
        t = out["thresholds_and_metrics_F,c"].as_data_frame()
        assert len(t) == 0 and list(t.columns) == list(out["thresholds_and_metrics_M,a"].as_data_frame().columns)
        # the other groups: only their share of the counted rows moves
        full = fairness_metrics(ScoredModel("score"), fr, PROT, REF, favorable)["overview"].as_data_frame()
        loss = ["logloss", "AIR_logloss"]       # f64 sums: on a GPU atomic, so not the same bits from call to call
        same = [c for c in ov.columns if c not in ["relativeSize", "AIR_relativeSize"] + loss]
        keep = [i for i in range(12) if i != 2]
        pd.testing.assert_frame_equal(ov.loc[keep, same], full.loc[keep, same], check_exact=True)
        np.testing.assert_allclose(ov.loc[keep, loss].to_numpy(), full.loc[keep, loss].to_numpy(), rtol=0, atol=1e-12)
    da = disparate_analysis([ScoredModel("score")], to_frame(holed), PROT, REF, "yes").as_data_frame()
    assert da["air_min"].iloc[0] == ov_min(holed)


def ov_min(df):
    rows = brute_overview(df, "score", PROT, [SEX, RACE], REF, "yes")
    return min(r["AIR_selectedRatio"] for r in rows if r["AIR_selectedRatio"] == r["AIR_selectedRatio"]
               and (r["sex"], r["race"]) != ("M", "a"))


def test_p_value_fisher_exact_enumeration():
    from h2o3_amd.models.fairness import table_p_value
    rng = np.random.default_rng(4)
    tables = [(3, 1, 1, 3), (0, 5, 5, 0), (10, 5, 8, 7), (1, 0, 0, 1), (7, 7, 7, 7), (0, 0, 3, 4), (12, 0, 9, 3)]
    tables += [tuple(int(v) for v in rng.integers(0, 16, 4)) for _ in range(40)]
    for a, b, c, d in tables:
        assert max(a + b, c + d, a + c, b + d) <= 30
        got = table_p_value(a, b, c, d)
        if a + b == 0 or c + d == 0:
            assert math.isnan(got)
        else:
            assert got == pytest.approx(fisher_exact(a, b, c, d), rel=1e-9, abs=1e-14), (a, b, c, d)


def test_p_value_g_test_closed_form():
    from h2o3_amd.models import fairness
    a, b, c, d = 150_000, 160_000, 140_500, 170_000
    assert min(a + b, c + d, a + c, b + d) > fairness.FISHER_MAX_MARGIN
    n = a + b + c + d
    G = 2 * sum(o * math.log(o / (r * k / n)) for o, r, k in
                ((a, a + b, a + c), (b, a + b, b + d), (c, c + d, a + c), (d, c + d, b + d)))
    assert fairness.table_p_value(a, b, c, d) == pytest.approx(math.erfc(math.sqrt(G / 2)), rel=1e-9)
    # the switch is on the smallest margin: one margin of 100 000 is still Fisher's test
    small = fairness.table_p_value(50_000, 50_000, 200_000, 190_000)
    assert small == pytest.approx(fairness._fisher_two_sided(50_000, 50_000, 200_000, 190_000))
    assert small == pytest.approx(fairness._g_test(50_000, 50_000, 200_000, 190_000), rel=1e-3)


def test_disparate_analysis_equals_overview_statistics(data, gbm):
    from h2o3_amd.models.fairness import disparate_analysis, fairness_metrics
    _, fr = data
    models = [gbm, ScoredModel("score2")]
    for metric in ("selectedRatio", "tpr"):
        da = disparate_analysis(models, fr, PROT, REF, "yes", air_metric=metric, alpha=0.2).as_data_frame()
        assert list(da.columns) == ["model_id", "auc", "logloss", "num_of_features", "air_min", "air_mean",
                                    "air_median", "air_max", "cair", "significant_air_min", "p.value_min",
                                    "p.value_mean", "p.value_median", "p.value_max"]
        assert list(da["model_id"]) == [gbm.model_id, "scored_score2"]
        assert da["auc"].iloc[0] == pytest.approx(gbm.auc()) and math.isnan(da["auc"].iloc[1])
        assert list(da["num_of_features"]) == [5, 1]
        for i, m in enumerate(models):
            ov = fairness_metrics(m, fr, PROT, REF, "yes")["overview"].as_data_frame()
            ov = ov[~((ov["sex"] == "M") & (ov["race"] == "a"))]
            air, pv = ov["AIR_" + metric].to_numpy(float), ov["p.value"].to_numpy(float)
            assert len(air) == 11 and not np.isnan(air).any()
            sig = air[pv < 0.2]
            want = {"air_min": air.min(), "air_mean": air.mean(), "air_median": np.median(air), "air_max": air.max(),
                    "cair": (ov["relativeSize"].to_numpy(float) * air).sum(),
                    "significant_air_min": sig.min() if sig.size else float("nan"), "p.value_min": pv.min(),
                    "p.value_mean": pv.mean(), "p.value_median": np.median(pv), "p.value_max": pv.max()}
            for k, v in want.items():
                assert _same(float(da[k].iloc[i]), float(v), 1e-12), (metric, i, k, da[k].iloc[i], v)
    # a model that is not binomial is left out of the table
    other = ScoredModel("score", model_id="three_classes")
    other._spec.nclasses = 3
    assert list(disparate_analysis(models + [other], fr, PROT, REF, "yes").as_data_frame()["model_id"]) == \
        [gbm.model_id, "scored_score2"]


def test_fair_shap_equals_group_by(data, gbm):
    from h2o3_amd.models.fairness import fair_shap
    df, fr = data
    got = fair_shap(gbm, fr, PROT).as_data_frame()
    c = gbm.predict_contributions(fr).as_data_frame().astype(np.float64)    # f32 columns: average them in f64
    feats = [n for n in c.columns if n != "BiasTerm"]
    keys = pd.DataFrame({"g_sex": df["sex"].fillna("NA").to_numpy(), "g_race": df["race"].fillna("NA").to_numpy()})
    by = ["g_sex", "g_race"]
    mean = c[feats].join(keys).groupby(by)[feats].mean()
    mabs = c[feats].abs().join(keys).groupby(by)[feats].mean()
    size = keys.groupby(by).size()
    assert len(got) == 12 * len(feats) and set(feats) == {"x", "score", "score2", "sex", "race"}
    for _, r in got.iterrows():
        key = (r["sex"], r["race"])
        assert r["mean_contribution"] == pytest.approx(mean.loc[key, r["feature"]], abs=1e-12)
        assert r["mean_abs_contribution"] == pytest.approx(mabs.loc[key, r["feature"]], abs=1e-12)
        assert r["rows"] == size.loc[key]


def test_fair_pd_equals_partial_plot_of_filtered_frame(data, gbm):
    from h2o3_amd.models.fairness import fair_pd
    df, fr = data
    got = fair_pd(gbm, fr, "score2", ["sex"], nbins=5).as_data_frame()
    assert list(got.columns) == ["sex", "score2", "mean_response", "stddev_response", "std_error_mean_response"]
    lev = df["sex"].fillna("NA").to_numpy()
    for s in ("F", "M", "NA"):
        sub = fr[torch.tensor(lev == s)]
        want = gbm.partial_plot(sub, cols=["score2"], nbins=5)[0]
        g = got[got["sex"] == s]
        assert len(g) == len(want) == 5
        for k in ("score2", "mean_response", "stddev_response", "std_error_mean_response"):
            np.testing.assert_allclose(g[k].to_numpy(float), want[k].to_numpy(float), rtol=0, atol=1e-12)


def test_inspect_model_fairness_tables(data, gbm):
    _, fr = data
    out = gbm.inspect_model_fairness(fr, PROT, REF, "yes")
    top = [r[0] for r in gbm.varimp() if r[0] not in PROT][:3]
    assert {"overview", "shap"} <= set(out) and {"pd_" + c for c in top} <= set(out) and len(top) == 3
    # two calls: equal but for the last bits of the loss sums where they are atomic sums on a GPU
    pd.testing.assert_frame_equal(out["overview"].as_data_frame(),
                                  gbm.fairness_metrics(fr, PROT, REF, "yes")["overview"].as_data_frame(),
                                  check_exact=False, rtol=0, atol=1e-12)
    only = gbm.inspect_model_fairness(fr, PROT, REF, "yes", columns=["x"])
    assert [k for k in only if k.startswith("pd_")] == ["pd_x"]


def test_value_errors(data):
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    from h2o3_amd.models.fairness import fairness_metrics
    _, fr = data
    reg = H2OGradientBoostingEstimator(ntrees=1, max_depth=2, seed=1)
    reg.train(x=["score2"], y="x", training_frame=fr)
    with pytest.raises(ValueError, match="binomial"):
        reg.fairness_metrics(fr, PROT, REF, "yes")
    m = ScoredModel("score")
    with pytest.raises(ValueError, match="'x'"):
        fairness_metrics(m, fr, ["sex", "x"], REF, "yes")              # not an enum column
    with pytest.raises(ValueError, match="'nope'"):
        fairness_metrics(m, fr, ["sex", "nope"], REF, "yes")           # not a column
    with pytest.raises(ValueError, match="'z'"):
        fairness_metrics(m, fr, PROT, ["M", "z"], "yes")               # not a level of race
    with pytest.raises(ValueError, match="one level per protected column"):
        fairness_metrics(m, fr, PROT, ["M"], "yes")
    with pytest.raises(ValueError, match="'maybe'"):
        fairness_metrics(m, fr, PROT, REF, "maybe")


def test_compat_imports_resolve():
    import h2o
    from h2o.explanation import disparate_analysis, inspect_model_fairness
    from h2o3_amd.models import fairness
    assert disparate_analysis is fairness.disparate_analysis
    assert inspect_model_fairness is fairness.inspect_model_fairness
    assert callable(h2o.disparate_analysis) and callable(h2o.inspect_model_fairness)
    from h2o.explanation._explain import disparate_analysis as da2
    assert da2 is fairness.disparate_analysis


def test_sketch_torch_skips_filtered_rows():
    """The oracle's own row filter and flip, on 6 rows by hand."""
    from h2o3_amd.ops.fairness_ops import group_sketch
    p = torch.tensor([0.5, 0.9, float("nan"), 0.2, 0.7, 0.4], dtype=torch.float32)
    y = torch.tensor([1, 0, 1, 2, -1, 0], dtype=torch.int32)
    g = torch.tensor([0, 1, 0, 0, 1, 5], dtype=torch.int32)
    r = group_sketch(p, y, g, 2, 0.5, nb=8)
    assert not r.kernel and r.why == "CPU tensors"
    assert r.cm.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0]] and int(r.cnt.sum()) == 2
    f = group_sketch(p, y, g, 2, 0.5, flip=True, nb=8)
    assert f.cm.tolist() == [[0, 0, 1, 0], [0, 0, 0, 1]]               # p == thr is not selected once flipped
    assert f.cnt[0, 0].sum() == 1 and f.cnt[1, 1].sum() == 1
    assert f.sums[0, 0].item() == pytest.approx(-math.log(0.5))


# ------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(world, out):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", H2O3_DIST_BACKEND="gloo",
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "fairness_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    with open(out) as f:
        return json.load(f)


def test_two_ranks_equal_one_rank(tmp_path):
    """Rows sharded over 2 gloo ranks: the sketches are summed, so the
    overview equals the 1-rank one (the counts exactly; the logloss sums are
    added in another order)."""
    one = _run_ranks(1, str(tmp_path / "w1.json"))
    two = _run_ranks(2, str(tmp_path / "w2.json"))
    assert two["local_rows"] < one["local_rows"] == 400
    assert one["columns"] == two["columns"] and one["tables"] == two["tables"]
    a, b = one["overview"], two["overview"]
    assert len(a) == len(b) == 12
    for ra, rb in zip(a, b):
        for k, va, vb in zip(one["columns"], ra, rb):
            if isinstance(va, str) or k in ("tp", "fp", "tn", "fn", "total", "selected"):
                assert va == vb, (k, va, vb)
            else:
                assert _same(float("nan") if va is None else va, float("nan") if vb is None else vb, 1e-12), (k, va, vb)
