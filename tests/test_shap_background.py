"""Baseline (interventional) SHAP: predict_contributions with a background
frame.  The torch implementation against the 2^F subset enumeration, the
public API on trained models, the REST route and a 2-rank run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd as h2o
from h2o3_amd.estimators import (H2OGradientBoostingEstimator, H2ORandomForestEstimator,
                                 H2OXGBoostEstimator)
from h2o3_amd.ops import shap_ops
from shap_bg_common import enumerate_all, hand_forest, hand_rows

HERE = os.path.dirname(os.path.abspath(__file__))
X_COLS = list("abcd") + ["k"]


def _df(n=600, seed=0):
    """The frame of test_shap.py's _df()."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 4))
    X[rng.random(n) < 0.05, 2] = np.nan
    df = pd.DataFrame(X, columns=list("abcd"))
    df["k"] = rng.choice(["u", "v", "w"], n)
    df["y"] = 2 * X[:, 0] - X[:, 1] * (df["k"] == "u") + np.nan_to_num(X[:, 2]) + rng.normal(scale=0.2, size=n)
    df["yb"] = np.where(df["y"] > 0, "p", "n")
    return df


# ------------------------------------------------------------ enumeration
def test_torch_rule_matches_subset_enumeration():
    """Hand-built forest (3 trees, depth <= 4, 6 features, one categorical
    split, NaNs and out-of-range codes in both frames): every one of the
    5 x 4 pairs equals the exact Shapley values of the hybrid-row game."""
    fo = hand_forest()
    X, Z = hand_rows(5, 1), hand_rows(4, 2)
    ref = enumerate_all(fo, X, Z)
    dev = torch.device("cpu")
    P, PT = fo.pack(dev), fo.leaf_paths(dev)
    phi, fz = shap_ops.background_shap_torch(P, PT, torch.tensor(X), torch.tensor(Z), 6, per_reference=True)
    np.testing.assert_allclose(phi.numpy(), ref, rtol=0, atol=1e-12)
    avg, _ = shap_ops.background_shap_torch(P, PT, torch.tensor(X), torch.tensor(Z), 6)
    np.testing.assert_allclose(avg.numpy(), ref.reshape(5, 4, 7).mean(1), rtol=0, atol=1e-12)
    res = shap_ops.background_shap(P, PT, torch.tensor(X), torch.tensor(Z), 6, per_reference=True)
    assert not res.kernel and res.why == "CPU tensors"
    np.testing.assert_allclose(res.phi.numpy(), ref, rtol=0, atol=1e-12)


def test_leaf_path_table_is_cached_and_dropped_with_the_pack():
    fo = hand_forest()
    dev = torch.device("cpu")
    PT = fo.leaf_paths(dev)
    assert fo.leaf_paths(dev) is PT
    assert PT["L"] == sum(len(t.leaves()) for t in fo.trees) and PT["max_path"] == 4
    # conditions index the packed node arrays
    P = fo.pack(dev)
    assert torch.equal(P["feat"][PT["cond_node"].long()],
                       PT["el_feat"][torch.repeat_interleave(torch.arange(PT["el_feat"].numel()),
                                                             torch.diff(PT["cond_off"]).long())])
    fo.add(fo.trees[0], 0)
    assert fo.leaf_paths(dev) is not PT and fo.leaf_paths(dev)["L"] > PT["L"]


def test_plan_tiles_fit_the_budget_and_empty_input():
    fo = hand_forest()
    PT = fo.leaf_paths(torch.device("cpu"))
    lmin = PT["max_tree_leaves"]
    rt, bt, chunks = shap_ops._plan(PT, 0, 9, 1 << 30, False)
    assert rt >= 64 and bt == 9 and chunks == [(0, PT["L"])]
    for scale in (False, True):
        budget = 4 * lmin * (64 + 5) + (40 * 64 * 5 if scale else 0)
        rt, bt, chunks = shap_ops._plan(PT, 1000, 33, budget, scale)
        assert rt == 64 and bt <= 5 and len(chunks) == len(fo.trees)
        for l0, l1 in chunks:
            assert 4 * (l1 - l0) * (rt + bt) + (40 * rt * bt if scale else 0) <= budget
    with pytest.raises(ValueError):
        shap_ops._plan(PT, 1000, 33, 100, False)


# ------------------------------------------------------------ trained models
@pytest.fixture(scope="module")
def trained():
    h2o.init()
    fr = h2o.H2OFrame(_df())
    bg = h2o.H2OFrame(_df(40, seed=5))
    ms = {}
    ms["gbm_bernoulli"] = H2OGradientBoostingEstimator(ntrees=10, max_depth=4, seed=1)
    ms["gbm_bernoulli"].train(x=X_COLS, y="yb", training_frame=fr)
    ms["gbm_gaussian"] = H2OGradientBoostingEstimator(ntrees=10, max_depth=5, seed=1)
    ms["gbm_gaussian"].train(x=X_COLS, y="y", training_frame=fr)
    ms["xgboost"] = H2OXGBoostEstimator(ntrees=5, max_depth=4, seed=2)
    ms["xgboost"].train(x=X_COLS, y="y", training_frame=fr)
    ms["drf_regression"] = H2ORandomForestEstimator(ntrees=5, max_depth=5, seed=2)
    ms["drf_regression"].train(x=X_COLS, y="y", training_frame=fr)
    ms["drf_binomial"] = H2ORandomForestEstimator(ntrees=5, max_depth=5, seed=2)
    ms["drf_binomial"].train(x=X_COLS, y="yb", training_frame=fr)
    return fr, bg, ms


MODELS = ["gbm_bernoulli", "gbm_gaussian", "xgboost", "drf_regression", "drf_binomial"]


def _link_and_response(m, fr):
    """(link-space prediction, response-space prediction) as f64 arrays; for
    DRF both are model.predict's p1 / prediction."""
    pr = m.predict(fr).as_data_frame()
    resp = pr["p"].values if "p" in pr.columns else pr["predict"].values
    if m.algo == "drf":
        return resp.astype(np.float64), resp.astype(np.float64)
    f = m._forest.predict(m._score_matrix(fr), 1)[:, 0].double().cpu().numpy() + float(m._init_f[0])
    return f, resp.astype(np.float64)


@pytest.mark.parametrize("name", MODELS)
def test_background_contributions_on_trained_models(trained, name):
    fr, bg, ms = trained
    m = ms[name]
    N, B = fr.nrows, bg.nrows
    fx, px = _link_and_response(m, fr)
    fz, pz = _link_and_response(m, bg)
    atol = 1e-5 * max(1.0, np.abs(fx).max(), np.abs(fz).max())
    cols = X_COLS + ["BiasTerm"]
    c = m.predict_contributions(fr, background_frame=bg).as_data_frame()
    assert list(c.columns) == cols
    # rows sum to the link-space prediction; the bias is the mean background prediction
    np.testing.assert_allclose(c[cols].values.astype(np.float64).sum(1), fx, rtol=0, atol=atol)
    np.testing.assert_allclose(c["BiasTerm"].values, np.full(N, fz.mean()), rtol=0, atol=atol)
    # per reference: names, order, mean == averaged output, rows sum to f(x), bias f(z)
    pr = m.predict_contributions(fr, background_frame=bg, output_per_reference=True).as_data_frame()
    assert list(pr.columns) == cols + ["RowIdx", "BackgroundRowIdx"]
    assert pr.shape[0] == N * B
    np.testing.assert_array_equal(pr["RowIdx"].values, np.repeat(np.arange(N), B))
    np.testing.assert_array_equal(pr["BackgroundRowIdx"].values, np.tile(np.arange(B), N))
    mean = pr.groupby("RowIdx")[cols].mean().values
    np.testing.assert_allclose(mean, c[cols].values, rtol=0, atol=atol)
    np.testing.assert_allclose(pr[cols].values.astype(np.float64).sum(1), np.repeat(fx, B), rtol=0, atol=atol)
    np.testing.assert_allclose(pr["BiasTerm"].values, np.tile(fz, N), rtol=0, atol=atol)
    # output space: rows sum to the response-space prediction, pairs to p(x) - p(z)
    atol_p = 1e-5 * max(1.0, np.abs(px).max(), np.abs(pz).max())
    co = m.predict_contributions(fr, background_frame=bg, output_space=True).as_data_frame()
    np.testing.assert_allclose(co[cols].values.astype(np.float64).sum(1), px, rtol=0, atol=atol_p)
    po = m.predict_contributions(fr, background_frame=bg, output_space=True,
                                 output_per_reference=True).as_data_frame()
    np.testing.assert_allclose(po[X_COLS].values.astype(np.float64).sum(1),
                               np.repeat(px, B) - np.tile(pz, N), rtol=0, atol=atol_p)
    np.testing.assert_allclose(po["BiasTerm"].values, np.tile(pz, N), rtol=0, atol=atol_p)
    if m.algo == "drf" or m._dist.link == "identity":           # output space is the link space
        np.testing.assert_allclose(co[cols].values, c[cols].values, rtol=0, atol=atol)


def test_sorted_output_and_unchanged_default(trained):
    fr, bg, ms = trained
    m = ms["gbm_bernoulli"]
    top = m.predict_contributions(fr, top_n=2, bottom_n=1, background_frame=bg,
                                  output_per_reference=True).as_data_frame()
    assert list(top.columns) == ["top_feature_1", "top_value_1", "top_feature_2", "top_value_2",
                                 "bottom_feature_1", "bottom_value_1", "BiasTerm", "RowIdx", "BackgroundRowIdx"]
    full = m.predict_contributions(fr, background_frame=bg, output_per_reference=True).as_data_frame()
    np.testing.assert_allclose(top["top_value_1"].values, full[X_COLS].values.max(1))
    np.testing.assert_allclose(top["bottom_value_1"].values, full[X_COLS].values.min(1))
    # no background frame: the path-dependent TreeSHAP of before (cover-weighted bias)
    c0 = m.predict_contributions(fr).as_data_frame()
    assert list(c0.columns) == X_COLS + ["BiasTerm"]
    cb = m.predict_contributions(fr, background_frame=bg).as_data_frame()
    assert abs(c0["BiasTerm"].values[0] - cb["BiasTerm"].values[0]) > 1e-4


def test_argument_errors(trained):
    fr, bg, ms = trained
    for m in (ms["gbm_bernoulli"], ms["drf_regression"], ms["xgboost"]):
        with pytest.raises(ValueError):
            m.predict_contributions(fr, output_space=True)
        with pytest.raises(ValueError):
            m.predict_contributions(fr, output_per_reference=True)
    d2 = H2ORandomForestEstimator(ntrees=2, max_depth=3, seed=2, binomial_double_trees=True)
    d2.train(x=X_COLS, y="yb", training_frame=fr)
    with pytest.raises(ValueError):
        d2.predict_contributions(fr, background_frame=bg)
    df3 = _df()
    df3["y3"] = np.where(df3.a > 0.5, "hi", np.where(df3.a < -0.5, "lo", "mid"))
    m3 = H2OGradientBoostingEstimator(ntrees=2, max_depth=3, seed=1)
    m3.train(x=X_COLS, y="y3", training_frame=h2o.H2OFrame(df3))
    with pytest.raises(ValueError):
        m3.predict_contributions(fr, background_frame=bg)


def test_generic_tree_mojo_forwards_background_frame(trained, tmp_path):
    fr, bg, ms = trained
    m = ms["gbm_bernoulli"]
    path = m.download_mojo(str(tmp_path))
    g = h2o.import_mojo(path)
    ref = m.predict_contributions(fr, background_frame=bg, output_per_reference=True).as_data_frame()
    got = g.predict_contributions(fr, background_frame=bg, output_per_reference=True).as_data_frame()
    assert list(got.columns) == list(ref.columns)
    np.testing.assert_allclose(got.values.astype(np.float64), ref.values.astype(np.float64), rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        g.predict_contributions(fr, output_per_reference=True)


# ------------------------------------------------------------ REST
def test_rest_predictions_route_forwards_background_frame():
    from fastapi.testclient import TestClient
    from h2o3_amd.core import dkv
    from h2o3_amd.server import create_app
    from test_rest import _wait
    c = TestClient(create_app())
    df = _df(200, seed=3)[X_COLS + ["yb"]].fillna(0.0)
    bgd = _df(7, seed=4)[X_COLS + ["yb"]].fillna(0.0)
    for d, key in ((df, "shapbg_train.hex"), (bgd, "shapbg_bg.hex")):
        r = c.post("/3/PostFile", json={"data": d.to_dict(orient="list"), "destination_frame": key})
        assert r.json()["destination_frame"] == key
    r = c.post("/3/ModelBuilders/gbm", json={"training_frame": "shapbg_train.hex", "response_column": "yb",
                                              "ntrees": 3, "max_depth": 3, "model_id": "gbm_shapbg"})
    assert _wait(c, r.json()["job"])["status"] == "DONE"
    pr = c.post("/3/Predictions/models/gbm_shapbg/frames/shapbg_train.hex",
                json={"predict_contributions": True, "background_frame": "shapbg_bg.hex",
                      "output_per_reference": True, "predictions_frame": "shapbg_contrib"}).json()
    assert pr["predictions_frame"]["name"] == "shapbg_contrib"
    out = dkv.get("shapbg_contrib")
    assert out.names == X_COLS + ["BiasTerm", "RowIdx", "BackgroundRowIdx"]
    assert out.nrows == 200 * 7
    # the sorting arguments the client sends reach the model too
    pr = c.post("/3/Predictions/models/gbm_shapbg/frames/shapbg_train.hex",
                json={"predict_contributions": True, "top_n": 1, "bottom_n": 0, "compare_abs": True,
                      "predictions_frame": "shapbg_top"}).json()
    assert dkv.get(pr["predictions_frame"]["name"]).names == ["top_feature_1", "top_value_1", "BiasTerm"]


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
                   MASTER_PORT=str(port), CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "shap_bg_worker.py"), out], env=env,
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
    """Background frame and test frame row-sharded over 2 gloo ranks: the
    background rows are gathered, so the result equals the 1-rank one."""
    one = _run_ranks(1, str(tmp_path / "w1.json"))
    two = _run_ranks(2, str(tmp_path / "w2.json"))
    assert one["trees"] == two["trees"]
    assert two["bg_local_rows"] < one["bg_local_rows"] == 30
    for k in ("avg", "per_ref"):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.shape == b.shape
        np.testing.assert_allclose(b, a, rtol=0, atol=1e-6)
    assert one["per_ref_cols"] == two["per_ref_cols"]
