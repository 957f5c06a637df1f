"""shap_path_kernel (ops/csrc/tree_shap.hip, path-dependent TreeSHAP) against
the node recursion and the torch implementation of the leaf-path rule, both
computed on CPU copies of the inputs, and against the scoring kernel's
decisions (Forest.predict).  Model level: predict_contributions on the kernel
against the same call under H2O3_TREE_SHAP=torch."""

import numpy as np
import pandas as pd
import pytest
import torch

from shap_path_common import chain_forest, covers_by_share, covers_from_rows, hand_forest, hand_rows

pytestmark = pytest.mark.gpu

# f64 atomic sums of O(1) leaf values (the tolerances of test_shap_background_gpu.py)
RTOL, ATOL = 1e-10, 1e-9
N_TEST = 777
CPU = torch.device("cpu")


def _run(fo, X, F, **kw):
    from h2o3_amd.ops import shap_ops
    dev = X.device
    return shap_ops.path_shap(fo.pack(dev), fo.leaf_paths(dev), X, F, **kw)


def _oracles(fo, X, F, vscale=1.0, tree_class=0):
    """(recursion, torch leaf-path rule) on CPU copies: [N, F] feature columns."""
    from h2o3_amd.models.tree.shap import forest_contributions
    from h2o3_amd.ops import shap_ops
    Xc = X.cpu()
    trees = [t for t, k in zip(fo.trees, fo.tclass) if k == tree_class]
    rec = forest_contributions(trees, Xc, F, scale=vscale)[:, :F]
    tor = shap_ops.path_shap_torch(fo.pack(CPU), fo.leaf_paths(CPU), Xc, F, vscale, tree_class)[:, :F]
    return rec.numpy(), tor.numpy()


def _check(res, oracles, F):
    assert res.kernel and res.why is None
    got = res.phi.cpu().numpy()
    assert not got[:, F].any()                             # the bias column is the caller's
    for want in oracles:
        np.testing.assert_allclose(got[:, :F], want, rtol=RTOL, atol=ATOL)


def _bias(fo, vscale=1.0, tree_class=0):
    return vscale * sum(sum(t.value[j] * max(t.weight[j], 0.0) for j in t.leaves()) / t.weight[0]
                        for t, k in zip(fo.trees, fo.tclass) if k == tree_class)


@pytest.mark.parametrize("rows", [6, 40])
def test_hand_built_forest(rows):
    """Covers counted from 6 routed rows leave zero-cover children; features
    repeat on a path; a categorical split; NaN and out-of-range codes."""
    fo = covers_from_rows(hand_forest(), hand_rows(rows, 3))
    X = torch.tensor(hand_rows(70, 1), device="cuda")
    _check(_run(fo, X, 6), _oracles(fo, X, 6), 6)
    _check(_run(fo, X, 6, vscale=0.25), _oracles(fo, X, 6, vscale=0.25), 6)


@pytest.fixture(scope="module")
def gbm_case():
    """The GBM of test_shap_background_gpu.py's gbm_case (10 trees, depth 5,
    numeric + categorical columns with NAs); the 777-row score matrix gets NaN
    and out-of-range categorical codes; the CPU oracles are computed once."""
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    rng = np.random.default_rng(11)
    n = 1500
    A = rng.normal(size=(n, 5))
    A[rng.random(n) < 0.06, 1] = np.nan
    df = pd.DataFrame(A, columns=[f"x{i}" for i in range(5)])
    df["c1"] = rng.choice(list("abcdefg"), n)
    df["c2"] = rng.choice(["u", "v", "w"], n)
    df.loc[rng.random(n) < 0.05, "c1"] = None
    df["y"] = (A[:, 0] + np.nan_to_num(A[:, 1]) * (df["c2"] == "u") - 0.7 * (df["c1"].isin(["a", "d"])) +
               0.5 * A[:, 2] * A[:, 3] + rng.normal(scale=0.2, size=n))
    fr = h2o.H2OFrame(df)
    x = [f"x{i}" for i in range(5)] + ["c1", "c2"]
    m = H2OGradientBoostingEstimator(ntrees=10, max_depth=5, seed=1, min_rows=5)
    m.train(x=x, y="y", training_frame=fr)
    M = m._score_matrix(fr).clone()
    assert M.is_cuda
    X = M[:, :N_TEST].contiguous()
    X[5, 0], X[5, 1], X[5, 2], X[6, 3], X[6, 4] = float("nan"), 40.0, -3.0, 3.0, float("nan")
    X[0, 5] = float("nan")
    fo = m._forest
    F = len(x)
    assert fo.leaf_paths(X.device)["L"] > 100
    return fo, X, F, _oracles(fo, X, F)


def test_trained_gbm_default_scratch(gbm_case):
    fo, X, F, ref = gbm_case
    res = _run(fo, X, F)
    assert (res.row_tiles, res.tree_chunks) == (1, 1)
    assert res.phi.shape == (N_TEST, F + 1)
    _check(res, ref, F)


def test_trained_gbm_tiled(gbm_case):
    """A scratch bound that holds one tree's masks for 256 rows: 4 row tiles
    (777 rows) and at least 3 tree chunks."""
    fo, X, F, ref = gbm_case
    PT = fo.leaf_paths(X.device)
    res = _run(fo, X, F, max_scratch_bytes=4 * PT["max_tree_leaves"] * 256)
    assert res.row_tiles >= 3 and res.tree_chunks >= 3, (res.row_tiles, res.tree_chunks)
    _check(res, ref, F)


def test_empty_row_shard(gbm_case):
    fo, X, F, _ = gbm_case
    res = _run(fo, X[:, :0].contiguous(), F)
    assert res.kernel and res.phi.shape == (0, F + 1)


def test_row_sums_match_forest_predict(gbm_case):
    """The kernel and the scoring kernel take the same decisions: feature
    columns + bias sum to the forest's score.  Forest.predict sums in f32."""
    from h2o3_amd.models.tree.shap import forest_path_contributions
    fo, X, F, _ = gbm_case
    fx = fo.predict(X, 1)[:, 0].double()
    info = {}
    phi = forest_path_contributions(fo, X, F, info=info)
    assert info == {"kernel": True, "why": None}
    torch.testing.assert_close(phi.sum(1), fx, rtol=0, atol=1e-5)
    torch.testing.assert_close(phi[:, F], torch.full_like(fx, _bias(fo)), rtol=0, atol=1e-12)


def test_deep_drf_scores_class_0_trees_only():
    """DRF, 4 iterations of double trees (8 trees, 4 of class 0), depth 12,
    min_rows = 1: many leaves, longer paths, vscale = 1 / ntrees."""
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2ORandomForestEstimator
    rng = np.random.default_rng(5)
    n = 1500
    A = rng.normal(size=(n, 6))
    A[rng.random(n) < 0.05, 2] = np.nan
    df = pd.DataFrame(A, columns=[f"x{i}" for i in range(6)])
    df["c"] = rng.choice(list("abcd"), n)
    df["y"] = np.where(A[:, 0] + np.nan_to_num(A[:, 2]) * A[:, 1] + rng.normal(scale=0.5, size=n) > 0, "p", "n")
    fr = h2o.H2OFrame(df)
    x = [f"x{i}" for i in range(6)] + ["c"]
    m = H2ORandomForestEstimator(ntrees=4, max_depth=12, min_rows=1, seed=3, binomial_double_trees=True)
    m.train(x=x, y="y", training_frame=fr)
    fo = m._forest
    assert sorted(set(fo.tclass)) == [0, 1] and fo.tclass.count(0) == 4
    X = m._score_matrix(fr)[:, :300].contiguous()
    assert X.is_cuda and fo.leaf_paths(X.device)["L"] > 500
    _check(_run(fo, X, 7, vscale=0.25), _oracles(fo, X, 7, vscale=0.25), 7)
    _check(_run(fo, X, 7, vscale=0.25, tree_class=1), _oracles(fo, X, 7, vscale=0.25, tree_class=1), 7)


@pytest.mark.parametrize("width", [32, 33])
def test_wide_paths(width):
    """A chain tree whose longest path has exactly 32 distinct features runs
    on the kernel; with 33 the torch implementation runs and the result says
    why.  Covers: every split sends 0.4 / 0.6 of its cover left / right."""
    fo = covers_by_share(chain_forest(width, seed=4), left=0.4)
    F = width + 1
    g = torch.Generator().manual_seed(5)
    X = torch.randn(F, 70, generator=g)
    X[3, 0] = X[31, 1] = float("nan")
    X = X.cuda()
    assert fo.leaf_paths(X.device)["max_path"] == width
    res = _run(fo, X, F)
    if width <= 32:
        _check(res, _oracles(fo, X, F), F)
    else:
        assert not res.kernel and "33 distinct features" in res.why
        for want in _oracles(fo, X, F):
            np.testing.assert_allclose(res.phi.cpu().numpy()[:, :F], want, rtol=RTOL, atol=ATOL)
    from h2o3_amd.models.tree.shap import forest_path_contributions
    fx = fo.predict(X, 1)[:, 0].double()
    torch.testing.assert_close(forest_path_contributions(fo, X, F).sum(1), fx, rtol=0, atol=1e-5)


@pytest.mark.parametrize("F", [40, 120, 320])
def test_many_features(F):
    """One F per launch form: per-row LDS sums within 64 KiB (F = 40), above
    it (F = 120) and, past the LDS of a CU (F = 320), global f64 atomics.  The
    forest splits on features spread over 0 .. F-1 and 130 rows span three
    blocks, the last one ragged."""
    from h2o3_amd.ops import _native
    lib = _native.get_lib("tree_shap", required=True)
    lds = lib.h2o_shap_path_lds_bytes(F)
    if F == 40:
        assert lds <= (64 << 10)
    elif F == 120:
        assert (64 << 10) < lds <= (160 << 10)
    else:
        assert lds > (160 << 10)
    feats = [int(v) for v in np.linspace(0, F - 1, 20)]
    fo = covers_by_share(chain_forest(20, seed=6, feats=feats), left=0.4)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(F, 130, generator=g)
    X[feats[3], 0] = float("nan")
    X = X.cuda()
    res = _run(fo, X, F)
    _check(res, _oracles(fo, X, F), F)
    fx = fo.predict(X, 1)[:, 0].double()
    torch.testing.assert_close(res.phi.sum(1) + _bias(fo), fx, rtol=0, atol=1e-5)


# ------------------------------------------------------------------ model level
def _model_frame():
    rng = np.random.default_rng(2)
    n = 500
    A = rng.normal(size=(n, 4)).astype(np.float32).astype(np.float64)
    A[rng.random(n) < 0.05, 2] = np.nan
    df = pd.DataFrame(A, columns=list("abcd"))
    df["k"] = rng.choice(["u", "v", "w"], n)
    eta = 2 * A[:, 0] - A[:, 1] * (df["k"] == "u") + np.nan_to_num(A[:, 2])
    df["yb"] = np.where(eta + rng.normal(scale=0.3, size=n) > 0, "p", "n")
    df["y"] = eta + rng.normal(scale=0.2, size=n)
    return df


def _ab(model, fr, monkeypatch):
    """predict_contributions on the kernel and under H2O3_TREE_SHAP=torch."""
    monkeypatch.delenv("H2O3_TREE_SHAP", raising=False)
    got = model.predict_contributions(fr).as_data_frame()
    assert model._shap_path_why is None
    top = model.predict_contributions(fr, top_n=2, bottom_n=1).as_data_frame()
    monkeypatch.setenv("H2O3_TREE_SHAP", "torch")
    want = model.predict_contributions(fr).as_data_frame()
    assert model._shap_path_why == "H2O3_TREE_SHAP=torch"
    top_want = model.predict_contributions(fr, top_n=2, bottom_n=1).as_data_frame()
    monkeypatch.delenv("H2O3_TREE_SHAP")
    assert list(got.columns) == list(want.columns) and got.columns[-1] == "BiasTerm"
    np.testing.assert_allclose(got.values, want.values, rtol=RTOL, atol=ATOL)
    names = [c for c in top.columns if "feature" in c]
    assert len(names) == 3 and list(top.columns) == list(top_want.columns)
    for c in names:
        assert list(top[c]) == list(top_want[c])
    return got


@pytest.mark.parametrize("algo", ["gbm", "drf", "xgboost", "generic"])
def test_model_contributions_match_recursion(algo, monkeypatch, tmp_path):
    import h2o3_amd as h2o
    from h2o3_amd.estimators import (H2OGradientBoostingEstimator, H2ORandomForestEstimator,
                                     H2OXGBoostEstimator)
    h2o.init(verbose=False)
    fr = h2o.H2OFrame(_model_frame())
    x = list("abcd") + ["k"]
    if algo == "drf":
        m = H2ORandomForestEstimator(ntrees=4, max_depth=4, seed=2)
    elif algo == "xgboost":
        m = H2OXGBoostEstimator(ntrees=4, max_depth=4, seed=2)
    else:
        m = H2OGradientBoostingEstimator(ntrees=4, max_depth=4, seed=1)
    m.train(x=x, y="y" if algo == "xgboost" else "yb", training_frame=fr)
    if algo == "generic":
        from h2o3_amd.models.generic import H2OGenericEstimator
        native = m.predict_contributions(fr).as_data_frame()
        m = H2OGenericEstimator.from_file(m.download_mojo(str(tmp_path), format="h2o"))
    got = _ab(m, fr, monkeypatch)
    if algo == "generic":
        np.testing.assert_allclose(got.values, native.values, rtol=1e-6, atol=2e-6)
