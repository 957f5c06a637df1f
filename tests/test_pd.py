"""2-D partial dependence (col_pairs_2dpdp) for tree and non-tree models, the
REST route, Forest.predict_grid against explicit override + predict, and the
forest-grid route of partial_plot / ice / h against the replacement loop
(H2O3_TREE_PD=torch).  CPU: the primitive's torch implementation runs.

Tolerances.  A table's mean is an f64 mean of per-row responses; the frame
model.predict returns may hold them rounded to f32 (eps 6e-8), so means are
compared with predict at 1e-6.  The forest-grid route and the loop see
bit-equal per-row responses and differ in the order of f64 sums only: 1e-10
relative, 1e-9 absolute (the SHAP kernel tests' pair)."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd as h2o
from h2o3_amd.estimators import H2OGeneralizedLinearEstimator, H2OGradientBoostingEstimator

from shap_path_common import hand_forest, hand_rows

STATS = ["mean_response", "stddev_response", "std_error_mean_response"]
X = list("abcd") + ["k"]
RTOL, ATOL = 1e-10, 1e-9


def _df(n=300, seed=1):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, 4))
    df = pd.DataFrame(A, columns=list("abcd"))
    df["k"] = rng.choice(["u", "v"], n)
    df["y"] = 3 * A[:, 0] + A[:, 1] * A[:, 2] * 2 + (df["k"] == "u") + rng.normal(scale=0.1, size=n)
    df["y3"] = np.where(df["y"] < -1.5, "lo", np.where(df["y"] < 1.5, "mid", "hi"))
    df["w"] = rng.uniform(0.5, 2.0, n)
    return df


@pytest.fixture(scope="module")
def data():
    h2o.init()
    df = _df()
    return df, h2o.H2OFrame(df)


@pytest.fixture(scope="module")
def gbm(data):
    m = H2OGradientBoostingEstimator(ntrees=8, max_depth=3, seed=1)
    m.train(x=X, y="y", training_frame=data[1])
    return m


@pytest.fixture(scope="module")
def glm(data):
    m = H2OGeneralizedLinearEstimator(family="gaussian", lambda_=0.0)
    m.train(x=X, y="y", training_frame=data[1])
    return m


def _by_hand(model, df, values, column="predict"):
    """model.predict's column on df with the columns of `values` set by hand."""
    d = df.copy()
    for c, v in values.items():
        d[c] = v
    return model.predict(h2o.H2OFrame(d)).as_data_frame()[column].values.astype(np.float64)


def _check_pair_table(model, df, tab, c1, c2, shape, weights=None, column="predict"):
    assert list(tab.columns) == [c1, c2] + STATS
    assert len(tab) == shape[0] * shape[1]
    v1, v2 = list(dict.fromkeys(tab[c1])), list(dict.fromkeys(tab[c2]))
    assert (len(v1), len(v2)) == shape
    # col1 is the outer loop, col2 the inner one
    assert [(a, b) for a, b in zip(tab[c1], tab[c2])] == [(a, b) for a in v1 for b in v2]
    for _, row in tab.iterrows():
        p = _by_hand(model, df, {c1: row[c1], c2: row[c2]}, column)
        np.testing.assert_allclose(row["mean_response"], np.average(p, weights=weights), rtol=1e-6, atol=1e-6)
    return tab


@pytest.mark.parametrize("algo", ["gbm", "glm"])
def test_pair_tables_follow_the_1d_tables(algo, data, gbm, glm):
    df, fr = data
    m = gbm if algo == "gbm" else glm
    tabs = m.partial_plot(fr, cols=["a"], col_pairs_2dpdp=[["a", "k"], ["b", "c"]], nbins=4)
    assert len(tabs) == 3
    assert list(tabs[0].columns) == ["a"] + STATS and len(tabs[0]) == 4
    _check_pair_table(m, df, tabs[1], "a", "k", (4, 2))
    _check_pair_table(m, df, tabs[2], "b", "c", (4, 4))
    assert (tabs[1]["stddev_response"] > 0).all()
    if algo == "glm":
        assert "not a tree model" in m._pd_why
    # cols may be empty when pairs are given
    only = m.partial_plot(fr, col_pairs_2dpdp=[["b", "c"]], nbins=4)
    assert len(only) == 1
    pd.testing.assert_frame_equal(only[0], tabs[2])


def test_pairs_include_na(data, gbm):
    df, fr = data
    tab = gbm.partial_plot(fr, cols=[], col_pairs_2dpdp=[["a", "k"]], nbins=3, include_na=True)[0]
    assert len(tab) == 4 * 3
    a_na = tab["a"].isna()
    k_na = tab["k"].apply(lambda v: isinstance(v, float) and v != v)
    assert a_na.sum() == 3 and k_na.sum() == 4 and (a_na & k_na).sum() == 1
    for _, row in tab.iterrows():
        kv = None if row["k"] != row["k"] else row["k"]
        p = _by_hand(gbm, df, {"a": row["a"], "k": kv})
        np.testing.assert_allclose(row["mean_response"], p.mean(), rtol=1e-6, atol=1e-6)


def test_pairs_row_index(data, gbm):
    """As in 1-D, the grid is taken from the one-row frame: the row's own value
    of a numeric column, every level of an enum column."""
    df, fr = data
    tab = gbm.partial_plot(fr, cols=[], col_pairs_2dpdp=[["a", "k"]], nbins=4, row_index=3)[0]
    one = gbm.partial_plot(fr, cols=["a"], nbins=4, row_index=3)[0]
    assert list(one["a"]) == [tab["a"][0]] and len(one) == 1
    _check_pair_table(gbm, df.iloc[[3]], tab, "a", "k", (1, 2))
    assert (tab["stddev_response"] == 0).all()
    tab = gbm.partial_plot(fr, cols=[], col_pairs_2dpdp=[["a", "b"]], row_index=3,
                           user_splits={"a": [-1.0, 0.5, 2.0]})[0]
    _check_pair_table(gbm, df.iloc[[3]], tab, "a", "b", (3, 1))


def test_pairs_weight_column(data, gbm):
    df, fr = data
    tab = gbm.partial_plot(fr, cols=[], col_pairs_2dpdp=[["b", "c"]], nbins=3, weight_column="w")[0]
    _check_pair_table(gbm, df, tab, "b", "c", (3, 3), weights=df["w"].values)
    plain = gbm.partial_plot(fr, cols=[], col_pairs_2dpdp=[["b", "c"]], nbins=3)[0]
    assert not np.allclose(tab["mean_response"], plain["mean_response"], rtol=1e-9, atol=0)


def test_pairs_targets_multinomial(data):
    df, fr = data
    m = H2OGradientBoostingEstimator(ntrees=3, max_depth=3, seed=1)
    m.train(x=X, y="y3", training_frame=fr)
    tabs = m.partial_plot(fr, cols=["a"], col_pairs_2dpdp=[["a", "k"]], nbins=3, targets=["hi", "lo"])
    assert [t.attrs["target"] for t in tabs] == ["hi", "lo", "hi", "lo"]
    assert list(tabs[0].columns) == ["a"] + STATS
    for t in tabs[2:]:
        _check_pair_table(m, df, t, "a", "k", (3, 2), column=t.attrs["target"])


def test_rest_route_returns_pair_tables(data):
    from fastapi.testclient import TestClient
    from h2o3_amd.server import create_app
    df, _ = data
    c = TestClient(create_app())
    c.post("/3/PostFile", json={"data": df[X + ["y"]].to_dict(orient="list"), "destination_frame": "pd2.hex"})
    assert c.post("/3/ModelBuilders/gbm", json={"training_frame": "pd2.hex", "response_column": "y", "ntrees": 3,
                                                "max_depth": 3, "model_id": "pd2_gbm"}).status_code == 200
    r = c.post("/3/PartialDependence/", json={"model_id": "pd2_gbm", "frame_id": "pd2.hex", "cols": ["a"],
                                              "nbins": 4, "col_pairs_2dpdp": [["a", "k"], ["b", "c"]],
                                              "destination_key": "pd2_out"})
    assert r.status_code == 200
    out = c.get("/3/PartialDependence/pd2_out").json()["partial_dependence_data"]
    assert len(out) == 3
    assert out[1]["name"] == "PartialDependence for a and k" and out[2]["name"] == "PartialDependence for b and c"
    assert [col["name"] for col in out[1]["columns"]][-5:] == ["a", "k"] + STATS
    assert out[1]["rowcount"] == 8 and out[2]["rowcount"] == 16
    # pairs alone, in the form-encoded list-of-lists spelling
    r = c.post("/3/PartialDependence/", data={"model_id": "pd2_gbm", "frame_id": "pd2.hex", "nbins": "3",
                                              "col_pairs_2dpdp": "[[a,k]]", "destination_key": "pd2_only"})
    assert r.status_code == 200
    out = c.get("/3/PartialDependence/pd2_only").json()["partial_dependence_data"]
    assert len(out) == 1 and out[0]["rowcount"] == 6


@pytest.mark.parametrize("cols", [[0], [4], [2, 4], [3, 0]])
def test_predict_grid_is_override_plus_predict(cols):
    """Forest.predict_grid on CPU tensors, on the hand-built forest (features
    repeat on a path, feature 4 is categorical): bit-equal to predict on a
    matrix with the rows overridden."""
    fo = hand_forest()
    Xm = torch.tensor(hand_rows(70, 1))
    axis = {0: [0.1, -0.8, float("nan"), 2.0], 2: [0.4, 0.0, -1.0, float("nan")],
            3: [-0.2, 0.9, float("inf"), 0.2], 4: [-1.0, 0.0, 3.0, float("nan")]}
    grid = torch.tensor([axis[c] for c in cols], dtype=torch.float32)
    got = fo.predict_grid(Xm, 1, cols, grid)
    assert got.shape == (4, 70, 1) and got.dtype == torch.float32
    for g in range(4):
        Xg = Xm.clone()
        for s, c in enumerate(cols):
            Xg[c] = grid[s, g]
        torch.testing.assert_close(got[g], fo.predict(Xg, 1), rtol=0, atol=0, equal_nan=True)
    assert any(not torch.equal(got[0], got[g]) for g in range(1, 4))
    with pytest.raises(ValueError):
        fo.predict_grid(Xm, 1, [0, 0], grid[[0, 0]])


def test_forest_grid_route_matches_the_loop(data, gbm, monkeypatch):
    """partial_plot, ice and h of a tree model: the forest-grid route (its
    torch implementation here) against the replacement loop."""
    from h2o3_amd.models.explain import ice
    _, fr = data
    kw = dict(cols=["a", "k"], col_pairs_2dpdp=[["a", "k"]], nbins=5, include_na=True)
    monkeypatch.delenv("H2O3_TREE_PD", raising=False)
    tabs = gbm.partial_plot(fr, **kw)
    assert gbm._pd_why == "CPU tensors"                 # the primitive ran, without a GPU
    curves = ice(gbm, fr, "b", nbins=6, max_rows=20)
    hval = gbm.h(fr, ["a", "c"])
    monkeypatch.setenv("H2O3_TREE_PD", "torch")
    want = gbm.partial_plot(fr, **kw)
    assert gbm._pd_why == "H2O3_TREE_PD=torch"
    want_curves = ice(gbm, fr, "b", nbins=6, max_rows=20)
    want_h = gbm.h(fr, ["a", "c"])
    assert len(tabs) == len(want) == 3
    for a, b in zip(tabs, want):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
        for c in a.columns:
            if c in STATS:
                np.testing.assert_allclose(a[c].values, b[c].values, rtol=RTOL, atol=ATOL)
            else:
                assert [str(v) for v in a[c]] == [str(v) for v in b[c]]
    assert list(curves.columns) == list(want_curves.columns) == ["row", "b", "response"]
    assert list(curves["row"]) == list(want_curves["row"])
    np.testing.assert_allclose(curves["b"].values, want_curves["b"].values, rtol=0, atol=0)
    np.testing.assert_allclose(curves["response"].values, want_curves["response"].values, rtol=0, atol=0)
    assert want_h > 0.01
    np.testing.assert_allclose(hval, want_h, rtol=RTOL, atol=ATOL)


def test_row_tiles_and_grid_chunks(data, gbm, monkeypatch):
    """A scratch bound of 100 rows per tile (3 tiles of the 300 rows) and 81
    grid points (two chunks of 64): the tiles' responses laid side by side
    are the one-tile responses, bit for bit."""
    from h2o3_amd.models.explain import _ForestGrid, _grid
    monkeypatch.delenv("H2O3_TREE_PD", raising=False)
    _, fr = data
    cs = ["a", "b"]
    vecs = [fr.vec(c) for c in cs]
    va, vb = (_grid(v, 9)[0] for v in vecs)
    axes = [[a for a in va for _ in vb], [b for _ in va for b in vb]]

    def collect(fg):
        assert fg.why_not(cs) is None
        out = torch.full((81, 300), float("nan"), dtype=torch.float64)
        seen = []
        for g0, r0, (r,) in fg.responses(cs, fg.adapt(cs, vecs, axes)):
            out[g0:g0 + r.shape[0], r0:r0 + r.shape[1]] = r
            seen.append((g0, r0, tuple(r.shape)))
        return out, seen
    one, seen1 = collect(_ForestGrid(gbm, fr))
    assert seen1 == [(0, 0, (64, 300)), (64, 0, (17, 300))]
    tiled, seen3 = collect(_ForestGrid(gbm, fr, max_scratch_bytes=4 * 64 * 100))
    assert [s[:2] for s in seen3] == [(g, r) for r in (0, 100, 200) for g in (0, 64)]
    assert not torch.isnan(one).any()
    torch.testing.assert_close(tiled, one, rtol=0, atol=0)
