"""pd_node_mask_kernel + pd_walk_kernel (ops/csrc/tree_pd.hip) against
Forest._predict_torch on CPU copies of the score matrix with the rows
overridden: bit for bit (rtol = atol = 0), since the kernel adds the same f32
leaf values in tree order.  Model level: partial_plot / h / ice on the kernel
against the same calls under H2O3_TREE_PD=torch; the per-row responses are
bit-equal there, so the tables differ in the order of f64 sums only (RTOL,
ATOL of test_shap_path_gpu.py)."""
import numpy as np
import pandas as pd
import pytest
import torch

from shap_path_common import chain_forest, hand_forest, hand_rows
from test_shap_path_gpu import _model_frame

from h2o3_amd.ops import pd_ops

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-9
N_TEST = 777
CPU = torch.device("cpu")
NAN, INF = float("nan"), float("inf")


def _run(fo, X, K, cols, grid, **kw):
    return pd_ops.forest_grid_sums(fo.pack(X.device), X, K, cols, grid.to(X.device), **kw)


def _oracle(fo, X, K, cols, grid):
    """[G, N, K]: Forest._predict_torch on CPU copies of X, rows overridden."""
    from h2o3_amd.models.tree.shared import Forest
    P = fo.pack(CPU)
    Xc = X.cpu().clone()
    out = []
    for g in range(grid.shape[1]):
        for s, c in enumerate(cols):
            Xc[c] = grid[s, g]
        out.append(Forest._predict_torch(Xc, K, P))
    return torch.stack(out) if out else torch.zeros((0, X.shape[1], K))


def _check(res, want, chunks=None):
    assert res.kernel and res.why is None
    if chunks is not None:
        assert res.grid_chunks == chunks
    assert res.sums.dtype == torch.float32 and res.sums.shape == want.shape
    torch.testing.assert_close(res.sums.cpu(), want, rtol=0, atol=0)


def _f32(*v):
    return torch.tensor(v, dtype=torch.float32)


# ------------------------------------------------------------------ hand-built forest
def test_hand_forest_numeric_column():
    """Feature 0 splits at 0.1, -0.8 and 0.0: the grid holds two of the
    thresholds exactly (x < thr is false there), the float below one of
    them, both infinities and NaN."""
    fo = hand_forest()
    X = torch.tensor(hand_rows(70, 1), device="cuda")
    t = np.float32(0.1)
    grid = _f32(t, np.float32(-0.8), np.nextafter(t, np.float32(-1)), INF, -INF, NAN, 0.05, -3.0).view(1, -1)
    want = _oracle(fo, X, 1, [0], grid)
    assert not torch.equal(want[0], want[2])               # the threshold and the float below it part ways
    _check(_run(fo, X, 1, [0], grid), want, chunks=1)


def test_hand_forest_categorical_column():
    """Feature 4 has 4 levels: codes -1, 0 .. 4 (= card), card + 3 and NaN."""
    fo = hand_forest()
    X = torch.tensor(hand_rows(70, 1), device="cuda")
    grid = _f32(-1, 0, 1, 2, 3, 4, 7, NAN).view(1, -1)
    _check(_run(fo, X, 1, [4], grid), _oracle(fo, X, 1, [4], grid), chunks=1)


def test_hand_forest_numeric_and_categorical_columns():
    fo = hand_forest()
    X = torch.tensor(hand_rows(70, 1), device="cuda")
    num = [-0.5, -0.2, 0.2, 0.9, NAN]
    cat = [0, 1, 2, 3, 9, NAN]
    grid = _f32(*[[a for a in num for _ in cat], [b for _ in num for b in cat]])
    assert grid.shape == (2, 30)
    _check(_run(fo, X, 1, [3, 4], grid), _oracle(fo, X, 1, [3, 4], grid))


# ------------------------------------------------------------------ trained GBM
@pytest.fixture(scope="module")
def gbm_case():
    """The GBM of test_shap_path_gpu.py's gbm_case (10 trees, depth 5, numeric
    + categorical columns with NAs); the 777-row score matrix (four blocks of
    256, the last one ragged) gets NaN and out-of-range categorical codes and
    an 8th row no tree splits on.  The oracle of the 130-point grid on x0 is
    computed once; the smaller grids are its prefixes."""
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
    X = torch.cat([M[:, :N_TEST], torch.randn(1, N_TEST, device=M.device)]).contiguous()
    X[5, 0], X[5, 1], X[5, 2], X[6, 3], X[6, 4] = NAN, 40.0, -3.0, 3.0, NAN
    X[0, 5] = NAN
    fo = m._forest
    assert pd_ops.max_depth(fo.pack(X.device)) == 5
    g = torch.Generator().manual_seed(3)
    grid = torch.cat([torch.randn(126, generator=g) * 1.5, _f32(NAN, INF, -INF, 0.0)]).view(1, -1)
    grid = grid[:, torch.randperm(130, generator=g)]
    return fo, X, grid, _oracle(fo, X, 1, [0], grid)


@pytest.mark.parametrize("G,chunks", [(20, 1), (64, 1), (65, 2), (130, 3)])
def test_trained_gbm_grid_sizes(gbm_case, G, chunks):
    """G = 64 is the full mask (1 << 64 would be the trap), G = 65 a second
    chunk of one bit."""
    fo, X, grid, want = gbm_case
    _check(_run(fo, X, 1, [0], grid[:, :G].contiguous()), want[:G], chunks=chunks)


def test_trained_gbm_two_columns(gbm_case):
    """x1 (numeric, has NAs) and c1 (7 levels)."""
    fo, X, _, _ = gbm_case
    num = [-1.0, 0.0, 0.7, NAN]
    cat = [0, 2, 3, 6, 7, NAN]
    grid = _f32(*[[a for a in num for _ in cat], [b for _ in num for b in cat]])
    _check(_run(fo, X, 1, [1, 5], grid), _oracle(fo, X, 1, [1, 5], grid))


def test_column_without_splits(gbm_case):
    """Row 7 of the matrix is a column the forest never splits on: the mask
    never splits and all G outputs equal predict."""
    fo, X, _, _ = gbm_case
    grid = _f32(-1.0, 0.0, NAN, 5.0).view(1, -1)
    res = _run(fo, X, 1, [7], grid)
    assert res.kernel and res.why is None
    want = fo.predict(X, 1)
    for g in range(4):
        torch.testing.assert_close(res.sums[g], want, rtol=0, atol=0)
    torch.testing.assert_close(want.cpu(), _oracle(fo, X, 1, [7], grid[:, :1])[0], rtol=0, atol=0)


def test_row_tile_in_place(gbm_case):
    """Rows [256, 600) through the row offset and X's leading dimension."""
    fo, X, grid, want = gbm_case
    res = _run(fo, X, 1, [0], grid[:, :20].contiguous(), row0=256, nrows=344)
    _check(res, want[:20, 256:600])


def test_empty_row_shard(gbm_case):
    fo, X, grid, _ = gbm_case
    res = _run(fo, X[:, :0].contiguous(), 1, [0], grid[:, :20].contiguous())
    assert res.kernel and res.sums.shape == (20, 0, 1)


def test_forest_without_trees(gbm_case):
    from h2o3_amd.models.tree.shared import Forest
    _, X, grid, _ = gbm_case
    res = _run(Forest(), X, 1, [0], grid[:, :20].contiguous())
    assert res.kernel and res.sums.shape == (20, N_TEST, 1) and not res.sums.any()


def test_launch_shape():
    """The default grid keeps a 256-row block; 64 points on a depth-20 forest
    fit one block into the 160 KiB of a CU."""
    assert pd_ops.launch_shape(20, 8) == (256, 256 * (8 * 12 + 20 * 4))
    th, lds = pd_ops.launch_shape(64, 20)
    assert th == 256 and lds == 256 * (20 * 12 + 64 * 4) <= (160 << 10)
    th, lds = pd_ops.launch_shape(64, pd_ops.MAX_DEPTH)
    assert th == 128 and lds <= (160 << 10)


# ------------------------------------------------------------------ other forests
def test_deep_drf_two_classes():
    """DRF, 4 iterations of double trees, depth 12, min_rows = 1 (the forest
    of test_deep_drf_scores_class_0_trees_only): K = 2 goes through the class
    filter; 64 grid points on the most-split column drive the stack hardest."""
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
    P = fo.pack(X.device)
    assert X.is_cuda and 8 <= pd_ops.max_depth(P) <= 12
    inner = P["left"] >= 0
    col = int(torch.bincount(P["feat"][inner].long(), minlength=7).argmax())
    assert col < 6                                          # a numeric column
    grid = torch.cat([torch.linspace(-2.5, 2.5, 63), _f32(NAN)]).view(1, -1)
    want = _oracle(fo, X, 2, [col], grid)
    assert want[:, :, 0].any() and want[:, :, 1].any()
    _check(_run(fo, X, 2, [col], grid), want, chunks=1)


def test_multinomial_gbm():
    """3 classes x 3 iterations, depth 4, 300 rows, K = 3."""
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    df = _model_frame().iloc[:300].copy()
    df["y3"] = pd.qcut(df["y"], 3, labels=["lo", "mid", "hi"]).astype(str)
    fr = h2o.H2OFrame(df)
    m = H2OGradientBoostingEstimator(ntrees=3, max_depth=4, seed=1)
    m.train(x=list("abcd") + ["k"], y="y3", training_frame=fr)
    fo = m._forest
    assert len(fo) == 9 and sorted(set(fo.tclass)) == [0, 1, 2]
    X = m._score_matrix(fr)
    num = [-1.5, -0.3, 0.0, 0.4, 1.2, NAN]
    cat = [0, 1, 2, NAN]
    grid = _f32(*[[a for a in num for _ in cat], [b for _ in num for b in cat]])
    want = _oracle(fo, X, 3, [0, 4], grid)
    assert all(want[:, :, k].any() for k in range(3))
    _check(_run(fo, X, 3, [0, 4], grid), want)


@pytest.mark.parametrize("width", [64, 65])
def test_depth_cap(width):
    """A chain tree with 64 splits on its longest path runs on the kernel; with
    65 the torch implementation runs and the result says why."""
    assert pd_ops.MAX_DEPTH == 64
    fo = chain_forest(width, seed=4)
    F = width + 1
    g = torch.Generator().manual_seed(5)
    X = torch.randn(F, 70, generator=g)
    X[3, 0] = X[31, 1] = NAN
    X = X.cuda()
    assert pd_ops.max_depth(fo.pack(X.device)) == width
    cols = [0, 3, 30, width - 1]
    grid = torch.randn(4, 64, generator=g) - 1.0
    grid[1, 5] = NAN
    want = _oracle(fo, X, 1, cols, grid)
    res = _run(fo, X, 1, cols, grid)
    if width <= 64:
        _check(res, want, chunks=1)
    else:
        assert not res.kernel and "65 splits deep" in res.why
        torch.testing.assert_close(res.sums.cpu(), want, rtol=0, atol=0)


# ------------------------------------------------------------------ model level
def _tables_close(got, want, stats=("mean_response", "stddev_response")):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
        assert (b["stddev_response"] >= 1e-3).all()        # keeps svv/sw - mean^2's cancellation out of it
        for c in stats:
            np.testing.assert_allclose(a[c].values, b[c].values, rtol=RTOL, atol=ATOL)
        for c in a.columns[:-3]:
            assert [str(v) for v in a[c]] == [str(v) for v in b[c]]


@pytest.mark.parametrize("algo", ["gbm", "drf", "xgboost", "generic"])
def test_model_partial_dependence_matches_the_loop(algo, monkeypatch, tmp_path):
    import h2o3_amd as h2o
    from h2o3_amd.estimators import (H2OGradientBoostingEstimator, H2ORandomForestEstimator,
                                     H2OXGBoostEstimator)
    from h2o3_amd.models.explain import ice
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
        m = H2OGenericEstimator.from_file(m.download_mojo(str(tmp_path), format="h2o"))
    kw = dict(cols=["a", "k"], col_pairs_2dpdp=[["a", "k"]], include_na=True)

    def run():
        out = [m.partial_plot(fr, **kw)]
        why = [m._pd_why]
        out.append(m.h(fr, ["a", "b"]))
        why.append(m._pd_why)
        out.append(ice(m, fr, "a"))
        why.append(m._pd_why)
        return out, why
    monkeypatch.delenv("H2O3_TREE_PD", raising=False)
    (tabs, hval, curves), why = run()
    assert why == [None, None, None]
    monkeypatch.setenv("H2O3_TREE_PD", "torch")
    (want, want_h, want_curves), why = run()
    assert why == ["H2O3_TREE_PD=torch"] * 3
    assert [len(t) for t in tabs] == [21, 4, 84]
    _tables_close(tabs, want)
    np.testing.assert_allclose(hval, want_h, rtol=RTOL, atol=ATOL)
    assert list(curves["row"]) == list(want_curves["row"])
    np.testing.assert_allclose(curves["a"].values, want_curves["a"].values, rtol=0, atol=0)
    np.testing.assert_allclose(curves["response"].values, want_curves["response"].values, rtol=RTOL, atol=ATOL)
