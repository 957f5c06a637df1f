"""forest_predict_kernel (ops/csrc/tree_predict.hip, through Forest.predict)
against forest_predict_common.oracle, a per-row walk over the Tree lists that
never reads Forest.pack(): exact (rtol = atol = 0), since the kernel only adds
f32 leaf values in tree order and the oracle does the same adds.  The case
table is the one test_forest_predict.py runs on the CPU twin; here it also
runs from fresh device packs, on prefixes and ranges of the forest, on other
input layouts, on trained models, and in child processes with 1 and 4 trees
walked together per thread (every other test runs the default of 2)."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from forest_predict_common import (CASE_NAMES, WORKER_CASE_NAMES, as_f32, leaf_sums, oracle, reference, same_trees)

# 1e300 overflows to +inf in pack()'s f32 cast, as the edge forest means it to
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast:RuntimeWarning")]

NAN, INF = float("nan"), float("inf")
LAYOUT_CASES = ["edge_n777", "lane_T5_n255", "class_K4_shuffled_n255"]


def _dev(X):
    return torch.tensor(np.asarray(X), device="cuda")


def _exact(got, want):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    torch.testing.assert_close(got.cpu(), torch.from_numpy(want.copy()), rtol=0, atol=0)


def _same_leaf(got, want):
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want.copy()))


def _check(fo, Xd, K, orc):
    _exact(fo.predict(Xd, K), orc.sums)
    _same_leaf(fo.predict(Xd, K, leaf=True), orc.leaf)


def _rows(orc, a, b):
    """Rows [a, b) of an oracle result (every row is scored on its own)."""
    return orc._replace(sums=orc.sums[a:b], leaf=orc.leaf[a:b], sums64=orc.sums64[a:b])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_matches_oracle(name):
    fo, X, K, orc = reference(name)
    assert orc.sums.shape == (X.shape[1], K) and orc.leaf.shape == (X.shape[1], len(fo))
    _check(fo, _dev(X), K, orc)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_matches_oracle_from_fresh_pack(name):
    fo, X, K, orc = reference(name)
    fresh = same_trees(fo)
    assert fresh._packed is None
    _check(fresh, _dev(X), K, orc)
    assert fresh._packed[0][0].startswith("cuda")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_upto_and_predict_range_match_oracle(name):
    fo, X, K, orc = reference(name)
    Xd = _dev(X)
    T = len(fo)
    for u in range(T + 1):
        _exact(fo.predict(Xd, K, upto=u), leaf_sums(fo, orc.leaf, K, 0, u)[0])
        _same_leaf(fo.predict(Xd, K, upto=u, leaf=True), orc.leaf[:, :u])
    for a, b in {(0, T), (0, 0), (T, T), (0, T // 2), (T // 2, T), (1, T), (T - 1, T)}:
        if 0 <= a <= b:
            _exact(fo.predict_range(Xd, K, a, b), leaf_sums(fo, orc.leaf, K, a, b)[0])
    _exact(fo.predict(Xd, K), orc.sums)


@pytest.mark.parametrize("name", LAYOUT_CASES + ["class_K2_alt_n777"])
def test_no_rows(name):
    fo, X, K, _ = reference(name)
    Xd = torch.zeros((X.shape[0], 0), dtype=torch.float32, device="cuda")
    out = fo.predict(Xd, K)
    assert out.shape == (0, K) and out.dtype == torch.float32
    leaf = fo.predict(Xd, K, leaf=True)
    assert leaf.shape == (0, len(fo)) and leaf.dtype == torch.int32
    assert fo.predict(Xd, K, upto=0).shape == (0, K)


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_input_layouts(name):
    """X as a transposed view, as every second column of a wider tensor, as
    float64, and with two more feature rows no tree reads."""
    fo, X, K, orc = reference(name)
    Xd = _dev(X)
    F, N = Xd.shape
    view = Xd.t().contiguous().t()
    assert not view.is_contiguous() or N == 1
    _check(fo, view, K, orc)
    wide = torch.full((F, 2 * N), NAN, device="cuda")
    wide[:, ::2] = Xd
    assert not wide[:, ::2].is_contiguous() or N == 1
    _check(fo, wide[:, ::2], K, orc)
    _check(fo, Xd.double(), K, orc)
    _check(fo, torch.cat([Xd, torch.full((2, N), NAN, device="cuda")]), K, orc)


@pytest.mark.parametrize("name", ["edge_n777", "class_K3_gap_n777", "lane_T7_n777"])
def test_column_windows_of_a_larger_matrix(name):
    """257 rows (one thread past a full block) scored as a window of the
    777-row matrix and as a copy of just those columns; the kernel reads
    X[f * N + r], so a window that does not start at column 0 must be read
    with its own N."""
    fo, X, K, orc = reference(name)
    Xd = _dev(X)
    head = _rows(orc, 0, 257)
    a, b = fo.predict(Xd[:, :257], K), fo.predict(Xd[:, :257].clone(), K)
    assert torch.equal(a, b)
    _exact(a, head.sums)
    _same_leaf(fo.predict(Xd[:, :257], K, leaf=True), head.leaf)
    _check(fo, Xd[:, 256:513].contiguous(), K, _rows(orc, 256, 513))


# ------------------------------------------------------------------ trained models
@pytest.fixture(scope="module")
def frame():
    """The frame of test_pd_gpu.py's gbm_case (1500 rows, numeric columns with
    NAs, a 7-level categorical with NAs and a 3-level one) with a numeric, a
    3-class and a 2-class response."""
    import h2o3_amd as h2o
    rng = np.random.default_rng(11)
    n = 1500
    A = rng.normal(size=(n, 5))
    A[rng.random(n) < 0.06, 1] = np.nan
    A[rng.random(n) < 0.03, 3] = np.nan
    df = pd.DataFrame(A, columns=[f"x{i}" for i in range(5)])
    df["c1"] = rng.choice(list("abcdefg"), n)
    df["c2"] = rng.choice(["u", "v", "w"], n)
    df.loc[rng.random(n) < 0.05, "c1"] = None
    df.loc[rng.random(n) < 0.04, "c2"] = None
    y = (A[:, 0] + np.nan_to_num(A[:, 1]) * (df["c2"] == "u") - 0.7 * (df["c1"].isin(["a", "d"])) +
         0.5 * A[:, 2] * np.nan_to_num(A[:, 3]) + rng.normal(scale=0.2, size=n))
    df["y"] = y
    df["y3"] = np.where(y > 0.6, "hi", np.where(y > -0.4, "mid", "lo"))
    df["y2"] = np.where(y > 0.1, "p", "q")
    return h2o.H2OFrame(df), [f"x{i}" for i in range(5)] + ["c1", "c2"]


def _train(kind, fr, x):
    from h2o3_amd.estimators import (H2OGradientBoostingEstimator, H2OIsolationForestEstimator,
                                     H2ORandomForestEstimator, H2OXGBoostEstimator)
    if kind == "gbm_regression":
        m, y, K, T = H2OGradientBoostingEstimator(ntrees=10, max_depth=5, seed=1, min_rows=5), "y", 1, 10
    elif kind == "gbm_multinomial":
        m, y, K, T = H2OGradientBoostingEstimator(ntrees=3, max_depth=4, seed=1), "y3", 3, 9
    elif kind == "drf_double_trees":
        m = H2ORandomForestEstimator(ntrees=4, max_depth=12, min_rows=1, seed=1, binomial_double_trees=True)
        y, K, T = "y2", 2, 8
    elif kind == "xgboost":
        m, y, K, T = H2OXGBoostEstimator(ntrees=4, max_depth=4, seed=1), "y", 1, 4
    else:
        m, y, K, T = H2OIsolationForestEstimator(ntrees=5, seed=1), None, 1, 5
    if y is None:
        m.train(x=x, training_frame=fr)
    else:
        m.train(x=x, y=y, training_frame=fr)
    assert m._n_tree_classes() == K and len(m._forest) == T
    return m, K


@pytest.mark.parametrize("kind", ["gbm_regression", "gbm_multinomial", "drf_double_trees", "xgboost", "isofor"])
def test_trained_model_matches_tree_lists(kind, frame):
    """The forest a model trained, scored by the kernel, against the oracle on
    the model's own Tree lists: the first 600 rows of its score matrix, with
    NaN, +-inf and out-of-range level codes written in and 50 of the forest's
    thresholds (every numeric root's first) planted exactly into their
    feature's row: trained splits sit at bin edges that are often data values,
    where x < thr and x <= thr part ways."""
    fr, x = frame
    m, K = _train(kind, fr, x)
    fo = m._forest
    M = m._score_matrix(fr)
    assert M.is_cuda and M.shape == (len(x), 1500)
    X = M[:, :600].clone()
    X[5, 0], X[5, 1], X[5, 2], X[5, 3], X[5, 4], X[5, 5] = NAN, 7.0, 10.0, -1.0, INF, -INF
    X[6, 6], X[6, 7], X[6, 8], X[6, 9] = 3.0, 6.0, -1.0, NAN
    X[0, 10], X[0, 11], X[0, 12], X[1, 13] = NAN, INF, -INF, INF
    rng = np.random.default_rng(5)
    def numeric(t, i):
        return t.left[i] >= 0 and not (t.is_cat[i] and t.cat_left[i] is not None)
    cuts = [(int(t.feat[i]), as_f32(t.thr[i])) for t in fo.trees for i in range(1, t.n_nodes) if numeric(t, i)]
    roots = [(int(t.feat[0]), as_f32(t.thr[0])) for t in fo.trees if numeric(t, 0)]
    rest = [cuts[j] for j in rng.permutation(len(cuts))]
    assert roots and rest
    plant = [(roots + rest)[j % len(roots + rest)] for j in range(50)]     # a small forest has fewer: plant them twice
    for (f, v), r in zip(plant, 20 + rng.permutation(580)[:50]):
        X[f, int(r)] = v
    orc = oracle(fo, X.cpu().numpy(), K)
    assert orc.record["num_equal"] > 0 and orc.record["num_nan_left"] + orc.record["num_nan_right"] > 0
    if kind != "isofor":                                   # isolation trees split numerically on the level code
        assert orc.record["cat_bit1"] > 0 and orc.record["cat_eq_len"] + orc.record["cat_gt_len"] > 0
    _check(fo, X, K, orc)


# ------------------------------------------------------------------ TW = 1 and TW = 4
def test_one_and_four_trees_per_thread(tmp_path):
    """H2O3_PREDICT_TW is read once per process: forest_predict_worker.py
    scores the lane, class and edge cases in a fresh child for TW = 1 and
    then for TW = 4.  A child that fails ends the test; no further child is
    started."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "forest_predict_worker.py")
    for tw in ("1", "4"):
        path = str(tmp_path / f"tw{tw}.npz")
        try:
            r = subprocess.run([sys.executable, worker, path], env={**os.environ, "H2O3_PREDICT_TW": tw},
                               timeout=120, capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"TW={tw}: worker killed after {e.timeout} s\n{e.stdout}\n{e.stderr}")
        if r.returncode != 0:
            pytest.fail(f"TW={tw}: worker exit status {r.returncode}\n{r.stdout}\n{r.stderr}")
        got = np.load(path)
        for name in WORKER_CASE_NAMES:
            orc = reference(name).oracle
            sums, leaf = got[name + "/sums"], got[name + "/leaf"]
            assert sums.dtype == np.float32 and sums.shape == orc.sums.shape, (tw, name)
            assert leaf.dtype == np.int32 and np.array_equal(leaf, orc.leaf), (tw, name)
            np.testing.assert_allclose(sums, orc.sums, rtol=0, atol=0, err_msg=f"TW={tw} {name}")
