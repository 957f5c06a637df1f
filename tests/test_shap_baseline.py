"""Baseline SHAP for GLM, Deep Learning and Stacked Ensembles
(predict_contributions with a background frame): the DeepSHAP torch rule on
random networks and against subset enumeration, the three estimators, the
argument errors, explain() and a 2-rank run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import h2o3_amd as h2o
from h2o3_amd.estimators import (H2ODeepLearningEstimator, H2OGeneralizedAdditiveEstimator,
                                 H2OGeneralizedLinearEstimator, H2ONaiveBayesEstimator)
from h2o3_amd.ops import dl_shap_ops
from shap_baseline_common import (X_COLS, dl_link_score, enumerate_fn, make_df, net_f, rand_net, rand_rows,
                                  train_dl, train_ensemble)

HERE = os.path.dirname(os.path.abspath(__file__))
ACTS = ["tanh", "rectifier", "exprectifier"]


# ------------------------------------------------------------ the torch rule
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("widths", [[7, 20, 9, 1], [5, 16, 1]])
def test_torch_rule_is_efficient_on_random_nets(widths, act):
    """f64: every pair's contributions sum to f(x) - f(z) (1e-9); the pair
    whose background row is a copy of the test row, and the input two rows
    share, get exactly 0; the averaged output is the per-reference mean."""
    net = rand_net(widths, act, [0.8, 1.0], seed=3)
    N, B, P = 17, 5, widths[0]
    X, Z = rand_rows(N, B, P, seed=4)
    per = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, per_reference=True, out_b=net[4])
    phi = per.phi.view(N, B, P + 1).numpy()
    fx, fz = net_f(net, X).numpy(), net_f(net, Z).numpy()
    err = np.abs(phi[:, :, :P].sum(2) - (fx[:, None] - fz[None, :])).max()
    print("efficiency error", err, "max |phi|", np.abs(phi[:, :, :P]).max())
    assert err < 1e-9
    np.testing.assert_allclose(phi[:, :, P], np.broadcast_to(fz, (N, B)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(per.fx.numpy(), fx, rtol=0, atol=1e-12)
    assert (phi[3, 2, :P] == 0).all()           # background row 2 is test row 3
    assert phi[0, 1, P - 1] == 0                # the shared input
    assert np.abs(phi[0, 1, :P - 1]).min() > 0
    avg = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, out_b=net[4])
    assert avg.phi.shape == (N, P + 1) and not avg.kernel
    np.testing.assert_allclose(avg.phi.numpy(), phi.mean(1), rtol=0, atol=1e-12)
    # the public entry point takes the torch rule for CPU tensors and says why
    res = dl_shap_ops.deep_shap(*net[:4], X, Z, out_b=net[4])
    assert not res.kernel and res.why == "CPU tensors"
    assert torch.equal(res.phi, avg.phi)
    # a pair factor scales each pair before averaging
    fac = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, out_b=net[4],
                                      pair_scale=lambda a, b: (a.view(-1, 1) * 0 + b.view(1, -1)))
    want = (phi[:, :, :P] * fz[None, :, None]).mean(1)
    np.testing.assert_allclose(fac.phi.numpy()[:, :P], want, rtol=0, atol=1e-12)
    # row chunking under a tiny budget changes nothing
    small = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, out_b=net[4], max_scratch_bytes=4096)
    np.testing.assert_allclose(small.phi.numpy(), avg.phi.numpy(), rtol=0, atol=1e-13)


@pytest.mark.parametrize("act", ACTS)
def test_torch_rule_equals_enumeration_on_an_additive_net(act):
    """Diagonal first layer (5 inputs): the net is additive in its inputs, for
    which the rescale rule is exact -- equal to the 2^F subset enumeration."""
    g = torch.Generator().manual_seed(11)
    W = torch.diag(torch.randn(5, generator=g, dtype=torch.float64) * 1.5)
    b = torch.randn(5, generator=g, dtype=torch.float64) * 0.5
    net = ([(W, b)], [act], [0.9], torch.randn(5, generator=g, dtype=torch.float64), -0.5)
    X, Z = rand_rows(6, 4, 5, seed=12)
    per = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, per_reference=True, out_b=net[4]).phi.view(6, 4, 6).numpy()
    f = lambda H: net_f(net, torch.as_tensor(H)).numpy()
    want = np.stack([[enumerate_fn(f, X[r].numpy(), Z[c].numpy()) for c in range(4)] for r in range(6)])
    err = np.abs(per - want).max()
    print("enumeration error", err)
    assert err < 1e-9


def test_maxout_keeps_efficiency():
    net = rand_net([4, 6, 1], None, [0.7], seed=5, maxout=True)
    assert net[0][0][0].shape == (12, 4)
    X, Z = rand_rows(17, 5, 4, seed=6)
    per = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, per_reference=True, out_b=net[4]).phi.view(17, 5, 5).numpy()
    fx, fz = net_f(net, X).numpy(), net_f(net, Z).numpy()
    err = np.abs(per[:, :, :4].sum(2) - (fx[:, None] - fz[None, :])).max()
    print("maxout efficiency error", err)
    assert err < 1e-9
    assert (per[3, 2, :4] == 0).all()
    res = dl_shap_ops.deep_shap(*net[:4], X, Z, out_b=net[4])
    assert not res.kernel


def test_kernel_plan():
    assert dl_shap_ops.dl_shap_fits([100, 200, 200, 1])
    assert dl_shap_ops.dl_shap_lds_bytes([100, 200, 200, 1]) == 4 * 16 * (116 + 116 + 212 + 212 + 2 * 212)
    assert not dl_shap_ops.dl_shap_fits([100, 2048, 1])
    assert not dl_shap_ops.dl_shap_fits([4] * 11 + [1])
    rt, bt = dl_shap_ops._plan(1000, 100, 50, 16, 1 << 30, False, False)
    assert (rt, bt) == (1008, 112)
    rt, bt = dl_shap_ops._plan(1000, 100, 50, 16, 64 * 1024, True, False)
    assert rt % 16 == 0 and bt % 16 == 0 and 4 * (bt // 16) * rt * 50 + 44 * rt * bt <= 64 * 1024
    with pytest.raises(ValueError):
        dl_shap_ops._plan(1000, 100, 50, 16, 100, False, False)
    with pytest.raises(ValueError):
        dl_shap_ops.deep_shap_torch([], [], [], torch.ones(3), torch.ones(2, 3), torch.ones(2, 3))
    net = rand_net([5, 16, 1], "tanh", [1.0], seed=1)
    with pytest.raises(ValueError, match="no rows"):
        dl_shap_ops.deep_shap(*net[:4], torch.ones(2, 5, dtype=torch.float64), torch.ones(0, 5, dtype=torch.float64))


# ------------------------------------------------------------ trained models
@pytest.fixture(scope="module")
def frames():
    h2o.init()
    return h2o.H2OFrame(make_df()), h2o.H2OFrame(make_df(9, seed=5)), h2o.H2OFrame(make_df(12, seed=8))


def _cols(df, names):
    return df[list(names)].values.astype(np.float64)


@pytest.mark.parametrize("family", ["gaussian", "binomial"])
def test_glm(frames, family):
    fr, bg, te = frames
    m = H2OGeneralizedLinearEstimator(family=family, lambda_=1e-3, alpha=0.5, seed=1)
    m.train(x=X_COLS, y="yb" if family == "binomial" else "y", training_frame=fr)
    di = m._dinfo
    N, B, P = te.nrows, bg.nrows, di.P
    names = list(di.coef_names)
    assert sum(n.startswith("k.") for n in names) == 2 and P == 6
    beta = np.asarray(m._beta_std[:-1], dtype=np.float64)[:P]
    icpt = float(m._beta_std[-1])
    Xd = di.expand(te, pad=False)[0].double().numpy()
    Zd = di.expand(bg, pad=False)[0].double().numpy()
    per = m.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    assert list(per.columns) == names + ["BiasTerm", "RowIdx", "BackgroundRowIdx"]
    assert per["RowIdx"].tolist() == [r for r in range(N) for _ in range(B)]
    assert per["BackgroundRowIdx"].tolist() == list(range(B)) * N
    got = _cols(per, names + ["BiasTerm"]).reshape(N, B, P + 1)
    eta = lambda H: H @ beta + icpt
    want = np.stack([[enumerate_fn(eta, Xd[r], Zd[c]) for c in range(B)] for r in range(N)])
    scale = np.abs(want[:, :, :P]).max()
    assert np.abs(got - want).max() <= 1e-5 * max(scale, np.abs(want[:, :, P]).max())
    ex, ez = m._predict_link(te).numpy(), m._predict_link(bg).numpy()
    np.testing.assert_allclose(got[:, :, :P].sum(2), ex[:, None] - ez[None, :], rtol=0, atol=1e-5 * max(scale, 1))
    np.testing.assert_allclose(got[:, :, P], np.broadcast_to(ez, (N, B)), rtol=0, atol=1e-5 * max(scale, 1))
    avg = m.predict_contributions(te, background_frame=bg).as_data_frame()
    assert list(avg.columns) == names + ["BiasTerm"]
    np.testing.assert_allclose(_cols(avg, names + ["BiasTerm"]), got.mean(1), rtol=0, atol=1e-5 * max(scale, 1))
    # Compact: the categorical's one-hot group summed
    comp = m.predict_contributions(te, background_frame=bg, output_format="Compact").as_data_frame()
    assert list(comp.columns) == ["k", "a", "b", "c", "d", "BiasTerm"]
    np.testing.assert_allclose(comp["k"].values, avg[[n for n in names if n.startswith("k.")]].values.sum(1),
                               rtol=0, atol=1e-5 * max(scale, 1))
    np.testing.assert_allclose(_cols(comp, "abcd"), _cols(avg, "abcd"), rtol=0, atol=0)
    # output space: rows sum to mu(x) - mu(z), the bias term is mu(z)
    pr = m.predict(te).as_data_frame()
    pb = m.predict(bg).as_data_frame()
    mx = (pr["p"] if family == "binomial" else pr["predict"]).values.astype(np.float64)
    mz = (pb["p"] if family == "binomial" else pb["predict"]).values.astype(np.float64)
    out = m.predict_contributions(te, background_frame=bg, output_space=True, output_per_reference=True)
    o = _cols(out.as_data_frame(), names + ["BiasTerm"]).reshape(N, B, P + 1)
    np.testing.assert_allclose(o[:, :, :P].sum(2), mx[:, None] - mz[None, :], rtol=0, atol=1e-5 * max(scale, 1))
    np.testing.assert_allclose(o[:, :, P], np.broadcast_to(mz, (N, B)), rtol=0, atol=1e-5 * max(scale, 1))
    oa = _cols(m.predict_contributions(te, background_frame=bg, output_space=True).as_data_frame(),
               names + ["BiasTerm"])
    np.testing.assert_allclose(oa, o.mean(1), rtol=0, atol=1e-5 * max(scale, 1))


@pytest.fixture(scope="module")
def dl_models(frames):
    fr, _, _ = frames
    return {"binomial": train_dl(fr, "yb"), "gaussian": train_dl(fr, "y")}


@pytest.mark.parametrize("kind", ["binomial", "gaussian"])
def test_trained_deep_learning(frames, dl_models, kind):
    """Row sums + bias term reproduce the link-space score and, with
    output_space, the predict output.  The pair stage runs in f32 here (the
    design matrix's dtype): about 30 roundings of 6e-8 on values up to the
    score's scale, bounded by 2e-5 x that scale with a 10x margin."""
    fr, bg, te = frames
    m = dl_models[kind]
    names = list(m._dinfo.coef_names)
    assert len(names) == 7 and [L.drop for L in m._layers[:-1]] == [0.2, 0.1]
    N, B, P = te.nrows, bg.nrows, len(names)
    fx, fz = dl_link_score(m, te), dl_link_score(m, bg)
    tol = 2e-5 * max(1.0, np.abs(fx).max(), np.abs(fz).max())
    per = m.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    assert list(per.columns) == names + ["BiasTerm", "RowIdx", "BackgroundRowIdx"]
    got = _cols(per, names + ["BiasTerm"]).reshape(N, B, P + 1)
    assert np.abs(got[:, :, :P]).max() > 0.05
    np.testing.assert_allclose(got[:, :, :P].sum(2), fx[:, None] - fz[None, :], rtol=0, atol=tol)
    np.testing.assert_allclose(got[:, :, P], np.broadcast_to(fz, (N, B)), rtol=0, atol=tol)
    avg = m.predict_contributions(te, background_frame=bg).as_data_frame()
    np.testing.assert_allclose(_cols(avg, names + ["BiasTerm"]), got.mean(1), rtol=0, atol=tol)
    assert not m._last_shap.kernel and m._last_shap.why == "CPU tensors"
    comp = m.predict_contributions(te, background_frame=bg, output_format="Compact").as_data_frame()
    assert list(comp.columns) == ["k", "a", "b", "c", "d", "BiasTerm"]
    np.testing.assert_allclose(comp["k"].values, avg[["k.u", "k.v", "k.w"]].values.sum(1), rtol=0, atol=tol)
    pr, pb = m.predict(te).as_data_frame(), m.predict(bg).as_data_frame()
    col = "p" if kind == "binomial" else "predict"
    mx, mz = pr[col].values.astype(np.float64), pb[col].values.astype(np.float64)
    out = m.predict_contributions(te, background_frame=bg, output_space=True).as_data_frame()
    np.testing.assert_allclose(_cols(out, names).sum(1) + out["BiasTerm"].values, mx, rtol=0, atol=tol)
    np.testing.assert_allclose(out["BiasTerm"].values, mz.mean(), rtol=0, atol=tol)
    # sorted output is the full output, sorted
    top = m.predict_contributions(te, background_frame=bg, top_n=2, bottom_n=1).as_data_frame()
    assert list(top.columns) == ["top_feature_1", "top_value_1", "top_feature_2", "top_value_2",
                                 "bottom_feature_1", "bottom_value_1", "BiasTerm"]
    c = avg[names].values
    order = np.argsort(-c, axis=1)
    np.testing.assert_array_equal(top["top_value_1"].values, c[np.arange(N), order[:, 0]])
    np.testing.assert_array_equal(top["top_value_2"].values, c[np.arange(N), order[:, 1]])
    np.testing.assert_array_equal(top["bottom_value_1"].values, c[np.arange(N), order[:, -1]])
    assert top["top_feature_1"].tolist() == [names[j] for j in order[:, 0]]
    np.testing.assert_array_equal(top["BiasTerm"].values, avg["BiasTerm"].values)
    ab = m.predict_contributions(te, background_frame=bg, top_n=1, compare_abs=True).as_data_frame()
    np.testing.assert_array_equal(np.abs(ab["top_value_1"].values), np.abs(c).max(1))


def _naive_bayes(fr, y, kw):
    nb = H2ONaiveBayesEstimator(**kw)
    nb.train(x=X_COLS, y=y, training_frame=fr)
    return nb


@pytest.mark.parametrize("transform", ["NONE", "Logit"])
def test_stacked_ensemble(frames, transform):
    """GBM + GLM (no `d`) + DL (no `a`) under a GLM metalearner: per pair the
    contributions sum to eta(x) - eta(z) of the metalearner.  The base models'
    f32 predictions and the f32 level-one columns bound the agreement: 1e-4 of
    the score's scale (the logit transform divides a probability's 6e-8
    rounding by p (1 - p) >= 1e-3 here)."""
    fr, bg, te = frames
    se = train_ensemble(fr, "yb", transform)
    N, B, F = te.nrows, bg.nrows, len(X_COLS)
    lv = lambda f: h2o.H2OFrame.from_vecs(*se._level_one(se._base, f, use_cv=False))
    ex, ez = se._meta._predict_link(lv(te)).numpy(), se._meta._predict_link(lv(bg)).numpy()
    assert np.abs(ex[:, None] - ez[None, :]).max() > 0.1
    tol = 1e-4 * max(1.0, np.abs(ex).max(), np.abs(ez).max())
    per = se.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    assert list(per.columns) == X_COLS + ["BiasTerm", "RowIdx", "BackgroundRowIdx"]
    got = _cols(per, X_COLS + ["BiasTerm"]).reshape(N, B, F + 1)
    np.testing.assert_allclose(got[:, :, :F].sum(2), ex[:, None] - ez[None, :], rtol=0, atol=tol)
    np.testing.assert_allclose(got[:, :, F], np.broadcast_to(ez, (N, B)), rtol=0, atol=tol)
    for fmt in ("Original", "Compact"):
        avg = se.predict_contributions(te, background_frame=bg, output_format=fmt).as_data_frame()
        assert list(avg.columns) == X_COLS + ["BiasTerm"]
        np.testing.assert_allclose(_cols(avg, X_COLS + ["BiasTerm"]), got.mean(1), rtol=0, atol=tol)
    p1 = se.predict(te).as_data_frame()["p"].values.astype(np.float64)
    out = se.predict_contributions(te, background_frame=bg, output_space=True).as_data_frame()
    np.testing.assert_allclose(_cols(out, X_COLS).sum(1) + out["BiasTerm"].values, p1, rtol=0, atol=tol)
    # a tiny budget tiles the test rows and changes nothing beyond rounding
    from h2o3_amd.models.shap_baseline import se_contributions
    tiled = se_contributions(se, te, background_frame=bg, output_per_reference=True,
                             max_scratch_bytes=8 * 1024).as_data_frame()
    np.testing.assert_allclose(_cols(tiled, X_COLS + ["BiasTerm"]).reshape(N, B, F + 1), got, rtol=0, atol=1e-6)


def test_stacked_ensemble_regression_and_refusals(frames):
    fr, bg, te = frames
    se = train_ensemble(fr, "y")
    lv = lambda f: h2o.H2OFrame.from_vecs(*se._level_one(se._base, f, use_cv=False))
    ex, ez = se._meta._predict_link(lv(te)).numpy(), se._meta._predict_link(lv(bg)).numpy()
    tol = 1e-4 * max(1.0, np.abs(ex).max())
    avg = se.predict_contributions(te, background_frame=bg).as_data_frame()
    np.testing.assert_allclose(_cols(avg, X_COLS).sum(1) + avg["BiasTerm"].values, ex, rtol=0, atol=tol)
    np.testing.assert_allclose(avg["BiasTerm"].values, ez.mean(), rtol=0, atol=tol)
    with pytest.raises(ValueError, match="requires a background_frame"):
        se.predict_contributions(te)
    with pytest.raises(ValueError, match="no rows"):
        se.predict_contributions(te, background_frame=bg[[], :])
    nb_se = train_ensemble(fr, "yb", extra_base=[_naive_bayes])
    with pytest.raises(ValueError, match="naivebayes"):
        nb_se.predict_contributions(te, background_frame=bg)
    from h2o3_amd.estimators import H2OStackedEnsembleEstimator
    gbm_meta = H2OStackedEnsembleEstimator(base_models=se._base, metalearner_algorithm="gbm")
    gbm_meta.train(x=X_COLS, y="y", training_frame=fr)
    with pytest.raises(ValueError, match="gbm"):
        gbm_meta.predict_contributions(te, background_frame=bg)


def test_argument_errors(frames, dl_models):
    fr, bg, te = frames
    glm = H2OGeneralizedLinearEstimator(family="gaussian")
    glm.train(x=X_COLS, y="y", training_frame=fr)
    dl = dl_models["gaussian"]
    for m in (glm, dl):
        with pytest.raises(ValueError, match="requires a background_frame"):
            m.predict_contributions(te)
        with pytest.raises(ValueError, match="no rows"):
            m.predict_contributions(te, background_frame=bg[[], :])
        with pytest.raises(ValueError, match="output_format"):
            m.predict_contributions(te, background_frame=bg, output_format="Wide")
    multi = "Calculating contributions is currently not supported for multinomial models."
    m = H2OGeneralizedLinearEstimator(family="multinomial")
    m.train(x=list("abcd"), y="k", training_frame=fr)
    with pytest.raises(ValueError, match=multi):
        m.predict_contributions(te, background_frame=bg)
    m = H2ODeepLearningEstimator(hidden=[4], epochs=1, seed=1)
    m.train(x=list("abcd"), y="k", training_frame=fr)
    with pytest.raises(ValueError, match=multi):
        m.predict_contributions(te, background_frame=bg)
    m = H2ODeepLearningEstimator(hidden=[3], epochs=1, seed=1, autoencoder=True)
    m.train(x=X_COLS, training_frame=fr)
    with pytest.raises(ValueError, match="autoencoder"):
        m.predict_contributions(te, background_frame=bg)
    m = H2ODeepLearningEstimator(hidden=[4], epochs=1, seed=1, max_categorical_features=2)
    m.train(x=X_COLS, y="y", training_frame=fr)
    with pytest.raises(ValueError, match="max_categorical_features"):
        m.predict_contributions(te, background_frame=bg)
    for est in (H2OGeneralizedLinearEstimator(family="gaussian"), H2ODeepLearningEstimator(hidden=[4], epochs=1)):
        est.train(x=list("abc"), y="y", offset_column="d", training_frame=fr)
        with pytest.raises(ValueError, match="offset_column"):
            est.predict_contributions(te, background_frame=bg)
    gam = H2OGeneralizedAdditiveEstimator(family="gaussian", gam_columns=["a"])
    gam.train(x=["b", "c"], y="y", training_frame=fr)
    with pytest.raises(ValueError, match="GAM"):
        gam.predict_contributions(te, background_frame=bg)
    hg = H2OGeneralizedLinearEstimator(HGLM=True, family="gaussian", random_columns=[4], rand_family=["gaussian"])
    hg.train(x=X_COLS, y="y", training_frame=fr)
    with pytest.raises(ValueError, match="HGLM"):
        hg.predict_contributions(te, background_frame=bg)


def test_explain_takes_a_background_frame(frames):
    fr, bg, te = frames
    m = H2OGeneralizedLinearEstimator(family="gaussian")
    m.train(x=X_COLS, y="y", training_frame=fr)
    from h2o3_amd.models.explain import explain, explain_row
    assert "shap_summary" not in explain(m, te, include_explanations=["shap_summary"])
    out = explain(m, te, include_explanations=["shap_summary"], background_frame=bg)
    want = m.predict_contributions(te, background_frame=bg).as_data_frame()
    assert out["shap_summary"].equals(want)
    row = explain_row(m, te, 2, columns=["a"], background_frame=bg)
    np.testing.assert_array_equal(row["shap_explain_row"].values[0], want.values[2])
    assert "shap_explain_row" not in explain_row(m, te, 2, columns=["a"])
    # tree models: the keyword reaches predict_contributions instead of being dropped
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    g = H2OGradientBoostingEstimator(ntrees=3, max_depth=3, seed=1)
    g.train(x=X_COLS, y="y", training_frame=fr)
    out = explain(g, te, include_explanations=["shap_summary"], background_frame=bg)
    assert out["shap_summary"].equals(g.predict_contributions(te, background_frame=bg).as_data_frame())


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "shap_baseline_worker.py"), out], env=env,
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
    """Test and background frame row-sharded over 2 gloo ranks; the model's
    weights are set, not trained, so both runs explain the same model."""
    one = _run_ranks(1, str(tmp_path / "w1.json"))
    two = _run_ranks(2, str(tmp_path / "w2.json"))
    assert two["bg_local_rows"] < one["bg_local_rows"] == 10
    for k in ("glm_avg", "glm_per_ref", "dl_avg", "dl_per_ref"):
        a, b = np.asarray(one[k]), np.asarray(two[k])
        assert a.shape == b.shape and np.abs(a[:, :-1]).max() > 0
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-6)
    assert one["cols"] == two["cols"]
