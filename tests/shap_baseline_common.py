"""Shared pieces of the GLM / Deep Learning / Stacked Ensemble baseline-SHAP
tests (test_shap_baseline*.py): random networks, an independent f64 forward,
the 2^F subset-enumeration oracle of any scalar function, the trained models."""
import itertools
import math

import numpy as np
import pandas as pd
import torch

X_COLS = list("abcd") + ["k"]


# ------------------------------------------------------------------ networks
def rand_net(widths, act, scales, seed, dtype=torch.float64, maxout=False):
    """(layers, acts, scales, out_w, out_b) of a random net with
    widths = [inputs, hidden ..., 1]."""
    g = torch.Generator().manual_seed(seed)
    k = 2 if maxout else 1
    layers = []
    for fin, fout in zip(widths[:-2], widths[1:-1]):
        W = torch.randn((fout * k, fin), generator=g, dtype=torch.float64) * (1.5 / math.sqrt(fin))
        b = torch.randn(fout * k, generator=g, dtype=torch.float64) * 0.5
        layers.append((W.to(dtype), b.to(dtype)))
    out_w = torch.randn(widths[-2], generator=g, dtype=torch.float64).to(dtype)
    nl = len(layers)
    return layers, ["maxout" if maxout else act] * nl, list(scales)[:nl], out_w, 0.25


def rand_rows(N, B, P, seed, dtype=torch.float64):
    """X [N, P] and Z [B, P].  With B >= 3 and N >= 4: background row 2 is a
    copy of test row 3, and background row 1 shares input P-1 with test row 0."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((N, P), generator=g, dtype=torch.float64)
    Z = torch.randn((B, P), generator=g, dtype=torch.float64)
    if B >= 3 and N >= 4:
        Z[2] = X[3]
        Z[1, P - 1] = X[0, P - 1]
    return X.to(dtype), Z.to(dtype)


def net_f(net, X):
    """f of every row of X in f64, written out independently of dl_ops."""
    layers, acts, scales, out_w, out_b = net
    A = X.to(torch.float64)
    for (W, b), act, s in zip(layers, acts, scales):
        a = A @ W.to(torch.float64).t() + b.to(torch.float64)
        if act == "maxout":
            h = a.view(a.shape[0], -1, 2).max(2).values
        elif act == "tanh":
            h = torch.tanh(a)
        elif act == "rectifier":
            h = a.clamp_min(0)
        else:
            h = torch.where(a > 0, a, torch.expm1(a))
        A = h * s
    return A @ out_w.to(torch.float64) + out_b


def enumerate_fn(f, x, z):
    """Exact Shapley values of the game v(S) = f(x on S, z elsewhere) for a
    function f of a [rows, F] f64 array: [F+1], last entry f(z)."""
    F = len(x)
    subsets = [S for k in range(F + 1) for S in itertools.combinations(range(F), k)]
    H = np.tile(np.asarray(z, dtype=np.float64), (len(subsets), 1))
    for r, S in enumerate(subsets):
        H[r, list(S)] = np.asarray(x, dtype=np.float64)[list(S)]
    v = dict(zip(map(frozenset, subsets), np.asarray(f(H), dtype=np.float64)))
    phi = np.zeros(F + 1)
    for i in range(F):
        others = [j for j in range(F) if j != i]
        for k in range(F):
            w = math.factorial(k) * math.factorial(F - k - 1) / math.factorial(F)
            for S in itertools.combinations(others, k):
                s = frozenset(S)
                phi[i] += w * (v[s | {i}] - v[s])
    phi[F] = v[frozenset()]
    return phi


# ------------------------------------------------------------------ frames and models
def make_df(n=300, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 4))
    X[rng.random(n) < 0.05, 2] = np.nan
    df = pd.DataFrame(X, columns=list("abcd"))
    df["k"] = rng.choice(["u", "v", "w"], n)
    df["y"] = 2 * X[:, 0] - X[:, 1] * (df["k"] == "u") + np.nan_to_num(X[:, 2]) + rng.normal(scale=0.2, size=n)
    df["yb"] = np.where(df["y"] > 0, "p", "n")
    return df


def train_dl(fr, y, x=None, **kw):
    from h2o3_amd.estimators import H2ODeepLearningEstimator
    p = dict(hidden=[8, 5], activation="RectifierWithDropout", hidden_dropout_ratios=[0.2, 0.1], epochs=5, seed=7,
             reproducible=True)
    p.update(kw)
    m = H2ODeepLearningEstimator(**p)
    m.train(x=x or X_COLS, y=y, training_frame=fr)
    return m


def train_ensemble(fr, y, transform="NONE", extra_base=()):
    """GBM on every feature, GLM without `d`, DL without `a`: features absent
    from single base models."""
    from h2o3_amd.estimators import (H2OGeneralizedLinearEstimator, H2OGradientBoostingEstimator,
                                     H2OStackedEnsembleEstimator)
    kw = dict(nfolds=2, fold_assignment="Modulo", keep_cross_validation_predictions=True, seed=1)
    g = H2OGradientBoostingEstimator(ntrees=4, max_depth=3, **kw)
    g.train(x=X_COLS, y=y, training_frame=fr)
    l = H2OGeneralizedLinearEstimator(family="binomial" if y == "yb" else "gaussian", **kw)
    l.train(x=["a", "b", "c", "k"], y=y, training_frame=fr)
    d = train_dl(fr, y, x=["b", "c", "d", "k"], epochs=3, **{k: v for k, v in kw.items() if k != "seed"})
    base = [g, l, d] + [b(fr, y, kw) for b in extra_base]
    se = H2OStackedEnsembleEstimator(base_models=base, metalearner_transform=transform,
                                     metalearner_algorithm="glm")
    se.train(x=X_COLS, y=y, training_frame=fr)
    return se


def dl_link_score(m, fr):
    """The explained scalar of a DL model for every row of fr, from the
    model's own scoring forward (f64 array)."""
    X, _ = m._design(fr)
    with torch.no_grad():
        _, zs = m._forward(X, False)
    Lo = m._layers[-1]
    zo = (zs[-1] + Lo.b.view(1, -1)).double().cpu().numpy()
    if m._K == 2:
        return zo[:, 1] - zo[:, 0]
    return zo[:, 0] * m._ysd + m._ymu
