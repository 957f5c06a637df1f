"""The fused multinomial GLM pass (ops/csrc/glm_multi.hip, reached through
linalg_ops.glm_multinomial_pass and fit_multinomial) against plain torch fp64
on the same f32-rounded X, B, b0 and w.

Bounds (fixed beforehand, not fitted to the kernel): 1e-6 on each of
  |gB - ref|.max() / (max_j sum_i |x_ij| * max w)   (GRAD_BOUND of test_glm_oracle_gpu, |r| <= w),
  |gb - ref|.max() / sum w,    |loss - ref| / ref.
The kernel rounds like f32 eta, f32 softmax, f32 sums over one 64-row chunk
and f64 beyond (a CPU emulation of that arithmetic: 2e-9 to 1.4e-8); one
mishandled row of 8269 moves a figure by about 1.2e-4.  Each test prints the
figures it measured (ERR lines) before it asserts.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd
from h2o3_amd.estimators import H2OGeneralizedLinearEstimator
from h2o3_amd.ops import linalg_ops

pytestmark = pytest.mark.gpu

BOUND = 1e-6
DEV_BOUND = 1e-4


@functools.lru_cache(maxsize=None)
def _case(n, P, Pp, K, scale=1.0):
    """Inputs on the device and figures(out, "w" | "none"): the three errors of
    a pass's (loss, gB, gb) against the fp64 reference with w or with w = None."""
    g = torch.Generator().manual_seed(1000 * n + 10 * Pp + K)
    X = torch.zeros(n, Pp)
    X[:, :P] = torch.randn(n, P, generator=g)
    B = torch.zeros(Pp, K, dtype=torch.float64)
    B[:P] = torch.randn(P, K, generator=g, dtype=torch.float64) * (2 * scale / P ** 0.5)
    b0 = torch.randn(K, generator=g, dtype=torch.float64)
    y = torch.randint(0, K, (n,), generator=g, dtype=torch.int32)
    w = torch.rand(n, generator=g) * 2
    i = torch.arange(n)
    w[i % 7 == 6] = 0
    y[i % 21 == 6] = -1
    X, B, b0, y, w = (t.cuda() for t in (X, B, b0, y, w))
    Xd = X.double()
    eta = Xd @ B.float().double() + b0.float().double()
    live = (y >= 0).double()
    onehot = torch.nn.functional.one_hot(y.clamp(min=0).long(), K).double()
    refs = {}
    for key, wd in (("w", w.double() * live), ("none", live)):
        R = wd.view(-1, 1) * (torch.softmax(eta, 1) - onehot)
        loss = (wd * (torch.logsumexp(eta, 1) - (eta * onehot).sum(1))).sum()
        refs[key] = (loss, Xd.T @ R, R.sum(0), float(Xd.abs().sum(0).max() * wd.max()), float(wd.sum()))

    def figures(out, key):
        (loss, gB, gb), (rl, rB, rb, gscale, wsum) = out, refs[key]
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gB).all()) and bool(torch.isfinite(gb).all())
        return (float((gB - rB).abs().max()) / gscale, float((gb - rb).abs().max()) / wsum,
                abs(float(loss) - float(rl)) / float(rl))
    return X, y, w, B, b0, figures


SHAPES = [(n, 30, 32, 3) for n in (1, 63, 64, 65, 200, 8269)] + \
         [(8269, P, Pp, K) for P, Pp, K in ((100, 128, 7), (100, 128, 16), (100, 128, 17), (200, 256, 33),
                                             (250, 256, 64))]


@pytest.mark.parametrize("n,P,Pp,K", SHAPES)
def test_pass_matches_fp64(n, P, Pp, K):
    X, y, w, B, b0, figures = _case(n, P, Pp, K)
    first = linalg_ops.glm_multinomial_pass(X, y, w, B, b0, K)
    runs = [("default", first, "w"), ("slabs=1", linalg_ops.glm_multinomial_pass(X, y, w, B, b0, K, slabs=1), "w"),
            ("w=None", linalg_ops.glm_multinomial_pass(X, y, None, B, b0, K), "none")]
    if n == 200:
        runs.append(("slabs=3", linalg_ops.glm_multinomial_pass(X, y, w, B, b0, K, slabs=3), "w"))
    figs = {name: figures(out, key) for name, out, key in runs}
    for name, f in figs.items():
        print(f"ERR n={n} Pp={Pp} K={K} {name}: gB {f[0]:.3g} gb {f[1]:.3g} loss {f[2]:.3g}")
    assert first[1].shape == (Pp, K) and first[2].shape == (K,)
    assert bool((first[1][P:] == 0).all())
    again = linalg_ops.glm_multinomial_pass(X, y, w, B, b0, K)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(max(f) < BOUND for f in figs.values()), figs


def test_saturated():
    X, y, w, B, b0, figures = _case(8269, 100, 128, 7, scale=25.0)
    eta_max = float((X.double() @ B).abs().max())
    f = figures(linalg_ops.glm_multinomial_pass(X, y, w, B, b0, 7), "w")
    print(f"ERR saturated |eta| max {eta_max:.0f}: gB {f[0]:.3g} gb {f[1]:.3g} loss {f[2]:.3g}")
    assert eta_max > 100
    assert max(f) < BOUND, f


@pytest.mark.parametrize("kw", [dict(lambda_=0), dict(alpha=0.5, lambda_=1e-3)], ids=["lbfgs", "fista"])
def test_fit_uses_kernel(kw, monkeypatch):
    rng = np.random.RandomState(3)
    n, K = 3000, 4
    Xn = rng.randn(n, 6)
    c = rng.choice(list("pqr"), n)
    score = Xn[:, :K] + 0.8 * (c == "q")[:, None] * np.eye(K)[1] + rng.gumbel(size=(n, K))
    codes = score.argmax(1)
    df = pd.DataFrame(Xn, columns=[f"x{i}" for i in range(6)])
    df["cat"] = c
    df["y"] = np.array([f"c{k}" for k in range(K)])[codes]
    fr = h2o3_amd.H2OFrame(df)
    xs = [f"x{i}" for i in range(6)] + ["cat"]

    calls = []
    real = linalg_ops.glm_multinomial_pass
    monkeypatch.setattr(linalg_ops, "glm_multinomial_pass", lambda *a, **k: calls.append(1) or real(*a, **k))
    est = H2OGeneralizedLinearEstimator(family="multinomial", **kw)
    est.train(x=xs, y="y", training_frame=fr)
    assert len(calls) > 2
    ncalls = len(calls)
    monkeypatch.setenv("H2O3_GLM_MULTI", "torch")
    ref = H2OGeneralizedLinearEstimator(family="multinomial", **kw)
    ref.train(x=xs, y="y", training_frame=fr)
    assert len(calls) == ncalls

    X, _ = est._dinfo.expand(fr)
    P = est._dinfo.P
    eta = X[:, :P].double() @ est._multi["B"] + est._multi["b0"]
    yt = torch.as_tensor(codes, device=eta.device)
    dev64 = 2 * float((torch.logsumexp(eta, 1) - eta[torch.arange(n, device=eta.device), yt]).sum())
    dev, dev_ref = est.residual_deviance(), ref.residual_deviance()
    print(f"ERR fit {kw}: deviance kernel {dev:.10g} (fp64 of its coefficients {dev64:.10g}) torch {dev_ref:.10g}")
    assert abs(dev - dev64) / dev64 < 1e-6
    assert dev <= dev_ref * (1 + DEV_BOUND)
