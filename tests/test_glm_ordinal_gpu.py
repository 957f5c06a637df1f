"""The fused proportional-odds pass (ops/csrc/glm_multi.hip glm_ordinal_kernel,
reached through linalg_ops.glm_ordinal_pass and fit_multinomial) against
_loss_grad_ordinal's formula in torch float64 on the CPU (autograd for the
gradients), fed the same f32-rounded X, beta, cuts and w.

Bound per entry of loss, g_beta and g_cuts: 16 * max(e32, 2^-24) * S, S the sum
over rows of the absolute value of that row's term, e32 the worst
|ref32 - ref| / S of the same formula in float32 torch on the CPU, 16 = TAU_M
of tests/dl_oracle_common.py.  Each case prints rho = error / max(e32, 2^-24)
per quantity (RHO lines) before it asserts.
Measured on an MI355X (profiles/glm_ordinal_mb.txt has every case): worst rho
over the six shapes and three weight forms 0.12 (loss), 0.49 (g_beta), 0.11
(g_cuts), all at N = 1; error / S at most 8.6e-9, 5.3e-8, 7.1e-9.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd
from h2o3_amd.estimators import H2OGeneralizedLinearEstimator
from h2o3_amd.ops import _native, linalg_ops

pytestmark = pytest.mark.gpu

TAU_M, FLOOR = 16, 2.0 ** -24
NAMES = ("loss", "g_beta", "g_cuts")


def reference(X, y, w, beta, cuts, K, dtype=torch.float64):
    """((loss, g_beta, g_cuts), (S of each entry), rows with pk < 1e-15) on the CPU."""
    X, beta, cuts = X.to(dtype), *(t.to(dtype).clone().requires_grad_(True) for t in (beta, cuts))
    live = (y >= 0) & (y < K)
    wl = (torch.ones(len(y)) if w is None else w).to(dtype) * live
    yi = y.long().clamp(0, K - 1)
    inf = torch.full((1,), float("inf"), dtype=dtype)
    ext = torch.cat([-inf, cuts, inf])
    eta = X @ beta
    a, b = ext[yi + 1] - eta, ext[yi] - eta
    for t in (eta, a, b):
        t.retain_grad()
    pk = torch.sigmoid(a) - torch.sigmoid(b)
    terms = -wl * torch.log(pk.clamp_min(1e-15))
    terms.sum().backward()
    k = torch.arange(K - 1).view(-1, 1)
    s_cuts = ((yi == k) * a.grad.abs() + (yi - 1 == k) * b.grad.abs()).sum(1)
    return ((terms.sum().detach(), beta.grad, cuts.grad),
            (terms.detach().abs().sum(), X.abs().T @ eta.grad.abs(), s_cuts), int(((pk < 1e-15) & (wl != 0)).sum()))


def inputs(N, P, K, wform, close=False):
    g = torch.Generator().manual_seed(100 * N + P + K)
    X = torch.randn(N, P, generator=g)
    beta = (torch.randn(P, generator=g) / P ** 0.5).float()
    cuts = torch.sort(torch.randn(K - 1, generator=g) * 1.5).values.float()
    if close:
        cuts[2] = cuts[1] + 1e-3
    y = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    i = torch.arange(N)
    y[i % 23 == 5] = -1
    y[i % 29 == 9] = K
    w = None
    if wform != "none":
        w = torch.rand(N, generator=g) * 2
        w[i % 7 == 6] = 0
        if wform == "class":
            w[y == 1] = 0
    return X, y, w, beta, cuts


def check(got, X, y, w, beta, cuts, K, tag):
    ref, S, clamped = reference(X, y, w, beta, cuts, K)
    ref32 = reference(X, y, w, beta, cuts, K, torch.float32)[0]
    assert clamped == 0
    for name, o, r, r32, s in zip(NAMES, got, ref, ref32, S):
        o, r, r32, s = (t.detach().double().cpu().reshape(-1) for t in (o, r, r32, s))
        if name == "g_beta":
            assert bool(((s > 0) | ((r == 0) & (o == 0))).all())
        pos = s > 0
        e32 = max(float(((r32 - r).abs()[pos] / s[pos]).max()), FLOOR) if pos.any() else FLOOR
        err = float(((o - r).abs()[pos] / s[pos]).max()) if pos.any() else 0.0
        print(f"RHO {tag} {name}: err/S {err:.3g} e32 {e32:.3g} rho {err / e32:.3g}")
        assert bool(((o - r).abs() <= TAU_M * e32 * s).all()), (tag, name, err, e32)


@pytest.mark.parametrize("N,P,K", [(1, 4, 2), (63, 36, 3), (65, 32, 3), (129, 100, 7), (200, 260, 5), (130, 1024, 64)])
def test_pass_matches_fp64(N, P, K):
    for wform in ("none", "mixed", "class"):
        X, y, w, beta, cuts = inputs(N, P, K, wform, close=(N == 129 and wform == "mixed"))
        Xd = X.cuda()
        kw = {}
        if N == 63:                         # X stored wider than Pp, the extra columns never read
            Xd = torch.cat([X, torch.full((N, 4), float("nan"))], 1).cuda()
            kw = {"width": P}
        dev = [t if t is None else t.cuda() for t in (y, w, beta, cuts)]
        for slabs in ((None, 1, 3) if N == 129 else (None,)):
            got = linalg_ops.glm_ordinal_pass(Xd, *dev, K, slabs=slabs, **kw)
            again = linalg_ops.glm_ordinal_pass(Xd, *dev, K, slabs=slabs, **kw)
            assert all(torch.equal(p, q) for p, q in zip(got, again))
            assert got[1].shape == (P,) and got[2].shape == (K - 1,)
            check(got, X, y, w, beta, cuts, K, f"N={N} P={P} K={K} w={wform} slabs={slabs}")


def test_clamped_row():
    """One row at pk < 1e-15 adds -w log 1e-15 to the loss and nothing else."""
    N, P, K = 65, 32, 3
    X, y, w, beta, cuts = inputs(N, P, K, "mixed")
    X[7], y[7], w[7] = 60 * beta / (beta @ beta), 0, 1.25
    assert reference(X, y, w, beta, cuts, K)[2] == 1
    w0 = w.clone()
    w0[7] = 0
    Xd, yd, bd, cd = X.cuda(), y.cuda(), beta.cuda(), cuts.cuda()
    got = linalg_ops.glm_ordinal_pass(Xd, yd, w.cuda(), bd, cd, K)
    without = linalg_ops.glm_ordinal_pass(Xd, yd, w0.cuda(), bd, cd, K)
    term = -1.25 * np.log(1e-15)
    assert abs(float(got[0] - without[0]) - term) <= 2.0 ** -23 * term
    assert torch.equal(got[1], without[1]) and torch.equal(got[2], without[2])


@pytest.mark.parametrize("Pp,K", [(32, 65), (1028, 3), (6, 3)])
def test_rejected_shapes(Pp, K):
    assert not linalg_ops.glm_ordinal_supported(Pp, K)
    ldx = -(-Pp // 4) * 4
    X, y = torch.zeros(64, ldx, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    part = torch.zeros(ldx + K, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _native.get_lib("glm_multi").h2o_glm_multinomial(p(X), 64, Pp, ldx, p(y), None, p(X), p(X), K, 1, 1, 64,
                                                         p(part), _native.stream())
    assert rc == -1
    with pytest.raises(ValueError):
        linalg_ops.glm_ordinal_pass(X, y, None, X[0, :Pp], X[0, :K - 1], K, width=Pp)


def test_fit_uses_kernel(monkeypatch):
    """Both routes minimise the same convex objective f (per unit weight) by
    L-BFGS, which stops at |f - f_next| < tol max(1, |f|), tol = 1e-7.  The
    deviance is 2 wsum f: the routes may differ by TOL_STEPS stopping steps.
    The coefficients of two points that close in f differ by at most
    sqrt(2 TOL_STEPS tol / mu), mu = 0.05 a floor on the curvature of f along
    any standardised coefficient.  Measured: profiles/glm_ordinal_mb.txt."""
    TOL_STEPS, tol, mu = 10, 1e-7, 0.05
    rng = np.random.RandomState(11)
    n, K = 2000, 4
    Xn = rng.randn(n, 8)
    codes = np.digitize(Xn[:, :3] @ [1.0, -0.7, 0.4] + rng.logistic(size=n), [-1.2, 0.1, 1.5])
    df = pd.DataFrame(Xn, columns=[f"x{i}" for i in range(8)])
    df["y"] = np.array([f"c{k}" for k in range(K)])[codes]
    fr = h2o3_amd.H2OFrame(df)
    calls = []
    real = linalg_ops.glm_ordinal_pass
    monkeypatch.setattr(linalg_ops, "glm_ordinal_pass", lambda *a, **k: calls.append(1) or real(*a, **k))
    est = H2OGeneralizedLinearEstimator(family="ordinal", lambda_=0)
    est.train(y="y", training_frame=fr)
    ncalls = len(calls)
    assert ncalls > 2
    monkeypatch.setenv("H2O3_GLM_MULTI", "torch")
    ref = H2OGeneralizedLinearEstimator(family="ordinal", lambda_=0)
    ref.train(y="y", training_frame=fr)
    assert len(calls) == ncalls
    dev, dev_ref = est.residual_deviance(), ref.residual_deviance()
    th, th_ref = (torch.cat([m._multi["beta"], m._multi["theta"]]) for m in (est, ref))
    dcoef = float((th - th_ref).abs().max())
    print(f"FIT deviance kernel {dev:.12g} torch {dev_ref:.12g} diff {abs(dev - dev_ref):.3g}  max coef diff {dcoef:.3g}")
    assert abs(dev - dev_ref) <= TOL_STEPS * tol * max(2 * n, dev_ref)
    assert dcoef <= (2 * TOL_STEPS * tol / mu) ** 0.5
