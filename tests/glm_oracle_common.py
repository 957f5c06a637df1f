"""An fp64 oracle of one IRLS pass, written from the GLM definitions, and the
cases the GLM kernels of ops/csrc/gram.hip are checked at.

Nothing here imports the product's family code (models.glm) or its kernels'
wrappers (ops): a formula that is wrong in the kernel and in the product's
own reference must not be wrong here as well.  Everything is numpy float64;
the inputs are the float32 arrays the kernel gets, each cast to float64 once.

Per row
    eta = x.beta + b0 + offset        mu = g^-1(eta)        d = dmu/deta
    W   = w d^2 / V(mu)               z  = (eta - offset) + (y - mu) / d
    r   = w (y - mu) d / V(mu)        dev = unit deviance(y, mu)
(gaussian / identity: W = w, z = y - offset), and from these the augmented
Gram [X | 1 | z]' W [X | 1 | z], sum w dev and the gradient (X'r, sum r).
"""
from typing import NamedTuple

import numpy as np

# Floors that belong to the project's contract (kernel and product reference
# share them by design).  No case but the saturation case reaches one; every
# result records whether one was reached (IrlsRef.floors_hit).
D_V_FLOOR = 1e-10        # contract: max(., 1e-10) on dmu/deta and on V(mu)
LOG_ETA_MAX = 80.0       # contract: eta <= 80 in the log link
INV_ETA_MIN = 1e-10      # contract: |eta| >= 1e-10 in the inverse link

# The saturation case only: the deviance of the f32 kernel clamps mu to
# [1e-15, 1 - 2^-23] (1.f - 1e-7f rounds to 1 - 2^-23).  This is the one
# constant the oracle takes from the kernel.
SAT_MU_CLAMP = (1e-15, 1.0 - 2.0 ** -23)

BINOMIAL = ("binomial", "quasibinomial", "fractionalbinomial")


class Case(NamedTuple):
    """(X, beta, b0, y, w, offset, family, link, tvp, theta): X [N, Pp] f32
    with the first P columns filled, beta [Pp] f32, y / w / offset [N] f32."""
    X: np.ndarray
    beta: np.ndarray
    b0: float
    y: np.ndarray
    w: np.ndarray
    offset: np.ndarray
    family: str
    link: str
    tvp: float
    theta: float


class IrlsRef(NamedTuple):
    G: np.ndarray        # [P + 2, P + 2] augmented Gram
    dev: float           # sum w dev
    grad: np.ndarray     # [P + 1]: X'r, then sum r
    eta: np.ndarray
    mu: np.ndarray
    W: np.ndarray
    z: np.ndarray
    r: np.ndarray
    floors_hit: bool


def _softplus(x):
    return np.logaddexp(0.0, x)


def _xlogy(a, b):
    """a log b with 0 log 0 = 0."""
    out = np.zeros_like(a)
    nz = a != 0
    out[nz] = a[nz] * np.log(b[nz])
    return out


def linkinv(link, eta):
    """(mu, dmu/deta before its floor, whether a floor of the link was reached)."""
    if link == "identity":
        return eta, np.ones_like(eta), False
    if link == "logit":
        mu = np.exp(-_softplus(-eta))                      # 1 / (1 + exp(-eta)), no overflow
        return mu, np.exp(-_softplus(-eta) - _softplus(eta)), False
    if link == "log":
        hit = bool((eta > LOG_ETA_MAX).any())
        mu = np.exp(np.minimum(eta, LOG_ETA_MAX))
        return mu, mu, hit
    if link == "inverse":
        hit = bool((np.abs(eta) < INV_ETA_MIN).any())
        e = np.where(np.abs(eta) < INV_ETA_MIN, np.where(eta < 0, -INV_ETA_MIN, INV_ETA_MIN), eta)
        mu = 1.0 / e
        return mu, -mu * mu, hit
    raise ValueError(link)


def variance(family, mu, tvp, theta):
    if family == "gaussian":
        return np.ones_like(mu)
    if family in BINOMIAL:
        return mu * (1.0 - mu)
    if family == "poisson":
        return mu
    if family == "gamma":
        return mu * mu
    if family == "tweedie":
        return mu ** tvp if tvp != 0 else np.ones_like(mu)
    if family == "negativebinomial":
        return mu + theta * mu * mu
    raise ValueError(family)


def _dev_poisson(y, mu):
    return 2.0 * (_xlogy(y, y / mu) - (y - mu))


def _dev_gamma(y, mu):
    return 2.0 * (-np.log(y / mu) + (y - mu) / mu)


def unit_deviance(family, link, y, mu, eta, tvp, theta, mu_clamp=None):
    if family == "gaussian":
        return (y - mu) ** 2
    if family in BINOMIAL:
        ent = _xlogy(y, y) + _xlogy(1.0 - y, 1.0 - y)     # 0 for 0/1 responses
        if mu_clamp is not None:
            m = np.clip(mu, *mu_clamp)
            return 2.0 * (ent - _xlogy(y, m) - _xlogy(1.0 - y, 1.0 - m))
        if link != "logit":
            raise ValueError("binomial families: logit link only")
        # -log mu = softplus(-eta), -log(1 - mu) = softplus(eta): for 0/1
        # responses this is 2 (softplus(eta) - y eta); no cancellation, no clamp
        return 2.0 * (ent + _softplus(eta) - y * eta)
    if family == "poisson":
        return _dev_poisson(y, mu)
    if family == "gamma":
        return _dev_gamma(y, mu)
    if family == "tweedie":
        p = tvp
        if p == 0:
            return (y - mu) ** 2
        if p == 1:
            return _dev_poisson(y, mu)
        if p == 2:
            return _dev_gamma(y, mu)
        a = np.zeros_like(y)
        nz = y > 0
        a[nz] = y[nz] ** (2.0 - p) / ((1.0 - p) * (2.0 - p))
        return 2.0 * (a - y * mu ** (1.0 - p) / (1.0 - p) + mu ** (2.0 - p) / (2.0 - p))
    if family == "negativebinomial":
        # log((1 + theta y) / (1 + theta mu)) = log1p(theta (y - mu) / (1 + theta mu))
        t2 = (y + 1.0 / theta) * np.log1p(theta * (y - mu) / (1.0 + theta * mu))
        return 2.0 * (_xlogy(y, y / mu) - t2)
    raise ValueError(family)


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def irls_pass(X, beta, b0, y, w, offset, family, link, tvp=0.0, theta=1e-10, P=None, mu_clamp=None):
    """One IRLS pass in fp64.  X [N, >= P], beta [>= P]; w / offset may be
    None (1 / 0).  beta and b0 may be float64 (the finite-difference test)."""
    Xd = f64(X)
    P = Xd.shape[1] if P is None else P
    Xd = Xd[:, :P]
    n = Xd.shape[0]
    yd = f64(y)
    wd = np.ones(n) if w is None else f64(w)
    od = np.zeros(n) if offset is None else f64(offset)
    eta = Xd @ f64(beta)[:P] + float(b0) + od
    mu, d0, hit = linkinv(link, eta)
    if family == "gaussian" and link == "identity":
        W, z, r = wd.copy(), yd - od, wd * (yd - mu)
    else:
        v0 = variance(family, mu, tvp, theta)
        floor_d = link in ("logit", "log")                 # the contract floors d of these two links
        hit = hit or bool((v0 < D_V_FLOOR).any()) or (floor_d and bool((d0 < D_V_FLOOR).any()))
        d = np.maximum(d0, D_V_FLOOR) if floor_d else d0
        v = np.maximum(v0, D_V_FLOOR) if family != "gaussian" else v0
        W = wd * d * d / v
        z = (eta - od) + (yd - mu) / d
        r = wd * (yd - mu) * d / v
    dev = float((wd * unit_deviance(family, link, yd, mu, eta, tvp, theta, mu_clamp))[wd != 0].sum())
    A = np.concatenate([Xd, np.ones((n, 1)), z[:, None]], 1)
    G = A.T @ (A * W[:, None])
    grad = np.concatenate([Xd.T @ r, [r.sum()]])
    return IrlsRef(G, dev, grad, eta, mu, W, z, r, hit)


def external_gram(X, W, z, P):
    """[X | 1 | z]' W [X | 1 | z] for caller-supplied W and z, and the same
    with |W| (the error scale when W is signed)."""
    A = np.concatenate([f64(X)[:, :P], np.ones((X.shape[0], 1)), f64(z)[:, None]], 1)
    Wd = f64(W)
    return A.T @ (A * Wd[:, None]), A.T @ (A * np.abs(Wd)[:, None])


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------

def gram_error(A, B, scale_from=None):
    """max |A - B| / sqrt(S_ii S_jj), S = B (or `scale_from`: the |W| Gram when
    W is signed -- the sum of a product's absolute terms is bounded by
    sqrt(S_ii S_jj) only for non-negative weights), diagonal clamped at 1e-300."""
    A, B = f64(A), f64(B)
    S = B if scale_from is None else f64(scale_from)
    dg = np.sqrt(np.maximum(np.abs(np.diagonal(S)), 1e-300))
    return float((np.abs(A - B) / (dg[:, None] * dg[None, :])).max())


def grad_scale(X, y, w, P):
    """The scale of test_linalg_gpu._assert_grad_close: the largest column
    sum of |x| times (max |y| + 1) times max w."""
    return float(np.abs(f64(X)[:, :P]).sum(0).max() * (np.abs(f64(y)).max() + 1.0) *
                 (1.0 if w is None else float(np.max(w))))


def grad_error(g, ref, X, y, w, P):
    return float(np.abs(f64(g) - ref).max() / grad_scale(X, y, w, P))


def dev_error(d, ref):
    return abs(float(d) - ref) / abs(ref)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

# (family, link, tvp, theta): the family sweep
FAMILY_SWEEP = [
    ("gaussian", "identity", 0.0, 0.0), ("gaussian", "log", 0.0, 0.0), ("gaussian", "inverse", 0.0, 0.0),
    ("binomial", "logit", 0.0, 0.0), ("quasibinomial", "logit", 0.0, 0.0), ("fractionalbinomial", "logit", 0.0, 0.0),
    ("poisson", "log", 0.0, 0.0), ("poisson", "identity", 0.0, 0.0),
    ("gamma", "inverse", 0.0, 0.0), ("gamma", "log", 0.0, 0.0), ("gamma", "identity", 0.0, 0.0),
    ("tweedie", "log", 0.0, 0.0), ("tweedie", "log", 1.0, 0.0), ("tweedie", "log", 1.5, 0.0),
    ("tweedie", "log", 2.0, 0.0), ("tweedie", "log", 3.0, 0.0), ("tweedie", "identity", 1.5, 0.0),
    ("negativebinomial", "log", 0.0, 1e-10), ("negativebinomial", "log", 0.0, 0.5),
    ("negativebinomial", "log", 0.0, 2.0), ("negativebinomial", "identity", 0.0, 1e-10),
    ("negativebinomial", "identity", 0.0, 0.5), ("negativebinomial", "identity", 0.0, 2.0),
]


def family_id(f):
    family, link, tvp, theta = f
    s = f"{family}-{link}"
    if family == "tweedie":
        s += f"-p{tvp:g}"
    if family == "negativebinomial":
        s += f"-th{theta:g}"
    return s


def _positive_mean(family, tvp):
    return family in ("poisson", "gamma", "negativebinomial") or (family == "tweedie" and tvp != 0)


def intercept_for(family, link, tvp):
    """b0 (exact in f32) keeping mu inside the family's domain for every row:
    x.beta + offset lies in [-1.1, 1.1]."""
    if link == "logit":
        return -0.25
    if link == "log":
        return 0.5
    if link == "inverse":
        return 2.0                                   # eta in [1, 3] before the offset
    return 2.0 if _positive_mean(family, tvp) else 0.25


def _draw_y(rng, family, mu, tvp, theta, n):
    idx = np.arange(n)
    if family == "gaussian" or (family == "tweedie" and tvp == 0):
        return mu + 0.5 * rng.standard_normal(n)
    if family == "binomial":
        return (rng.random(n) < mu).astype(np.float64)
    if family in ("quasibinomial", "fractionalbinomial"):
        y = np.clip(mu + 0.2 * rng.standard_normal(n), 0.01, 0.99)
        y[idx % 10 == 1] = 0.0
        y[idx % 10 == 2] = 1.0
        return y
    if family == "poisson" or (family == "tweedie" and tvp == 1):
        y = rng.poisson(mu).astype(np.float64)
    elif family == "gamma" or (family == "tweedie" and tvp == 2):
        return np.maximum(rng.gamma(2.0, mu / 2.0), 1e-3)
    elif family == "tweedie" and 1 < tvp < 2:
        # compound Poisson-gamma with dispersion 1: mean mu, variance mu^p
        lam = mu ** (2.0 - tvp) / (2.0 - tvp)
        alpha = (2.0 - tvp) / (tvp - 1.0)
        scale = (tvp - 1.0) * mu ** (tvp - 1.0)
        k = rng.poisson(lam)
        y = np.where(k > 0, rng.gamma(np.maximum(k, 1) * alpha, scale), 0.0)
    elif family == "tweedie" and tvp == 3:
        return np.maximum(rng.wald(mu, 1.0), 1e-3)   # inverse Gaussian: variance mu^3
    elif family == "negativebinomial":
        if theta < 1e-6:
            y = rng.poisson(mu).astype(np.float64)   # the theta -> 0 limit
        else:
            y = rng.negative_binomial(1.0 / theta, 1.0 / (1.0 + theta * mu)).astype(np.float64)
    else:
        raise ValueError((family, tvp))
    y[idx % 10 == 3] = 0.0                           # at least 10 % zero counts
    return y


def make_case(family, link, tvp=0.0, theta=0.0, n=200, P=30, Pp=32, seed=0, plain=False):
    """One valid case.  plain: no prior weights and no offset (w, offset None)."""
    rng = np.random.default_rng([seed, n, P])
    X = np.zeros((n, Pp), dtype=np.float32)
    X[:, :P] = rng.uniform(-1.0, 1.0, (n, P)).astype(np.float32)
    b = rng.standard_normal(P)
    beta = np.zeros(Pp, dtype=np.float32)
    beta[:P] = (0.95 * b / np.abs(b).sum()).astype(np.float32)
    assert np.abs(f64(beta)).sum() <= 1.0
    b0 = intercept_for(family, link, tvp)
    assert float(np.float32(b0)) == b0
    offset = None if plain else rng.uniform(-0.1, 0.1, n).astype(np.float32)
    w = None
    if not plain:
        w = rng.uniform(0.5, 1.5, n).astype(np.float32)
        w[6::7] = 0.0                                # every 7th row carries no weight, y stays finite
    eta = f64(X) @ f64(beta) + b0 + (0.0 if offset is None else f64(offset))
    mu = linkinv(link, eta)[0]
    y = _draw_y(rng, family, mu, tvp, theta, n).astype(np.float32)
    assert np.isfinite(y).all()
    return Case(X, beta, b0, y, w, offset, family, link, float(tvp), float(theta))


def make_saturated_case(n=1000, P=30, Pp=32, seed=0):
    """binomial / logit with one column scaled so that eta spans [-30, 30];
    y drawn at mu, every 100th row's label flipped."""
    rng = np.random.default_rng([seed, n, P, 77])
    X = np.zeros((n, Pp), dtype=np.float32)
    X[:, :P] = rng.uniform(-1.0, 1.0, (n, P)).astype(np.float32)
    b = rng.standard_normal(P)
    b[0] = 0.0
    beta = np.zeros(Pp, dtype=np.float32)
    beta[:P] = (0.65 * b / np.abs(b).sum()).astype(np.float32)
    beta[0] = 0.25
    X[:, 0] *= 117.0                                 # 0.25 * 117 = 29.25, the rest adds at most 0.75
    offset = rng.uniform(-0.1, 0.1, n).astype(np.float32)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    w[6::7] = 0.0
    eta = f64(X) @ f64(beta) + f64(offset)
    mu = linkinv("logit", eta)[0]
    y = (rng.random(n) < mu).astype(np.float32)
    y[50::100] = 1.0 - y[50::100]
    return Case(X, beta, 0.0, y, w, offset, "binomial", "logit", 0.0, 0.0)


def oracle(c, P, mu_clamp=None):
    return irls_pass(c.X, c.beta, c.b0, c.y, c.w, c.offset, c.family, c.link, c.tvp, c.theta, P=P,
                     mu_clamp=mu_clamp)


# ---------------------------------------------------------------------------
# the negative-binomial deviance in f32, both forms (arithmetic only)
# ---------------------------------------------------------------------------

def nb_deviance_f32(y, mu, theta, stable):
    """Unit deviance in numpy float32.  stable: gi_dev's form of gram.hip --
    log1p(u), u = theta (y - mu) / (1 + theta mu), by four series terms below
    |u| = 2^-6 and log(1 + u) beyond; otherwise the ratio form
    log((1 + theta y) / (1 + theta mu))."""
    f = np.float32
    y, mu, th, one = f(y), f(mu), f(theta), f(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = np.where(y > 0, y * np.log(np.where(y > 0, y, one) / mu), f(0.0)).astype(f)
    if stable:
        u = th * (y - mu) / (one + th * mu)
        series = u * (one - u * (f(0.5) - u * (f(0.33333334) - f(0.25) * u)))
        l1p = np.where(np.abs(u) < f(0.015625), series, np.log(one + u))
        assert l1p.dtype == f
        t2 = (y + one / th) * l1p
    else:
        t2 = (y + one / th) * np.log((one + th * y) / (one + th * mu))
    out = f(2.0) * (t1 - t2)
    assert out.dtype == f
    return out
