"""The fp64 IRLS oracle of tests/glm_oracle_common.py checked against itself
(identities that tie its formulas together) and against the product's own
reference, on the CPU.  The kernels meet the oracle in test_glm_oracle_gpu.py.
"""
import numpy as np
import pytest
import torch

import glm_oracle_common as oc

FAMS = pytest.mark.parametrize("fam", oc.FAMILY_SWEEP, ids=oc.family_id)
N, P, PP = 200, 30, 32


def _case(fam, plain=False):
    family, link, tvp, theta = fam
    return oc.make_case(family, link, tvp, theta, n=N, P=P, Pp=PP, plain=plain)


@FAMS
@pytest.mark.parametrize("plain", [False, True], ids=["w_off", "plain"])
def test_cases_are_valid(fam, plain):
    """The builders keep what they promise: no floor is reached, mu is inside
    the family's domain, zero weights and zero counts are present."""
    c = _case(fam, plain)
    ref = oc.oracle(c, P)
    assert not ref.floors_hit
    assert np.abs(c.beta.astype(np.float64)).sum() <= 1.0 and np.abs(c.X).max() <= 1.0
    assert not c.X[:, P:].any() and not c.beta[P:].any()
    if c.family in oc.BINOMIAL:
        assert ref.mu.min() > 0.1 and ref.mu.max() < 0.9
    elif oc._positive_mean(c.family, c.tvp):
        assert ref.mu.min() > 0.3
    if c.link == "inverse":
        assert ref.eta.min() >= 0.9
    if not plain:
        assert (c.w[6::7] == 0).all() and np.abs(c.offset).max() <= 0.1
    if c.family in ("poisson", "negativebinomial") or (c.family == "tweedie" and 1 < c.tvp < 2):
        assert (c.y == 0).mean() >= 0.10
    if c.family in ("quasibinomial", "fractionalbinomial"):
        assert (c.y == 0).any() and (c.y == 1).any() and ((c.y > 0) & (c.y < 1)).any()
    if c.family == "gamma" or (c.family == "tweedie" and c.tvp >= 2):
        assert c.y.min() > 0
    assert np.isfinite(ref.G).all() and np.isfinite(ref.dev) and np.isfinite(ref.grad).all()


@FAMS
def test_gradient_identity(fam):
    """d(sum w dev)/d(beta, b0) along a direction equals -2 g.direction: the
    deviance, the variance, the link and the residual are four formulas
    written apart; a wrong sign or power in any one breaks this."""
    c = _case(fam)
    ref = oc.oracle(c, P)
    rng = np.random.default_rng(5)
    h = 1e-6
    b = c.beta.astype(np.float64)[:P]
    for k in range(8):
        u = rng.standard_normal(P + 1)
        u /= np.abs(u).sum()                                 # keeps eta inside the case's range
        dp = oc.irls_pass(c.X, b + h * u[:P], c.b0 + h * u[P], c.y, c.w, c.offset, c.family, c.link, c.tvp,
                          c.theta, P=P).dev
        dm = oc.irls_pass(c.X, b - h * u[:P], c.b0 - h * u[P], c.y, c.w, c.offset, c.family, c.link, c.tvp,
                          c.theta, P=P).dev
        fd = (dp - dm) / (2 * h)
        an = -2.0 * float(ref.grad @ u)
        assert abs(fd - an) <= 1e-6 * abs(an), (k, fd, an)


@FAMS
def test_working_response_identity(fam):
    """X'Wz = X'W(eta - offset) + X'r, and the same for the intercept row."""
    c = _case(fam)
    ref = oc.oracle(c, P)
    Xa = np.concatenate([c.X[:, :P].astype(np.float64), np.ones((N, 1))], 1)
    lin = ref.eta - c.offset.astype(np.float64)
    rhs = Xa.T @ (ref.W * lin) + ref.grad
    lhs = ref.G[:P + 1, P + 1]
    scale = np.abs(Xa * (ref.W * np.abs(ref.z))[:, None]).sum(0)
    assert (np.abs(lhs - rhs) <= 1e-12 * scale).all(), np.abs((lhs - rhs) / scale).max()


def _product_fam(c):
    """The product's family object and fused-kernel codes of a case.  Tweedie
    goes through the product's own "tweedie" link with link power 0 (log) or 1
    (identity), as a fitted model would."""
    from h2o3_amd.models.glm.glm import _Fam
    from h2o3_amd.ops import linalg_ops
    if c.family == "tweedie":
        tlp = {"log": 0.0, "identity": 1.0}[c.link]
        return (_Fam("tweedie", "tweedie", tvp=c.tvp, tlp=tlp),
                linalg_ops.glm_fused_codes("tweedie", "tweedie", tlp))
    kw = {"theta": c.theta} if c.family == "negativebinomial" else {}
    return _Fam(c.family, c.link, tvp=c.tvp, **kw), linalg_ops.glm_fused_codes(c.family, c.link)


LINK_CODE = {"identity": 0, "logit": 1, "log": 2, "inverse": 3}
VAR_CODE = {"gaussian": 0, "binomial": 1, "quasibinomial": 1, "fractionalbinomial": 1, "poisson": 2, "gamma": 3,
            "tweedie": 4, "negativebinomial": 5}


@FAMS
@pytest.mark.parametrize("plain", [False, True], ids=["w_off", "plain"])
def test_product_reference_matches_oracle(fam, plain):
    """glm_irls_reference on _Fam against the oracle, per entry.

    Differences by design (none is reached by this data, so none is excused
    below):
      * _Fam("tweedie", link="tweedie", tlp=1) floors eta at 1e-10 before the
        power; the kernel route maps link power 1 to the plain identity link.
        The cases keep eta >= 0.9.
      * _Fam's log link caps eta at 700, the kernel's at 80 (f32 range); the
        cases keep |eta| < 2.
      * _Fam clamps mu to [1e-15, 1 - 1e-15] in the binomial deviance, the
        kernel to [1e-15, 1 - 2^-23]; the cases keep mu in (0.1, 0.9).
      * _Fam guards log(y) with max(y, 1e-300) where the kernel uses 1e-30;
        gamma responses here are >= 1e-3 and zero counts take the y == 0 branch.
    """
    from h2o3_amd.ops import linalg_ops
    c = _case(fam, plain)
    ref = oc.oracle(c, P)
    pf, codes = _product_fam(c)
    assert codes == (LINK_CODE[c.link], VAR_CODE[c.family])    # the route GLMDriver takes for this family
    t = lambda a: None if a is None else torch.from_numpy(a)
    Gr, dr = linalg_ops.glm_irls_reference(t(c.X), aug=P, beta=t(c.beta), b0=c.b0, y=t(c.y), wprior=t(c.w),
                                           offset=t(c.offset), fam=pf)
    Gr = Gr.numpy()
    assert oc.gram_error(Gr[:P + 2, :P + 2], ref.G) <= 1e-9
    assert oc.dev_error(dr.item(), ref.dev) <= 1e-9
    assert not Gr[P + 2:].any() and not Gr[:, P + 2:].any()


@pytest.mark.parametrize("theta", [1e-10, 1e-6, 1e-3, 0.5])
def test_negbin_deviance_f32_forms(theta):
    """Why gi_dev (gram.hip) writes the negative-binomial deviance through
    log1p(theta (y - mu) / (1 + theta mu)): in f32, 1 + theta y == 1 at small
    theta and the 1 / theta factor turns the lost term (about y - mu) into the
    answer.  Arithmetic only, numpy f32, the kernel's own series / log split.
    That form is held to 1e-5 of the fp64 oracle, in total and per row; the
    ratio form's error is printed, not asserted."""
    rng = np.random.default_rng(1)
    n = 4096
    mu = np.exp(rng.normal(0.2, 0.6, n)).astype(np.float32)
    y = rng.poisson(mu).astype(np.float32)
    ref = oc.unit_deviance("negativebinomial", "log", y.astype(np.float64), mu.astype(np.float64), None, 0.0,
                           theta)
    tot = ref.sum()
    stable = oc.nb_deviance_f32(y, mu, theta, True).astype(np.float64)
    ratio = oc.nb_deviance_f32(y, mu, theta, False).astype(np.float64)
    e_st, e_ra = abs(stable.sum() - tot) / tot, abs(ratio.sum() - tot) / tot
    print(f"NBDEV theta={theta:g}: stable form total err {e_st:.3e} (per row max {np.abs(stable - ref).max():.3e}); "
          f"ratio form total err {e_ra:.3e} (per row max {np.abs(ratio - ref).max():.3e})")
    assert e_st <= 1e-5
    assert np.abs(stable - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


def test_saturated_case_spans_the_range():
    c = oc.make_saturated_case()
    ref = oc.oracle(c, P, mu_clamp=oc.SAT_MU_CLAMP)
    assert ref.eta.min() < -28 and ref.eta.max() > 28 and np.abs(ref.eta).max() <= 30.2
    assert ref.floors_hit                                    # the one case that reaches a floor
    free = oc.oracle(c, P)
    assert np.isfinite(ref.dev) and np.isfinite(free.dev)
    assert np.array_equal(ref.G, free.G) and np.array_equal(ref.grad, free.grad)   # the clamp touches the deviance only
