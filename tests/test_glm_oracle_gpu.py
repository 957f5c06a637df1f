"""The fused IRLS kernels of ops/csrc/gram.hip (glm_irls_ws_kernel,
glm_irls_kernel, glm_wide_split_kernel and the two wide Gram kernels), each
reached through linalg_ops, against the fp64 oracle of
tests/glm_oracle_common.py: every (family, link) pair the fused routes accept,
row counts around one 64-row chunk and at the first two-split size, and a
saturated binomial case.

Every entry of the augmented Gram is compared on the sqrt(G_ii G_jj) scale,
with the deviance, the exact-gradient channel, the symmetry and the zero
padding.  Bounds (none is taken from what the kernels give):
  2e-5  f32 MFMA and bf16x3 on the narrow routes (also the bound of
        test_linalg_gpu.test_glm_irls_bf3_elementwise).  bf16 carries 8
        significant bits (unit roundoff 2^-8), so one bf16x3 product -- hi hi
        + hi lo + lo hi with lo rounded to bf16 -- can be off by 3 * 2^-16 =
        4.6e-5 of |x_i x_j|; an entry meets 2e-5 of sqrt(G_ii G_jj) only where
        the roundings of many rows average out.  A single row on the bf16x3
        kernel measured 2.30e-5 (binomial) and 2.48e-5 (poisson, and external
        W), so linalg_ops.glm_irls sends passes of fewer than 64 rows (one
        chunk) to the f32 MFMA; from n = 64 on the bf16x3 routes measured at
        most 6.8e-6.  test_row_counts asserts which tier each row count ran.
  5e-5  the wide split + library GEMM route, 3e-5 the fused wide bf16x3 Gram.
  8e-3  the one-MFMA bf16 tiers (2 * 2^-9 = 3.9e-3 per product).
  1e-4  deviance, relative; 1e-6 gradient, on the scale of
        test_linalg_gpu._assert_grad_close.
Each test prints the figures it measured (ERR lines) before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from h2o3_amd.ops import linalg_ops

import glm_oracle_common as oc

pytestmark = pytest.mark.gpu

DEV_BOUND = 1e-4
GRAD_BOUND = 1e-6


class Route:
    """One way into the kernels: kind ws | irls | wide_split | wide_fused."""

    def __init__(self, name, kind, P, Pp, bound, **kw):
        self.name, self.kind, self.P, self.Pp, self.bound, self.kw = name, kind, P, Pp, bound, kw
        self.narrow = kw.pop("narrow", False)

    def __repr__(self):
        return self.name


FUSED_ROUTES = [
    Route("ws_f32_30_32", "ws", 30, 32, 2e-5, bf3=False),
    Route("ws_f32_50_64", "ws", 50, 64, 2e-5, bf3=False),
    Route("ws_f32_100_128", "ws", 100, 128, 2e-5, bf3=False),
    Route("ws_bf3_100_128", "ws", 100, 128, 2e-5, bf3=True),
    Route("ws_bf3_narrow_100_128", "ws", 100, 128, 2e-5, bf3=True, narrow=True),
    Route("ws_bf16_100_128", "ws", 100, 128, 8e-3, bf3="bf16"),
    Route("irls_200_256", "irls", 200, 256, 2e-5),
    Route("irls_400_512", "irls", 400, 512, 2e-5),
    Route("wide_split_130", "wide_split", 130, 130, 5e-5),
    Route("wide_split_300", "wide_split", 300, 300, 5e-5),
    Route("wide_split_601", "wide_split", 601, 601, 5e-5),
] + [Route(f"wide_fused_{P}_t{tile}_{'bf3' if bf3 else 'bf16'}", "wide_fused", P, P, 3e-5 if bf3 else 8e-3,
           tile=tile, bf3=bf3)
     for P in (127, 130, 601) for tile, bf3 in ((128, True), (256, True), (256, False))]
WS_ROUTES = [r for r in FUSED_ROUTES if r.kind == "ws"]

# (name, P, Pp): caller-supplied W and z; ws kernel at 32 / 128, glm_irls_kernel at 96 / 224
EXTERNAL_ROUTES = [("ws_ext_30_32", 30, 32), ("ws_ext_100_128", 100, 128), ("irls_ext_70_96", 70, 96),
                   ("irls_ext_200_224", 200, 224)]

ROW_COUNTS = [1, 63, 64, 65, 200, 8192 + 77]
ROW_FAMS = [("binomial", "logit", 0.0, 0.0), ("poisson", "log", 0.0, 0.0)]


@functools.lru_cache(maxsize=None)
def _case(fam, plain, n, P, Pp):
    family, link, tvp, theta = fam
    c = oc.make_case(family, link, tvp, theta, n=n, P=P, Pp=Pp, plain=plain)
    ref = oc.oracle(c, P)
    assert not ref.floors_hit
    return c, ref


def _codes(c):
    """Through glm_fused_codes, as GLMDriver does; tweedie by its link power."""
    if c.family == "tweedie":
        codes = linalg_ops.glm_fused_codes("tweedie", "tweedie", {"log": 0.0, "identity": 1.0}[c.link])
    else:
        codes = linalg_ops.glm_fused_codes(c.family, c.link)
    assert codes is not None
    return codes


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Spy:
    """Forwards to the gram library and keeps the arguments of h2o_glm_irls."""

    def __init__(self, lib):
        self._lib, self.irls_args = lib, None

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != "h2o_glm_irls":
            return f

        def call(*a):
            self.irls_args = a
            return f(*a)
        return call


def _run(route, c, **extra):
    """(G, deviance, gradient [P + 1] or None, full gradient vector or None) on the host."""
    P, Pp = route.P, route.Pp
    fam_kw = dict(codes=_codes(c), tvp=c.tvp, theta=c.theta)
    if route.kind in ("ws", "irls"):
        X = c.X[:, :P] if route.narrow else c.X
        grad = route.kind == "ws"
        out = linalg_ops.glm_irls(_cu(X), aug=P, beta=_cu(c.beta), b0=c.b0, y=_cu(c.y), wprior=_cu(c.w),
                                  offset=_cu(c.offset), width=Pp, grad=grad, **fam_kw, **route.kw, **extra)
        G, dev = out[0].cpu().numpy(), out[1].item()
        if not grad:
            return G, dev, None, None
        gv = out[2].cpu().numpy()
        assert gv.shape == (Pp + 1,)
        return G, dev, np.concatenate([gv[:P], gv[Pp:]]), gv[:Pp]
    fused = route.kind == "wide_fused"
    G, dev, gv = linalg_ops.glm_wide_irls(_cu(c.X[:, :P]), P, _cu(c.beta[:P]), c.b0, _cu(c.y), _cu(c.w),
                                          _cu(c.offset), fused=fused, **fam_kw, **route.kw, **extra)
    gv = gv.cpu().numpy()
    assert gv.shape == (-(-(P + 2) // 64) * 64,)
    return G.cpu().numpy(), dev.item(), gv[:P + 1], gv


def _check(route, c, ref, tag, G, dev, g, gv):
    P = route.P
    # the fused wide Gram carries no z column
    m = P + 1 if route.kind == "wide_fused" else P + 2
    e_g = oc.gram_error(G[:m, :m], ref.G[:m, :m])
    e_d = oc.dev_error(dev, ref.dev)
    e_r = None if g is None else oc.grad_error(g, ref.grad, c.X, c.y, c.w, P)
    asym = float(np.abs(G - G.T).max())
    print(f"ERR {route.name} {tag}: gram {e_g:.3e} (bound {route.bound:g}) dev {e_d:.3e} "
          f"grad {'n/a' if e_r is None else format(e_r, '.3e')} asym {asym:.3e}")
    assert np.isfinite(G).all() and np.isfinite(dev)
    assert e_g <= route.bound, e_g
    assert e_d <= DEV_BOUND, (dev, ref.dev)
    if g is not None:
        assert np.isfinite(gv).all()
        assert e_r <= GRAD_BOUND, e_r
        assert not gv[P + 1:].any() and (route.kind != "ws" or not gv[P:].any())   # padding carries no gradient
    assert np.array_equal(G, G.T)
    # nothing beyond the augmented block (for the fused wide Gram: an empty z slot)
    assert G.shape[0] >= P + 2 and not G[m:].any() and not G[:, m:].any()


FAM_IDS = [oc.family_id(f) for f in oc.FAMILY_SWEEP]


@pytest.mark.parametrize("plain", [False, True], ids=["w_off", "plain"])
@pytest.mark.parametrize("fam", oc.FAMILY_SWEEP, ids=FAM_IDS)
@pytest.mark.parametrize("route", FUSED_ROUTES, ids=repr)
def test_family_sweep(route, fam, plain):
    c, ref = _case(fam, plain, 200, route.P, route.Pp)
    _check(route, c, ref, f"{oc.family_id(fam)} {'plain' if plain else 'w_off'} n=200", *_run(route, c))


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("fam", ROW_FAMS, ids=[oc.family_id(f) for f in ROW_FAMS])
@pytest.mark.parametrize("route", FUSED_ROUTES, ids=repr)
def test_row_counts(route, fam, n, monkeypatch):
    """Below, at and just past one 64-row chunk, and the smallest row count
    that the default target_blocks cuts into two row splits."""
    c, ref = _case(fam, False, n, route.P, route.Pp)
    spy = _Spy(linalg_ops._lib())
    monkeypatch.setattr(linalg_ops, "_lib", lambda: spy)
    out = _run(route, c)
    if route.kind in ("ws", "irls"):
        n_splits, rpb = spy.irls_args[6], spy.irls_args[7]
        # the Hessian tier handed to the kernel: bf16x3 only from one 64-row chunk on
        want = route.kw.get("bf3", True)
        assert spy.irls_args[24] == (2 if want == "bf16" else int(bool(want) and n >= 64))
        assert n_splits == (2 if n > 8192 else 1) and n_splits * rpb >= n > (n_splits - 1) * rpb
    _check(route, c, ref, f"{oc.family_id(fam)} n={n}", *out)


@pytest.mark.parametrize("P,Pp", [(70, 96), (200, 224)])
def test_fused_call_at_other_widths_raises(P, Pp):
    """The fused kernels exist at power-of-two widths only: the entry point
    refuses (-3) before any launch and the wrapper raises."""
    c, _ = _case(ROW_FAMS[0], False, 200, P, Pp)
    with pytest.raises(RuntimeError, match="h2o_glm_irls failed: error -3"):
        linalg_ops.glm_irls(_cu(c.X), aug=P, beta=_cu(c.beta), b0=c.b0, y=_cu(c.y), wprior=_cu(c.w),
                            offset=_cu(c.offset), codes=_codes(c))


@pytest.mark.parametrize("P,Pp", [(200, 256), (400, 512)])
def test_gradient_channel_beyond_128_raises(P, Pp):
    """glm_irls_kernel has no exact-gradient channel (-6)."""
    c, _ = _case(ROW_FAMS[0], False, 200, P, Pp)
    with pytest.raises(RuntimeError, match="h2o_glm_irls failed: error -6"):
        linalg_ops.glm_irls(_cu(c.X), aug=P, beta=_cu(c.beta), b0=c.b0, y=_cu(c.y), wprior=_cu(c.w),
                            offset=_cu(c.offset), codes=_codes(c), grad=True)


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("name,P,Pp", EXTERNAL_ROUTES, ids=[r[0] for r in EXTERNAL_ROUTES])
def test_external_routes(name, P, Pp, signed, n, monkeypatch):
    """Caller-supplied W and z (the oracle's, of a poisson / log pass, rounded
    to f32); signed: every third weight negated.  With signed weights the
    error scale is the Gram of |W| (the bound on a product's absolute terms
    needs non-negative weights); for W >= 0 the two are the same."""
    c, ref = _case(ROW_FAMS[1], False, n, P, Pp)
    W, z = ref.W.astype(np.float32), ref.z.astype(np.float32)
    if signed:
        W[::3] *= -1.0
    spy = _Spy(linalg_ops._lib())
    monkeypatch.setattr(linalg_ops, "_lib", lambda: spy)
    G, dev = linalg_ops.glm_irls(_cu(c.X), aug=P, W=_cu(W), z=_cu(z))
    assert spy.irls_args[6] == (2 if n > 8192 else 1) and bool(spy.irls_args[20]) == bool((W < 0).any())
    assert spy.irls_args[24] == int(n >= 64)               # bf16x3 (Pp = 128, unsigned) from one chunk on
    G = G.cpu().numpy()
    Gr, Gabs = oc.external_gram(c.X, W, z, P)
    e_g = oc.gram_error(G[:P + 2, :P + 2], Gr, scale_from=Gabs)
    print(f"ERR {name} {'signed' if signed else 'unsigned'} n={n}: gram {e_g:.3e} (bound 2e-05) "
          f"asym {np.abs(G - G.T).max():.3e}")
    assert dev is None and np.isfinite(G).all()
    assert e_g <= 2e-5, e_g
    assert np.array_equal(G, G.T)
    assert not G[P + 2:].any() and not G[:, P + 2:].any()


@pytest.mark.parametrize("route", WS_ROUTES, ids=repr)
def test_saturated_binomial(route):
    """eta over [-30, 30], 1 % of the labels flipped.  Gram and gradient
    within the route's bounds; the deviance against the oracle evaluated with
    mu clamped to [1e-15, 1 - 2^-23] -- the kernel's own clamp of the f32 mean,
    the one constant the oracle takes from the kernel (oc.SAT_MU_CLAMP)."""
    c = oc.make_saturated_case(n=1000, P=route.P, Pp=route.Pp)
    ref = oc.oracle(c, route.P, mu_clamp=oc.SAT_MU_CLAMP)
    free = oc.oracle(c, route.P)
    print(f"SAT {route.name}: clamped deviance {ref.dev:.6f}, unclamped {free.dev:.6f}, "
          f"relative difference {abs(ref.dev - free.dev) / free.dev:.3e}")
    _check(route, c, ref, "saturated n=1000", *_run(route, c))
