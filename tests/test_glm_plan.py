"""The GLM IRLS plan: the switches record, the route a driver takes and the
precision-tier loop of `GLMDriver.step`.

No device and no compiled library is needed: routes are decided by a pure
function, and the tier loop runs on a driver whose statistics pass and kappa
estimators are scripted stubs (3 x 3 host systems).

The expected routes are read off the predicates this function replaced
(`GLMDriver._native`, `_irls_stats_native`, `_wide_eta_codes`, `_irls_stats`,
`_narrow_bf16_ok`, `_wide_bf16_ok`, `_tier_raise`, `linalg_ops.glm_grad_supported`);
each row names the one that decides it.  The expected tier-loop event lists were
recorded by running `_run_step` below, unchanged, on the commit before the three
loops (`_check_tier`, `_check_tier_dev`, `_step_dev`) were folded into
`_settle_tier`."""
import os
import re
import types

import numpy as np
import pytest
import torch

from h2o3_amd.models.glm import glm as glm_mod
from h2o3_amd.models.glm.glm import GLMDriver, GlmSwitches, IrlsRoute, irls_route
from h2o3_amd.ops import linalg_ops

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "h2o3_amd")
F32 = torch.float32
BINOMIAL = linalg_ops.glm_fused_codes("binomial", "logit")

# (what the row shows and which predicate decided it before,
#  environment, device, dtype, P, Pp, codes) -> (kind, grad, bf16_ok, tier0, wide_eta)
ROUTES = [
    ("cpu: _irls_stats, device test", {}, "cpu", F32, 100, 128, BINOMIAL, ("f64", True, False, "f64", False)),
    ("Pp 32: _native, glm_grad_supported, _tier_raise ws_bf3", {}, "cuda", F32, 30, 32, BINOMIAL,
     ("narrow_fused", True, False, "f32", False)),
    ("Pp 64: the same", {}, "cuda", F32, 60, 64, BINOMIAL, ("narrow_fused", True, False, "f32", False)),
    ("Pp 96: _irls_stats_native, power-of-two test", {}, "cuda", F32, 90, 96, BINOMIAL,
     ("narrow_external", False, False, "f32", False)),
    ("Pp 128: _narrow_bf16_ok", {}, "cuda", F32, 100, 128, BINOMIAL, ("narrow_fused", True, True, "bf16", False)),
    ("Pp 128 without room for the two augmented columns: _native", {}, "cuda", F32, 127, 128, BINOMIAL,
     ("generic", False, False, "f32", False)),
    ("f64 rows: _native", {}, "cuda", torch.float64, 100, 128, BINOMIAL, ("generic", False, False, "f32", False)),
    ("Pp 256, narrow_max 128: _irls_stats wide predicate, _wide_bf16_ok", {}, "cuda", F32, 200, 256, BINOMIAL,
     ("wide_fused", True, True, "bf16", True)),
    ("Pp 256, narrow_max 512: _native; glm_grad_supported false at 256", {"H2O3_GLM_NARROW_MAX": "512"}, "cuda", F32,
     200, 256, BINOMIAL, ("narrow_fused", False, False, "f32", False)),
    ("P + 2 = 1024: _irls_stats wide predicate", {}, "cuda", F32, 1022, 1024, BINOMIAL,
     ("wide_fused", True, True, "bf16", True)),
    ("P + 2 = 1025: _irls_stats falls to weighted_gram_aug", {}, "cuda", F32, 1023, 1056, BINOMIAL,
     ("wide_gemm", False, False, "f32", False)),
    ("unsupported family / link, narrow: _irls_stats_native external mode", {}, "cuda", F32, 100, 128, None,
     ("narrow_external", False, False, "bf3", False)),
    ("unsupported family / link, wide: _irls_stats falls to weighted_gram_aug", {}, "cuda", F32, 600, 640, None,
     ("wide_gemm", False, False, "f32", False)),
    # every switch flipped once
    ("H2O3_GLM_BF16=0: _narrow_bf16_ok", {"H2O3_GLM_BF16": "0"}, "cuda", F32, 100, 128, BINOMIAL,
     ("narrow_fused", True, False, "bf3", False)),
    ("H2O3_GLM_BF3=0: _narrow_bf16_ok, _tier_raise ws_bf3", {"H2O3_GLM_BF3": "0"}, "cuda", F32, 100, 128, BINOMIAL,
     ("narrow_fused", True, False, "f32", False)),
    ("H2O3_GLM_EXACT_GRAD=0 narrow: glm_grad_supported", {"H2O3_GLM_EXACT_GRAD": "0"}, "cuda", F32, 100, 128,
     BINOMIAL, ("narrow_fused", False, False, "bf3", False)),
    ("H2O3_GLM_EXACT_GRAD=0 wide: _irls_stats `fused`; _wide_eta_codes does not ask for it",
     {"H2O3_GLM_EXACT_GRAD": "0"}, "cuda", F32, 600, 640, BINOMIAL, ("wide_split", False, False, "f32", True)),
    ("H2O3_GLM_WIDE_FUSED=0: _irls_stats `fused`, _wide_eta_codes, _wide_bf16_ok", {"H2O3_GLM_WIDE_FUSED": "0"},
     "cuda", F32, 600, 640, BINOMIAL, ("wide_split", True, False, "bf3", False)),
    ("H2O3_GLM_WIDE_BF16=0: _wide_bf16_ok", {"H2O3_GLM_WIDE_BF16": "0"}, "cuda", F32, 600, 640, BINOMIAL,
     ("wide_fused", True, False, "bf3", True)),
    ("H2O3_WIDE_TILE=128: _wide_bf16_ok", {"H2O3_WIDE_TILE": "128"}, "cuda", F32, 600, 640, BINOMIAL,
     ("wide_fused", True, False, "bf3", True)),
    ("H2O3_WIDE_GRAM=f32: _irls_stats wide predicate (_wide_mode)", {"H2O3_WIDE_GRAM": "f32"}, "cuda", F32, 600, 640,
     BINOMIAL, ("wide_gemm", False, False, "f32", False)),
    # switches that choose launch shapes or solvers, not the route
    ("H2O3_GLM_DEV_SOLVE=0", {"H2O3_GLM_DEV_SOLVE": "0"}, "cuda", F32, 600, 640, BINOMIAL,
     ("wide_fused", True, True, "bf16", True)),
    ("H2O3_GLM_TIERS=0", {"H2O3_GLM_TIERS": "0"}, "cuda", F32, 100, 128, BINOMIAL,
     ("narrow_fused", True, True, "bf16", False)),
    ("H2O3_GLM_F64_MFMA=0", {"H2O3_GLM_F64_MFMA": "0"}, "cuda", F32, 100, 128, BINOMIAL,
     ("narrow_fused", True, True, "bf16", False)),
    ("H2O3_WIDE_SLICES / ETA_BLOCKS / GROUP / OVERLAP, H2O3_GI_BLOCKS",
     {"H2O3_WIDE_SLICES": "8", "H2O3_WIDE_ETA_BLOCKS": "512", "H2O3_WIDE_GROUP": "2", "H2O3_WIDE_OVERLAP": "1",
      "H2O3_GI_BLOCKS": "512"}, "cuda", F32, 600, 640, BINOMIAL, ("wide_fused", True, True, "bf16", True)),
]


@pytest.mark.parametrize("why,env,device,dtype,P,Pp,codes,want", ROUTES, ids=[r[0].split(":")[0] for r in ROUTES])
def test_route_table(why, env, device, dtype, P, Pp, codes, want):
    rt = irls_route(GlmSwitches.from_env(env), device, dtype, P, Pp, codes)
    assert isinstance(rt, IrlsRoute)
    assert (rt.kind, rt.grad, rt.bf16_ok, rt.tier0, rt.wide_eta) == want, why
    assert rt.codes == (codes if rt.kind in ("narrow_fused", "wide_fused", "wide_split") else None)


def test_switch_defaults_and_reader():
    d = GlmSwitches.from_env({})
    assert d == GlmSwitches() == GlmSwitches(
        narrow_max=128, bf16=True, bf3=True, wide_bf16=True, dev_solve=True, exact_grad=True, f64_mfma=True,
        tiers=True, wide_fused=True, wide_gram="bf3", wide_tile=256, wide_slices=0, wide_eta_blocks=0, wide_group=4,
        wide_overlap=False, gi_blocks=1024)
    flipped = GlmSwitches.from_env({
        "H2O3_GLM_NARROW_MAX": "512", "H2O3_GLM_BF16": "0", "H2O3_GLM_BF3": "0", "H2O3_GLM_WIDE_BF16": "0",
        "H2O3_GLM_DEV_SOLVE": "0", "H2O3_GLM_EXACT_GRAD": "0", "H2O3_GLM_F64_MFMA": "0", "H2O3_GLM_TIERS": "0",
        "H2O3_GLM_WIDE_FUSED": "0", "H2O3_WIDE_GRAM": "f32", "H2O3_WIDE_TILE": "128", "H2O3_WIDE_SLICES": "8",
        "H2O3_WIDE_ETA_BLOCKS": "512", "H2O3_WIDE_GROUP": "2", "H2O3_WIDE_OVERLAP": "1", "H2O3_GI_BLOCKS": "512"})
    assert flipped == GlmSwitches(512, False, False, False, False, False, False, False, False, "f32", 128, 8, 512, 2,
                                  True, 512)
    with pytest.raises(AttributeError):      # frozen
        d.bf3 = False


def test_driver_reads_switches_once(monkeypatch):
    from h2o3_amd.core.frame import H2OFrame
    from h2o3_amd.models.base import TrainSpec
    from h2o3_amd.models.glm.glm import H2OGeneralizedLinearEstimator
    g = np.random.default_rng(0)
    X = g.standard_normal((200, 3))
    fr = H2OFrame({"a": X[:, 0], "b": X[:, 1], "c": X[:, 2], "y": X @ [1.0, -1.0, 0.5] + 0.1 * g.standard_normal(200)})
    monkeypatch.setenv("H2O3_GLM_TIERS", "0")
    monkeypatch.delenv("H2O3_WIDE_TILE", raising=False)
    est = H2OGeneralizedLinearEstimator(family="gaussian", lambda_=0.0)
    spec = TrainSpec(fr, ["a", "b", "c"], "y")
    est._spec = spec
    drv = GLMDriver(est, spec)
    assert drv.sw == GlmSwitches.from_env() and drv.sw.tiers is False and drv.sw.wide_tile == 256
    before, route = drv.sw, drv.route
    monkeypatch.setenv("H2O3_GLM_TIERS", "1")
    monkeypatch.setenv("H2O3_WIDE_TILE", "128")
    drv.step()
    assert drv.sw is before and drv.sw.tiers is False and drv.sw.wide_tile == 256 and drv.route is route
    assert GLMDriver(est, spec).sw == GlmSwitches.from_env() != before


# ---- the tier loop -------------------------------------------------------------------------------------------

def _run_step(flavour, Pp, hprec, it, kappas, l1):
    """One `step()` of a driver built without a frame: 2 coefficients and an
    intercept, the statistics pass and the three kappa sources stubbed.  The
    k-th statistics pass returns the system (k + 1) I, so every event can say
    which statistics it saw.  Events, in order:
      ("stats", tier, on device)           a statistics pass at that tier
      ("kappa", source, diagonal)          a condition estimate of that matrix (ridge included)
      ("solve", where, solution, deviance) the step taken (it names the system that was solved: the k-th is
                                           (k + 1) I), and the deviance reported with it
    and last ("end", tier, kappa)."""
    P = 2
    ev = []
    drv = GLMDriver.__new__(GLMDriver)
    wide = Pp > 128
    drv.X = types.SimpleNamespace(device=types.SimpleNamespace(type="cuda"), dtype=F32)
    drv.P, drv.Pp, drv.iter, drv._hprec, drv.hessian_kappa = P, Pp, it, hprec, None
    drv.lam, drv.alpha = (0.25, 0.5) if l1 else (0.25, 0.0)
    drv.obj_reg, drv.intercept, drv.rho, drv.active, drv.lower, drv.upper = 1.0, True, None, None, None, None
    drv.est = types.SimpleNamespace(_parms={}, _gam_penalty=None)
    drv.beta = np.zeros(P + 1)
    if hasattr(glm_mod, "irls_route"):
        drv.sw = GlmSwitches()
        drv.route = irls_route(drv.sw, "cuda", F32, P, Pp, BINOMIAL)
        assert drv.route.kind == ("wide_fused" if wide else "narrow_fused")
    count = [0]

    def stats(*a):
        on_dev = a[0] if a else getattr(drv, "_sys_on_dev", False)
        ev.append(("stats", drv._hprec, bool(on_dev)))
        drv._gexact = object()                         # both routes carry the gradient channel
        count[0] += 1
        Ga, b = np.eye(P + 1) * (count[0] + 1), np.ones(P + 1)
        return (torch.as_tensor(Ga), torch.as_tensor(b), 100.0 + count[0]) if on_dev else (Ga, b, 100.0 + count[0])

    def kappa(source):
        def fn(A, *rest):
            ev.append(("kappa", source, tuple(float(v) for v in np.asarray(torch.as_tensor(A).diagonal()))))
            return kappas.pop(0)
        return fn

    solve_dev, where = drv._step_solve_dev, ["host"]

    def step_solve_dev(Gn, bn, l2, L, info):
        # the factor belongs to the system being solved
        assert torch.equal(L, torch.linalg.cholesky(Gn + torch.diag(torch.tensor([l2, l2, 0.0], dtype=Gn.dtype))))
        where[0] = "device"
        return solve_dev(Gn, bn, l2, L, info)

    def finish(new, gmax, dev, l1_, l2):
        ev.append(("solve", where[0], tuple(float(v) for v in np.round(new, 6)), dev))
        return 0.0

    drv._irls_stats = stats
    drv._scaled_cond, drv._scaled_cond_dev, drv._kappa_from_factor = kappa("host"), kappa("dev"), kappa("factor")
    drv._step_solve_dev, drv._finish_step = step_solve_dev, finish
    drv._dev_system_ok = lambda: flavour == "dev_solve"
    drv._dev_tier_ok = lambda: flavour == "dev_tier"
    drv.step()
    assert not kappas, "unused kappa estimates"
    return ev + [("end", drv._hprec, drv.hessian_kappa)]


INF = float("inf")
# scenario -> (Pp, tier before, iterations done, scripted kappas)
SCENARIOS = {
    "stay": (128, None, 0, [10.0]),
    "not_due": (128, "bf16", 2, []),
    "bf16_to_bf3": (128, None, 0, [100.0, 100.0]),
    "bf3_to_f32_to_f64": (128, "bf3", 1, [1e4, 1e6]),
    "wide_bf3_to_f64": (256, "bf3", 1, [1e4]),
    "wide_bf16_to_bf3": (256, None, 0, [100.0, 1000.0]),
    "cholesky_failed": (128, None, 0, [INF]),
}
EXPECTED = {('bf16_to_bf3', 'dev_solve'): [('stats', None, True),
                                ('kappa', 'factor', (2.25, 2.25, 2.0)),
                                ('stats', 'bf3', True),
                                ('kappa', 'factor', (3.25, 3.25, 3.0)),
                                ('solve', 'device', (0.307692, 0.307692, 0.333333), 102.0),
                                ('end', 'bf3', 100.0)],
 ('bf16_to_bf3', 'dev_tier'): [('stats', None, True),
                               ('kappa', 'dev', (2.125, 2.125, 2.0)),
                               ('stats', 'bf3', True),
                               ('kappa', 'dev', (3.125, 3.125, 3.0)),
                               ('solve', 'host', (0.28, 0.28, 0.333333), 102.0),
                               ('end', 'bf3', 100.0)],
 ('bf16_to_bf3', 'host'): [('stats', None, False),
                           ('kappa', 'host', (2.25, 2.25, 2.0)),
                           ('stats', 'bf3', False),
                           ('kappa', 'host', (3.25, 3.25, 3.0)),
                           ('solve', 'host', (0.307692, 0.307692, 0.333333), 102.0),
                           ('end', 'bf3', 100.0)],
 ('bf3_to_f32_to_f64', 'dev_solve'): [('stats', 'bf3', True),
                                      ('kappa', 'factor', (2.25, 2.25, 2.0)),
                                      ('stats', 'f32', True),
                                      ('kappa', 'factor', (3.25, 3.25, 3.0)),
                                      ('stats', 'f64', True),
                                      ('solve', 'device', (0.235294, 0.235294, 0.25), 103.0),
                                      ('end', 'f64', 1000000.0)],
 ('bf3_to_f32_to_f64', 'dev_tier'): [('stats', 'bf3', True),
                                     ('kappa', 'dev', (2.125, 2.125, 2.0)),
                                     ('stats', 'f32', True),
                                     ('kappa', 'dev', (3.125, 3.125, 3.0)),
                                     ('stats', 'f64', True),
                                     ('solve', 'host', (0.212121, 0.212121, 0.25), 103.0),
                                     ('end', 'f64', 1000000.0)],
 ('bf3_to_f32_to_f64', 'host'): [('stats', 'bf3', False),
                                 ('kappa', 'host', (2.25, 2.25, 2.0)),
                                 ('stats', 'f32', False),
                                 ('kappa', 'host', (3.25, 3.25, 3.0)),
                                 ('stats', 'f64', False),
                                 ('solve', 'host', (0.235294, 0.235294, 0.25), 103.0),
                                 ('end', 'f64', 1000000.0)],
 ('cholesky_failed', 'dev_solve'): [('stats', None, True),
                                    ('kappa', 'factor', (2.25, 2.25, 2.0)),
                                    ('stats', 'f64', True),
                                    ('solve', 'device', (0.307692, 0.307692, 0.333333), 102.0),
                                    ('end', 'f64', INF)],
 ('cholesky_failed', 'dev_tier'): [('stats', None, True),
                                   ('kappa', 'dev', (2.125, 2.125, 2.0)),
                                   ('stats', 'f64', True),
                                   ('solve', 'host', (0.28, 0.28, 0.333333), 102.0),
                                   ('end', 'f64', INF)],
 ('cholesky_failed', 'host'): [('stats', None, False),
                               ('kappa', 'host', (2.25, 2.25, 2.0)),
                               ('stats', 'f64', False),
                               ('solve', 'host', (0.307692, 0.307692, 0.333333), 102.0),
                               ('end', 'f64', INF)],
 ('not_due', 'dev_solve'): [('stats', 'bf16', True),
                            ('solve', 'device', (0.444444, 0.444444, 0.5), 101.0),
                            ('end', 'bf16', None)],
 ('not_due', 'dev_tier'): [('stats', 'bf16', True),
                           ('solve', 'host', (0.411765, 0.411765, 0.5), 101.0),
                           ('end', 'bf16', None)],
 ('not_due', 'host'): [('stats', 'bf16', False),
                       ('solve', 'host', (0.444444, 0.444444, 0.5), 101.0),
                       ('end', 'bf16', None)],
 ('stay', 'dev_solve'): [('stats', None, True),
                         ('kappa', 'factor', (2.25, 2.25, 2.0)),
                         ('solve', 'device', (0.444444, 0.444444, 0.5), 101.0),
                         ('end', 'bf16', 10.0)],
 ('stay', 'dev_tier'): [('stats', None, True),
                        ('kappa', 'dev', (2.125, 2.125, 2.0)),
                        ('solve', 'host', (0.411765, 0.411765, 0.5), 101.0),
                        ('end', 'bf16', 10.0)],
 ('stay', 'host'): [('stats', None, False),
                    ('kappa', 'host', (2.25, 2.25, 2.0)),
                    ('solve', 'host', (0.444444, 0.444444, 0.5), 101.0),
                    ('end', 'bf16', 10.0)],
 ('wide_bf16_to_bf3', 'dev_solve'): [('stats', None, True),
                                     ('kappa', 'factor', (2.25, 2.25, 2.0)),
                                     ('stats', 'bf3', True),
                                     ('kappa', 'factor', (3.25, 3.25, 3.0)),
                                     ('solve', 'device', (0.307692, 0.307692, 0.333333), 102.0),
                                     ('end', 'bf3', 1000.0)],
 ('wide_bf16_to_bf3', 'dev_tier'): [('stats', None, True),
                                    ('kappa', 'dev', (2.125, 2.125, 2.0)),
                                    ('stats', 'bf3', True),
                                    ('kappa', 'dev', (3.125, 3.125, 3.0)),
                                    ('solve', 'host', (0.28, 0.28, 0.333333), 102.0),
                                    ('end', 'bf3', 1000.0)],
 ('wide_bf16_to_bf3', 'host'): [('stats', None, False),
                                ('kappa', 'host', (2.25, 2.25, 2.0)),
                                ('stats', 'bf3', False),
                                ('kappa', 'host', (3.25, 3.25, 3.0)),
                                ('solve', 'host', (0.307692, 0.307692, 0.333333), 102.0),
                                ('end', 'bf3', 1000.0)],
 ('wide_bf3_to_f64', 'dev_solve'): [('stats', 'bf3', True),
                                    ('kappa', 'factor', (2.25, 2.25, 2.0)),
                                    ('stats', 'f64', True),
                                    ('solve', 'device', (0.307692, 0.307692, 0.333333), 102.0),
                                    ('end', 'f64', 10000.0)],
 ('wide_bf3_to_f64', 'dev_tier'): [('stats', 'bf3', True),
                                   ('kappa', 'dev', (2.125, 2.125, 2.0)),
                                   ('stats', 'f64', True),
                                   ('solve', 'host', (0.28, 0.28, 0.333333), 102.0),
                                   ('end', 'f64', 10000.0)],
 ('wide_bf3_to_f64', 'host'): [('stats', 'bf3', False),
                               ('kappa', 'host', (2.25, 2.25, 2.0)),
                               ('stats', 'f64', False),
                               ('solve', 'host', (0.307692, 0.307692, 0.333333), 102.0),
                               ('end', 'f64', 10000.0)]}


@pytest.mark.parametrize("flavour", ["host", "dev_tier", "dev_solve"])
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_tier_loop_events(scenario, flavour):
    Pp, hprec, it, kappas = SCENARIOS[scenario]
    ev = _run_step(flavour, Pp, hprec, it, list(kappas), l1=flavour == "dev_tier")
    assert ev == EXPECTED[scenario, flavour]


# ---- source text ---------------------------------------------------------------------------------------------

def test_no_environment_reads_outside_the_switches():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    assert "getenv" not in read("ops", "csrc", "gram.hip")
    assert "os.environ" not in read("ops", "linalg_ops.py") and "getenv" not in read("ops", "linalg_ops.py")
    src = read("models", "glm", "glm.py")
    start = src.index("class GlmSwitches")
    end = src.index("\nclass ", start + 1)
    outside = src[:start] + src[end:]
    assert "os.environ" in src[start:end]
    assert "os.environ" not in outside and not re.search(r"\bgetenv\b", outside)
    assert not re.search(r"H2O3_(GLM|WIDE|GI|WG2)_\w+", outside)
