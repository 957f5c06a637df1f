"""The GBM boosting plan: the switches record and the route a driver takes.

No device and no compiled library is needed: the route is decided by a pure
function of the switches and plain facts.

The expected routes are read off the predicates this function replaced in
`GBMDriver.step` (`simple`, `posleaf`, `onepass`, the device-sums test of the
gamma pass, the multinomial condition) and off `devtree.supported`; each row
names the one that decides it."""
import inspect
import os
import re

import numpy as np
import pytest

from h2o3_amd.models.tree import devtree, gbm
from h2o3_amd.models.tree.gbm import GBMDriver, GbmRoute, GbmSwitches, gbm_route

OFF = "disabled (H2O3_DEV_TREE=0)"
# facts of a driver: device, K, family, link, monotone, noise bandwidth, 0/1 weights, payload path, devtree.supported
BERN = dict(device="cuda", K=1, family="bernoulli", link="logit", mono_on=False, noise_bw=0.0, base_unit=True,
            payload_ok=True, why=OFF)
GAUSS = dict(BERN, family="gaussian", link="identity")
MULTI = dict(BERN, K=3, family="multinomial", link="softmax", why="distribution")

# (what the row shows and which predicate decided it before, environment, facts) -> kind
ROUTES = [
    # one row per kind
    ("devtree: step's `K == 1 and _devtree_ok()`, devtree.supported is None", {}, dict(BERN, why=None), "devtree"),
    ("onepass: `onepass` = posleaf and _base_unit and pos_payload_ok and H2O3_GBM_GRAD", {}, BERN, "onepass"),
    ("posleaf: `posleaf` = simple and H2O3_POS_LEAF; `onepass` false without the payload path", {},
     dict(BERN, payload_ok=False), "posleaf"),
    ("leaf_pass: `simple` false with prediction noise; the gamma pass's device-sums test holds", {},
     dict(GAUSS, noise_bw=0.5, why="constraints / prediction noise"), "leaf_pass"),
    ("host: the device-sums test fails for poisson", {}, dict(BERN, family="poisson", link="log", why="distribution"),
     "host"),
    ("multi_dev: the multinomial condition of step", {}, MULTI, "multi_dev"),
    ("multi_host: the multinomial condition, no GPU", {}, dict(MULTI, device="cpu", why="no GPU"), "multi_host"),
    # every switch flipped once
    ("H2O3_DEV_TREE=0: devtree.supported answers `disabled`", {"H2O3_DEV_TREE": "0"}, GAUSS, "onepass"),
    ("H2O3_POS_LEAF=0: `posleaf`", {"H2O3_POS_LEAF": "0"}, BERN, "leaf_pass"),
    ("H2O3_POS_LEAF=0, K = 3: the multinomial condition", {"H2O3_POS_LEAF": "0"}, MULTI, "multi_host"),
    ("H2O3_GBM_GRAD=0: `onepass`", {"H2O3_GBM_GRAD": "0"}, BERN, "posleaf"),
    # switches that choose a launch or an update inside a route, not the route
    ("H2O3_LEAF_SCATTER=0: _scatter_ok, inside onepass", {"H2O3_LEAF_SCATTER": "0"}, BERN, "onepass"),
    ("H2O3_LEAF_SCATTER=0, K = 3: _scatter_ok, inside multi_dev", {"H2O3_LEAF_SCATTER": "0"}, MULTI, "multi_dev"),
    ("H2O3_DEV_TREE_GRAPH=0: DevTreeGBM.run", {"H2O3_DEV_TREE_GRAPH": "0"}, dict(BERN, why=None), "devtree"),
    ("H2O3_LEAF_GATHER=0 H2O3_DEV_LAST_LEVEL=0: DevTreeGBM.__init__",
     {"H2O3_LEAF_GATHER": "0", "H2O3_DEV_LAST_LEVEL": "0"}, dict(BERN, why=None), "devtree"),
    # interactions
    ("monotone on with bernoulli: `simple` false, so not posleaf", {},
     dict(BERN, mono_on=True, why="constraints / prediction noise"), "leaf_pass"),
    ("non-0/1 weights: `onepass` needs _base_unit, `posleaf` does not", {},
     dict(BERN, base_unit=False, why="row weights other than 0/1"), "posleaf"),
    ("K > 1 with noise: the multinomial condition", {}, dict(MULTI, noise_bw=0.5), "multi_host"),
    ("K > 1 with non-0/1 weights: the multinomial condition", {}, dict(MULTI, base_unit=False), "multi_host"),
    ("K > 1 without the payload path: the multinomial condition", {}, dict(MULTI, payload_ok=False), "multi_host"),
    ("K > 1 never asks devtree.supported: step tests K first", {}, dict(MULTI, why=None), "multi_dev"),
    ("no GPU, bernoulli: `simple` and the device-sums test both need cuda", {}, dict(BERN, device="cpu", why="no GPU"),
     "host"),
    ("monotone on with H2O3_GBM_GRAD=0 stays leaf_pass", {"H2O3_GBM_GRAD": "0"},
     dict(GAUSS, mono_on=True, why="constraints / prediction noise"), "leaf_pass"),
    ("an offset: devtree.supported answers `offset`, the level loop's onepass serves", {}, dict(BERN, why="offset"),
     "onepass"),
    ("laplace on the GPU: the device-sums test fails", {},
     dict(GAUSS, family="laplace", why="distribution"), "host"),
]


@pytest.mark.parametrize("why,env,facts,want", ROUTES, ids=[r[0].split(":")[0] for r in ROUTES])
def test_route_table(why, env, facts, want):
    f = facts
    rt = gbm_route(GbmSwitches.from_env(env), f["device"], f["K"], f["family"], f["link"], f["mono_on"],
                   f["noise_bw"], f["base_unit"], f["payload_ok"], f["why"])
    assert isinstance(rt, GbmRoute)
    assert rt.kind == want, why
    assert rt.devtree_why == (None if want == "devtree" else f["why"])


def test_route_kinds_are_all_tabled():
    assert {r[3] for r in ROUTES} == {"devtree", "onepass", "posleaf", "leaf_pass", "host", "multi_dev", "multi_host"}


def test_switch_defaults_and_reader():
    d = GbmSwitches.from_env({})
    assert d == GbmSwitches() == GbmSwitches(dev_tree=True, dev_tree_graph=True, leaf_gather=True,
                                             dev_last_level=True, pos_leaf=True, gbm_grad=True, leaf_scatter=True)
    flipped = GbmSwitches.from_env({
        "H2O3_DEV_TREE": "0", "H2O3_DEV_TREE_GRAPH": "0", "H2O3_LEAF_GATHER": "0", "H2O3_DEV_LAST_LEVEL": "0",
        "H2O3_POS_LEAF": "0", "H2O3_GBM_GRAD": "0", "H2O3_LEAF_SCATTER": "0"})
    assert flipped == GbmSwitches(False, False, False, False, False, False, False)
    with pytest.raises(AttributeError):      # frozen
        d.pos_leaf = False


def test_driver_reads_switches_once_and_declares_its_state(monkeypatch):
    from h2o3_amd.core.frame import H2OFrame
    from h2o3_amd.models.base import TrainSpec
    from h2o3_amd.models.tree.gbm import H2OGradientBoostingEstimator
    g = np.random.default_rng(0)
    X = g.standard_normal((300, 3))
    fr = H2OFrame({"a": X[:, 0], "b": X[:, 1], "c": X[:, 2], "y": X @ [1.0, -1.0, 0.5] + 0.1 * g.standard_normal(300)})
    monkeypatch.setenv("H2O3_LEAF_SCATTER", "0")
    monkeypatch.delenv("H2O3_POS_LEAF", raising=False)
    est = H2OGradientBoostingEstimator(ntrees=3, max_depth=3, seed=1)
    spec = TrainSpec(fr, ["a", "b", "c"], "y")
    est._spec = spec
    drv = GBMDriver(est, spec)
    assert drv.sw == GbmSwitches.from_env() and drv.sw.leaf_scatter is False and drv.sw.pos_leaf is True
    declared = set(vars(drv))
    before, route = drv.sw, drv.route
    monkeypatch.setenv("H2O3_LEAF_SCATTER", "1")
    monkeypatch.setenv("H2O3_POS_LEAF", "0")
    drv.step()
    drv.step()
    assert drv.sw is before and drv.route is route and len(drv.forest) == 2
    assert set(vars(drv)) == declared            # a step adds no attribute
    # where a GPU serves this frame the route is the device tree, built by the first step
    assert (drv._devtree is not None) == (route.kind == "devtree") == (route.devtree_why is None)
    assert drv._devtree_why == route.devtree_why
    assert GBMDriver(est, spec).sw == GbmSwitches.from_env() != before


# ---- source text ---------------------------------------------------------------------------------------------

def test_no_environment_reads_or_undeclared_state_in_the_drivers():
    bad = re.compile(r"os\.environ|getenv|__dict__|getattr\(self, \"_|hasattr\(self")
    assert not bad.search(inspect.getsource(GBMDriver))
    assert not bad.search(inspect.getsource(devtree.DevTreeGBM))
    assert "os.environ" in inspect.getsource(GbmSwitches.from_env)
    src = inspect.getsource(gbm)
    assert src.count("os.environ") == 1
    # the switches are named in the record alone
    names = "H2O3_(DEV_TREE|DEV_TREE_GRAPH|LEAF_GATHER|DEV_LAST_LEVEL|POS_LEAF|GBM_GRAD|LEAF_SCATTER|FUSED_LEAF)\\b"
    start = src.index("class GbmSwitches")
    end = src.index("\nclass ", start + 1)
    assert not re.search(names, src[:start] + src[end:])
    dsrc = inspect.getsource(devtree)
    assert "os.environ" not in dsrc and not re.search(r"^import os$", dsrc, re.M)
