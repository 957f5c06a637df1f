"""Dump what the GBM boosting driver computes, one .npz entry set per case, to
compare two commits bit for bit:

    python scripts/gbm_route_dump.py OUT.npz [case-name filter]
    python scripts/gbm_route_dump.py --compare A.npz B.npz

Each case drives GBMDriver for a few trees on a small seeded frame and saves
every tree's arrays, init_f and drv.f.  Without a GPU the cases cover the
distributions and options of the host routes; with one, each route kind of
gbm.gbm_route and every switch of GbmSwitches flipped once.  Under a launcher
that sets RANK / WORLD_SIZE every rank runs the cases and rank 0 writes.

Compare two dumps of the same commit first: the device-resident tree sums its
leaf statistics with f64 atomics, so a leaf value of a `devtree_*` case can move
in its last bit between two runs of one build (drv.f, float32, does not)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

TREE_ARRAYS = ("feat", "left", "right", "thr", "na_left", "value", "weight")
NUM = [f"x{j}" for j in range(16)]
MONO = {"x0": 1, "x1": -1}
LEVEL_LOOP = {"H2O3_DEV_TREE": "0"}
# name -> (response, estimator parameters, environment, TrainSpec keywords)
CPU_CASES = {
    "gaussian": ("yr", {}, {}, {}),
    "bernoulli": ("yb", {}, {}, {}),
    "poisson": ("yc", dict(distribution="poisson"), {}, {}),
    "laplace": ("yr", dict(distribution="laplace"), {}, {}),
    "quantile": ("yr", dict(distribution="quantile", quantile_alpha=0.3), {}, {}),
    "huber": ("yr", dict(distribution="huber"), {}, {}),
    "multinomial": ("ym", {}, {}, {}),
    "monotone": ("yr", dict(monotone_constraints=MONO), {}, {}),
    "monotone_bernoulli": ("yb", dict(monotone_constraints=MONO), {}, {}),
    "noise": ("yr", dict(pred_noise_bandwidth=0.5), {}, {}),
    "noise_multinomial": ("ym", dict(pred_noise_bandwidth=0.5), {}, {}),
    "sample_rate": ("yb", dict(sample_rate=0.7), {}, {}),
    "sample_rate_per_class": ("yb", dict(sample_rate_per_class=[0.6, 0.9]), {}, {}),
    "col_per_tree": ("yb", dict(col_sample_rate_per_tree=0.6), {}, {}),
    "col_per_level": ("yb", dict(col_sample_rate=0.6, col_sample_rate_change_per_level=0.9), {}, {}),
    "offset": ("yb", {}, {}, dict(offset="off")),
    "weights": ("yr", {}, {}, dict(weights="wt")),
    "annealing_maxabs": ("yb", dict(learn_rate_annealing=0.9, max_abs_leafnode_pred=0.05), {}, {}),
    "checkpoint": ("yb", dict(resume=True), {}, {}),
}
GPU_CASES = {
    "devtree_bernoulli": ("yb", {}, {}, {}),
    "devtree_gaussian": ("yr", {}, {}, {}),
    "devtree_no_graph": ("yb", {}, {"H2O3_DEV_TREE_GRAPH": "0"}, {}),
    "devtree_scatter": ("yb", {}, {"H2O3_LEAF_GATHER": "0", "H2O3_DEV_LAST_LEVEL": "0"}, {}),
    "devtree_row_sampling": ("yb", dict(sample_rate=0.7), {}, {}),
    "devtree_col_sampling": ("yb", dict(col_sample_rate=0.7, col_sample_rate_per_tree=0.8), {}, {}),
    "devtree_sampling": ("yb", dict(sample_rate=0.7, col_sample_rate=0.7, col_sample_rate_per_tree=0.8), {}, {}),
    "devtree_checkpoint": ("yb", dict(resume=True), {}, {}),
    "onepass": ("yb", {}, LEVEL_LOOP, {}),
    "onepass_gaussian": ("yr", {}, LEVEL_LOOP, {}),
    "onepass_sampling": ("yb", dict(sample_rate=0.7), LEVEL_LOOP, {}),
    "onepass_no_scatter": ("yb", {}, dict(LEVEL_LOOP, H2O3_LEAF_SCATTER="0"), {}),
    "posleaf_no_grad": ("yb", {}, dict(LEVEL_LOOP, H2O3_GBM_GRAD="0"), {}),
    "leaf_pass_no_posleaf": ("yb", {}, dict(LEVEL_LOOP, H2O3_POS_LEAF="0"), {}),
    "posleaf_weights": ("yb", {}, {}, dict(weights="wt")),
    "leaf_pass_monotone": ("yb", dict(monotone_constraints=MONO), {}, {}),
    "leaf_pass_noise": ("yr", dict(pred_noise_bandwidth=0.5), {}, {}),
    "host_poisson": ("yc", dict(distribution="poisson"), {}, {}),
    "host_huber": ("yr", dict(distribution="huber"), {}, {}),
    "onepass_offset": ("yb", {}, {}, dict(offset="off")),
    "multi_dev": ("ym", {}, {}, {}),
    "multi_dev_no_scatter": ("ym", {}, {"H2O3_LEAF_SCATTER": "0"}, {}),
    "multi_host_no_posleaf": ("ym", {}, {"H2O3_POS_LEAF": "0"}, {}),
    "multi_host_noise": ("ym", dict(pred_noise_bandwidth=0.5), {}, {}),
}
SWITCHES = ("H2O3_DEV_TREE", "H2O3_DEV_TREE_GRAPH", "H2O3_LEAF_GATHER", "H2O3_DEV_LAST_LEVEL", "H2O3_POS_LEAF",
            "H2O3_GBM_GRAD", "H2O3_LEAF_SCATTER")


def frame(n):
    from h2o3_amd.core.frame import H2OFrame
    g = np.random.default_rng(17)
    X = g.standard_normal((n, 16)).astype(np.float32)
    eta = X[:, 0] - 0.7 * X[:, 1] + 0.5 * np.sin(2 * X[:, 2]) * X[:, 3]
    cols = {f"x{j}": X[:, j] for j in range(16)}
    cols["yr"] = eta + 0.3 * g.standard_normal(n)
    cols["yb"] = (g.random(n) < 1 / (1 + np.exp(-eta))).astype(int)
    cols["yc"] = g.poisson(np.exp(0.4 * eta)).astype(np.float64)
    cols["ym"] = np.digitize(eta + 0.3 * g.standard_normal(n), [-0.6, 0.6])
    cols["off"] = 0.2 * X[:, 4].astype(np.float64)
    cols["wt"] = g.integers(0, 4, n) * 0.5
    fr = H2OFrame(cols)
    for c in ("yb", "ym"):
        fr[c] = fr[c].asfactor()
    return fr


def run_case(fr, y, parms, env, spec_kw, ntrees=4):
    from h2o3_amd.models.base import TrainSpec
    from h2o3_amd.models.tree.gbm import GBMDriver, H2OGradientBoostingEstimator
    parms = dict(parms)
    resume = parms.pop("resume", False)
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        kw = dict(max_depth=4, seed=7, ignore_const_cols=False, histogram_type="QuantilesGlobal", nbins=255, **parms)
        prev = None
        if resume:
            prev = H2OGradientBoostingEstimator(ntrees=2, **kw)
            prev.train(x=NUM, y=y, training_frame=fr)
            kw["checkpoint"] = prev
        est = H2OGradientBoostingEstimator(ntrees=ntrees, **kw)
        spec = TrainSpec(fr, NUM, y, **spec_kw)
        est._spec = spec
        drv = GBMDriver(est, spec)
        if resume:
            est._K = drv.K
            est._resume_from(drv, prev)
        while drv.iter < ntrees:
            drv.step()
        out = {"init_f": np.asarray(drv.init_f, dtype=np.float64), "f": drv.f.detach().cpu().numpy()}
        route = getattr(drv, "route", None)
        for i, t in enumerate(drv.forest.trees):
            for a in TREE_ARRAYS:
                out[f"tree{i}.{a}"] = np.asarray(getattr(t, a))
        return out, (route.kind if route is not None else "?")
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    bad += [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k], equal_nan=True)]
    cases = sorted({k.split("/")[0] for k in A.files})
    print(f"{len(cases)} cases, {len(A.files)} arrays, {len(bad)} differ")
    for k in bad[:40]:
        both = k in A.files and k in B.files and A[k].shape == B[k].shape
        print("  differs:", k, "largest difference %.3g" % np.abs(A[k].astype(np.float64) - B[k]).max() if both else "")
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--compare":
        return compare(argv[1], argv[2])
    import torch
    import h2o3_amd
    from h2o3_amd.parallel import cloud
    h2o3_amd.init(verbose=False)
    gpu = torch.cuda.is_available()
    cases = GPU_CASES if gpu else CPU_CASES
    pick = argv[1] if len(argv) > 1 else ""
    fr = frame(40_000 if gpu else 4_000)
    out = {}
    for name, (y, parms, env, spec_kw) in cases.items():
        if pick not in name:
            continue
        arrays, kind = run_case(fr, y, parms, env, spec_kw)
        ntree = sum(k.startswith("tree") for k in arrays) // len(TREE_ARRAYS)
        print(f"{name}: route {kind}, {ntree} trees", flush=True)
        out.update({f"{name}/{k}": v for k, v in arrays.items()})
    if cloud.rank() == 0:
        np.savez(argv[0], **out)
    if cloud.world() > 1:
        cloud.barrier()
        cloud.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
