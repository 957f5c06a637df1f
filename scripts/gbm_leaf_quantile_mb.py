"""GBM laplace / huber leaf values: the radix-select kernel route
(H2O3_LEAF_QUANTILE=1, ops/quantile_ops.py) against the sort + host loop
(=0), alternating in one process, and the three kernels alone by device events.

    python scripts/gbm_leaf_quantile_mb.py [--sizes 1000000,10000000] [--reps 5]

Writes profiles/gbm_leaf_quantile_mb.txt: per size and family the median and
min / max of the `gbm.gamma` phase and of the whole tree (both synchronised),
then the kernels' times and the bytes they move against the HBM peak."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from h2o3_amd.core.frame import H2OFrame  # noqa: E402
from h2o3_amd.models.base import TrainSpec  # noqa: E402
from h2o3_amd.models.tree.gbm import GBMDriver, H2OGradientBoostingEstimator  # noqa: E402
from h2o3_amd.ops import quantile_ops  # noqa: E402
from h2o3_amd.utils import timer  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, MI355X
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stats(v):
    return f"median {statistics.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f} ms"


def trees(N, P, fam, reps):
    g = np.random.default_rng(3)
    X = g.standard_normal((N, P)).astype(np.float32)
    cols = {f"x{j}": X[:, j] for j in range(P)}
    cols["y"] = X[:, 0] - 0.7 * X[:, 1] + np.sin(2 * X[:, 2]) + 0.3 * g.standard_t(3, N)
    fr = H2OFrame(cols)
    del X, cols
    est = H2OGradientBoostingEstimator(ntrees=reps + 1, max_depth=6, seed=1, distribution=fam)
    spec = TrainSpec(fr, [f"x{j}" for j in range(P)], "y")
    est._spec = spec
    bd = est._bin(spec)
    drv = {}
    for sw in ("0", "1"):
        os.environ["H2O3_LEAF_QUANTILE"] = sw
        drv[sw] = GBMDriver(est, spec, bd=bd)
        drv[sw].step()                                   # warm-up: first launches, allocator
    res = {sw: ([], []) for sw in drv}
    for _ in range(reps):
        for sw in ("0", "1"):                            # alternate: drift hits both alike
            timer.report()
            torch.cuda.synchronize()
            t = time.perf_counter()
            drv[sw].step()
            torch.cuda.synchronize()
            res[sw][1].append((time.perf_counter() - t) * 1e3)
            res[sw][0].append(timer.report().get("gbm.gamma", (0.0, 0))[0])
    for sw, name in (("0", "sort + host loop"), ("1", "radix select  ")):
        say(f"  {fam:8s} {name}  gamma {stats(res[sw][0])}   tree {stats(res[sw][1])}")
    for i, what in enumerate(("gamma", "tree")):
        old, new = res["0"][i], res["1"][i]
        say(f"  {fam:8s} {what:5s} old median / new median = {statistics.median(old) / statistics.median(new):6.2f}; "
            f"new median {'<' if statistics.median(new) < min(old) else '>='} old min")


def kernels(N, L, reps):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    ridx = torch.randperm(N, generator=g, device=dev).to(torch.int32)
    y = torch.randn(N, generator=g, device=dev)
    f = torch.randn(N, generator=g, device=dev).mul_(0.1)
    w = torch.rand(N, generator=g, device=dev)
    st = [i * (N // L) for i in range(L)]
    ct = [N // L] * (L - 1) + [N - st[-1]]
    S = quantile_ops.weight_scale_bits(1.0, N, False)
    T = {}

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        T.setdefault(name, []).append(a.elapsed_time(b))
        return out

    for r in range(reps + 1):
        s = timed("keys", lambda: quantile_ops.LeafQuantile(ridx, y, f, w, list(range(L)), st, ct, L, 0.5, S))
        for k in range(4):
            h = timed(f"hist {k} (with its zero fill)", lambda: s.hist(k))
            timed(f"select {k}", lambda: s.select(k, h))
    by = {"keys": N * (16 + 12), "hist 0 (with its zero fill)": N * 12}
    for name, v in T.items():
        v = v[1:]                                        # the first round warms up
        extra = ""
        if name in by:
            gbs = by[name] / (statistics.median(v) * 1e-3)
            extra = f"   {by[name] / 1e6:8.1f} MB  {gbs / 1e9:7.1f} GB/s = {100 * gbs / HBM_PEAK:4.1f} % of peak"
        elif name.startswith("hist"):
            extra = f"   >= {N * 4 / 1e6:8.1f} MB of keys, weights where the prefix matches"
        say(f"  {name:28s} {stats(v)}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--cols", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbm_leaf_quantile_mb.txt"))
    a = ap.parse_args()
    timer.ENABLED = True
    say(f"GBM leaf quantiles, depth 6, {a.cols} columns, {a.reps} alternating trees per route after one warm-up; "
        f"{torch.cuda.get_device_name(0)}")
    for N in map(int, a.sizes.split(",")):
        say(f"N = {N}")
        for fam in ("laplace", "huber"):
            trees(N, a.cols, fam, a.reps)
        say(f"  kernels alone, {N} rows in 64 leaves, general f32 weights (device events)")
        kernels(N, 64, a.reps)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
