"""Ordinal GLM loss/gradient evaluation: the fused HIP pass
(ops/csrc/glm_multi.hip glm_ordinal_kernel) against the torch route
(_loss_grad_ordinal: library GEMV, f64 CDF table over [N, K+1], autograd
backward), alternating in one process, device events after warm-up, about a
second per route.

Per shape: median / min / max ms per evaluation (loss and gradient over
[beta | theta]) on each route, peak memory allocated above the inputs, and
the time of glm_ordinal_pass alone with its achieved bytes/s (N * Pp * 4
over that time).  Then the wall time of a whole family="ordinal" fit on
each route.

    python scripts/glm_ordinal_mb.py [--rows 10000000] [--wide-rows 1000000] [--fit-rows 10000000]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

import h2o3_amd  # noqa: E402
from h2o3_amd.models.glm import glm_multi  # noqa: E402
from h2o3_amd.ops import _native, linalg_ops  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return f"median {np.median(ms):8.3f}  min {min(ms):8.3f}  max {max(ms):8.3f} ms  ({len(ms)} runs)"


def evaluation(N, P, Pp, K):
    g = torch.Generator(device="cuda").manual_seed(N % 1000 + Pp + K)
    X = torch.zeros((N, Pp), device="cuda")
    for a in range(0, N, 1 << 20):
        X[a:a + (1 << 20), :P] = torch.randn((min(1 << 20, N - a), P), device="cuda", generator=g)
    y = torch.randint(0, K, (N,), device="cuda", generator=g)
    w = torch.rand(N, device="cuda", generator=g, dtype=torch.float64) * 2
    beta = torch.zeros(Pp, device="cuda", dtype=torch.float64)
    beta[:P] = torch.randn(P, device="cuda", generator=g, dtype=torch.float64) / P ** 0.5
    theta = torch.randn(K - 1, device="cuda", generator=g, dtype=torch.float64)
    y32, w32 = y.to(torch.int32), w.to(torch.float32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()

    def torch_route():
        t = torch.cat([beta, theta]).requires_grad_(True)
        ll, _ = glm_multi._loss_grad_ordinal(X, y, w, t[:Pp], t[Pp:], 1.0, K)
        ll.backward()
        return ll.detach(), t.grad

    routes = {"kernel": lambda: glm_multi._loss_grad_ordinal_pass(X, y32, w32, beta, theta, K), "torch": torch_route}
    peak, outs, ms = {}, {}, {k: [] for k in routes}
    for name, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        outs[name] = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    one = max(timed(routes["torch"]), 1e-3)
    for _ in range(max(5, min(200, int(1000 / one)))):
        for name in ("kernel", "torch"):
            ms[name].append(timed(routes[name]))
    fk, ft = outs["kernel"], outs["torch"]
    print(f"N={N} P={P} Pp={Pp} K={K}   inputs {base / 2**30:.2f} GiB")
    for name in ("kernel", "torch"):
        print(f"  {name:6s} {stats(ms[name])}  peak above inputs {peak[name] / 2**30:7.3f} GiB")
    print(f"  speed-up (medians) {np.median(ms['torch']) / np.median(ms['kernel']):.2f}x   "
          f"loss rel diff {abs(float(fk[0] - ft[0])) / abs(float(ft[0])):.2e}  "
          f"gradient max diff / max {float((fk[1] - ft[1]).abs().max() / ft[1].abs().max()):.2e}")
    cuts = glm_multi._ordinal_cuts(theta)
    kms = [timed(lambda: linalg_ops.glm_ordinal_pass(X, y32, w32, beta, cuts, K)) for _ in range(len(ms["kernel"]))]
    print(f"  pass alone (launch + sum of slab records) {stats(kms)}  "
          f"{N * Pp * 4 / (np.median(kms) * 1e-3) / 1e12:.2f} TB/s of X", flush=True)


def fit(N, P, K):
    from h2o3_amd.estimators import H2OGeneralizedLinearEstimator
    rng = np.random.RandomState(7)
    Xn = rng.randn(N, P).astype(np.float32)
    eta = Xn[:, :8] @ np.linspace(1.0, -1.0, 8).astype(np.float32) + rng.logistic(size=N).astype(np.float32)
    codes = np.digitize(eta, np.quantile(eta[:100000], np.arange(1, K) / K))
    import pandas as pd
    df = pd.DataFrame(Xn, columns=[f"x{i}" for i in range(P)])
    df["y"] = pd.Categorical.from_codes(codes, [f"c{k}" for k in range(K)])
    fr = h2o3_amd.H2OFrame(df)
    xs = [f"x{i}" for i in range(P)]
    for rep in range(2):
        for route in ("kernel", "torch"):
            os.environ["H2O3_GLM_MULTI"] = route
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            m = H2OGeneralizedLinearEstimator(family="ordinal", lambda_=0)
            m.train(x=xs, y="y", training_frame=fr)
            torch.cuda.synchronize()
            print(f"fit N={N} P={P} K={K} lambda=0 {route:6s} run {rep}: {time.perf_counter() - t0:7.3f} s  "
                  f"deviance {m.residual_deviance():.8g}  peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB",
                  flush=True)
    os.environ.pop("H2O3_GLM_MULTI")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--fit-rows", type=int, default=10_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available() or _native.get_lib("glm_multi") is None:
        sys.exit("needs a GPU and the built glm_multi library")
    h2o3_amd.init(device="cuda:0")
    for N, P, Pp, K in ((a.rows, 100, 128, 5), (a.rows, 100, 128, 10), (a.wide_rows, 1000, 1024, 5)):
        evaluation(N, P, Pp, K)
    if a.fit_rows:
        fit(a.fit_rows, 100, 5)
