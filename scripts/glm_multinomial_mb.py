"""Multinomial GLM loss/gradient evaluation: the fused HIP pass
(ops/csrc/glm_multi.hip) against the torch route (library GEMM, f64 softmax,
chunked bmm), both through glm_multi._loss_grad_multinomial, alternating in
one process, device events after warm-up, about a second per route.

Per shape: median / min / max ms per evaluation on each route, peak memory
allocated above the inputs, and the time of the kernel launch alone with its
achieved bytes/s (N * Pp * 4 over that time).  Then the wall time of a whole
family="multinomial" fit at 1M x 100, K = 10 on each route.

    python scripts/glm_multinomial_mb.py [--rows 10000000] [--fit-rows 1000000]
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
    B = torch.zeros((Pp, K), device="cuda", dtype=torch.float64)
    B[:P] = torch.randn((P, K), device="cuda", generator=g, dtype=torch.float64) * (2 / P ** 0.5)
    b0 = torch.randn(K, device="cuda", generator=g, dtype=torch.float64)
    wsum = float(w.sum())
    y32, w32 = y.to(torch.int32), w.to(torch.float32)
    routes = {"kernel": lambda: glm_multi._loss_grad_multinomial(X, y32, w32, B, b0, wsum)}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    Y = torch.nn.functional.one_hot(y, K).to(torch.float64)     # the torch route keeps it for the whole fit
    routes["torch"] = lambda: glm_multi._loss_grad_multinomial(X, Y, w, B, b0, wsum)
    peak, outs, ms = {}, {}, {k: [] for k in routes}
    for name, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base - (0 if name == "torch" else Y.numel() * 8)
        outs[name] = out
    one = max(timed(routes["torch"]), 1e-3)
    for _ in range(max(5, min(200, int(1000 / one)))):
        for name in ("kernel", "torch"):
            ms[name].append(timed(routes[name]))
    fk, ft = outs["kernel"], outs["torch"]
    print(f"N={N} P={P} Pp={Pp} K={K}   inputs {base / 2**30:.2f} GiB")
    for name in ("kernel", "torch"):
        print(f"  {name:6s} {stats(ms[name])}  peak above inputs {peak[name] / 2**30:7.3f} GiB")
    print(f"  speed-up (medians) {np.median(ms['torch']) / np.median(ms['kernel']):.2f}x   "
          f"loss rel diff {abs(fk[0] - ft[0]) / abs(ft[0]):.2e}  "
          f"gB max diff / max {float((fk[1] - ft[1]).abs().max() / ft[1].abs().max()):.2e}")
    kms = [timed(lambda: linalg_ops.glm_multinomial_pass(X, y32, w32, B, b0, K)) for _ in range(len(ms["kernel"]))]
    print(f"  pass alone (launch + sum of slab records) {stats(kms)}  "
          f"{N * Pp * 4 / (np.median(kms) * 1e-3) / 1e12:.2f} TB/s of X", flush=True)


def fit(N, P, K):
    import pandas as pd
    from h2o3_amd.estimators import H2OGeneralizedLinearEstimator
    rng = np.random.RandomState(7)
    Xn = rng.randn(N, P).astype(np.float32)
    codes = (Xn[:, :K] + rng.gumbel(size=(N, K))).argmax(1)
    df = pd.DataFrame(Xn, columns=[f"x{i}" for i in range(P)])
    df["y"] = np.array([f"c{k}" for k in range(K)])[codes]
    fr = h2o3_amd.H2OFrame(df)
    xs = [f"x{i}" for i in range(P)]
    for rep in range(2):
        for route in ("kernel", "torch"):
            os.environ["H2O3_GLM_MULTI"] = route
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            m = H2OGeneralizedLinearEstimator(family="multinomial", lambda_=0)
            m.train(x=xs, y="y", training_frame=fr)
            torch.cuda.synchronize()
            print(f"fit N={N} P={P} K={K} lambda=0 {route:6s} run {rep}: {time.perf_counter() - t0:7.3f} s  "
                  f"deviance {m.residual_deviance():.8g}  peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB",
                  flush=True)
    os.environ.pop("H2O3_GLM_MULTI")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--fit-rows", type=int, default=1_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available() or _native.get_lib("glm_multi") is None:
        sys.exit("needs a GPU and the built glm_multi library")
    h2o3_amd.init(device="cuda:0")
    for P, Pp, K in ((100, 128, 10), (100, 128, 3), (200, 256, 30)):
        evaluation(a.rows, P, Pp, K)
    if a.fit_rows:
        fit(a.fit_rows, 100, 10)
