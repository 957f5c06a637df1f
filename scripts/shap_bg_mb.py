"""Baseline SHAP throughput: a GBM of T depth-D trees on F = 100 features,
predict_contributions' kernel path (ops/shap_ops.background_shap:
tree_shap.hip) for N test rows against B background rows already on the
device, averaged mode.  The torch implementation of the same rule on the same
device is the reference (the path-dependent code cannot do this at all).

Times (median of repeats after a warm-up run, stream-synchronised): the
kernel at N = 100k and N = 10k (5 repeats), the torch implementation at
N = 10k (3 repeats).  Writes the lines to argv[1] if given.
Env: SHAP_MB_T / _D / _B / _N1 / _N2 / _TORCH_N / _TORCH_REPS."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    T = int(os.environ.get("SHAP_MB_T", 100))
    D = int(os.environ.get("SHAP_MB_D", 8))
    B = int(os.environ.get("SHAP_MB_B", 100))
    N1 = int(os.environ.get("SHAP_MB_N1", 100_000))
    N2 = int(os.environ.get("SHAP_MB_N2", 10_000))
    NT = int(os.environ.get("SHAP_MB_TORCH_N", N2))
    F = 100
    import pandas as pd
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    from h2o3_amd.ops import shap_ops
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n0 = 100_000
    Xs = rng.standard_normal((n0, F)).astype(np.float32)
    y = (Xs[:, :10].sum(1) + 0.5 * rng.standard_normal(n0) > 0).astype(int)
    df = pd.DataFrame(Xs, columns=[f"x{j}" for j in range(F)])
    df["y"] = np.where(y == 1, "a", "b")
    m = H2OGradientBoostingEstimator(ntrees=T, max_depth=D, seed=1, min_rows=1, learn_rate=0.05)
    m.train(y="y", training_frame=h2o.H2OFrame(df))
    fo = m._forest
    dev = torch.device("cuda")
    P, PT = fo.pack(dev), fo.leaf_paths(dev)
    L = PT["L"]
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(F, N1, device="cuda", generator=g)
    Z = torch.randn(F, B, device="cuda", generator=g)
    lines = [f"forest: {len(fo.trees)} trees, depth {D}, {L} leaves, longest path {PT['max_path']} features; "
             f"F={F}, B={B}"]
    res = None
    for N in (N1, N2):
        Xn = X[:, :N].contiguous()

        def run():
            nonlocal res
            res = shap_ops.background_shap(P, PT, Xn, Z, F)
        dt = _timed(run, reps=5)
        assert res.kernel
        tm = {}
        shap_ops.background_shap(P, PT, Xn, Z, F, timing=tm)
        lines.append(f"kernel  N={N}: {dt * 1e3:.2f} ms, {N * B * L / dt / 1e9:.1f} G pair-leaves/s "
                     f"(row tiles {res.row_tiles}, tree chunks {res.tree_chunks}; device time: masks "
                     f"{tm['masks_ms']:.2f} ms, pairs {tm['pairs_ms']:.2f} ms)")
        if N == N2:
            t_k, phi_k = dt, res.phi
    Xn = X[:, :NT].contiguous()
    ref = None

    def run_t():
        nonlocal ref
        ref = shap_ops.background_shap_torch(P, PT, Xn, Z, F)[0]
    treps = int(os.environ.get("SHAP_MB_TORCH_REPS", 3))
    t_t = _timed(run_t, reps=treps, warm=1)
    lines.append(f"torch   N={NT}: {t_t * 1e3:.0f} ms (median of {treps} after one warm-up run)")
    if NT == N2:
        err = float((ref - phi_k).abs().max())
        lines.append(f"kernel vs torch at N={N2}: {t_t / t_k:.0f}x faster, max abs difference {err:.2e}")
    else:
        lines.append(f"torch per row {t_t / NT * 1e6:.1f} us vs kernel {t_k / N2 * 1e6:.3f} us")
    for ln in lines:
        print(ln, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
