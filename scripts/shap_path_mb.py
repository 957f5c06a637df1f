"""Path-dependent TreeSHAP throughput (predict_contributions without a
background frame): shap_path_kernel (ops/shap_ops.path_shap: tree_shap.hip)
against the node recursion of models/tree/shap.py on the same GPU, for a GBM
on F = 100 features with the score matrix already on the device.

  python scripts/shap_path_mb.py ab   [out.txt]   recursion (H2O3_TREE_SHAP=torch) and kernel through
                                                  shap_dispatch: 10 depth-6 trees, 10k rows
  python scripts/shap_path_mb.py big  [out.txt]   kernel alone: 100 depth-8 trees, 100k rows, with the
                                                  stages' device time, and Forest.predict on the same rows

Each mode is one process; the lines are appended to out.txt if given.  Times
are medians of repeats after a warm-up run, stream-synchronised.
Env: SHAP_MB_T / _D / _N / _REPS / _REC_REPS override the mode's shape."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = 100


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


def _train(T, D):
    import pandas as pd
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n0 = 100_000
    Xs = rng.standard_normal((n0, F)).astype(np.float32)
    y = (Xs[:, :10].sum(1) + 0.5 * rng.standard_normal(n0) > 0).astype(int)
    df = pd.DataFrame(Xs, columns=[f"x{j}" for j in range(F)])
    df["y"] = np.where(y == 1, "a", "b")
    m = H2OGradientBoostingEstimator(ntrees=T, max_depth=D, seed=1, min_rows=1, learn_rate=0.05)
    m.train(y="y", training_frame=h2o.H2OFrame(df))
    return m


def _head(fo, PT, D, N):
    return (f"forest: {len(fo.trees)} trees, depth {D}, {PT['L']} leaves, longest path {PT['max_path']} features; "
            f"F={F}, N={N}")


def mode_ab():
    from h2o3_amd.models.tree.shap import shap_dispatch
    T = int(os.environ.get("SHAP_MB_T", 10))
    D = int(os.environ.get("SHAP_MB_D", 6))
    N = int(os.environ.get("SHAP_MB_N", 10_000))
    m = _train(T, D)
    fo = m._forest
    PT = fo.leaf_paths(torch.device("cuda"))
    X = torch.randn(F, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = {}

    class Holder:
        pass
    h = Holder()

    def run(tag):
        out[tag] = shap_dispatch(h, fo, X, F)
    os.environ.pop("H2O3_TREE_SHAP", None)
    t_k = _timed(lambda: run("kernel"), reps=int(os.environ.get("SHAP_MB_REPS", 5)))
    assert h._shap_path_why is None
    os.environ["H2O3_TREE_SHAP"] = "torch"
    rreps = int(os.environ.get("SHAP_MB_REC_REPS", 3))
    t_r = _timed(lambda: run("rec"), reps=rreps)
    assert h._shap_path_why == "H2O3_TREE_SHAP=torch"
    os.environ.pop("H2O3_TREE_SHAP")
    err = float((out["kernel"] - out["rec"]).abs().max())
    return [_head(fo, PT, D, N),
            f"recursion (H2O3_TREE_SHAP=torch): {t_r * 1e3:.0f} ms (median of {rreps} after one warm-up run)",
            f"kernel (masks + paths + host bias): {t_k * 1e3:.2f} ms, {N * PT['L'] / t_k / 1e9:.2f} G row-leaves/s",
            f"kernel vs recursion: {t_r / t_k:.0f}x faster, max abs difference {err:.2e}"]


def mode_big():
    from h2o3_amd.ops import shap_ops
    T = int(os.environ.get("SHAP_MB_T", 100))
    D = int(os.environ.get("SHAP_MB_D", 8))
    N = int(os.environ.get("SHAP_MB_N", 100_000))
    reps = int(os.environ.get("SHAP_MB_REPS", 5))
    m = _train(T, D)
    fo = m._forest
    dev = torch.device("cuda")
    P, PT = fo.pack(dev), fo.leaf_paths(dev)
    X = torch.randn(F, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = None

    def run():
        nonlocal res
        res = shap_ops.path_shap(P, PT, X, F)
    dt = _timed(run, reps=reps)
    assert res.kernel
    tm = {}
    shap_ops.path_shap(P, PT, X, F, timing=tm)
    t_p = _timed(lambda: fo.predict(X, 1), reps=reps)
    fx = fo.predict(X, 1)[:, 0].double()
    bias = sum(sum(t.value[j] * max(t.weight[j], 0.0) for j in t.leaves()) / t.weight[0] for t in fo.trees)
    gap = float((res.phi.sum(1) + bias - fx).abs().max())
    return [_head(fo, PT, D, N),
            f"kernel: {dt * 1e3:.2f} ms, {N * PT['L'] / dt / 1e9:.1f} G row-leaves/s, {N / dt / 1e6:.2f} M rows/s "
            f"(row tiles {res.row_tiles}, tree chunks {res.tree_chunks}; device time: masks_ms "
            f"{tm['masks_ms']:.2f}, path_ms {tm['path_ms']:.2f})",
            f"Forest.predict on the same rows: {t_p * 1e3:.2f} ms, {N / t_p / 1e6:.0f} M rows/s",
            f"row sums + bias against Forest.predict (f32 sums): max abs difference {gap:.2e}"]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    lines = {"ab": mode_ab, "big": mode_big}[mode]()
    for ln in lines:
        print(ln, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
