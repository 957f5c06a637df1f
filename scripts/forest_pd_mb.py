"""Partial dependence of a tree model on the forest-grid primitive
(ops/pd_ops.forest_grid_sums: tree_pd.hip) against the replacement loop, for a
GBM of 100 depth-8 trees on F = 100 features, everything on one GPU.

  python scripts/forest_pd_mb.py prim  [out.txt]   the primitive at 1M and 10M rows, G = 20 on the most-split
                                                   column, against 20 Forest.predict calls on matrices whose
                                                   row is already overridden (device events, the override is
                                                   not timed); the two are alternated in one process
  python scripts/forest_pd_mb.py model [out.txt]   partial_plot of 5 columns, one 20 x 20 pair and h() on two
                                                   variables at 1M rows: the primitive, and the replacement
                                                   loop of H2O3_TREE_PD=torch (what every call did before the
                                                   primitive), host clock around a device synchronise

Each mode is one process and needs a GPU; the lines are appended to out.txt if
given.  Times are medians of repeats after a warm-up run.
Env: PD_MB_T / _D / _REPS / _N (model mode's rows) override the shape."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = 100
G = 20


def _train(T, D):
    import pandas as pd
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n0 = 100_000
    Xs = rng.standard_normal((n0, F)).astype(np.float32)
    y = Xs[:, :10].sum(1) + Xs[:, 0] * Xs[:, 1] + 0.5 * rng.standard_normal(n0)
    df = pd.DataFrame(Xs, columns=[f"x{j}" for j in range(F)])
    df["y"] = y
    m = H2OGradientBoostingEstimator(ntrees=T, max_depth=D, seed=1, min_rows=1, learn_rate=0.05)
    m.train(y="y", training_frame=h2o.H2OFrame(df))
    return m


def _most_split(P, k=1):
    inner = P["left"] >= 0
    cnt = torch.bincount(P["feat"][inner].long(), minlength=F)
    return [int(c) for c in cnt.argsort(descending=True)[:k]], cnt


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def mode_prim():
    from h2o3_amd.ops import pd_ops
    T = int(os.environ.get("PD_MB_T", 100))
    D = int(os.environ.get("PD_MB_D", 8))
    reps = int(os.environ.get("PD_MB_REPS", 5))
    m = _train(T, D)
    fo = m._forest
    dev = torch.device("cuda")
    P = fo.pack(dev)
    (col,), cnt = _most_split(P)
    th, lds = pd_ops.launch_shape(G, pd_ops.max_depth(P))
    lines = [f"forest: {len(fo.trees)} trees, depth {pd_ops.max_depth(P)}, {int(P['node'].shape[0])} nodes; F={F}, "
             f"G={G} on feature {col} ({int(cnt[col])} of {int(cnt.sum())} splits); walk kernel: {th} threads, "
             f"{lds} B LDS per block"]
    grid = torch.linspace(-2.5, 2.5, G, device=dev).view(1, G)
    for N in (1_000_000, 10_000_000):
        X = torch.randn(F, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        keep = X[col].clone()
        t_prim, t_loop = [], []
        same = None
        for rep in range(reps + 1):                       # round 0 is the warm-up
            dt, res = _events(lambda: pd_ops.forest_grid_sums(P, X, 1, [col], grid))
            assert res.kernel
            tl = 0.0
            for g in range(G):
                X[col] = grid[0, g]
                torch.cuda.synchronize()
                d, out = _events(lambda: fo.predict(X, 1))
                tl += d
                if rep == 0:
                    same = (same is None or same) and torch.equal(out, res.sums[g])
            X[col] = keep
            if rep:
                t_prim.append(dt)
                t_loop.append(tl)
            del res
        a, b = statistics.median(t_prim), statistics.median(t_loop)
        lines.append(f"N={N}: primitive {a * 1e3:.2f} ms (min {min(t_prim) * 1e3:.2f}), {N * G / a / 1e9:.2f} G "
                     f"row-points/s; {G} Forest.predict calls {b * 1e3:.2f} ms (min {min(t_loop) * 1e3:.2f}): "
                     f"{b / a:.2f}x; bit-equal to the {G} predicts: {same} (medians of {reps})")
        del X, keep
    return lines


def _timed(fn, reps, warm=1):
    """(median seconds, the last call's result)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def mode_model():
    from h2o3_amd.core.frame import H2OFrame
    from h2o3_amd.core.vec import T_REAL, Vec
    T = int(os.environ.get("PD_MB_T", 100))
    D = int(os.environ.get("PD_MB_D", 8))
    N = int(os.environ.get("PD_MB_N", 1_000_000))
    reps = int(os.environ.get("PD_MB_REPS", 3))
    m = _train(T, D)
    dev = torch.device("cuda")
    cols, _ = _most_split(m._forest.pack(dev), 5)
    names = [f"x{j}" for j in range(F)]
    X = torch.randn(F, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    fr = H2OFrame.from_vecs([Vec(X[j].contiguous(), T_REAL) for j in range(F)], names)
    del X
    c5 = [names[c] for c in cols]
    calls = [("partial_plot, 5 columns x 20 values", lambda: m.partial_plot(fr, cols=c5)),
             ("partial_plot, one 20 x 20 pair", lambda: m.partial_plot(fr, cols=[], col_pairs_2dpdp=[c5[:2]])),
             ("h() on two variables (200 sampled rows)", lambda: m.h(fr, c5[:2]))]
    lines = [f"model: GBM {T} trees depth {D}; frame {N} rows x {F} columns; columns {c5}"]
    for what, fn in calls:
        os.environ.pop("H2O3_TREE_PD", None)
        t_k, got = _timed(fn, reps)
        assert m._pd_why is None, m._pd_why
        os.environ["H2O3_TREE_PD"] = "torch"
        t_l, want = _timed(fn, 1, warm=0)
        os.environ.pop("H2O3_TREE_PD")
        if isinstance(got, float):
            err = abs(got - want)
        else:
            err = max(float(np.abs(a["mean_response"].values - b["mean_response"].values).max())
                      for a, b in zip(got, want))
        lines.append(f"{what}: primitive {t_k * 1e3:.1f} ms (median of {reps}), replacement loop "
                     f"{t_l * 1e3:.0f} ms (one run): {t_l / t_k:.1f}x; max abs difference {err:.1e}")
    return lines


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "prim"
    if not torch.cuda.is_available():
        sys.exit("forest_pd_mb.py needs a GPU: nothing was measured")
    lines = {"prim": mode_prim, "model": mode_model}[mode]()
    for ln in lines:
        print(ln, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
