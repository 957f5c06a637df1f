"""Uplift DRF split search: the kernels of ops/csrc/tree_uplift.hip against
the torch route (H2O3_UPLIFT_SPLIT=torch, the only route before the kernels
existed; its code is unchanged).

(a) the per-phase share of one upliftdrf training at the survey shape (1M rows,
    10 numeric columns, ntrees 20, the configuration of scripts/algo_survey2.py)
    on both routes, from the phase() timers (a device synchronise around every
    phase, so this run is slower than an untimed one);
(b) the split search alone on synthetic level histograms, frontier sizes 1, 64
    and 4096, Fl = 50: B = 20 numeric columns, and B = 256 with one 256-level
    categorical column; both routes must return the same splits;
(c) end-to-end train_s on both routes, alternating them in one process after a
    warm-up of each, a device synchronise inside the timed window.

    python scripts/uplift_split_mb.py --out profiles/uplift_split_mb.txt
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import h2o3_amd as h2o                                            # noqa: E402
from h2o3_amd.core.frame import H2OFrame                          # noqa: E402
from h2o3_amd.core.vec import T_ENUM, T_REAL, Vec                 # noqa: E402
from h2o3_amd.estimators import H2OUpliftRandomForestEstimator    # noqa: E402
from h2o3_amd.models.tree.engine import TreeGrower                # noqa: E402
from h2o3_amd.ops import tree_ops                                 # noqa: E402
from h2o3_amd.utils import timer                                  # noqa: E402

OUT = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def spread(ts):
    return f"median {statistics.median(ts) * 1e3:9.2f} ms  min {min(ts) * 1e3:9.2f}  max {max(ts) * 1e3:9.2f}"


def survey_frame(n, P=20):
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn((n, P), generator=g, device="cuda")
    eta = X @ (torch.randn(P, generator=g, device="cuda") / P ** 0.5)
    y = (torch.rand(n, generator=g, device="cuda") < torch.sigmoid(eta)).to(torch.int32)
    tr = torch.randint(0, 2, (n,), generator=g, device="cuda").to(torch.int32)
    vecs = [Vec(X[:, j].contiguous(), T_REAL) for j in range(P)]
    vecs += [Vec(y, T_ENUM, ["0", "1"]), Vec(tr, T_ENUM, ["control", "treatment"])]
    return H2OFrame.from_vecs(vecs, [f"x{j}" for j in range(P)] + ["y", "treat"])


def train(fr, route):
    os.environ["H2O3_UPLIFT_SPLIT"] = route
    torch.cuda.synchronize()
    t = time.perf_counter()
    m = H2OUpliftRandomForestEstimator(ntrees=20, treatment_column="treat", seed=1)
    m.train(x=[f"x{j}" for j in range(10)], y="y", training_frame=fr)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    os.environ.pop("H2O3_UPLIFT_SPLIT", None)
    return dt, m


def phases(fr, route):
    timer.ENABLED = True
    timer.report()
    dt, _ = train(fr, route)
    rep = timer.report()
    timer.ENABLED = False
    say(f"  route {route:5s}  train with phase timers {dt:6.2f} s")
    for k in ("tree.hist", "tree.split", "tree.partition", "tree.nid"):
        if k in rep:
            say(f"    {k:15s} {rep[k][0]:9.1f} ms  {rep[k][1]:5d} calls  {100 * rep[k][0] / (dt * 1e3):5.1f} % of the training")


def level_hist(n, Fl, B, cat, seed):
    """[Fl, n, B + 1, 4] f64 of integer counts with empty bins; feature 0 categorical if cat."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randint(0, 50, (Fl, n, B + 1, 2), generator=g, device="cuda").double()
    w[:, :, B // 3] = 0
    wy = torch.floor(w * torch.rand(w.shape, generator=g, device="cuda", dtype=torch.float64))
    H = torch.stack([w[..., 0], wy[..., 0], w[..., 1], wy[..., 1]], -1).contiguous()
    return H, torch.tensor([cat] + [False] * (Fl - 1), device="cuda")


def torch_route(H, is_cat, crit, min_rows):
    Fl, n = H.shape[0], H.shape[1]
    g = SimpleNamespace(p=SimpleNamespace(criterion=crit, min_rows=min_rows, use_bounds=False), is_cat_t=is_cat,
                        bd=SimpleNamespace(F=Fl), f0=0, W=1, _bnd_dev=lambda n: None)
    g._find_splits_torch_core = lambda *a: TreeGrower._find_splits_torch_core(g, *a)
    cm = torch.ones((n, Fl), dtype=torch.bool, device=H.device)
    return lambda: TreeGrower._find_splits_torch(g, H, cm)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def search_alone(repeats):
    good = True
    for B, cat, label in ((20, False, "B 20, numeric"), (256, True, "B 256, feature 0 a 256-level categorical")):
        for n in (1, 64, 4096):
            H, is_cat = level_hist(n, 50, B, cat, seed=n + B)
            ok = torch.ones((n, 50), dtype=torch.uint8, device="cuda")
            hip = lambda: tree_ops.uplift_splits(H, ok, is_cat, 0, 50, "uplift_kl", 10.0)   # noqa: E731
            ref = torch_route(H, is_cat, "uplift_kl", 10.0)
            _, a = timed(hip)
            _, b = timed(ref)
            fin = torch.isfinite(b["gain"])
            same = bool((a["gain"][fin] - b["gain"][fin]).abs().max() <= 1e-12) if bool(fin.any()) else True
            same &= all(torch.equal(a[k][fin], b[k][fin]) for k in ("feat", "t", "opt", "mask", "L", "R"))
            same &= torch.equal(torch.isfinite(a["gain"]), fin)
            good &= same
            tk, tt = [], []
            for _ in range(repeats):
                tk.append(timed(hip)[0])
                tt.append(timed(ref)[0])
            say(f"  Fl 50, {label}, frontier {n:5d}: same splits {same}")
            say(f"    kernels  {spread(tk)}")
            say(f"    torch    {spread(tt)}   {statistics.median(tt) / statistics.median(tk):7.1f}x by medians")
            del H
            torch.cuda.empty_cache()
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("uplift_split_mb: needs a GPU")
    if a.out:
        global OUT
        OUT = a.out
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        open(OUT, "w").close()                  # a run replaces the file
    h2o.init(device="cuda:0", verbose=False)
    say(f"# uplift_split_mb  device {torch.cuda.get_device_name(0)}  rows {a.rows}  repeats {a.repeats}")
    say(f"# python scripts/uplift_split_mb.py --rows {a.rows} --repeats {a.repeats}")
    fr = survey_frame(a.rows)
    cold = {r: train(fr, r)[0] for r in ("hip", "torch")}          # also the warm-up of each route
    say(f"(c) upliftdrf train_s, {a.rows} rows x 10 columns, ntrees 20, default depth")
    say(f"  first training in the process: kernels {cold['hip']:.2f} s (it ran first), torch {cold['torch']:.2f} s")
    tk, tt = [], []
    for _ in range(a.repeats):
        tk.append(train(fr, "hip")[0])
        tt.append(train(fr, "torch")[0])
    say(f"  kernels  {spread(tk)}")
    say(f"  torch    {spread(tt)}")
    say(f"  slowest kernel repeat under fastest torch repeat: {max(tk) < min(tt)}")
    say("(a) phases of one training (synchronised timers)")
    phases(fr, "torch")
    phases(fr, "hip")
    del fr
    torch.cuda.empty_cache()
    say("(b) split search alone, uplift_kl, min_rows 10")
    sys.exit(0 if search_alone(a.repeats) else 1)


if __name__ == "__main__":
    main()
