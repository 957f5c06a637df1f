"""Extended Isolation Forest scoring: the sparse hyperplane-forest kernel
(ops/csrc/tree_eif.hip) against the dense torch rule (H2O3_TREE_EIF=torch).

For each shape (2M x 50, the survey shape, and 10M x 100) and each
extension_level of 0, 1 and P - 1 it trains 100 trees on 256-row samples and
times model.predict on the training frame on both routes, alternating them in
one process after a warm-up of each, with a device synchronise inside the
timed window; it reports the median and min / max of the repeats.  It also
times the kernel alone with device events for every launch plan (trees in
flight, LDS row tile on / off) and sets the bytes of X over that time against
the HBM bandwidth, and it checks the two routes' mean_length against each
other: rows where they differ must be ambiguous by tests/eif_common.oracle
(which is also run on the first rows to count ambiguous ones).

    python scripts/eif_score_mb.py --out profiles/eif_score_mb.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import h2o3_amd as h2o                                            # noqa: E402
from h2o3_amd.core.frame import H2OFrame                          # noqa: E402
from h2o3_amd.core.vec import T_REAL, Vec                         # noqa: E402
from h2o3_amd.estimators import H2OExtendedIsolationForestEstimator  # noqa: E402
from h2o3_amd.ops import eif_ops                                  # noqa: E402

from eif_common import oracle                                     # noqa: E402

HBM_TBS = 6.29        # measured float4-copy bandwidth of the MI355X (8.0 spec)
OUT = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def make_frame(n, P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    vecs = []
    for j in range(P):
        c = torch.randn(n, device="cuda", generator=g)
        if j % 7 == 0:
            c[torch.rand(n, device="cuda", generator=g) < 0.02] = float("nan")
        vecs.append(Vec(c, T_REAL))
    return H2OFrame.from_vecs(vecs, [f"x{j}" for j in range(P)])


def timed_predict(m, fr, route):
    if route == "torch":
        os.environ["H2O3_TREE_EIF"] = "torch"
    else:
        os.environ.pop("H2O3_TREE_EIF", None)
    torch.cuda.synchronize()
    t = time.perf_counter()
    p = m.predict(fr)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    os.environ.pop("H2O3_TREE_EIF", None)
    return dt, p


def spread(ts):
    return f"median {statistics.median(ts) * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f}  max {max(ts) * 1e3:9.1f}"


def kernel_only(m, X, repeats):
    pack = m._sparse_pack()
    out = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
    P = int(X.shape[1])
    for tile in (False, True):
        if tile and P > eif_ops.TILE_MAX_P:
            continue
        for tw in eif_ops.TREES_IN_FLIGHT:
            eif_ops.hyperplane_forest_lengths(pack, X, out=out, plan=(tw, tile))
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eif_ops.hyperplane_forest_lengths(pack, X, out=out, plan=(tw, tile))
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            med = statistics.median(ms)
            tbs = X.numel() * 4 / (med * 1e-3) / 1e12
            say(f"    kernel only  trees_in_flight {tw}  tile {'on ' if tile else 'off'}  median {med:8.2f} ms"
                f"  min {min(ms):8.2f}  max {max(ms):8.2f}   X bytes / time {tbs:5.2f} TB/s"
                f" = {100 * tbs / HBM_TBS:5.1f} % of {HBM_TBS} TB/s")


def agreement(m, fr, pk, pd_, sample):
    a, b = pk.vec("mean_length").data, pd_.vec("mean_length").data
    diff = torch.nonzero(a != b).flatten()
    X = m._dinfo.expand(fr, pad=False)[0]
    head = oracle(m._trees, X[:sample].cpu().numpy())
    T = len(m._trees)
    ok = ~head.ambiguous
    same = np.array_equal(a[:sample].cpu().numpy()[ok], (head.sums / T).astype(np.float32)[ok])
    say(f"    first {sample} rows: {int(head.ambiguous.sum())} ambiguous; kernel mean_length equals the oracle"
        f" bit for bit on the others: {same}")
    rows = diff[:5000]
    amb = int(oracle(m._trees, X[rows].cpu().numpy()).ambiguous.sum()) if rows.numel() else 0
    say(f"    kernel vs dense mean_length: {diff.numel()} of {a.numel()} rows differ;"
        f" of the first {rows.numel()} of them {amb} are ambiguous (all of them must be)")
    return same and amb == rows.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000000x50,10000000x100")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=20000, help="rows the numpy oracle is run on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eif_score_mb: needs a GPU")
    if a.out:
        global OUT
        OUT = a.out
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        open(OUT, "w").close()                  # a run replaces the file
    h2o.init(device="cuda:0", verbose=False)
    say(f"# eif_score_mb  device {torch.cuda.get_device_name(0)}  repeats {a.repeats}"
        f"  ntrees 100  sample_size 256")
    say(f"# python scripts/eif_score_mb.py --shapes {a.shapes} --repeats {a.repeats} --sample {a.sample}")
    say(f"# LDS row tile for X of up to {eif_ops.TILE_MAX_P} columns; trees in flight {eif_ops.TREES_IN_FLIGHT},"
        f" default {eif_ops.launch_plan(1).trees_in_flight}")
    good = True
    for shape in a.shapes.split(","):
        n, P = (int(v) for v in shape.split("x"))
        fr = make_frame(n, P, seed=P)
        for ext in (0, 1, P - 1):
            t = time.perf_counter()
            m = H2OExtendedIsolationForestEstimator(ntrees=100, sample_size=256, extension_level=ext, seed=1)
            m.train(training_frame=fr)
            torch.cuda.synchronize()
            say(f"{n} x {P}  extension_level {ext}   train {time.perf_counter() - t:7.2f} s")
            _, pk = timed_predict(m, fr, "hip")           # warm-up of each route at this shape
            _, pd_ = timed_predict(m, fr, "torch")
            tk, td = [], []
            for _ in range(a.repeats):
                tk.append(timed_predict(m, fr, "hip")[0])
                td.append(timed_predict(m, fr, "torch")[0])
            say(f"    predict  kernel route  {spread(tk)}")
            say(f"    predict  dense rule    {spread(td)}")
            faster = max(tk) < min(td)
            say(f"    kernel route {statistics.median(td) / statistics.median(tk):6.1f}x the dense rule by medians;"
                f" slowest kernel repeat under fastest dense repeat: {faster}")
            X = m._dinfo.expand(fr, pad=False)[0]
            kernel_only(m, X, a.repeats)
            del X
            good &= agreement(m, fr, pk, pd_, a.sample)
            del m, pk, pd_
        del fr
        torch.cuda.empty_cache()
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    main()
