"""fairness_metrics on the grouped score sketch (ops/fairness_ops.group_sketch:
fairness.hip) against the per-group loop built from what existed before it: a
row filter plus `binomial_metrics` per group.  One GPU.

  python scripts/fairness_mb.py model  [out.txt]  a GBM of 20 depth-5 trees scored on N rows with 4 x 3 x 4 = 48
                                                  occupied groups: fairness_metrics (scoring included), the
                                                  scoring alone, and the loop (the frame scored once, then per
                                                  group a boolean filter of score and response,
                                                  binomial_metrics and the four counts), alternated in one
                                                  process; host clock around a device synchronise
  python scripts/fairness_mb.py sketch [out.txt]  group_sketch alone on N rows x 48 groups, f32 scores: uniform
                                                  random scores and 7 distinct scores (an early boosting
                                                  round), device events
  python scripts/fairness_mb.py trace             5 launches of the random-score sketch and nothing else, for a
                                                  kernel trace

Each mode is one process and needs a GPU; the lines are appended to out.txt if
given.  Times are medians of FAIR_MB_REPS (5) repeats after a warm-up run.
Env: FAIR_MB_N (10 000 000) overrides the rows; FAIR_MB_PROFILE=1 prints a host
profile (cProfile) of one fairness_metrics call in model mode."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N = int(os.environ.get("FAIR_MB_N", 10_000_000))
REPS = int(os.environ.get("FAIR_MB_REPS", 5))
PROT = ["region", "band", "origin"]
CARD = [4, 3, 4]


def _frame(n, seed):
    from h2o3_amd.core.frame import H2OFrame
    from h2o3_amd.core.vec import T_REAL, Vec, make_enum
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, 4), generator=g, device=dev)
    codes = [torch.randint(0, c, (n,), generator=g, device=dev, dtype=torch.int32) for c in CARD]
    logit = X[:, 0] - 0.7 * X[:, 1] + 0.4 * (codes[0] == 1) - 0.6 * (codes[2] == 2)
    y = (torch.rand(n, generator=g, device=dev) < torch.sigmoid(logit)).to(torch.int32)
    vecs = [Vec(X[:, j].contiguous(), T_REAL) for j in range(4)]
    vecs += [make_enum(c, [f"{nm}{i}" for i in range(k)]) for c, nm, k in zip(codes, PROT, CARD)]
    vecs.append(make_enum(y, ["no", "yes"]))
    return H2OFrame.from_vecs(vecs, list("abcd") + PROT + ["y"])


def _clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def _loop(m, fr, groups):
    """What a caller could do before the sketch: score once, then per group
    filter the score and the response and build the binomial metrics."""
    from h2o3_amd.models import metrics as mm
    p1 = m._predict_raw(fr)[:, -1]
    y = m._spec.y_tensor(fr)
    thr = m._label_threshold()
    rows = []
    for k in range(groups.G):
        mask = groups.ids == k
        pk, yk = p1[mask], y[mask]
        bm = mm.binomial_metrics(yk.to(torch.float64), pk)
        sel = pk.to(torch.float64) >= thr
        cm = torch.stack([(sel & (yk == 1)).sum(), (sel & (yk == 0)).sum(), (~sel & (yk == 0)).sum(),
                          (~sel & (yk == 1)).sum()]).tolist()
        rows.append((cm, bm.auc(), bm.aucpr(), bm.logloss()))
    return rows


def model(say):
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    from h2o3_amd.models.fairness import ProtectedGroups, fairness_metrics
    h2o.init(verbose=False)
    m = H2OGradientBoostingEstimator(ntrees=20, max_depth=5, seed=1)
    m.train(x=list("abcd") + PROT, y="y", training_frame=_frame(200_000, 1))
    fr = _frame(N, 2)
    ref = [f"{nm}0" for nm in PROT]
    groups = ProtectedGroups(fr, PROT)
    new = lambda: fairness_metrics(m, fr, PROT, ref, "yes")["overview"].as_data_frame()   # noqa: E731
    old = lambda: _loop(m, fr, groups)                                                    # noqa: E731
    score = lambda: m._predict_raw(fr)                                                    # noqa: E731
    _, ov = _clock(new)
    _, rows = _clock(old)
    _clock(score)
    assert m._fairness_why is None and len(ov) == groups.G == 48
    # same results at the timed size
    d_cnt = max(abs(int(ov[c].iloc[k]) - rows[k][0][j]) for k in range(48)
                for j, c in enumerate(("tp", "fp", "tn", "fn")))
    d_auc = max(abs(ov["auc"].iloc[k] - rows[k][1]) for k in range(48))
    d_pr = max(abs(ov["aucpr"].iloc[k] - rows[k][2]) for k in range(48))
    d_ll = max(abs(ov["logloss"].iloc[k] - rows[k][3]) for k in range(48))
    if os.environ.get("FAIR_MB_PROFILE"):
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        new()
        torch.cuda.synchronize()
        pr.disable()
        pstats.Stats(pr).sort_stats("cumulative").print_stats(30)
    tn, to, ts = [], [], []
    for _ in range(REPS):
        tn.append(_clock(new)[0])
        to.append(_clock(old)[0])
        ts.append(_clock(score)[0])
    med = statistics.median
    say(f"model  N={N} groups=48 trees=20 depth=5 reps={REPS} (medians, host clock around a synchronise)")
    say(f"  fairness_metrics (scoring + sketch + tables)   {med(tn) * 1e3:9.1f} ms   "
        f"min {min(tn) * 1e3:.1f} max {max(tn) * 1e3:.1f}")
    say(f"  per-group loop (scoring + 48 x filter/metrics) {med(to) * 1e3:9.1f} ms   "
        f"min {min(to) * 1e3:.1f} max {max(to) * 1e3:.1f}")
    say(f"  scoring alone (_predict_raw)                   {med(ts) * 1e3:9.1f} ms")
    say(f"  loop / fairness_metrics = {med(to) / med(tn):.2f}x")
    say(f"  max |difference| over the 48 groups: counts {d_cnt}, auc {d_auc:.3g}, aucpr {d_pr:.3g}, logloss {d_ll:.3g}")


def _sketch_inputs(kind):
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "random":
        p = torch.rand(N, generator=g, device="cuda")
    else:
        p = torch.sigmoid(torch.randint(-3, 4, (N,), generator=g, device="cuda").float())
    y = (torch.rand(N, generator=g, device="cuda") < 0.3).to(torch.int32)
    grp = torch.randint(0, 48, (N,), generator=g, device="cuda", dtype=torch.int32)
    return p, y, grp


def sketch(say):
    from h2o3_amd.ops import fairness_ops as fo
    say(f"sketch N={N} groups=48 nb=2^18 f32 scores reps={REPS} (medians, device events; zeroing the 201 MB of cnt "
        f"included)")
    for kind in ("random", "seven distinct"):
        p, y, grp = _sketch_inputs(kind)
        out = tuple(torch.zeros(s, dtype=d, device="cuda") for s, d in
                    (((48, 2, 1 << 18), torch.int64), ((48, 4), torch.int64), ((48, 2), torch.float64)))
        fo.group_sketch(p, y, grp, 48, 0.5)
        t_all = [_events(lambda: fo.group_sketch(p, y, grp, 48, 0.5))[0] for _ in range(REPS)]
        t_k = [_events(lambda: fo.group_sketch(p, y, grp, 48, 0.5, out=out))[0] for _ in range(REPS)]
        assert int(out[1].sum()) == REPS * N
        # bytes the pass must read: 4 (score) + 4 (response) + 4 (group) per row
        say(f"  {kind:15s} group_sketch {statistics.median(t_all) * 1e3:8.3f} ms; into given outputs "
            f"{statistics.median(t_k) * 1e3:8.3f} ms = {12 * N / statistics.median(t_k) * 1e-9:.0f} GB/s of row reads")


def trace(say):
    from h2o3_amd.ops import fairness_ops as fo
    p, y, grp = _sketch_inputs("random")
    for _ in range(5):
        r = fo.group_sketch(p, y, grp, 48, 0.5)
    torch.cuda.synchronize()
    say(f"trace: 5 launches, N={N}, counted rows {int(r.cm.sum())}")


if __name__ == "__main__":
    mode = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else None

    def say(line):
        print(line, flush=True)
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")
    if not torch.cuda.is_available():
        sys.exit("fairness_mb.py needs a GPU")
    {"model": model, "sketch": sketch, "trace": trace}[mode](say)
