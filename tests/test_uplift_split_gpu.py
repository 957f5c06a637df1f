"""Uplift split search kernels (ops/csrc/tree_uplift.hip) through
tree_ops.uplift_splits against a plain fp64 oracle that loops over node,
feature and candidate with the formulae of TreeGrower._find_splits_torch_core,
and an Uplift DRF trained on the kernels against one trained on the torch path.

The histograms hold small non-negative integers, so every channel sum is exact
in f64 in any order and only the divergence arithmetic can differ: about 30
f64 operations on values of magnitude <= 14 (log 1e6), a few 1e-15; gains are
compared within 1e-12 and everything else with equality.  The seed is fixed so
that, in the oracle alone, the best and the second-best distinct gain of every
node with a valid split lie more than 1e-9 apart (asserted)."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd as h2o
from h2o3_amd.ops import tree_ops

pytestmark = pytest.mark.gpu

CRITERIA = ["uplift_kl", "uplift_chisquared", "uplift_euclidean"]
MIN_ROWS, F0, SEED = 10.0, 3, 7
NINF = -math.inf


def _diverg(S, crit):
    wt, wty, wc, wcy = S
    if not (wt > 0 and wc > 0):
        return 0.0
    pt = min(max(wty / max(wt, 1e-300), 1e-6), 1 - 1e-6)
    pc = min(max(wcy / max(wc, 1e-300), 1e-6), 1 - 1e-6)
    if crit == "uplift_kl":
        return pt * math.log(pt / pc) + (1 - pt) * math.log((1 - pt) / (1 - pc))
    if crit == "uplift_chisquared":
        return (pt - pc) ** 2 / pc + ((1 - pt) - (1 - pc)) ** 2 / (1 - pc)
    return (pt - pc) ** 2 + ((1 - pt) - (1 - pc)) ** 2


def _gain(L, R, sT, crit):
    nl, nr = L[0] + L[2], R[0] + R[2]
    if not (nl >= MIN_ROWS and nr >= MIN_ROWS and L[0] > 0 and L[2] > 0 and R[0] > 0 and R[2] > 0):
        return NINF
    nt = max(nl + nr, 1e-300)
    g = (nl / nt) * _diverg(L, crit) + (nr / nt) * _diverg(R, crit) - sT
    return g if g > 1e-12 else NINF


def _order(bins, cat):
    """Bins in split order: as they are, or stably by treatment - control rate, empty bins last."""
    B = len(bins)
    if not cat:
        return list(range(B))
    key = [b[1] / max(b[0], 1e-300) - b[3] / max(b[2], 1e-300) if b[0] + b[2] > 0 else math.inf for b in bins]
    return sorted(range(B), key=lambda b: (key[b], b))


def oracle(H, mask, is_cat, crit):
    """The split record of every node, its go-left mask, and the smallest gap
    between the best and the next distinct gain over the nodes with a split."""
    Fl, n, Bs, _ = H.shape
    B = Bs - 1
    out = {k: [] for k in ("gain", "feat", "t", "opt", "L", "R", "mask")}
    gap = math.inf
    for i in range(n):
        best, gains = (NINF, 0, 0, H[0, i, :0].sum(0)), set()     # gain, feature, k, L
        for f in range(Fl):
            bins, na = H[f, i, :B], H[f, i, B]
            order = _order(bins, is_cat[f])
            cum = np.cumsum(bins[order], 0)
            totnn, T = cum[-1], cum[-1] + na
            sT, has_na = _diverg(T, crit), na[0] + na[2] > 0
            cands = [(t, cum[t], (totnn - cum[t]) + na) for t in range(B - 1)]
            cands += [(B - 1 + t, cum[t] + na, totnn - cum[t]) if has_na else (B - 1 + t, None, None) for t in range(B - 1)]
            cands += [(2 * (B - 1), totnn, na) if has_na else (2 * (B - 1), None, None)]
            for k, L, R in cands:
                g = _gain(L, R, sT, crit) if (L is not None and mask[i, f]) else NINF
                gains.add(g)
                if g > best[0]:
                    best = (g, f, k, L)
        g, f, k, L = best
        opt = 0 if k < B - 1 else (1 if k < 2 * (B - 1) else 2)
        t = k if opt == 0 else (k - (B - 1) if opt == 1 else 0)
        bins = H[f, i, :B]
        rank = np.empty(B, dtype=np.int64)
        rank[_order(bins, is_cat[f])] = np.arange(B)
        left = np.ones(B, bool) if opt == 2 else rank <= t
        if is_cat[f]:
            left = np.where(bins[:, 0] + bins[:, 2] <= 0, opt == 1, left)
        for key, v in zip(out, (g, F0 + f, t, opt, L, H[f, i].sum(0) - L, np.append(left, opt == 1))):
            out[key].append(v)
        top = sorted(gains - {NINF})
        if len(top) > 1:
            gap = min(gap, top[-1] - top[-2])
    out["tot"] = H[0].sum(1)
    return out, gap


def _hist(rng, n, Fl, B, kind):
    """[Fl, n, B + 1, 4] of small integers: runs of empty bins, feature 0 without NA rows,
    the last feature with; kind 'nocontrol' / 'minrows' rewrites every node that way."""
    wt, wc = rng.integers(0, 40, (2, Fl, n, B + 1))
    H = np.stack([wt, rng.integers(0, wt + 1), wc, rng.integers(0, wc + 1)], -1).astype(np.float64)
    for s in {B // 7, B // 7 + 1, B // 2, B - 2, B - 1} & set(range(B)) if B > 2 else ():
        H[:, :, s] = 0
    H[:, :, B] += [12, 3, 12, 4]
    if Fl > 1 or kind == "na0":
        H[0, :, B] = 0
    if kind == "nocontrol":
        H[..., 2:] = 0
    if kind == "minrows":
        H[:] = 0
        H[:, :, [0, B // 2, B - 1]] = [3, 1, 3, 2]
        H[:, :, B] = [1, 0, 1, 0]
    return H


def _problems(B, n, Fl, seed=SEED):
    """(H, mask, is_cat) problems of one case.  n = 5: node 1 without control rows, node 2
    emptied by min_rows, node 3 with every feature masked, feature 1 masked at node 0, feature 1
    categorical.  n = 1: the same variants as separate single-pair problems."""
    rng = np.random.default_rng([seed, B, n])
    if n == 1:
        return [(_hist(rng, 1, 1, B, kind), np.array([[kind != "masked"]]), [cat])
                for kind, cat in (("na0", False), ("na", True), ("nocontrol", True), ("minrows", False), ("masked", False))]
    H = _hist(rng, n, Fl, B, "")
    H[:, 1] = _hist(rng, 1, Fl, B, "nocontrol")[:, 0]
    H[:, 2] = _hist(rng, 1, Fl, B, "minrows")[:, 0]
    mask = np.ones((n, Fl), bool)
    mask[3], mask[0, 1] = False, False
    return [(H, mask, [False, True, False])]


@pytest.mark.parametrize("n,Fl", [(1, 1), (5, 3)])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 300])
@pytest.mark.parametrize("crit", CRITERIA)
def test_kernel_matches_oracle(crit, B, n, Fl):
    dev = torch.device("cuda:0")
    for H, mask, is_cat in _problems(B, n, Fl):
        ref, gap = oracle(H, mask, is_cat, crit)
        assert gap > 1e-9, gap
        res = tree_ops.uplift_splits(torch.tensor(H, device=dev), torch.tensor(mask, device=dev),
                                     torch.tensor(is_cat, device=dev), F0, F0 + Fl, crit, MIN_ROWS)
        got = {k: v.cpu().numpy() for k, v in res.items()}
        print(crit, B, n, Fl, "gain", got["gain"], "ref", ref["gain"], "gap", gap)
        assert got["feat"].dtype == got["t"].dtype == got["opt"].dtype == np.int64 and got["na_left"].dtype == bool
        assert got["mask"].dtype == np.uint8 and got["mask"].shape == (n, B + 1)
        np.testing.assert_array_equal(got["tot"], ref["tot"])
        for i in range(n):
            if ref["gain"][i] == NINF:
                assert got["gain"][i] == NINF
                continue
            assert abs(got["gain"][i] - ref["gain"][i]) <= 1e-12
            for k in ("feat", "t", "opt", "L", "R", "mask"):
                np.testing.assert_array_equal(got[k][i], ref[k][i], err_msg=f"{k} of node {i}")
            assert got["na_left"][i] == (ref["opt"][i] == 1)


def _data(n=4000, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 3))
    t = rng.integers(0, 2, n)
    effect = np.where(X[:, 0] > 0, 0.4, -0.1)
    y = (rng.random(n) < np.clip(0.3 + t * effect, 0.01, 0.99)).astype(int)
    df = pd.DataFrame(X, columns=["a", "b", "c"])
    df.loc[rng.random(n) < 0.05, "b"] = np.nan
    lev = rng.integers(0, 12, n)
    df["g"] = pd.Series(np.where(rng.random(n) < 0.05, None, np.char.add("l", lev.astype(str))), dtype=object)
    df["treatment"] = np.where(t == 1, "treatment", "control")
    df["y"] = np.where(y == 1, "1", "0")
    return df


@pytest.mark.parametrize("metric", ["KL", "ChiSquared", "Euclidean"])
def test_forest_matches_torch_path(metric, monkeypatch):
    from h2o3_amd.estimators import H2OUpliftRandomForestEstimator
    h2o.init(device="cuda:0", verbose=False)
    fr = h2o.H2OFrame(_data())
    preds = []
    for path in ("hip", "torch"):
        monkeypatch.setenv("H2O3_UPLIFT_SPLIT", path)
        m = H2OUpliftRandomForestEstimator(ntrees=3, max_depth=5, min_rows=20, seed=1, treatment_column="treatment",
                                           uplift_metric=metric)
        m.train(x=["a", "b", "c", "g"], y="y", training_frame=fr)
        preds.append(m.predict(fr).as_data_frame().values.astype(np.float64))
    assert preds[0].shape == (4000, 3)
    assert np.abs(preds[0] - preds[1]).max() <= 1e-6
