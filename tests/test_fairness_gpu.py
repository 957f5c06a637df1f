"""fairness_metrics of a small GBM on the GPU (the sketch kernel of
ops/csrc/fairness.hip) against the per-group loop built from existing code:
the frame filtered to each group, `binomial_metrics` on its rows for auc /
aucpr / logloss and plain tensor counts at the labelling threshold.

Tolerances: both sides read identical integer histograms, and f64 trapezoid
sums over at most 2^18 terms of size at most 1 differ by at most 2^18 x 2^-53,
about 3e-11, between summation orders: 1e-10 for auc / aucpr / gini; 1e-9 for
logloss (two f64 sums of a few hundred terms in different orders)."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

PROT = ["region", "sex"]


@pytest.fixture(scope="module")
def fitted():
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    rng = np.random.default_rng(7)
    n = 3000
    X = rng.normal(size=(n, 4))
    region = rng.choice(["north", "south", "west"], n, p=[0.5, 0.3, 0.2]).astype(object)
    sex = rng.choice(["F", "M"], n).astype(object)
    lift = np.where(region == "south", -0.8, 0.0) + np.where(sex == "M", 0.5, 0.0)
    y = (X[:, 0] - 0.7 * X[:, 1] + lift + rng.normal(scale=0.7, size=n) > 0).astype(int)
    region[rng.random(n) < 0.04] = None
    sex[rng.random(n) < 0.03] = None
    resp = np.where(y == 1, "approved", "denied").astype(object)
    df = pd.DataFrame(X, columns=list("abcd"))
    df["region"], df["sex"], df["y"] = region, sex, resp
    df.loc[rng.random(n) < 0.02, "y"] = None
    fr = h2o.H2OFrame(df, column_types={"region": "enum", "sex": "enum", "y": "enum"})
    m = H2OGradientBoostingEstimator(ntrees=10, max_depth=3, seed=4)
    m.train(x=list("abcd") + PROT, y="y", training_frame=fr)
    return df, fr, m


def _oracle(df, fr, m, favorable):
    """One dict per occupied group, in the overview's order."""
    from h2o3_amd.models import metrics as mm
    dom = m._spec.response_domain
    assert dom == ["approved", "denied"]
    flip = favorable == dom[0]
    thr = m._label_threshold()
    lev = [df[c].fillna("NA").to_numpy() for c in PROT]
    order = [["north", "south", "west", "NA"], ["F", "M", "NA"]]
    rows = []
    for r in order[0]:
        for s in order[1]:
            mask = (lev[0] == r) & (lev[1] == s)
            if not mask.any():
                continue
            sub = fr[torch.tensor(mask, device=fr.vec("a").data.device)]
            p1 = m._predict_raw(sub)[:, -1].to(torch.float64)
            y = m._spec.y_tensor(sub)
            ok = (y >= 0) & ~torch.isnan(p1)
            sel = p1 >= thr
            yy = torch.where(y >= 0, y.to(torch.float64), torch.full_like(p1, float("nan")))
            if flip:
                y, sel, yy, p1 = 1 - y, ~sel, 1 - yy, 1.0 - p1
            bm = mm.binomial_metrics(yy, p1)
            rows.append({"region": r, "sex": s, "tp": int((ok & sel & (y == 1)).sum()),
                         "fp": int((ok & sel & (y == 0)).sum()), "tn": int((ok & ~sel & (y == 0)).sum()),
                         "fn": int((ok & ~sel & (y == 1)).sum()), "total": int(ok.sum()), "auc": bm.auc(),
                         "aucpr": bm.aucpr(), "gini": bm.gini(), "logloss": bm.logloss()})
    return rows


@pytest.mark.parametrize("favorable", ["denied", "approved"])
def test_fairness_metrics_equals_per_group_loop(fitted, favorable):
    df, fr, m = fitted
    out = m.fairness_metrics(fr, PROT, ["north", "F"], favorable)
    assert m._fairness_why is None, "the sketch must come from the HIP kernel on a GPU"
    ov = out["overview"].as_data_frame()
    want = _oracle(df, fr, m, favorable)
    assert len(ov) == len(want) == 12
    for i, w in enumerate(want):
        got = ov.iloc[i]
        assert (got["region"], got["sex"]) == (w["region"], w["sex"])
        for k in ("tp", "fp", "tn", "fn", "total"):
            assert int(got[k]) == w[k], (i, k, got[k], w[k])
        for k, tol in (("auc", 1e-10), ("aucpr", 1e-10), ("gini", 1e-10), ("logloss", 1e-9)):
            assert abs(got[k] - w[k]) <= tol, (i, k, got[k], w[k])
        assert int(got["selected"]) == w["tp"] + w["fp"]
    total = sum(w["total"] for w in want)
    assert total < 3000
    assert ov["relativeSize"].to_numpy() == pytest.approx([w["total"] / total for w in want], abs=1e-15)
    ref = ov.iloc[0]
    assert ref["AIR_selectedRatio"] == 1.0 and math.isnan(ref["p.value"])
    assert ov["AIR_selectedRatio"].to_numpy() == pytest.approx(
        (ov["selectedRatio"] / ref["selectedRatio"]).to_numpy(), abs=1e-15)
    assert ov["p.value"].iloc[1:].between(0, 1).all()
    assert len([k for k in out if k.startswith("thresholds_and_metrics_")]) == 12


def test_disparate_analysis_and_fair_shap_on_the_gpu(fitted):
    from h2o3_amd.models.fairness import disparate_analysis, fair_shap
    df, fr, m = fitted
    da = disparate_analysis([m], fr, PROT, ["north", "F"], "approved").as_data_frame()
    ov = m.fairness_metrics(fr, PROT, ["north", "F"], "approved")["overview"].as_data_frame().iloc[1:]
    assert da["air_min"].iloc[0] == ov["AIR_selectedRatio"].min()
    assert da["cair"].iloc[0] == pytest.approx((ov["relativeSize"] * ov["AIR_selectedRatio"]).sum(), abs=1e-12)
    sh = fair_shap(m, fr, PROT).as_data_frame()
    c = m.predict_contributions(fr).as_data_frame().astype(np.float64)
    mask = ((df["region"] == "south") & (df["sex"] == "M")).to_numpy()
    r = sh[(sh["region"] == "south") & (sh["sex"] == "M") & (sh["feature"] == "a")].iloc[0]
    assert r["rows"] == mask.sum()
    assert r["mean_contribution"] == pytest.approx(c["a"][mask].mean(), abs=1e-12)
    assert r["mean_abs_contribution"] == pytest.approx(c["a"][mask].abs().mean(), abs=1e-12)
