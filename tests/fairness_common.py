"""Shared pieces of the fairness tests: a hand-made frame, a model that scores
with a column of the frame (so the tests control every score), and a
pure-numpy brute force of the overview table."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pandas as pd
import torch

SCORES = np.array([0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95])    # 0.5 is the threshold itself
SEX = ["F", "M"]
RACE = ["a", "b", "c"]
THR = 0.5


def make_df(n=400, seed=0):
    """sex x race with NAs in both, a response that depends on the score, and
    two score columns.  Group (M, a), the reference, has every positive
    selected (fn = 0) and no negative selected (fp = 0), so the AIR of fn and
    fp divides by zero there."""
    rng = np.random.default_rng(seed)
    sex = rng.choice(SEX, n).astype(object)
    race = rng.choice(RACE, n, p=[0.5, 0.3, 0.2]).astype(object)
    sex[rng.random(n) < 0.06] = None
    race[rng.random(n) < 0.05] = None
    score = rng.choice(SCORES, n)
    score2 = rng.choice(SCORES, n)
    y = (rng.random(n) < 0.25 + 0.5 * score).astype(int)
    ref = (sex == "M") & (race == "a")
    y[ref] = (score[ref] >= THR).astype(int)
    resp = np.where(y == 1, "yes", "no").astype(object)
    resp[rng.random(n) < 0.03] = None
    score[5::57] = np.nan
    return pd.DataFrame({"x": rng.normal(size=n), "sex": sex, "race": race, "score": score, "score2": score2,
                         "y": resp})


def to_frame(df):
    import h2o3_amd as h2o
    return h2o.H2OFrame(df, column_types={"sex": "enum", "race": "enum", "y": "enum"})


class ScoredModel:
    """A binomial 'model' whose P(yes) is a column of the frame."""

    def __init__(self, column="score", thr=THR, model_id=None):
        self.column, self.thr = column, thr
        self.model_id = model_id or f"scored_{column}"
        self._spec = SimpleNamespace(nclasses=2, y="y", x=[column], response_domain=["no", "yes"],
                                     y_tensor=lambda fr: fr.vec("y").data.to(torch.int64))

    def _predict_raw(self, frame):
        p = frame.vec(self.column).as_float(torch.float64)
        return torch.stack([1 - p, p], 1)

    def _label_threshold(self):
        return self.thr


def fisher_exact(a, b, c, d):
    """Two-sided Fisher p of [[a, b], [c, d]] by exact enumeration."""
    r1, r2, c1 = a + b, c + d, a + c
    den = math.comb(r1 + r2, c1)
    pr = {x: Fraction(math.comb(r1, x) * math.comb(r2, c1 - x), den) for x in range(max(0, c1 - r2), min(r1, c1) + 1)}
    return float(sum(v for v in pr.values() if v <= pr[a]))


def _auc_pairs(sp, sn):
    if len(sp) == 0 or len(sn) == 0:
        return float("nan")
    gt = (sp[:, None] > sn[None, :]).sum()
    eq = (sp[:, None] == sn[None, :]).sum()
    return (gt + 0.5 * eq) / (len(sp) * len(sn))


def _aucpr_steps(s, y):
    P = int(y.sum())
    if P == 0 or P == len(y):
        return float("nan")
    rec, prec = [0.0], []
    tp = fp = 0
    for v in sorted(set(s.tolist()), reverse=True):
        tp += int(((s == v) & (y == 1)).sum())
        fp += int(((s == v) & (y == 0)).sum())
        prec.append(tp / (tp + fp))
        rec.append(tp / P)
    prec = [prec[0]] + prec
    return float(sum((rec[i] - rec[i - 1]) * (prec[i] + prec[i - 1]) / 2 for i in range(1, len(rec))))


def _div(a, b):
    return a / b if b > 0 else float("nan")


def brute_overview(df, column, protected, domains, reference, favorable="yes", thr=THR):
    """The overview table as a list of dicts, one per occupied group in
    mixed-radix order (domain order, NA last), by filtering the rows of each
    group."""
    score = df[column].to_numpy(dtype=np.float32).astype(float)      # a frame keeps real columns in f32
    yraw = df["y"].to_numpy(dtype=object)
    y = np.array([-1 if v is None or v != v else int(v == "yes") for v in yraw])
    sel = score >= thr
    p = score.copy()
    if favorable == "no":
        y = np.where(y >= 0, 1 - y, y)
        p = 1.0 - score
        sel = ~sel
    lev = [np.array(["NA" if v is None or v != v else v for v in df[c].to_numpy(dtype=object)], dtype=object)
           for c in protected]
    keys = sorted({tuple(l[i] for l in lev) for i in range(len(df))},
                  key=lambda t: tuple((d + ["NA"]).index(v) for d, v in zip(domains, t)))
    counted = ~np.isnan(score) & (y >= 0)
    rows = []
    for k in keys:
        m = counted & np.all([l == v for l, v in zip(lev, k)], axis=0)
        yy, pp, ss = y[m], p[m], sel[m]
        tp, fp = int((ss & (yy == 1)).sum()), int((ss & (yy == 0)).sum())
        tn, fn = int((~ss & (yy == 0)).sum()), int((~ss & (yy == 1)).sum())
        total = int(m.sum())
        auc = _auc_pairs(pp[yy == 1], pp[yy == 0])
        pc = np.clip(pp, 1e-15, 1 - 1e-15)
        r = dict(zip(protected, k))
        r.update({"tp": tp, "fp": fp, "tn": tn, "fn": fn, "total": total, "relativeSize": _div(total, counted.sum()),
                  "accuracy": _div(tp + tn, total), "precision": _div(tp, tp + fp),
                  "f1": _div(2 * tp, 2 * tp + fp + fn), "tpr": _div(tp, tp + fn), "tnr": _div(tn, tn + fp),
                  "fpr": _div(fp, fp + tn), "fnr": _div(fn, fn + tp), "auc": auc, "aucpr": _aucpr_steps(pp, yy),
                  "gini": 2 * auc - 1, "selected": tp + fp, "selectedRatio": _div(tp + fp, total),
                  "logloss": _div(float(-(np.where(yy == 1, np.log(pc), np.log(1 - pc))).sum()), total)})
        rows.append(r)
    metrics = [c for c in rows[0] if c not in protected]
    ref = next((r for r in rows if tuple(r[c] for c in protected) == tuple(reference)), None)
    for r in rows:
        for mname in metrics:
            rv = ref[mname] if ref is not None else 0
            r["AIR_" + mname] = r[mname] / rv if ref is not None and rv == rv and rv != 0 else float("nan")
        if ref is None or r is ref or r["total"] == 0 or ref["total"] == 0:
            r["p.value"] = float("nan")
        else:
            r["p.value"] = fisher_exact(r["selected"], r["total"] - r["selected"],
                                        ref["selected"], ref["total"] - ref["selected"])
    return rows
