"""Fairness metrics of binomial models over intersections of protected columns.

Reference: water/rapids/ast/prims/models/AstFairnessMetrics.java (one
filtered frame and one ModelMetricsBinomial per intersection of protected
levels; adverse impact ratios against a reference group; Fisher's exact test
or the G-test on the selected / not selected counts) and
h2o-py/h2o/explanation/_explain.py (disparate_analysis,
inspect_model_fairness, fair_pd, fair_shap).

Here the frame is scored once and read once: every row carries a dense group
id, and the grouped score sketch (ops/fairness_ops.py, csrc/fairness.hip)
fills a logit histogram of favourable / unfavourable rows per group, the
confusion matrix at the model's labelling threshold per group and the loss
sums per group.  One all-reduce merges the ranks' sketches and every table is
read off the merged sketch with the functions `binomial_metrics` uses for the
whole frame (models/metrics.py _hist_auc, _threshold_table_hist).  No row
leaves its rank and no per-group frame is materialised.  Fairness tables count
rows: a weights column is ignored and every row counts 1.
"""
from __future__ import annotations

import math

import numpy as np
import pandas as pd
import torch

from ..core.frame import H2OFrame
from ..core.vec import T_ENUM, T_INT, T_REAL, Vec, make_enum_from_strings
from ..parallel import cloud
from ..parallel import collectives as coll
from . import metrics as mm

METRICS = ["tp", "fp", "tn", "fn", "total", "relativeSize", "accuracy", "precision", "f1", "tpr", "tnr", "fpr", "fnr",
           "auc", "aucpr", "gini", "selected", "selectedRatio", "logloss"]
FISHER_MAX_MARGIN = 100_000     # Fisher's exact test up to this smallest margin (at most 100 001 terms)
MAX_INTERSECTIONS = 1 << 24     # product of (cardinality + 1) over the protected columns
_NAN = float("nan")


# ------------------------------------------------------------------ p.value
def _fisher_two_sided(a, b, c, d):
    """Two-sided Fisher's exact test of [[a, b], [c, d]]: the sum of the
    probabilities of all tables with these margins no more likely than the
    observed one (relative slack 1e-7)."""
    r1, c1, n = a + b, a + c, a + b + c + d
    lo, hi = max(0, c1 - (c + d)), min(r1, c1)
    x = torch.arange(lo, hi + 1, dtype=torch.float64)

    def lg(v):
        return torch.lgamma(torch.as_tensor(v, dtype=torch.float64) + 1.0)
    const = lg(r1) + lg(n - r1) + lg(c1) + lg(n - c1) - lg(n)
    logp = const - (lg(x) + lg(r1 - x) + lg(c1 - x) + lg(n - r1 - c1 + x))
    pr = torch.exp(logp)
    obs = pr[a - lo]
    return min(1.0, float(pr[pr <= obs * (1.0 + 1e-7)].sum()))


def _g_test(a, b, c, d):
    """G-test of independence of [[a, b], [c, d]], one degree of freedom:
    G = 2 sum O ln(O / E), p = erfc(sqrt(G / 2))."""
    n = a + b + c + d
    half_g = 0.0
    for o, r, k in ((a, a + b, a + c), (b, a + b, b + d), (c, c + d, a + c), (d, c + d, b + d)):
        if o > 0:
            half_g += o * math.log(o * n / (r * k))
    return math.erfc(math.sqrt(max(half_g, 0.0)))


def table_p_value(a, b, c, d):
    """p.value of the 2 x 2 table [[a, b], [c, d]] = (group, reference group)
    x (selected, not selected): Fisher's exact test when the smallest margin
    is at most FISHER_MAX_MARGIN (a bound on cost), else the G-test.  NaN for
    a table with an empty row."""
    a, b, c, d = int(a), int(b), int(c), int(d)
    if a + b == 0 or c + d == 0:
        return _NAN
    if min(a + b, c + d, a + c, b + d) <= FISHER_MAX_MARGIN:
        return _fisher_two_sided(a, b, c, d)
    return _g_test(a, b, c, d)


# ------------------------------------------------------------------ groups
class ProtectedGroups:
    """Dense ids of the occupied intersections of the protected columns.

    ids      [nlocal] int32: this rank's rows, 0 .. G - 1 in mixed-radix order
    levels   per group, the tuple of level names ("NA" for a missing value)
    G        number of occupied groups (over all ranks)
    """
    def __init__(self, frame: H2OFrame, protected_columns):
        cols = [protected_columns] if isinstance(protected_columns, str) else list(protected_columns or [])
        if not cols:
            raise ValueError("protected_columns: at least one column is needed")
        vecs = []
        for c in cols:
            if c not in frame.names:
                raise ValueError(f"protected column '{c}' is not in the frame")
            v = frame.vec(c)
            if v.type != T_ENUM:
                raise ValueError(f"protected column '{c}' must be categorical (enum), it is {v.type}")
            vecs.append(v)
        radix = [len(v.domain) + 1 for v in vecs]              # the last code of a column is NA
        size = int(np.prod([int(r) for r in radix], dtype=object))
        if size > MAX_INTERSECTIONS:
            raise ValueError(f"protected columns {cols} span {size} intersections, at most {MAX_INTERSECTIONS}")
        raw = torch.zeros(frame.nlocal, dtype=torch.int64, device=vecs[0].data.device)
        for v, r in zip(vecs, radix):
            code = v.data.to(torch.int64)
            raw = raw * r + torch.where(code < 0, torch.full_like(code, r - 1), code)
        occ = torch.bincount(raw, minlength=size)
        coll.allreduce_(occ)
        occupied = torch.nonzero(occ > 0).flatten()
        remap = torch.full((size,), -1, dtype=torch.int32, device=raw.device)
        remap[occupied] = torch.arange(occupied.numel(), dtype=torch.int32, device=raw.device)
        self.columns = cols
        self.ids = remap[raw]
        self.G = int(occupied.numel())
        self._codes = {}
        self.levels = []
        for k, gid in enumerate(occupied.cpu().tolist()):
            digits = []
            for r in reversed(radix):
                digits.append(gid % r)
                gid //= r
            digits.reverse()
            self._codes[tuple(digits)] = k
            self.levels.append(tuple("NA" if dg == r - 1 else v.domain[dg] for dg, v, r in zip(digits, vecs, radix)))
        self._check = [(c, [str(x) for x in v.domain]) for c, v in zip(cols, vecs)]

    def group_of(self, reference):
        """Dense id of the group with these levels (one per protected column),
        None when no row has them."""
        ref = [reference] if isinstance(reference, str) else list(reference or [])
        if len(ref) != len(self.columns):
            raise ValueError(f"reference needs one level per protected column {self.columns}, got {ref}")
        digits = []
        for (c, dom), lev in zip(self._check, ref):
            if str(lev) not in dom:
                raise ValueError(f"reference level '{lev}' is not in the domain of protected column '{c}'")
            digits.append(dom.index(str(lev)))
        return self._codes.get(tuple(digits))


def _check_binomial(model):
    spec = getattr(model, "_spec", None)
    if spec is None or spec.nclasses != 2:
        raise ValueError(f"fairness metrics need a binomial model, '{getattr(model, 'model_id', model)}' is not one")
    return spec


def _response_codes(spec, frame):
    if spec.y not in frame.names:
        raise ValueError(f"the response column '{spec.y}' is not in the frame")
    y = spec.y_tensor(frame)
    if y.is_floating_point():
        y = torch.where(torch.isnan(y), torch.full_like(y, -1.0), y)
    return y.to(torch.int32)


def _favorable_flip(spec, favorable_class):
    dom = [str(d) for d in spec.response_domain]
    if str(favorable_class) not in dom:
        raise ValueError(f"favorable_class '{favorable_class}' is not in the response domain {dom}")
    return dom.index(str(favorable_class)) == 0


def _ratio(num, den):
    return num / den if den > 0 else _NAN


def _overview(model, frame, groups: ProtectedGroups, ref_group, y, flip, tables=True):
    """(overview DataFrame, {group levels: threshold table as a dict of
    arrays}) of one model."""
    from ..ops import fairness_ops
    p1 = model._predict_raw(frame)[:, -1]
    if p1.dtype not in (torch.float32, torch.float64):
        p1 = p1.to(torch.float64)
    G, nb = groups.G, mm._NB_BIN
    sk = fairness_ops.group_sketch(p1, y.to(p1.device), groups.ids.to(p1.device), G, model._label_threshold(),
                                   flip=flip, nb=nb)
    model._fairness_why = sk.why
    cnt, cm, sums = sk.cnt, sk.cm, sk.sums
    coll.allreduce_(cnt)
    coll.allreduce_(cm)
    coll.allreduce_(sums)
    cm_h = cm.cpu().numpy()
    sums_h = sums.cpu().numpy()
    # every group's occupied bins in one device-to-host copy (binomial_metrics reads the whole frame's the same
    # way), split by group on the host
    occ = cnt.sum(1) > 0
    gi, bi = torch.nonzero(occ, as_tuple=True)                          # by group, then by bin
    lower = mm._bin_lower_prob(nb, cnt.device)
    bins = torch.stack([cnt[gi, 1, bi].to(torch.float64), cnt[gi, 0, bi].to(torch.float64), lower[bi]]).cpu()
    ends = np.cumsum(occ.sum(1).cpu().numpy())
    all_rows = int(cm_h.sum())
    rows, thr_tabs = [], {}
    for k in range(G):
        tp, fp, tn, fn = (int(v) for v in cm_h[k])
        total = tp + fp + tn + fn
        c = bins[:, int(ends[k - 1]) if k else 0:int(ends[k])]           # positives, negatives, bin lower edge
        auc, aucpr = mm._hist_auc(c[0], c[1])
        if tables:
            # a group whose rows all have an NA response or a NaN score has no bin: a table of no rows
            thr_tabs[groups.levels[k]] = mm._threshold_table_hist(c[0], c[1], c[2]) if c.shape[1] else \
                mm._cm_family(c[2], c[0], c[1], 0.0, 0.0)
        sel = tp + fp
        rows.append({"tp": tp, "fp": fp, "tn": tn, "fn": fn, "total": total,
                     "relativeSize": _ratio(total, all_rows),
                     "accuracy": _ratio(tp + tn, total), "precision": _ratio(tp, tp + fp),
                     "f1": _ratio(2 * tp, 2 * tp + fp + fn), "tpr": _ratio(tp, tp + fn), "tnr": _ratio(tn, tn + fp),
                     "fpr": _ratio(fp, fp + tn), "fnr": _ratio(fn, fn + tp), "auc": auc, "aucpr": aucpr,
                     "gini": 2 * auc - 1 if auc == auc else _NAN, "selected": sel,
                     "selectedRatio": _ratio(sel, total), "logloss": _ratio(float(sums_h[k, 0]), total)})
    ref = rows[ref_group] if ref_group is not None else None
    for k, r in enumerate(rows):
        for m in METRICS:
            rv = ref[m] if ref is not None else 0
            r["AIR_" + m] = r[m] / rv if ref is not None and rv == rv and rv != 0 else _NAN
        if ref is None or k == ref_group:
            r["p.value"] = _NAN
        else:
            r["p.value"] = table_p_value(r["selected"], r["total"] - r["selected"],
                                         ref["selected"], ref["total"] - ref["selected"])
    df = pd.DataFrame(rows, columns=METRICS + ["AIR_" + m for m in METRICS] + ["p.value"])
    for j, c in enumerate(groups.columns):
        df.insert(j, c, [lv[j] for lv in groups.levels])
    return df, thr_tabs


def _table_cols(names, cols) -> H2OFrame:
    """A small result table, the same whole frame on every rank, from columns
    that are numpy arrays (numeric) or lists of strings (categorical).  All
    numeric columns travel in one copy and stay f64: ratios and p.values keep
    their digits."""
    num = [j for j, c in enumerate(cols) if isinstance(c, np.ndarray) and c.dtype != object]
    host = np.ascontiguousarray(np.stack([cols[j].astype(np.float64) for j in num])) if num else None
    block = torch.from_numpy(host).to(cloud.device()) if num else None
    row = {j: i for i, j in enumerate(num)}
    vecs = []
    for j, c in enumerate(cols):
        if j in row:
            a = host[row[j]]
            whole = a.size > 0 and bool(np.isfinite(a).all()) and bool((a == np.round(a)).all())
            v = Vec(block[row[j]], T_INT if whole else T_REAL)
        else:
            vals = list(c)
            v = make_enum_from_strings(vals, domain=sorted({str(x) for x in vals}))
        v.replicated = True
        vecs.append(v)
    return H2OFrame.from_vecs(vecs, [str(n) for n in names])


def _table(df: pd.DataFrame) -> H2OFrame:
    return _table_cols(list(df.columns), [df[c].to_numpy() if df[c].dtype != object else df[c].tolist()
                                          for c in df.columns])


def _prepare(model, frame, protected_columns, reference, favorable_class, groups=None):
    spec = _check_binomial(model)
    groups = groups if groups is not None else ProtectedGroups(frame, protected_columns)
    ref_group = groups.group_of(reference)
    return spec, groups, ref_group, _favorable_flip(spec, favorable_class)


def fairness_metrics(model, frame: H2OFrame, protected_columns, reference, favorable_class):
    """Fairness tables of a binomial model on `frame`.

    protected_columns  enum columns of the frame; every occupied intersection
                       of their levels is a group, NA being the level "NA"
    reference          one level per protected column: the reference group
    favorable_class    the level of the response that is the good outcome

    Returns {"overview": H2OFrame, "thresholds_and_metrics_<levels>": H2OFrame
    per group}.  The overview has the protected columns, then per group tp,
    fp, tn, fn, total, relativeSize, accuracy, precision, f1, tpr, tnr, fpr,
    fnr, auc, aucpr, gini, selected, selectedRatio, logloss (the favourable
    class positive, at the model's labelling threshold), AIR_<metric> = the
    metric over the reference group's (NaN when that is 0 or the reference
    group has no row) and the p.value of the (selected, not selected) x
    (group, reference group) table.  A group is occupied when a row has its
    levels; if all its rows have an NA response or a NaN score it counts no
    row: total 0, NaN ratios (and NaN AIR of them), a NaN p.value and a
    threshold table of no rows."""
    spec, groups, ref_group, flip = _prepare(model, frame, protected_columns, reference, favorable_class)
    df, tabs = _overview(model, frame, groups, ref_group, _response_codes(spec, frame), flip)
    out = {"overview": _table(df)}
    for lv, tab in tabs.items():
        out["thresholds_and_metrics_" + ",".join(lv)] = _table_cols(list(tab), list(tab.values()))
    return out


def _model_list(models):
    if hasattr(models, "_leaderboard") or hasattr(models, "leader"):       # an AutoML object
        lb = getattr(models, "_leaderboard", None)
        return list(lb.models) if lb is not None and lb.models else list(getattr(models, "models", []))
    if isinstance(models, (list, tuple)):
        return list(models)
    return [models]


def _board_metric(model, name):
    for kw in ({"xval": True}, {"valid": True}, {"train": True}):
        try:
            v = getattr(model, name)(**kw)
        except (ValueError, AttributeError, TypeError):
            v = None
        if v is not None:
            return float(v)
    return None


def disparate_analysis(models, frame: H2OFrame, protected_columns, reference, favorable_class,
                       air_metric="selectedRatio", alpha=0.05):
    """One row per binomial model of `models` (a list or an AutoML object):
    model_id, auc and logloss where the model has them, num_of_features, then
    over the occupied non-reference groups the minimum / mean / median /
    maximum of AIR_<air_metric> and of p.value, cair = sum of relativeSize x
    AIR, and significant_air_min = the smallest AIR among groups with
    p.value < alpha (NaN if none).  The groups and the response are computed
    once for all models."""
    if air_metric not in METRICS:
        raise ValueError(f"air_metric '{air_metric}' is not one of {METRICS}")
    ms = [m for m in _model_list(models) if getattr(getattr(m, "_spec", None), "nclasses", 0) == 2]
    if not ms:
        raise ValueError("disparate_analysis needs at least one binomial model")
    groups = ProtectedGroups(frame, protected_columns)
    y_of = {}
    rows = []
    for m in ms:
        spec, _, ref_group, flip = _prepare(m, frame, protected_columns, reference, favorable_class, groups)
        if spec.y not in y_of:
            y_of[spec.y] = _response_codes(spec, frame)
        df, _ = _overview(m, frame, groups, ref_group, y_of[spec.y], flip, tables=False)
        if ref_group is not None:
            df = df.drop(index=ref_group)
        air = df["AIR_" + air_metric].to_numpy(dtype=np.float64)
        pv = df["p.value"].to_numpy(dtype=np.float64)
        rel = df["relativeSize"].to_numpy(dtype=np.float64)
        row = {"model_id": m.model_id}
        for name in ("auc", "logloss"):
            v = _board_metric(m, name)
            if v is not None:
                row[name] = v
        row["num_of_features"] = len(spec.x)
        sig = air[pv < alpha]
        sig = sig[~np.isnan(sig)]
        with np.errstate(all="ignore"):
            row.update({"air_min": _nan_stat(np.nanmin, air), "air_mean": _nan_stat(np.nanmean, air),
                        "air_median": _nan_stat(np.nanmedian, air), "air_max": _nan_stat(np.nanmax, air),
                        "cair": float(np.nansum(rel * air)) if air.size else _NAN,
                        "significant_air_min": float(sig.min()) if sig.size else _NAN,
                        "p.value_min": _nan_stat(np.nanmin, pv), "p.value_mean": _nan_stat(np.nanmean, pv),
                        "p.value_median": _nan_stat(np.nanmedian, pv), "p.value_max": _nan_stat(np.nanmax, pv)})
        rows.append(row)
    cols = []
    for r in rows:
        cols += [c for c in r if c not in cols]
    head = [c for c in ("model_id", "auc", "logloss", "num_of_features") if c in cols]
    return _table(pd.DataFrame(rows, columns=head + [c for c in cols if c not in head]))


def _nan_stat(fn, a):
    a = a[~np.isnan(a)]
    return float(fn(a)) if a.size else _NAN


def fair_shap(model, frame: H2OFrame, protected_columns):
    """Per group and feature, the mean and the mean absolute SHAP contribution
    (model.predict_contributions): H2OFrame [protected columns, feature,
    mean_contribution, mean_abs_contribution, rows]."""
    from ..core.groupsum import group_sum
    groups = ProtectedGroups(frame, protected_columns)
    contrib = model.predict_contributions(frame)
    feats = [n for n in contrib.names if n != "BiasTerm"]
    C = torch.stack([contrib.vec(n).as_float(torch.float64) for n in feats], 1)
    ids = groups.ids.to(C.device).to(torch.int64)
    ones = torch.ones((C.shape[0], 1), dtype=torch.float64, device=C.device)
    s = group_sum(ids, torch.cat([C, C.abs(), ones], 1), groups.G)      # metrics_ops.group_sum on a GPU
    coll.allreduce_(s)
    s = s.cpu().numpy()
    F = len(feats)
    rows = []
    for k, lv in enumerate(groups.levels):
        n = s[k, 2 * F]
        for j, f in enumerate(feats):
            rows.append(tuple(lv) + (f, s[k, j] / n if n > 0 else _NAN, s[k, F + j] / n if n > 0 else _NAN, int(n)))
    return _table(pd.DataFrame(rows, columns=groups.columns + ["feature", "mean_contribution",
                                                              "mean_abs_contribution", "rows"]))


def fair_pd(model, frame: H2OFrame, column, protected_columns, nbins=20):
    """Partial dependence of `column` on each group's rows (model.partial_plot
    of the frame filtered to the group), stacked: H2OFrame [protected columns,
    column, mean_response, stddev_response, std_error_mean_response]."""
    groups = ProtectedGroups(frame, protected_columns)
    parts = []
    for k, lv in enumerate(groups.levels):
        df = model.partial_plot(frame[groups.ids == k], cols=[column], nbins=nbins)[0].copy()
        for j, c in enumerate(groups.columns):
            df.insert(j, c, lv[j])
        parts.append(df)
    return _table(pd.concat(parts, ignore_index=True))


def _has_contributions(model):
    from .base import H2OEstimator
    return type(model).predict_contributions is not H2OEstimator.predict_contributions


def inspect_model_fairness(model, frame: H2OFrame, protected_columns, reference, favorable_class, columns=None):
    """The tables behind the reference's fairness report of one model:
    everything `fairness_metrics` returns, "pd_<column>" = `fair_pd` for each
    of `columns` (default: the top 3 by variable importance, where the model
    has one) and "shap" = `fair_shap` where the model supports contributions."""
    out = dict(fairness_metrics(model, frame, protected_columns, reference, favorable_class))
    if columns is None:
        vi = model.varimp() if hasattr(model, "varimp") else None
        prot = [protected_columns] if isinstance(protected_columns, str) else list(protected_columns)
        columns = [r[0] for r in vi if r[0] in frame.names and r[0] not in prot][:3] if vi else []
    for c in columns:
        out["pd_" + c] = fair_pd(model, frame, c, protected_columns)
    if _has_contributions(model):
        out["shap"] = fair_shap(model, frame, protected_columns)
    return out
