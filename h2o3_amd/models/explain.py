"""Model explainability: partial dependence, permutation importance,
Friedman-Popescu H statistic, and the data behind h2o.explain().

Reference: hex/PartialDependence.java (grid over a column, mean / stddev /
std-error of the response with the column forced to each grid value),
water/rapids/PermutationVarImp.java (metric drop when one column is
permuted, n_repeats, n_samples), hex/tree/FriedmanPopescusH.java
(H^2 from centred partial dependences), h2o-py/h2o/explanation/_explain.py
(explain() / explain_row() assemble varimp, SHAP summary, PDP/ICE,
residual analysis, leaderboard).

Partial dependence (1-D and 2-D), ICE and the H statistic of a tree model
(GBM, DRF, XGBoost gbtree, Generic with a device forest) run on the
forest-grid primitive (ops/pd_ops.py, csrc/tree_pd.hip): the score matrix is
built once and one launch scores every row on up to 64 grid points.
H2O3_TREE_PD=torch forces the replacement loop (one batched device predict()
per grid point), which every other model uses and which is the reference;
model._pd_why says why the loop ran (None on the primitive).  Permutation
importance is one scoring pass per permutation.  explain() returns the tables
the reference plots and, with plot=True, the matplotlib figures too
(models/explain_plots.py).
"""
from __future__ import annotations

import itertools
import math
import os

import numpy as np
import pandas as pd
import torch

from ..core.frame import H2OFrame
from ..core.vec import T_ENUM, T_REAL, Vec
from ..parallel import cloud
from ..parallel import collectives as coll


def _replace(frame: H2OFrame, col: str, vec: Vec) -> H2OFrame:
    vecs = [vec if n == col else frame.vec(n) for n in frame.names]
    return H2OFrame.from_vecs(vecs, list(frame.names))


def _response(model, frame, target=None) -> torch.Tensor:
    """Per-row response used by PDP: p(class) for classifiers, predict otherwise."""
    return _resp_col(model, model._predict_raw(frame), target)


def _resp_col(model, raw, target=None) -> torch.Tensor:
    spec = model._spec
    if spec is not None and spec.nclasses >= 2:
        dom = spec.response_domain
        k = dom.index(target) if target is not None else (1 if spec.nclasses == 2 else 0)
        return raw[:, k].to(torch.float64)
    return raw[:, 0].to(torch.float64)


def _wstats(v: torch.Tensor, w: torch.Tensor | None):
    if w is None:
        w = torch.ones_like(v)
    ok = ~torch.isnan(v)
    v, w = v[ok], w[ok]
    s = torch.stack([w.sum(), (w * v).sum(), (w * v * v).sum(), torch.tensor(float(v.numel()),
                                                                             dtype=v.dtype, device=v.device)])
    return _wfinish(s)


def _wfinish(s: torch.Tensor):
    """(mean, stddev, std error) from this rank's [sum w, sum wv, sum wvv, n]."""
    coll.allreduce_(s)
    sw, sv, svv, n = (float(x) for x in s)
    mean = sv / sw if sw > 0 else float("nan")
    var = max(svv / sw - mean * mean, 0.0) * (n / (n - 1) if n > 1 else 1.0) if sw > 0 else float("nan")
    sd = math.sqrt(var) if var == var else float("nan")
    return mean, sd, (sd / math.sqrt(n) if n > 0 else float("nan"))


def _grid(vec: Vec, nbins, user_split=None, include_na=False):
    if vec.type == T_ENUM:
        levels = list(range(len(vec.domain)))
        vals = [float(i) for i in levels]
        labels = list(vec.domain)
    elif user_split is not None:
        vals = [float(v) for v in user_split]
        labels = vals
    else:
        r = vec.rollups()
        lo, hi = float(r["min"]), float(r["max"])
        if vec.type != T_REAL and hi - lo + 1 <= nbins:   # integer columns: every value
            vals = [float(v) for v in np.arange(lo, hi + 1)]
        else:
            vals = list(np.linspace(lo, hi, nbins)) if hi > lo else [lo]
        labels = vals
    if include_na:
        vals = vals + [float("nan")]
        labels = list(labels) + [float("nan")]
    return vals, labels


def _grid_vec(vec: Vec, vals) -> Vec:
    """One row per grid value of the column `vec`, typed as the replacement
    loop types its constant column: enum codes (NaN = NA = -1) in the
    column's own domain, numeric values cast to f32."""
    dev = vec.data.device if isinstance(vec.data, torch.Tensor) else cloud.device()
    if vec.type == T_ENUM:
        return Vec(torch.tensor([-1 if v != v else int(v) for v in vals], dtype=torch.int32, device=dev),
                   T_ENUM, vec.domain)
    return Vec(torch.tensor([float(v) for v in vals], dtype=torch.float32, device=dev), T_REAL)


def _const_frame(frame: H2OFrame, cols, vecs, point) -> H2OFrame:
    """The replacement loop's frame: every column of `cols` constant at its
    value of the grid point."""
    for c, vec, v in zip(cols, vecs, point):
        one = _grid_vec(vec, [v])
        frame = _replace(frame, c, Vec(one.data.expand(frame.nlocal).contiguous(), one.type, one.domain))
    return frame


class _ForestGrid:
    """Partial dependence of one frame on the forest-grid primitive
    (ops/pd_ops.py): the score matrix is built once, rows are tiled so that a
    tile's [64, rows, K] sums stay under max_scratch_bytes, and the model's
    _raw_from_sums turns every tile's sums into raw predictions."""

    def __init__(self, model, frame: H2OFrame, max_scratch_bytes=1 << 30):
        self.model, self.frame, self.max_scratch_bytes = model, frame, int(max_scratch_bytes)
        self._X = None

    def names(self):
        m = self.model
        return list(m._x) if m.algo == "generic" else list(m._spec.x)

    def why_not(self, cols):
        """Why these columns run on the replacement loop (None: the primitive)."""
        from ..ops import pd_ops
        m = self.model
        if os.environ.get("H2O3_TREE_PD", "").lower() == "torch":
            return "H2O3_TREE_PD=torch"
        if getattr(m, "_gblinear", None) is not None:
            return "booster=gblinear has no trees"
        if not hasattr(m, "_raw_from_sums") or getattr(m, "_forest", None) is None:
            return f"{m.algo} is not a tree model with a device forest"
        off = getattr(m._spec, "offset_column", None)
        if off and off in self.frame.names:
            return f"offset column {off} in the frame"
        if len(cols) > pd_ops.MAX_COLS:
            return f"{len(cols)} columns together, the primitive takes {pd_ops.MAX_COLS}"
        if len(set(cols)) != len(cols):
            return "a column is named twice"
        names = self.names()
        for c in cols:
            if c not in names:
                return f"column {c} is not a feature of the model"
        depth = pd_ops.max_depth(m._forest.pack(cloud.device()))
        if depth > pd_ops.MAX_DEPTH:
            return f"the forest is {depth} splits deep, the kernel takes {pd_ops.MAX_DEPTH}"
        return None

    def X(self):
        if self._X is None:
            self._X = self.model._score_matrix(self.frame)
        return self._X

    def adapt(self, cols, vecs, axes):
        """[S, G] f32 grid from per-column value lists (one entry per grid
        point): the values pass through the model's own adaptation of the
        column (_score_matrix of a G-row frame), so frame-domain enum codes
        become training-domain codes and unseen levels / NA become NaN."""
        names = self.names()
        fr = H2OFrame.from_vecs([_grid_vec(v, a) for v, a in zip(vecs, axes)], list(cols))
        return self.model._score_matrix(fr)[[names.index(c) for c in cols]]

    def responses(self, cols, grid, targets=(None,)):
        """Yields (g0, r0, [resp [gc, n] f64 per target]) over row tiles and
        chunks of 64 grid points."""
        from ..ops import pd_ops
        m = self.model
        names = self.names()
        fidx = [names.index(c) for c in cols]
        X = self.X()
        K = int(m._K)
        P = m._forest.pack(X.device)
        N, G = int(X.shape[1]), int(grid.shape[1])
        nt = max(1, self.max_scratch_bytes // (4 * K * min(max(G, 1), pd_ops.CHUNK)))
        if nt >= 256:
            nt -= nt % 256
        for r0 in range(0, N, nt):
            n = min(nt, N - r0)
            for g0 in range(0, G, pd_ops.CHUNK):
                gc = min(pd_ops.CHUNK, G - g0)
                res = pd_ops.forest_grid_sums(P, X, K, fidx, grid[:, g0:g0 + gc], r0, n)
                m._pd_why = res.why
                raw = m._raw_from_sums(res.sums.view(gc * n, K))
                yield g0, r0, [_resp_col(m, raw, t).view(gc, n) for t in targets]


def _wsums_grid(resp: torch.Tensor, w: torch.Tensor | None) -> torch.Tensor:
    """_wstats' sums for every row of resp [g, n]: [g, 4] f64."""
    ok = ~torch.isnan(resp)
    wv = ok.to(resp.dtype) if w is None else ok * w.view(1, -1)
    v = torch.where(ok, resp, torch.zeros_like(resp))
    return torch.stack([wv.sum(1), (wv * v).sum(1), (wv * v * v).sum(1), ok.sum(1).to(resp.dtype)], 1)


def partial_dependence(model, frame: H2OFrame, cols, nbins=20, weight_column=None, include_na=False,
                       user_splits=None, targets=None, row_index=None, col_pairs_2dpdp=None):
    """Returns one pandas DataFrame per column: [col, mean_response,
    stddev_response, std_error_mean_response] (PartialDependence.java), then
    one per pair of col_pairs_2dpdp: [col1, col2, mean_response, ...] over the
    Cartesian product of the two columns' grids, col1 outer and col2 inner.
    With `targets`, one table per column (pair) and target."""
    if isinstance(cols, str):
        cols = [cols]
    sets = [[c] for c in (cols or [])]
    for pair in col_pairs_2dpdp or []:
        if isinstance(pair, str) or len(pair) != 2:
            raise ValueError(f"col_pairs_2dpdp: every entry is a pair of column names, got {pair!r}")
        sets.append([str(pair[0]), str(pair[1])])
    w = frame.vec(weight_column).as_float(torch.float64) if weight_column else None
    if row_index is not None:
        frame = frame[int(row_index), :]
        w = None
    out = []
    tg = list(targets) if targets else [None]
    fg = _ForestGrid(model, frame)
    stat_cols = ["mean_response", "stddev_response", "std_error_mean_response"]
    for cs in sets:
        vecs = [frame.vec(c) for c in cs]
        axes = [_grid(v, nbins, (user_splits or {}).get(c), include_na) for c, v in zip(cs, vecs)]
        points = list(itertools.product(*[list(zip(vals, labels)) for vals, labels in axes]))
        model._pd_why = fg.why_not(cs)
        if model._pd_why is None:
            grid = fg.adapt(cs, vecs, [[p[s][0] for p in points] for s in range(len(cs))])
            sums = [torch.zeros((len(points), 4), dtype=torch.float64, device=grid.device) for _ in tg]
            for g0, r0, resp in fg.responses(cs, grid, tg):
                for acc, r in zip(sums, resp):
                    acc[g0:g0 + r.shape[0]] += _wsums_grid(r, None if w is None else w[r0:r0 + r.shape[1]])
            stats = [[_wfinish(s) for s in acc] for acc in sums]
        else:                                   # the replacement loop: one scoring pass per grid point
            stats = [[_wstats(_response(model, _const_frame(frame, cs, vecs, [v for v, _ in p]), t), w)
                      for p in points] for t in tg]
        for t, st in zip(tg, stats):
            rows = [tuple(lab for _, lab in p) + tuple(s) for p, s in zip(points, st)]
            df = pd.DataFrame(rows, columns=list(cs) + stat_cols)
            if t is not None:
                df.attrs["target"] = t
            out.append(df)
    return out


def ice(model, frame: H2OFrame, col, nbins=20, max_rows=50, seed=0):
    """Individual conditional expectation curves for up to max_rows rows:
    DataFrame [row, col value, response]."""
    n = frame.nrow
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(n, size=min(n, max_rows), replace=False))
    sub = frame[list(map(int, idx)), :]
    vec = sub.vec(col)
    vals, labels = _grid(vec, nbins)
    fg = _ForestGrid(model, sub)
    model._pd_why = fg.why_not([col])
    if model._pd_why is None:
        resp = torch.zeros((len(vals), sub.nlocal), dtype=torch.float64, device=cloud.device())
        for g0, r0, (r,) in fg.responses([col], fg.adapt([col], [vec], [vals])):
            resp[g0:g0 + r.shape[0], r0:r0 + r.shape[1]] = r
        m = resp.shape[1]
        return pd.DataFrame({"row": [int(i) for i in idx[:m]] * len(vals),
                             col: [lab for lab in labels for _ in range(m)],
                             "response": resp.reshape(-1).cpu().numpy()}, columns=["row", col, "response"])
    recs = []
    for v, lab in zip(vals, labels):
        r = _response(model, _const_frame(sub, [col], [vec], [v])).cpu().numpy()
        for i, rv in zip(idx, r):
            recs.append((int(i), lab, float(rv)))
    return pd.DataFrame(recs, columns=["row", col, "response"])


# ------------------------------------------------------------------ permutation varimp
_LOWER_BETTER = {"mse", "rmse", "mae", "rmsle", "logloss", "mean_per_class_error", "mean_residual_deviance"}
_METRIC_KEY = {"auc": "AUC", "aucpr": "pr_auc", "mse": "MSE", "rmse": "RMSE", "logloss": "logloss", "mae": "mae",
               "rmsle": "rmsle", "mean_per_class_error": "mean_per_class_error",
               "mean_residual_deviance": "mean_residual_deviance", "r2": "r2"}


def _perm_metric(model, frame, metric):
    mt = model.model_performance(frame)
    return float(mt.get(_METRIC_KEY.get(metric, metric)))


def permutation_importance(model, frame: H2OFrame, metric="AUTO", n_samples=10000, n_repeats=1, features=None,
                           seed=-1):
    """Metric degradation when a column is randomly permuted
    (PermutationVarImp.java).  Returns a pandas DataFrame: Variable,
    Relative Importance, Scaled Importance, Percentage (n_repeats == 1) or
    Variable, Run 1..Run n (n_repeats > 1)."""
    spec = model._spec
    metric = (metric or "AUTO").lower()
    if metric == "auto":
        metric = "logloss" if spec.nclasses >= 2 else "rmse"
    rng = np.random.default_rng(None if seed in (-1, None) else seed)
    if n_samples is not None and 0 < n_samples < frame.nrow:
        idx = np.sort(rng.choice(frame.nrow, size=n_samples, replace=False))
        frame = frame[list(map(int, idx)), :]
    base = _perm_metric(model, frame, metric)
    feats = list(features) if features else list(spec.x)
    runs = np.zeros((len(feats), n_repeats))
    for r in range(n_repeats):
        for i, c in enumerate(feats):
            vec = frame.vec(c)
            perm = torch.as_tensor(rng.permutation(frame.nlocal), device=vec.data.device)
            data = vec.data[perm] if isinstance(vec.data, torch.Tensor) else vec.data[perm.cpu().numpy()]
            nv = Vec(data, vec.type, vec.domain)
            val = _perm_metric(model, _replace(frame, c, nv), metric)
            runs[i, r] = (val - base) if metric in _LOWER_BETTER else (base - val)
    if n_repeats > 1:
        df = pd.DataFrame(runs, columns=[f"Run {i + 1}" for i in range(n_repeats)])
        df.insert(0, "Variable", feats)
        return df
    rel = runs[:, 0]
    order = np.argsort(-rel)
    mx = rel.max() if rel.size and rel.max() > 0 else 1.0
    tot = rel[rel > 0].sum() if (rel > 0).any() else 1.0
    return pd.DataFrame({"Variable": [feats[i] for i in order], "Relative Importance": rel[order],
                         "Scaled Importance": rel[order] / mx, "Percentage": rel[order] / tot})


# ------------------------------------------------------------------ Friedman-Popescu H
def h_statistic(model, frame: H2OFrame, variables, max_rows=200, seed=0):
    """Friedman & Popescu H statistic for the joint effect of `variables`
    (FriedmanPopescusH.java): H^2 = sum (F_S - sum_j F_j)^2 / sum F_S^2 over
    data points, with centred partial dependences evaluated AT the data."""
    variables = list(variables)
    n = frame.nrow
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(n, size=min(n, max_rows), replace=False))
    sub = frame[list(map(int, idx)), :]
    pts = {v: sub.vec(v).data.clone() for v in variables}
    m = sub.nlocal

    fg = _ForestGrid(model, sub)
    model._pd_why = fg.why_not(variables)

    def pd_at(vs):
        out = np.zeros(m)
        if model._pd_why is None:
            # one primitive call: the grid is the m sampled points' own (adapted) values
            # of the columns vs, the rows are the m sampled rows; ceil(m / 64) chunks
            names = fg.names()
            grid = fg.X()[[names.index(v) for v in vs]].clone()
            for g0, r0, (r,) in fg.responses(vs, grid):
                out[g0:g0 + r.shape[0]] += r.sum(1).cpu().numpy()
            out /= max(m, 1)
            return out - out.mean()
        for i in range(m):
            f = sub
            for v in vs:
                vec = sub.vec(v)
                val = pts[v][i]
                f = _replace(f, v, Vec(torch.full((m,), val.item(), dtype=vec.data.dtype, device=vec.data.device),
                                        vec.type, vec.domain))
            out[i] = float(_response(model, f).mean())
        return out - out.mean()

    joint = pd_at(variables)
    singles = [pd_at([v]) for v in variables]
    num = ((joint - sum(singles)) ** 2).sum()
    den = (joint ** 2).sum()
    return float(math.sqrt(num / den)) if den > 0 else 0.0


# ------------------------------------------------------------------ explain()
def _has_shap(model, background_frame):
    """Tree models always have a SHAP section; GLM, Deep Learning and Stacked
    Ensembles have one against a background frame."""
    if model._spec.nclasses > 2:
        return False
    if model.algo in ("gbm", "drf", "xgboost"):
        return True
    return background_frame is not None and model.algo in ("glm", "deeplearning", "stackedensemble")


def explain(models, frame: H2OFrame, columns=None, top_n_features=5, include_explanations="ALL",
            exclude_explanations=(), plot=False, background_frame=None, **kw):
    """h2o.explain(): dict of tables keyed like the reference's explanation
    sections; plot=True adds out["plots"][section] figures (varimp heatmap,
    model correlation, SHAP summary, PD / PD-multi, ICE, residual analysis,
    learning curve).  With a background_frame the SHAP section is baseline
    SHAP against its rows, and also appears for GLM, Deep Learning and Stacked
    Ensemble models."""
    if not isinstance(models, (list, tuple)):
        models = [models]
    ex = set(exclude_explanations or ())
    if include_explanations not in (None, "ALL"):
        inc = {include_explanations} if isinstance(include_explanations, str) else set(include_explanations)
        ex |= {"leaderboard", "varimp", "pdp", "shap_summary", "residual_analysis", "confusion_matrix", "ice",
               "varimp_heatmap", "model_correlation_heatmap", "learning_curve"} - inc
    out = {}
    m0 = models[0]
    if len(models) > 1 and "leaderboard" not in ex:
        from ..automl.leaderboard import Leaderboard
        out["leaderboard"] = Leaderboard(models, frame=frame).as_frame().as_data_frame()
    if "varimp" not in ex:
        vi = {}
        for m in models:
            try:
                vi[m.model_id] = m.varimp(use_pandas=True)
            except Exception:  # noqa: BLE001 - some algos have no varimp
                pass
        out["varimp"] = vi
    cols = columns
    if cols is None:
        cols = list(m0._spec.x)
        try:
            v = m0.varimp(use_pandas=True)
            if v is not None and len(v):
                cols = list(v["variable"])[:top_n_features]
        except Exception:  # noqa: BLE001
            cols = cols[:top_n_features]
    if "pdp" not in ex:
        out["pdp"] = {c: partial_dependence(m0, frame, c)[0] for c in cols}
    if "shap_summary" not in ex and _has_shap(m0, background_frame):
        out["shap_summary"] = m0.predict_contributions(frame, background_frame=background_frame).as_data_frame()
    if "residual_analysis" not in ex and m0._spec.nclasses < 2:
        p = m0.predict(frame).as_data_frame()["predict"].values
        y = frame[m0._spec.y].as_data_frame().iloc[:, 0].values
        out["residual_analysis"] = pd.DataFrame({"fitted": p, "residual": y - p})
    if "confusion_matrix" not in ex and m0._spec.nclasses >= 2:
        out["confusion_matrix"] = m0.model_performance(frame).confusion_matrix()
    if plot:
        from . import explain_plots as xp
        figs = {}
        if len(models) > 1:
            if "varimp_heatmap" not in ex:
                try:
                    figs["varimp_heatmap"] = xp.varimp_heatmap(models)
                except RuntimeError:
                    pass
            if "model_correlation_heatmap" not in ex:
                figs["model_correlation_heatmap"] = xp.model_correlation_heatmap(models, frame)
            if "pdp" not in ex:
                figs["pdp"] = {c: xp.pd_multi_plot(models, frame, c) for c in cols}
        else:
            if "varimp" not in ex and out.get("varimp"):
                figs["varimp"] = m0.varimp_plot(server=True)
            if "pdp" not in ex:
                figs["pdp"] = {c: xp.pd_plot(m0, frame, c) for c in cols}
            if "ice" not in ex:
                figs["ice"] = {c: xp.ice_plot(m0, frame, c) for c in cols}
        if "shap_summary" in out:
            figs["shap_summary"] = xp.shap_summary_plot(m0, frame, background_frame=background_frame)
        if "residual_analysis" in out:
            figs["residual_analysis"] = xp.residual_analysis_plot(m0, frame)
        if "learning_curve" not in ex:
            figs["learning_curve"] = xp.learning_curve_plot(m0)
        out["plots"] = figs
    return out


def explain_row(models, frame: H2OFrame, row_index, columns=None, top_n_features=5, plot=False,
                background_frame=None, **kw):
    if not isinstance(models, (list, tuple)):
        models = [models]
    m0 = models[0]
    row = frame[int(row_index), :]
    out = {}
    shap = _has_shap(m0, background_frame)
    if shap:
        out["shap_explain_row"] = m0.predict_contributions(row, background_frame=background_frame).as_data_frame()
    cols = columns or list(m0._spec.x)[:top_n_features]
    out["ice"] = {c: partial_dependence(m0, frame, c, row_index=row_index)[0] for c in cols}
    if plot:
        from . import explain_plots as xp
        figs = {"ice": {c: xp.pd_plot(m0, frame, c, row_index=row_index) for c in cols}}
        if shap:
            figs["shap_explain_row"] = xp.shap_explain_row_plot(m0, frame, row_index,
                                                                background_frame=background_frame)
        out["plots"] = figs
    return out
