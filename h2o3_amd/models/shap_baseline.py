"""Baseline (interventional) SHAP for GLM, Deep Learning and Stacked Ensembles,
and the output-frame code every predict_contributions shares.

All three explain a scalar f in link space for a test row x against a
background row z, in the model's expanded design space (DataInfo.expand:
imputed, standardized, one-hot); BiasTerm = f(z).

  GLM  exact: phi_j = beta_std_j (X_xj - X_zj), f = eta.
  DL   DeepSHAP with the rescale rule (ops/dl_shap_ops.py: HIP kernel on the
       GPU); f is the regression value before linkinv, or the logit of p1.
  SE   G-DeepSHAP through a GLM metalearner: every base model's per-pair
       contributions in its output space, rescaled to its level-one input and
       weighted by the metalearner's coefficient; f is the metalearner's eta.

output_space=True scales each pair's contributions by
(linkinv f(x) - linkinv f(z)) / (f(x) - f(z)) (0 where f(x) == f(z)), as the
tree path does.  These definitions are this project's own; they are tested for
efficiency (rows sum to f(x) - f(z)) and, where exact, against subset
enumeration.
"""
from __future__ import annotations

import numpy as np
import torch

from ..core.frame import H2OFrame
from ..core.vec import T_REAL, Vec, make_enum_from_strings

MULTINOMIAL_MSG = "Calculating contributions is currently not supported for multinomial models."


# ------------------------------------------------------------------ output frame
def contributions_frame(phi, names, extra=(), top_n=None, bottom_n=None, compare_abs=False):
    """The frame of predict_contributions from phi [rows, F+1] (BiasTerm last):
    one f32 column per name, or with top_n / bottom_n the sorted
    top_feature_i / top_value_i (+ bottom_*) columns; `extra` (vec, name)
    columns (RowIdx / BackgroundRowIdx) come last."""
    extra = list(extra)
    names = list(names)
    if top_n is None and bottom_n is None:
        vecs = [Vec(phi[:, j].to(torch.float32).contiguous(), T_REAL) for j in range(phi.shape[1])]
        return H2OFrame.from_vecs(vecs + [v for v, _ in extra], names + ["BiasTerm"] + [n for _, n in extra])
    c = phi[:, :-1]
    key = c.abs() if compare_abs else c
    order = torch.argsort(key, dim=1, descending=True).cpu().numpy()
    cn = c.cpu().numpy()
    cols, out_names = [], []
    F = c.shape[1]
    tn = F if top_n is not None and top_n < 0 else (top_n or 0)
    bn = F if bottom_n is not None and bottom_n < 0 else (bottom_n or 0)
    for i in range(min(tn, F)):
        j = order[:, i]
        cols.append(make_enum_from_strings([names[k] for k in j]))
        cols.append(Vec(torch.tensor(cn[np.arange(len(j)), j], dtype=torch.float32, device=phi.device), T_REAL))
        out_names += [f"top_feature_{i + 1}", f"top_value_{i + 1}"]
    for i in range(min(bn, F)):
        j = order[:, F - 1 - i]
        cols.append(make_enum_from_strings([names[k] for k in j]))
        cols.append(Vec(torch.tensor(cn[np.arange(len(j)), j], dtype=torch.float32, device=phi.device), T_REAL))
        out_names += [f"bottom_feature_{i + 1}", f"bottom_value_{i + 1}"]
    cols.append(Vec(phi[:, -1].to(torch.float32).contiguous(), T_REAL))
    out_names.append("BiasTerm")
    for v, n in extra:
        cols.append(v)
        out_names.append(n)
    return H2OFrame.from_vecs(cols, out_names)


# ------------------------------------------------------------------ shared pieces
def _gather_rows(Z):
    """Every rank gets all background rows ([B, P], rank order)."""
    from ..parallel import cloud, collectives as coll
    if not cloud.is_distributed():
        return Z
    return coll.all_gather_var(Z.contiguous())


def _require_background(model, background_frame):
    if background_frame is None:
        raise ValueError(f"{model.algo}: predict_contributions requires a background_frame")


def _refuse_common(model):
    spec = model._spec
    if spec.nclasses > 2:
        raise ValueError(MULTINOMIAL_MSG)
    if getattr(spec, "offset_column", None):
        raise ValueError(f"{model.algo}: contributions are not supported for a model with an offset_column")


def _check_format(output_format):
    fmt = str(output_format or "Original").lower()
    if fmt not in ("original", "compact"):
        raise ValueError(f"output_format must be Original or Compact, got {output_format}")
    return fmt


def _pair_scale(linkinv):
    """(fx, fz) -> [N, B] output-space factor of each pair."""
    def scale(fx, fz):
        d = fx.view(-1, 1) - fz.view(1, -1)
        g = linkinv(fx).view(-1, 1) - linkinv(fz).view(1, -1)
        return torch.where(d == 0, torch.zeros_like(d), g / torch.where(d == 0, torch.ones_like(d), d))
    return scale


def _set_bias(phi, fz, B, per_reference):
    if per_reference:
        phi.view(-1, B, phi.shape[1])[:, :, -1] = fz.view(1, B)
    else:
        phi[:, -1] = fz.mean()
    return phi


def _design_names(dinfo, phi, fmt):
    """Original: one column per design-matrix column.  Compact: every
    categorical's one-hot group summed (cat_cols + num_cols)."""
    if fmt == "original":
        return phi, list(dinfo.coef_names)
    grp, g = [], 0
    for c in dinfo.cat_cols:
        grp += [g] * (len(dinfo.domains[c]) - (0 if dinfo.use_all else 1))
        g += 1
    grp += list(range(g, g + len(dinfo.num_cols)))
    names = list(dinfo.cat_cols) + list(dinfo.num_cols)
    out = torch.zeros((phi.shape[0], len(names) + 1), dtype=phi.dtype, device=phi.device)
    out.index_add_(1, torch.as_tensor(grp + [len(names)], dtype=torch.long, device=phi.device), phi)
    return out, names


def _finish(model, frame, phi, dinfo, fmt, n_local, B, output_per_reference, top_n, bottom_n, compare_abs):
    from .tree.shap import _pair_index_vecs
    phi, names = _design_names(dinfo, phi, fmt) if dinfo is not None else (phi, list(model._spec.x))
    extra = []
    if output_per_reference:
        extra = list(zip(_pair_index_vecs(frame, n_local, B, phi.device), ["RowIdx", "BackgroundRowIdx"]))
    return contributions_frame(phi, names, extra, top_n, bottom_n, compare_abs)


# ------------------------------------------------------------------ GLM
def _glm_check(model):
    if getattr(model, "_multi", None) is not None:
        raise ValueError(MULTINOMIAL_MSG)
    if getattr(model, "_hglm", None) is not None:
        raise ValueError("glm: contributions are not supported for HGLM models")
    if model.algo == "gam" or not hasattr(model, "_beta_std"):
        raise ValueError(f"{model.algo}: contributions are not supported for GAM models")
    _refuse_common(model)


def glm_phi(model, X, Z, output_space=False, output_per_reference=False, max_scratch_bytes=1 << 30):
    """Exact contributions of a GLM in its design space for X [N, P] against
    all background rows Z [B, P]: [N, P+1] or [N*B, P+1] f64.  Link space
    needs no pair loop; output space is one S @ Z product."""
    dev = X.device
    X, Z = X.to(torch.float64), Z.to(torch.float64)
    N, B, P = X.shape[0], Z.shape[0], X.shape[1]
    beta = torch.as_tensor(np.asarray(model._beta_std[:-1], dtype=np.float64), device=dev)[:P]
    icpt = float(model._beta_std[-1])
    fx, fz = X @ beta + icpt, Z @ beta + icpt
    linkinv = model._fam.linkinv
    S = _pair_scale(linkinv)(fx, fz) if output_space else None
    if output_per_reference:
        phi = torch.zeros((N, B, P + 1), dtype=torch.float64, device=dev)
        step = max(1, int(max_scratch_bytes) // max(1, 8 * B * (P + 1)))
        for r0 in range(0, N, step):
            c = beta * (X[r0:r0 + step].unsqueeze(1) - Z.unsqueeze(0))
            phi[r0:r0 + step, :, :P] = c if S is None else c * S[r0:r0 + step].unsqueeze(2)
        phi = phi.view(N * B, P + 1)
    else:
        phi = torch.zeros((N, P + 1), dtype=torch.float64, device=dev)
        if S is None:
            phi[:, :P] = beta * (X - Z.mean(0, keepdim=True))
        else:
            phi[:, :P] = beta * (X * S.mean(1, keepdim=True) - (S @ Z) / B)
    return _set_bias(phi, linkinv(fz) if output_space else fz, B, output_per_reference)


def glm_contributions(model, frame, output_format="Original", top_n=None, bottom_n=None, compare_abs=False,
                      background_frame=None, output_space=False, output_per_reference=False):
    _glm_check(model)
    fmt = _check_format(output_format)
    _require_background(model, background_frame)
    di = model._dinfo
    X = di.expand(frame, pad=False)[0]
    Z = _gather_rows(di.expand(background_frame, pad=False)[0])
    if Z.shape[0] == 0:
        raise ValueError("background_frame has no rows")
    phi = glm_phi(model, X, Z, output_space, output_per_reference)
    return _finish(model, frame, phi, di, fmt, X.shape[0], Z.shape[0], output_per_reference, top_n, bottom_n,
                   compare_abs)


# ------------------------------------------------------------------ Deep Learning
def _dl_check(model):
    if getattr(model, "_ae", False):
        raise ValueError("deeplearning: contributions are not supported for autoencoders")
    if getattr(model, "_K", 1) > 2:
        raise ValueError(MULTINOMIAL_MSG)
    if getattr(model, "_cat_slots", None) is not None:
        raise ValueError("deeplearning: contributions are not supported with max_categorical_features hashing")
    _refuse_common(model)


def _dl_net(model):
    """(layers, acts, scales, out_w, out_b, linkinv) of the explained scalar:
    the regression value before linkinv, or the logit of p1 (the 2-way softmax
    collapses to one linear unit with weights W_out[1] - W_out[0])."""
    hidden = model._layers[:-1]
    Lo = model._layers[-1]
    layers = [(L.W, L.b) for L in hidden]
    acts = [L.act for L in hidden]
    scales = [1.0 - L.drop for L in hidden]
    if model._K == 2:
        return layers, acts, scales, Lo.W[1] - Lo.W[0], float(Lo.b[1] - Lo.b[0]), torch.sigmoid
    ysd, ymu = float(model._ysd), float(model._ymu)
    linkinv = (lambda f: f) if model._dist.family in ("gaussian", "laplace", "quantile", "huber") \
        else model._dist.linkinv
    return layers, acts, scales, Lo.W[0] * ysd, float(Lo.b[0]) * ysd + ymu, linkinv


def dl_phi(model, X, Z, output_space=False, output_per_reference=False, max_scratch_bytes=1 << 30,
           use_native=None):
    """DeepSHAP contributions in the design space for X [N, P] against all
    background rows Z [B, P]; returns (phi, DeepShapResult)."""
    from ..ops import dl_shap_ops
    layers, acts, scales, out_w, out_b, linkinv = _dl_net(model)
    with torch.no_grad():
        res = dl_shap_ops.deep_shap(layers, acts, scales, out_w, X, Z, per_reference=output_per_reference,
                                    pair_scale=_pair_scale(linkinv) if output_space else None,
                                    max_scratch_bytes=max_scratch_bytes, out_b=out_b, use_native=use_native)
    phi = res.phi
    if output_space:
        _set_bias(phi, linkinv(res.fz), Z.shape[0], output_per_reference)
    return phi, res


def dl_contributions(model, frame, output_format="Original", top_n=None, bottom_n=None, compare_abs=False,
                     background_frame=None, output_space=False, output_per_reference=False):
    _dl_check(model)
    fmt = _check_format(output_format)
    _require_background(model, background_frame)
    X = model._design(frame)[0]
    Z = _gather_rows(model._design(background_frame)[0])
    if Z.shape[0] == 0:
        raise ValueError("background_frame has no rows")
    phi, res = dl_phi(model, X, Z, output_space, output_per_reference)
    model._last_shap = res
    return _finish(model, frame, phi, model._dinfo, fmt, X.shape[0], Z.shape[0], output_per_reference, top_n,
                   bottom_n, compare_abs)


# ------------------------------------------------------------------ Stacked Ensemble
_TREE_ALGOS = ("gbm", "drf", "xgboost")


class _Base:
    """One base model's inputs: test-row and (gathered) background-row
    matrices, its output p and level-one input u for both, and how its
    features map onto the ensemble's."""

    def __init__(self, model, frame, background_frame, names, logit):
        self.model = model
        algo = model.algo
        if algo in _TREE_ALGOS and getattr(model, "_gblinear", None) is None:
            self.kind = "tree"
            from .tree.shap import _gather_background
            self.X = model._score_matrix(frame)                          # [F, N]
            self.Z = _gather_background(model._score_matrix(background_frame))
            feats = list(model._spec.x)
        elif algo == "glm":
            _glm_check(model)
            self.kind = "glm"
            self.X = model._dinfo.expand(frame, pad=False)[0]
            self.Z = _gather_rows(model._dinfo.expand(background_frame, pad=False)[0])
            feats = list(model._dinfo.cat_cols) + list(model._dinfo.num_cols)
        elif algo == "deeplearning":
            _dl_check(model)
            self.kind = "dl"
            self.X = model._design(frame)[0]
            self.Z = _gather_rows(model._design(background_frame)[0])
            feats = list(model._dinfo.cat_cols) + list(model._dinfo.num_cols)
        else:
            raise ValueError(f"stackedensemble: contributions are not supported for base model "
                             f"{model.model_id} ({algo})")
        if model._spec.nclasses > 2:
            raise ValueError(MULTINOMIAL_MSG)
        missing = [f for f in feats if f not in names]
        if missing:
            raise ValueError(f"stackedensemble: base model {model.model_id} uses features the ensemble does not "
                             f"have: {missing}")
        dev = self.X.device
        self.index = torch.as_tensor([names.index(f) for f in feats], dtype=torch.long, device=dev)
        self.px = self._p(model._predict_raw(frame))
        self.pz = _gather_rows(self._p(model._predict_raw(background_frame)))
        self.ux, self.uz = self._u(self.px, logit), self._u(self.pz, logit)

    @staticmethod
    def _p(raw):
        return raw[:, -1].to(torch.float64).contiguous()

    @staticmethod
    def _u(p, logit):
        # the level-one column as StackedEnsemble._level_one stores it (f32)
        u = torch.logit(p.clamp(1e-9, 1 - 1e-9)) if logit else p
        return u.to(torch.float32).to(torch.float64)

    def pairs(self, r0, r1, max_scratch_bytes):
        """[n * B, F_m] f64 per-pair contributions of rows [r0, r1) in the
        model's output space (they sum to p(x) - p(z))."""
        m = self.model
        if self.kind == "tree":
            from .tree.shap import model_background_phi
            phi = model_background_phi(m, self.X[:, r0:r1].contiguous(), self.Z, True, True, max_scratch_bytes)
            return phi[:, :-1]
        if self.kind == "glm":
            phi = glm_phi(m, self.X[r0:r1], self.Z, True, True, max_scratch_bytes)
        else:
            phi = dl_phi(m, self.X[r0:r1].contiguous(), self.Z, True, True, max_scratch_bytes)[0]
        return _design_names(m._dinfo, phi, "compact")[0][:, :-1]


def _meta_coefs(se):
    """Metalearner coefficients on the raw level-one columns, by base model,
    and its intercept."""
    meta = se._meta
    if meta.algo != "glm" or getattr(meta, "_multi", None) is not None or getattr(meta, "_hglm", None) is not None:
        raise ValueError(f"stackedensemble: contributions need a GLM metalearner (auto or glm), this one is "
                         f"{meta.algo}")
    if getattr(meta._spec, "offset_column", None):
        raise ValueError("stackedensemble: contributions are not supported for a metalearner with an offset_column")
    beta, icpt = meta._dinfo.destandardize(meta._beta_std[:-1][:meta._dinfo.P], meta._beta_std[-1])
    by_name = dict(zip(meta._dinfo.coef_names, beta.tolist()))
    return [float(by_name.get(n, 0.0)) for n in se._names], float(icpt)


def se_contributions(model, frame, output_format="Original", top_n=None, bottom_n=None, compare_abs=False,
                     background_frame=None, output_space=False, output_per_reference=False,
                     max_scratch_bytes=1 << 30):
    if model._spec.nclasses > 2:
        raise ValueError(MULTINOMIAL_MSG)
    _check_format(output_format)
    betas, icpt = _meta_coefs(model)
    _require_background(model, background_frame)
    names = list(model._spec.x)
    F = len(names)
    logit = str(model._parms.get("metalearner_transform") or "NONE").lower() == "logit" and \
        model._spec.nclasses == 2
    bases = [_Base(m, frame, background_frame, names, logit) for m in model._base]
    N, B = int(bases[0].px.shape[0]), int(bases[0].pz.shape[0])
    if B == 0:
        raise ValueError("background_frame has no rows")
    dev = bases[0].px.device
    linkinv = model._meta._fam.linkinv
    fx = sum(b * m.ux for b, m in zip(betas, bases)) + icpt
    fz = sum(b * m.uz for b, m in zip(betas, bases)) + icpt
    # rows per tile: the [rows * B, F + 1] f64 pair tensors (a base model's, the
    # sum, the grouped copy) stay within the budget
    step = max(1, int(max_scratch_bytes) // max(1, 4 * 8 * B * (F + 1)))
    phi = torch.zeros((N * B if output_per_reference else N, F + 1), dtype=torch.float64, device=dev)
    for r0 in range(0, N, step):
        r1 = min(N, r0 + step)
        acc = torch.zeros(((r1 - r0) * B, F), dtype=torch.float64, device=dev)
        for beta, m in zip(betas, bases):
            if beta == 0.0:
                continue
            dp = (m.px[r0:r1].view(-1, 1) - m.pz.view(1, -1)).reshape(-1)
            du = (m.ux[r0:r1].view(-1, 1) - m.uz.view(1, -1)).reshape(-1)
            w = beta * torch.where(dp == 0, torch.zeros_like(dp), du / torch.where(dp == 0, torch.ones_like(dp), dp))
            acc.index_add_(1, m.index, m.pairs(r0, r1, max_scratch_bytes // 4) * w.view(-1, 1))
        if output_space:
            acc *= _pair_scale(linkinv)(fx[r0:r1], fz).reshape(-1, 1)
        if output_per_reference:
            phi[r0 * B:r1 * B, :F] = acc
        else:
            phi[r0:r1, :F] = acc.view(r1 - r0, B, F).mean(1)
    _set_bias(phi, linkinv(fz) if output_space else fz, B, output_per_reference)
    return _finish(model, frame, phi, None, "original", N, B, output_per_reference, top_n, bottom_n, compare_abs)
