"""TreeSHAP feature contributions (predict_contributions).

Reference: hex/tree/SharedTreeModelWithContributions.java and
hex/genmodel/algos/tree/TreeSHAP.java (path-dependent TreeSHAP of Lundberg
et al., "Consistent Individualized Feature Attribution for Tree
Ensembles", Algorithm 2: EXTEND / UNWIND / UNWOUND-SUM over the unique
feature path, node covers as the background distribution).

MI355X design: the recursion is over TREE NODES only (a few hundred per
tree); every path element carries per-ROW tensors (one-fractions and path
weights), so each EXTEND / UNWIND step is a handful of elementwise kernels
over all rows at once instead of a per-row recursion.  Both children are
visited with one-fraction = "row goes this way" (0/1 per row), which is
the vectorised form of the reference's hot/cold recursion.

That recursion (`forest_contributions`) is the CPU path and the oracle.  On the
GPU, where every one of its steps is a kernel launch, the models call
`forest_path_contributions` instead: the same values, recursion-free over leaf
paths (`shap_path_kernel` of ops/csrc/tree_shap.hip, work = rows x leaves).
H2O3_TREE_SHAP=torch forces the recursion there too, for A/B runs.

With a background frame (`background_frame=`) the contributions are baseline
(interventional) SHAP instead: recursion-free over leaf paths, work = test
rows x background rows x leaves, on the HIP kernels of ops/shap_ops.py.
"""
from __future__ import annotations

import torch

from .engine import Tree


def _go_left(tree: Tree, j: int, X: torch.Tensor) -> torch.Tensor:
    x = X[tree.feat[j]]
    isn = torch.isnan(x)
    if tree.is_cat[j] and tree.cat_left[j] is not None:
        mask = torch.as_tensor(tree.cat_left[j], dtype=torch.bool, device=X.device)
        code = torch.nan_to_num(x, nan=-1).long()
        inr = (code >= 0) & (code < mask.numel())
        bit = mask[code.clamp(0, max(mask.numel() - 1, 0))]
        return torch.where(isn | ~inr, torch.full_like(isn, bool(tree.na_left[j])), bit)
    # split points are stored / compared in f32 like the scoring kernel
    thr = torch.tensor(float(tree.thr[j]), dtype=torch.float32, device=X.device)
    return torch.where(isn, torch.full_like(isn, bool(tree.na_left[j])), x.to(torch.float32) < thr)


class _El:
    __slots__ = ("d", "z", "o", "w")

    def __init__(self, d, z, o, w):
        self.d, self.z, self.o, self.w = d, z, o, w

    def copy(self):
        return _El(self.d, self.z, self.o, self.w)


def _extend(m, pz, po, pi, ones):
    depth = len(m)
    m.append(_El(pi, pz, po, ones.clone() if depth == 0 else torch.zeros_like(ones)))
    for i in range(depth - 1, -1, -1):
        m[i + 1].w = m[i + 1].w + po * m[i].w * ((i + 1) / (depth + 1))
        m[i].w = pz * m[i].w * ((depth - i) / (depth + 1))


def _safe(v):
    return torch.where(v == 0, torch.ones_like(v), v)


def _unwound_sum(m, k):
    depth = len(m) - 1
    one, zero = m[k].o, m[k].z
    nxt = m[depth].w
    total = torch.zeros_like(nxt)
    nz = one != 0
    for i in range(depth - 1, -1, -1):
        tmp = nxt * (depth + 1) / ((i + 1) * _safe(one))
        t_zero = (m[i].w / zero) / ((depth - i) / (depth + 1)) if zero != 0 else torch.zeros_like(tmp)
        total = total + torch.where(nz, tmp, t_zero)
        nxt = torch.where(nz, m[i].w - tmp * zero * ((depth - i) / (depth + 1)), nxt)
    return total


def tree_shap(tree: Tree, X: torch.Tensor, phi: torch.Tensor, scale: float = 1.0):
    """Adds one tree's contributions into phi [N, F+1] (last column = bias)."""
    N = X.shape[1]
    ones = torch.ones(N, dtype=torch.float64, device=X.device)
    cover = [max(float(c), 0.0) for c in tree.weight]
    root = cover[0] if cover[0] > 0 else 1.0
    # bias: cover-weighted mean leaf value
    bias = 0.0
    for j in tree.leaves():
        bias += tree.value[j] * cover[j] / root
    phi[:, -1] += scale * bias

    def rec(j, m, pz, po, pi):
        m = [e.copy() for e in m]
        _extend(m, pz, po, pi, ones)
        if tree.left[j] < 0:
            v = scale * float(tree.value[j])
            for i in range(1, len(m)):
                w = _unwound_sum(m, i)
                phi[:, m[i].d] += w * (m[i].o - m[i].z) * v
            return
        gl = _go_left(tree, j, X).to(torch.float64)
        cj = cover[j] if cover[j] > 0 else 1.0
        iz, io = 1.0, ones
        d = tree.feat[j]
        for k in range(1, len(m)):
            if m[k].d == d:
                iz, io = m[k].z, m[k].o
                _unwind_full(m, k)
                break
        rec(tree.left[j], m, cover[tree.left[j]] / cj * iz, io * gl, d)
        rec(tree.right[j], m, cover[tree.right[j]] / cj * iz, io * (1 - gl), d)

    rec(0, [], 1.0, ones, -1)


def _unwind_full(m, k):
    """UNWIND exactly as the reference: recompute weights, shift d/z/o down."""
    depth = len(m) - 1
    one, zero = m[k].o, m[k].z
    nxt = m[depth].w
    nz = one != 0
    for i in range(depth - 1, -1, -1):
        tmp = m[i].w
        w_one = nxt * (depth + 1) / ((i + 1) * _safe(one))
        w_zero = (tmp * (depth + 1) / (zero * (depth - i))) if zero != 0 else torch.zeros_like(tmp)
        m[i].w = torch.where(nz, w_one, w_zero)
        nxt = torch.where(nz, tmp - m[i].w * zero * ((depth - i) / (depth + 1)), nxt)
    for i in range(k, depth):
        m[i].d, m[i].z, m[i].o = m[i + 1].d, m[i + 1].z, m[i + 1].o
    m.pop()


def forest_contributions(trees, X: torch.Tensor, F: int, scale: float = 1.0) -> torch.Tensor:
    """Sum of TreeSHAP contributions over `trees`; returns [N, F+1] float64."""
    phi = torch.zeros((X.shape[1], F + 1), dtype=torch.float64, device=X.device)
    for t in trees:
        tree_shap(t, X, phi, scale)
    return phi


def forest_path_contributions(forest, X: torch.Tensor, F: int, scale: float = 1.0, tree_class: int = 0,
                              info: dict | None = None) -> torch.Tensor:
    """forest_contributions of `forest`'s trees of class `tree_class` without
    the recursion: path-dependent TreeSHAP over the leaf-path table
    (ops/shap_ops.path_shap: shap_path_kernel of tree_shap.hip on CUDA
    tensors), plus the bias column, which does not depend on the rows and is
    summed here as tree_shap does.  info (optional dict) gets "kernel" and
    "why" of the ShapResult."""
    import numpy as np
    from ...ops import shap_ops
    res = shap_ops.path_shap(forest.pack(X.device), forest.leaf_paths(X.device), X, F, vscale=scale,
                             tree_class=tree_class)
    if info is not None:
        info["kernel"], info["why"] = res.kernel, res.why
    bias = 0.0
    for t, k in zip(forest.trees, forest.tclass):
        if k != tree_class:
            continue
        cover = np.maximum(np.asarray(t.weight, dtype=np.float64), 0.0)
        root = cover[0] if cover[0] > 0 else 1.0
        leaf = np.asarray(t.left, dtype=np.int64) < 0
        bias += float(np.sum(np.asarray(t.value, dtype=np.float64)[leaf] * cover[leaf] / root))
    phi = res.phi
    phi[:, -1] += scale * bias
    return phi


def shap_dispatch(owner, forest, X: torch.Tensor, F: int, scale: float = 1.0) -> torch.Tensor:
    """Path-dependent contributions of the class-0 trees for a model's score
    matrix: the kernel path on the GPU, the recursion on CPU tensors or with
    H2O3_TREE_SHAP=torch (read at call time, for A/B runs).  Records on
    `owner` why the kernel did not run (_shap_path_why, None when it did)."""
    import os
    why = None
    if X.device.type != "cuda":
        why = "CPU tensors"
    elif os.environ.get("H2O3_TREE_SHAP", "") == "torch":
        why = "H2O3_TREE_SHAP=torch"
    if why is not None:
        owner._shap_path_why = why
        trees = [t for t, k in zip(forest.trees, forest.tclass) if k == 0]
        return forest_contributions(trees, X, F, scale)
    info = {}
    phi = forest_path_contributions(forest, X, F, scale, 0, info)
    owner._shap_path_why = info["why"]
    return phi


def background_contributions(forest, X, Z, F, vscale=1.0, bias=0.0, linkinv=None, output_space=False,
                             output_per_reference=False, max_scratch_bytes=1 << 30):
    """Baseline (interventional) SHAP of `forest`'s class-0 trees for the test
    rows X [F, N] against the background rows Z [F, B] (ops/shap_ops.py: HIP
    kernels on the GPU).  The link-space score of a row is bias + vscale *
    (sum of its leaves).  Returns [N, F+1] f64 (mean over the background
    rows) or [N*B, F+1] (one row per pair, test row major); the last column
    is the bias term f(z), or linkinv(f(z)) with output_space, which also
    rescales each pair's contributions to sum to linkinv(f(x)) - linkinv(f(z))."""
    from ...ops import shap_ops
    P = forest.pack(X.device)
    PT = forest.leaf_paths(X.device)
    B = Z.shape[1]
    scale = None
    if output_space and linkinv is not None:
        def scale(fx, fz):
            d = fx.view(-1, 1) - fz.view(1, -1)
            g = linkinv(fx + bias).view(-1, 1) - linkinv(fz + bias).view(1, -1)
            return torch.where(d == 0, torch.zeros_like(d), g / torch.where(d == 0, torch.ones_like(d), d))
    res = shap_ops.background_shap(P, PT, X, Z, F, per_reference=output_per_reference, vscale=vscale,
                                   pair_scale=scale, max_scratch_bytes=max_scratch_bytes)
    phi = res.phi
    bz = res.fz + bias
    if scale is not None:
        bz = linkinv(bz)
    if output_per_reference:
        phi.view(-1, B, F + 1)[:, :, F] = bz.view(1, B)
    else:
        phi[:, F] = bz.mean()
    return phi


def _gather_background(Z):
    """Every rank gets all background rows ([F, B], rank order)."""
    from ...parallel import cloud, collectives as coll
    if not cloud.is_distributed():
        return Z
    return coll.all_gather_var(Z.t().contiguous()).t().contiguous()


def _pair_index_vecs(frame, n_local, B, device):
    """RowIdx / BackgroundRowIdx (global row numbers) of per-reference output."""
    from ...core.vec import Vec, T_INT
    rows = torch.arange(n_local, dtype=torch.float64, device=device) + float(frame.row_offset())
    return [Vec(rows.repeat_interleave(B).contiguous(), T_INT),
            Vec(torch.arange(B, dtype=torch.float64, device=device).repeat(n_local).contiguous(), T_INT)]


def model_background_phi(model, X, Z, output_space=False, output_per_reference=False, max_scratch_bytes=1 << 30):
    """background_contributions of a trained GBM / XGBoost / DRF model for the
    score matrices X [F, N] and Z [F, B] (all background rows)."""
    F = len(model._spec.x)
    if model.algo == "drf":
        if model._n_tree_classes() > 1:
            raise ValueError("Calculating contributions with a background frame is not supported for DRF "
                             "with binomial_double_trees.")
        # the forest mean itself: P(class 1) (single-tree binomial) or the prediction
        ntrees = sum(1 for k in model._forest.tclass if k == 0)
        return background_contributions(model._forest, X, Z, F, vscale=1.0 / max(1, ntrees),
                                        output_per_reference=output_per_reference,
                                        max_scratch_bytes=max_scratch_bytes)
    return background_contributions(model._forest, X, Z, F, bias=float(model._init_f[0]),
                                    linkinv=model._dist.linkinv, output_space=output_space,
                                    output_per_reference=output_per_reference, max_scratch_bytes=max_scratch_bytes)


def tree_contributions(model, frame, top_n=None, bottom_n=None, compare_abs=False, background_frame=None,
                       output_space=False, output_per_reference=False):
    """predict_contributions for GBM / XGBoost / DRF (regression + binomial),
    in link space like the reference: row sum == raw margin prediction.
    With a background frame: baseline SHAP against its rows (bias term = mean
    background prediction) instead of path-dependent TreeSHAP."""
    spec = model._spec
    if background_frame is None:
        if output_space:
            raise ValueError("output_space can only be used with a background_frame")
        if output_per_reference:
            raise ValueError("output_per_reference can only be used with a background_frame")
    if spec.nclasses > 2:
        raise ValueError("Calculating contributions is currently not supported for multinomial models.")
    X = model._score_matrix(frame)
    names = list(spec.x)
    trees = [t for t, k in zip(model._forest.trees, model._forest.tclass) if k == 0]
    extra = []
    if background_frame is not None:
        Z = _gather_background(model._score_matrix(background_frame))
        if Z.shape[1] == 0:
            raise ValueError("background_frame has no rows")
        phi = model_background_phi(model, X, Z, output_space, output_per_reference)
        if output_per_reference:
            extra = list(zip(_pair_index_vecs(frame, X.shape[1], Z.shape[1], X.device),
                             ["RowIdx", "BackgroundRowIdx"]))
    elif model.algo == "drf":
        phi = shap_dispatch(model, model._forest, X, len(names), scale=1.0 / max(1, len(trees)))
        if spec.nclasses == 2:
            # the reference's binomial DRF form (ScoreContributionsTaskDRF,
            # DRFModel.java:97-106: its trees score P(class 0)): 1/(F+1) -
            # contribution to P0 per column, which still sums to P(class 1)
            r = 1.0 / (len(names) + 1)
            phi[:, :-1] += r
            phi[:, -1] += r - 1.0
    else:
        phi = shap_dispatch(model, model._forest, X, len(names))
        phi[:, -1] += float(model._init_f[0])
    from ..shap_baseline import contributions_frame
    return contributions_frame(phi, names, extra, top_n, bottom_n, compare_abs)
