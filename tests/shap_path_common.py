"""Shared pieces of the path-dependent TreeSHAP tests (test_shap_path*.py):
consistent node covers on top of shap_bg_common's hand-built forests (which
set every cover to 1.0) and the 2^F cover-weighted Shapley enumeration."""
import itertools
import math

import numpy as np

from shap_bg_common import build_tree, chain_forest, hand_forest, hand_rows  # noqa: F401  (re-exported)

from h2o3_amd.models.tree.shared import Forest


def goes_left(tree, i, row):
    """The scoring kernel's decision at node i (f32 compare; NaN and
    out-of-range codes follow na_left), as shap_bg_common.walk takes it."""
    x = np.float32(row[tree.feat[i]])
    nal = bool(tree.na_left[i])
    if tree.is_cat[i] and tree.cat_left[i] is not None:
        if np.isnan(x):
            return nal
        c = int(x)
        m = tree.cat_left[i]
        return nal if (c < 0 or c >= len(m)) else bool(m[c])
    return nal if np.isnan(x) else bool(x < np.float32(tree.thr[i]))


def _fresh(forest):
    """The forest's trees in a new Forest (no stale pack / leaf-path cache)."""
    fo = Forest()
    for t, k in zip(forest.trees, forest.tclass):
        fo.add(t, k)
    return fo


def covers_from_rows(forest, X):
    """Sets every node's cover to the number of columns (rows) of X [F, n]
    routed through it: children sum to their parent, nodes no row reaches
    get cover 0."""
    for t in forest.trees:
        w = [0.0] * t.n_nodes
        for r in range(X.shape[1]):
            i = 0
            w[i] += 1.0
            while t.left[i] >= 0:
                i = t.left[i] if goes_left(t, i, X[:, r]) else t.right[i]
                w[i] += 1.0
        t.weight = w
    return _fresh(forest)


def covers_by_share(forest, left=0.4, root=100.0):
    """Sets covers top-down: every split sends `left` of its cover to the left
    child and the rest to the right one."""
    for t in forest.trees:
        w = [0.0] * t.n_nodes
        w[0] = float(root)
        for i in range(t.n_nodes):                # build_tree numbers parents before children
            if t.left[i] >= 0:
                w[t.left[i]] = w[i] * left
                w[t.right[i]] = w[i] * (1.0 - left)
        t.weight = w
    return _fresh(forest)


def _cond_exp(tree, cover, row, i, S):
    if tree.left[i] < 0:
        return float(tree.value[i])
    l, r = tree.left[i], tree.right[i]
    if tree.feat[i] in S:
        return _cond_exp(tree, cover, row, l if goes_left(tree, i, row) else r, S)
    c = cover[i] if cover[i] > 0 else 1.0
    return (cover[l] * _cond_exp(tree, cover, row, l, S) + cover[r] * _cond_exp(tree, cover, row, r, S)) / c


def enumerate_path_shap(forest, x, F):
    """Exact Shapley values of the game v(S) = E[f | x_S], the expectation
    following x at splits on features of S and the node covers elsewhere:
    [F+1] f64, last entry v(empty set)."""
    covers = [[max(float(c), 0.0) for c in t.weight] for t in forest.trees]
    val = {}
    for k in range(F + 1):
        for S in itertools.combinations(range(F), k):
            s = frozenset(S)
            val[s] = sum(_cond_exp(t, c, x, 0, s) for t, c in zip(forest.trees, covers))
    phi = np.zeros(F + 1)
    for i in range(F):
        others = [j for j in range(F) if j != i]
        for k in range(F):
            w = math.factorial(k) * math.factorial(F - k - 1) / math.factorial(F)
            for S in itertools.combinations(others, k):
                s = frozenset(S)
                phi[i] += w * (val[s | {i}] - val[s])
    phi[F] = val[frozenset()]
    return phi
