"""Shared pieces of the baseline-SHAP tests (test_shap_background*.py):
hand-built forests and the 2^F subset-enumeration oracle in numpy f64."""
import itertools
import math

import numpy as np

from h2o3_amd.models.tree.engine import Tree
from h2o3_amd.models.tree.shared import Forest


def build_tree(spec):
    """spec: a leaf value, or (feat, thr, na_left, left, right) for a numeric
    split (x < thr goes left), or (feat, [level masks], na_left, left, right)
    for a categorical one (levels with mask 1 go left)."""
    t = Tree()

    def rec(s, depth):
        i = t.add_node(depth, 1.0)
        if not isinstance(s, tuple):
            t.value[i] = float(s)
            return i
        f, cut, nal, l, r = s
        t.feat[i] = f
        t.na_left[i] = bool(nal)
        if isinstance(cut, list):
            t.is_cat[i] = True
            t.cat_left[i] = np.asarray(cut, dtype=np.uint8)
        else:
            t.thr[i] = float(cut)
        t.left[i] = rec(l, depth + 1)
        t.right[i] = rec(r, depth + 1)
        return i
    rec(spec, 0)
    return t


def hand_forest():
    """3 trees, depth <= 4, 6 features; feature 4 is categorical (4 levels).
    Features repeat on a path (one path element, several conditions)."""
    t0 = (0, 0.1, True,
          (1, -0.3, False,
           (0, -0.8, False, 1.5, (2, 0.4, True, -0.7, 0.9)),
           (4, [1, 0, 1, 0], True, 0.3, -1.1)),
          (2, 0.0, False,
           (5, 0.5, True, 2.0, (1, 0.6, False, -0.4, 0.8)),
           -1.3))
    t1 = (4, [0, 1, 1, 0], False,
          (3, 0.2, True, (3, -0.5, False, 0.6, -0.2), (0, 0.0, True, 1.1, -0.9)),
          (5, -0.1, False, 0.45, (2, 0.7, True, (1, 0.0, False, -1.6, 0.25), 0.75)))
    t2 = (3, -0.2, False, 0.5, (3, 0.9, True, (5, 0.0, False, -0.35, 1.25), -0.65))
    fo = Forest()
    for s in (t0, t1, t2):
        fo.add(build_tree(s), 0)
    return fo


def hand_rows(n, seed):
    """[6, n] float32 score matrix: NaNs in numeric and categorical columns,
    out-of-range categorical codes."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(6, n)).astype(np.float32)
    X[4] = rng.integers(0, 4, n).astype(np.float32)
    X[:, 0][[1, 3]] = np.nan                 # row 0: NaN in features 1 and 3
    if n > 1:
        X[4, 1] = np.nan                     # NaN categorical
        X[0, 1] = np.nan
    if n > 2:
        X[4, 2] = 7.0                        # code past the bitset
    if n > 3:
        X[4, 3] = -2.0                       # negative code
        X[5, 3] = np.nan
    return X


def chain_forest(d, seed=0, feats=None):
    """One chain tree: node i splits on feature i (left = leaf, right = next
    node), so the deepest path has d distinct features; plus a shallow tree.
    Thresholds sit near -1: a row goes right at most nodes, so for some pairs
    (27 of 70 x 9 at d = 32, seed 4) every element of the deepest leaf holds
    for x or z and the leaf's full mask is used.  feats: the d feature ids
    (default 0 .. d-1)."""
    feats = list(range(d)) if feats is None else list(feats)
    rng = np.random.default_rng(seed)
    spec = float(rng.normal())
    for i in range(d - 1, -1, -1):
        spec = (feats[i], float(rng.normal() * 0.5 - 1.0), bool(i % 3 == 0), float(rng.normal()), spec)
    fo = Forest()
    fo.add(build_tree(spec), 0)
    fo.add(build_tree((1, 0.0, True, 0.5, (0, 0.3, False, -0.25, 0.75))), 0)
    return fo


def walk(tree, row):
    """Leaf value for one row: the scoring kernel's rule (f32 compare, NaN and
    out-of-range codes follow na_left)."""
    i = 0
    while tree.left[i] >= 0:
        x = np.float32(row[tree.feat[i]])
        nal = bool(tree.na_left[i])
        if tree.is_cat[i] and tree.cat_left[i] is not None:
            if np.isnan(x):
                go = nal
            else:
                c = int(x)
                m = tree.cat_left[i]
                go = nal if (c < 0 or c >= len(m)) else bool(m[c])
        else:
            go = nal if np.isnan(x) else bool(x < np.float32(tree.thr[i]))
        i = tree.left[i] if go else tree.right[i]
    return float(tree.value[i])


def forest_score(forest, row):
    return sum(walk(t, row) for t in forest.trees)


def enumerate_shap(forest, x, z):
    """Exact Shapley values of the game v(S) = f(x on S, z elsewhere): [F+1]
    f64, last entry f(z)."""
    F = len(x)
    val = {}
    for k in range(F + 1):
        for S in itertools.combinations(range(F), k):
            h = np.array(z, dtype=np.float32)
            for j in S:
                h[j] = x[j]
            val[frozenset(S)] = forest_score(forest, h)
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


def enumerate_all(forest, X, Z):
    """[N * B, F+1] per-reference oracle (test row major) for X [F, N], Z [F, B]."""
    return np.stack([enumerate_shap(forest, X[:, r], Z[:, b])
                     for r in range(X.shape[1]) for b in range(Z.shape[1])])
