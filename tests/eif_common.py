"""Shared pieces of the Extended Isolation Forest scoring tests
(test_eif_pack.py, test_eif_kernel_gpu.py): an oracle that walks the raw node
lists (it never sees a pack, model._packed or ops.eif_ops), hand-built and
seeded forests, and the case table.

The rule: xj = the f32 input as f64 with NaN -> 0, +-inf -> +-DBL_MAX; at an
inner node proj = sum over the non-zero normal components, in ascending j, of
n_j * (xj - p_j), every product rounded and then added (numpy has no FMA
here); left iff proj <= 0, so a NaN proj goes right; a leaf adds its value, in
tree order.

A row is *ambiguous* when at some visited node with two or more entries
|proj| <= (nnz + 2) * 2^-52 * sum_j |n_j (xj - p_j)|: twice the first-order
bound on what reordering or contracting nnz products and their sum can move
proj by.  One product's sign is exact, so single-entry nodes never make a row
ambiguous.  `compare` demands equal bits on every other row and fails a case
in which more than 1 row in 1000 is ambiguous.
"""
import functools
from collections import namedtuple

import numpy as np

DBL_MAX = np.finfo(np.float64).max
NAN, INF = float("nan"), float("inf")

Oracle = namedtuple("Oracle", "sums leaf ambiguous")


def clean(X):
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    X[np.isnan(X)] = 0.0
    return np.clip(X, -DBL_MAX, DBL_MAX)


def oracle(trees, X):
    """Per-row sum of leaf values (added in tree order), [n, T] tree-local leaf
    ids and the per-row ambiguous flag, for X [n, P] float32."""
    Xc = clean(X)
    n = Xc.shape[0]
    sums = np.zeros(n, dtype=np.float64)
    leaf = np.zeros((n, len(trees)), dtype=np.int32)
    amb = np.zeros(n, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for t, tr in enumerate(trees):
            val = np.zeros(n, dtype=np.float64)
            stack = [(0, np.arange(n))]
            while stack:
                i, idx = stack.pop()
                nv, pt, l, r, v = tr[i][:5]
                if l < 0:
                    leaf[idx, t] = i
                    val[idx] = v
                    continue
                nz = [j for j in range(len(nv)) if nv[j] != 0]
                proj = np.zeros(idx.size, dtype=np.float64)
                mag = np.zeros(idx.size, dtype=np.float64)
                for j in nz:
                    term = np.float64(nv[j]) * (Xc[idx, j] - np.float64(pt[j]))
                    proj = proj + term
                    mag = mag + np.abs(term)
                if len(nz) >= 2:
                    amb[idx] |= np.abs(proj) <= (len(nz) + 2) * 2.0 ** -52 * mag
                go = proj <= 0
                stack.append((l, idx[go]))
                stack.append((r, idx[~go]))
            sums = sums + val
    return Oracle(sums, leaf, amb)


def compare(orc, got_sums, got_leaf=None):
    """The comparison rule of the module docstring; got_* are numpy arrays."""
    n = orc.sums.shape[0]
    assert int(orc.ambiguous.sum()) * 1000 <= n, f"{int(orc.ambiguous.sum())} of {n} rows are ambiguous"
    ok = ~orc.ambiguous
    assert got_sums.dtype == np.float64 and got_sums.shape == orc.sums.shape
    bad = np.flatnonzero(ok & (got_sums != orc.sums))
    assert bad.size == 0, (bad[:5], got_sums[bad[:5]], orc.sums[bad[:5]])
    if got_leaf is not None:
        assert got_leaf.dtype == np.int32 and got_leaf.shape == orc.leaf.shape
        assert np.array_equal(got_leaf[ok], orc.leaf[ok])


# ------------------------------------------------------------------ forests
def _leaf(v):
    return (None, None, -1, -1, float(v), 1)


def _inner(P, entries, left, right):
    """entries: {column: (normal, point)}."""
    nv, pt = np.zeros(P), np.zeros(P)
    for j, (a, b) in entries.items():
        nv[j], pt[j] = a, b
    return (nv, pt, left, right, 0.0, 2)


HAND_P = 4


def hand_forest():
    """Root-only leaf, depth 1, a left-deep chain of 8 splits, nodes of 1, 2
    and P entries (columns 0 and P - 1 among them), a negative normal.  Every
    node of two or more entries has small positive normals, so rows with +inf
    or -inf inputs neither overflow nor cancel there."""
    P = HAND_P
    root_only = [_leaf(3.25)]
    depth1 = [_inner(P, {1: (1.5, 0.25)}, 1, 2), _leaf(1.0), _leaf(2.0)]
    chain = []
    for k in range(8):                      # inner 2k: left -> 2k + 2, right -> leaf 2k + 1
        chain.append(_inner(P, {k % P: (1.0, -0.5 * k)}, 2 * k + 2, 2 * k + 1))
        chain.append(_leaf(k + 1.125))
    chain.append(_leaf(8.3))
    counts = [_inner(P, {0: (0.2, 0.1), 1: (0.1, -0.3), 2: (0.15, 0.2), 3: (0.05, -0.1)}, 1, 2),
              _inner(P, {0: (0.2, -0.4), P - 1: (0.1, 0.6)}, 3, 4),
              _inner(P, {P - 1: (1.0, 0.5)}, 5, 6),
              _leaf(2.1), _leaf(2.2), _leaf(2.3), _leaf(2.7)]
    tie = [_inner(P, {2: (-2.0, 0.75)}, 1, 2), _leaf(1.3), _leaf(1.6)]
    return [root_only, depth1, chain, counts, tie]


def hand_rows():
    """Ties (x_j == p_j, f32-representable: goes left), one f32 ulp either side
    of p_j, NaN and same-sign infinities in every column, and seeded rows."""
    P = HAND_P
    up, dn = np.nextafter(np.float32(0.75), np.float32(2)), np.nextafter(np.float32(0.75), np.float32(0))
    rows = [[0, 0, 0, 0], [0, 0.25, 0.75, 0.5], [0, 0.25, up, 0.5], [0, 0.25, dn, 0.5],
            [0, np.nextafter(np.float32(0.25), np.float32(1)), 0.75, 0.5],
            [0, np.nextafter(np.float32(0.25), np.float32(0)), 0.75, 0.5],
            [NAN] * P, [INF] * P, [-INF] * P, [-3, -3, -3, -3], [3, 3, 3, 3], [0, -0.5, -1.0, -1.5]]
    for j in range(P):
        for v in (NAN, INF, -INF):
            r = [0.3, -0.2, 0.9, 0.1]
            r[j] = v
            rows.append(r)
    rng = np.random.default_rng(5)
    return np.concatenate([np.asarray(rows, dtype=np.float32), rng.normal(size=(100, P)).astype(np.float32)])


def inf_pair_forest():
    """A two-entry node whose products overflow: +inf and -inf inputs in its two
    columns give proj = inf - inf = NaN, which goes right."""
    return [[_inner(HAND_P, {0: (2.0, 0.5), 3: (2.0, -0.5)}, 1, 2), _leaf(1.0), _leaf(2.0)],
            [_inner(HAND_P, {0: (-3.0, 0.0), 3: (-3.0, 0.25)}, 1, 2), _leaf(1.5), _leaf(2.5)]]


def inf_pair_rows():
    rows = [[INF, 0, 0, -INF], [-INF, 0, 0, INF], [NAN, 0, 0, 2], [1, NAN, NAN, NAN], [1, 0, 0, 1], [-1, 0, 0, 0.25]]
    rng = np.random.default_rng(6)
    return np.concatenate([np.asarray(rows, dtype=np.float32), rng.normal(size=(60, HAND_P)).astype(np.float32)])


def random_forest(P, T, seed, max_depth=6):
    """T seeded trees over P columns; inner nodes have 1, 2 or P entries."""
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(T):
        nodes = []

        def build(d):
            me = len(nodes)
            nodes.append(None)
            if d >= max_depth or (d >= 2 and rng.random() < 0.25):
                nodes[me] = (None, None, -1, -1, d + float(rng.random()), 1)
                return me
            nnz = min(P, int(rng.choice([1, 2, P])))
            cols = rng.choice(P, size=nnz, replace=False)
            nv, pt = np.zeros(P), np.zeros(P)
            nv[cols] = rng.normal(size=nnz)
            pt[cols] = rng.uniform(-1, 1, size=nnz)
            l = build(d + 1)
            r = build(d + 1)
            nodes[me] = (nv, pt, l, r, 0.0, 2)
            return me
        build(0)
        trees.append(nodes)
    return trees


def random_rows(n, P, seed):
    """Gaussian f32 rows, 5 % NaN."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, P)).astype(np.float32)
    X[rng.random((n, P)) < 0.05] = NAN
    return X


TILE_MAX_P = 128          # ops.eif_ops.TILE_MAX_P, restated so that a change of the limit shows here

# every n of {1, 63, 64, 65, 255, 257, 777}, every P of {1, 3, 64, 65, just past
# the tile limit} and every T of {1, 5, 12} at least once
RANDOM_SHAPES = [(1, 1, 1), (63, 3, 5), (64, 64, 12), (65, 65, 5), (255, 1, 12), (257, TILE_MAX_P + 1, 5),
                 (777, 3, 12), (777, 64, 5), (257, 65, 1), (64, TILE_MAX_P + 1, 12), (255, 64, 1), (777, 65, 12)]
CASE_NAMES = ["hand", "inf_pair"] + [f"n{n}_P{P}_T{T}" for n, P, T in RANDOM_SHAPES]


def case_columns(name):
    """P of a case, without computing its reference."""
    return HAND_P if name in ("hand", "inf_pair") else RANDOM_SHAPES[CASE_NAMES.index(name) - 2][1]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(trees, X [n, P] f32, Oracle) of a case; computed once, shared, not to be written to."""
    if name == "hand":
        trees, X = hand_forest(), hand_rows()
    elif name == "inf_pair":
        trees, X = inf_pair_forest(), inf_pair_rows()
    else:
        i = CASE_NAMES.index(name)
        n, P, T = RANDOM_SHAPES[i - 2]
        trees, X = random_forest(P, T, seed=100 + i), random_rows(n, P, seed=200 + i)
    X = np.ascontiguousarray(X, dtype=np.float32)
    orc = oracle(trees, X)
    for a in (X, orc.sums, orc.leaf, orc.ambiguous):
        a.setflags(write=False)
    return trees, X, orc
