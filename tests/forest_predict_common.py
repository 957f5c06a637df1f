"""Shared pieces of the forest scoring tests (test_forest_predict*.py and
forest_predict_worker.py): an oracle that walks the `Tree` lists themselves
and never sees Forest.pack(), hand-built and seeded forests, the score
matrices that hit the edges of the decision rule, and the case table.

The rule is the one of shap_bg_common.walk: a numeric split compares
np.float32(x) < np.float32(thr), NaN follows na_left; a categorical split
truncates the code toward zero and a code < 0, >= len(mask) or with
|x| >= 2**31 (which includes +-inf) follows na_left; an is_cat node without a
mask is a numeric split.

The kernel's only arithmetic is the f32 add of leaf values in tree order into
column tclass[t]; the oracle does the same adds in the same order and type,
so every comparison with it uses tolerance zero."""
import functools
from collections import namedtuple

import numpy as np

from shap_bg_common import build_tree, chain_forest

from h2o3_amd.models.tree.shared import Forest

NUMERIC_OUTCOMES = ("num_left", "num_right", "num_equal", "num_nan_left", "num_nan_right", "num_pinf", "num_ninf")
CATEGORICAL_OUTCOMES = ("cat_bit1", "cat_bit0", "cat_nan_left", "cat_nan_right", "cat_negative", "cat_eq_len",
                        "cat_gt_len", "cat_fractional", "cat_huge")
INF, NAN = float("inf"), float("nan")

Oracle = namedtuple("Oracle", "sums leaf sums64 record")


def as_f32(v):
    """The f32 value of v as a Python float (1e300 becomes inf, -1e-46 becomes -0.0)."""
    with np.errstate(over="ignore", under="ignore"):
        return float(np.float32(v))


def _tree_lists(t):
    """Plain Python copies of one Tree's lists; thresholds as their f32 values
    (every f32 is a double, so the Python compare below is the f32 compare)."""
    n = t.n_nodes
    mask = [None] * n
    for i in range(n):
        if t.is_cat[i] and t.cat_left[i] is not None:
            mask[i] = [int(b) for b in np.asarray(t.cat_left[i]).reshape(-1)]
    return ([int(v) for v in t.feat], [int(v) for v in t.left], [int(v) for v in t.right],
            [bool(v) for v in t.na_left], [as_f32(v) for v in t.thr], mask)


def _walk(lists, row, rec):
    """Index of the leaf one row lands in; counts the decisions taken in rec."""
    feat, left, right, na_left, thr, mask = lists
    i = 0
    while left[i] >= 0:
        x = row[feat[i]]
        nal = na_left[i]
        m = mask[i]
        if m is None:
            if x != x:
                go = nal
                rec["num_nan_left" if nal else "num_nan_right"] += 1
            else:
                go = x < thr[i]
                rec["num_left" if go else "num_right"] += 1
                if x == thr[i]:
                    rec["num_equal"] += 1
                if x == INF:
                    rec["num_pinf"] += 1
                elif x == -INF:
                    rec["num_ninf"] += 1
        elif x != x:
            go = nal
            rec["cat_nan_left" if nal else "cat_nan_right"] += 1
        elif abs(x) >= 2147483648.0:
            go = nal
            rec["cat_huge"] += 1
        else:
            c = int(x)                                   # toward zero
            if c != x:
                rec["cat_fractional"] += 1
            if c < 0:
                go = nal
                rec["cat_negative"] += 1
            elif c >= len(m):
                go = nal
                rec["cat_eq_len" if c == len(m) else "cat_gt_len"] += 1
            else:
                go = m[c] != 0
                rec["cat_bit1" if go else "cat_bit0"] += 1
        i = left[i] if go else right[i]
    return i


def leaf_sums(forest, leaf, K, start=0, end=None):
    """(f32 [N, K], f64 [N, K]) sums of trees [start, end) from the oracle's
    leaf ids [N, T]: f32 adds of the f32 leaf values in tree order into column
    tclass[t], as the kernel does them; the f64 sums of the f64 values check
    the f32 ones (T values rounded to f32 and T adds, each within 2**-24 of
    the sum of magnitudes: T * 2**-23 of it in all).  The bound is taken
    relative to the sum of |values|, on purpose not to the sum itself: leaf
    values of both signs cancel, and no bound relative to the sum holds then."""
    end = len(forest.trees) if end is None else end
    N = leaf.shape[0]
    s32 = np.zeros((N, K), dtype=np.float32)
    s64 = np.zeros((N, K), dtype=np.float64)
    mag = np.zeros((N, K), dtype=np.float64)
    for t in range(start, end):
        v64 = np.asarray(forest.trees[t].value, dtype=np.float64)[leaf[:, t]]
        k = forest.tclass[t]
        s32[:, k] = s32[:, k] + v64.astype(np.float32)
        s64[:, k] += v64
        mag[:, k] += np.abs(v64)
    assert np.all(np.abs(s32.astype(np.float64) - s64) <= (end - start) * 2.0 ** -23 * mag), "oracle: f32 vs f64 sums"
    return s32, s64


def oracle(forest, X, K, upto=None):
    """Oracle(sums [N, K] f32, leaf [N, T] i32, sums64 [N, K] f64, record) for
    the first `upto` trees (all by default) on X [F, N]: every row walks every
    Tree from feat / thr / left / right / na_left / is_cat / cat_left / value
    only.  The leaf id is the node's index inside its tree; record counts the
    decision outcomes taken (NUMERIC_OUTCOMES, CATEGORICAL_OUTCOMES)."""
    T = len(forest.trees) if upto is None else upto
    X = np.asarray(X)
    assert X.dtype == np.float32
    rows = X.T.tolist()
    rec = dict.fromkeys(NUMERIC_OUTCOMES + CATEGORICAL_OUTCOMES, 0)
    leaf = np.zeros((len(rows), T), dtype=np.int32)
    for t in range(T):
        lists = _tree_lists(forest.trees[t])
        leaf[:, t] = [_walk(lists, row, rec) for row in rows]
    s32, s64 = leaf_sums(forest, leaf, K, 0, T)
    return Oracle(s32, leaf, s64, rec)


def assert_covered(record):
    """Every outcome of the decision rule was taken at least once: a condition
    on the inputs (forest and rows), evaluated from the oracle alone."""
    missing = [k for k in NUMERIC_OUTCOMES + CATEGORICAL_OUTCOMES if not record.get(k)]
    assert not missing, f"decision outcomes never taken: {missing}"


# ------------------------------------------------------------------ forests
def _forest(trees, tclass=None):
    fo = Forest()
    for i, t in enumerate(trees):
        fo.add(t, 0 if tclass is None else tclass[i])
    return fo


def edge_forest():
    """5 trees over 8 feature rows; 6 (4 levels) and 7 (300 levels) are
    categorical.  Masks of length 1, 4 and 300 on different nodes and trees
    (cat_off has to carry across trees); thresholds 0.0, 0.1 (no f32 value),
    -0.8, 1e300 (+inf in f32), -1e-45 (the smallest f32 subnormal, negative)
    and -1e-46 (-0.0 in f32); both na_left values on numeric and categorical
    nodes; an is_cat node without a mask; feature 0 split twice on a path."""
    rng = np.random.default_rng(300)
    ma, mb, mc = ([int(v) for v in rng.integers(0, 2, 300)] for _ in range(3))
    t0 = (0, 0.1, True,
          (6, [1, 0, 1, 0], False,
           (0, -0.8, False, 1.5, (1, 0.0, True, -0.7, 0.9)),
           (7, ma, True, 0.3, -1.1)),
          (2, 1e300, False, (3, -1e-45, True, 2.0, -0.4), -1.3))
    t1 = (7, mb, False,
          (6, [1], True, 0.6, -0.2),
          (4, 0.0, False, (6, [0, 1, 1, 0], True, 0.45, 0.25), (5, 0.1, True, -1.6, 0.75)))
    t2 = (6, 1.5, False, 0.5, (3, -1e-46, False, -0.35, 1.25))
    t3 = (1, -0.8, True,
          (2, 0.0, False, 0.11, -0.22),
          (7, mc, False, 0.33, (5, -1e-45, False, -0.44, 0.55)))
    t4 = (3, 0.0, True, (4, 1e300, True, 0.7, -0.9), (0, 0.0, False, 0.123, -0.456))
    trees = [build_tree(s) for s in (t0, t1, t2, t3, t4)]
    trees[2].is_cat[0] = True                            # is_cat with cat_left None: a numeric split at 1.5
    assert trees[2].cat_left[0] is None
    return _forest(trees)


def _features(forest):
    """(F, {feature: f32 thresholds of its numeric nodes}, {feature: longest mask})."""
    thr, card, F = {}, {}, 1
    for t in forest.trees:
        for i in range(t.n_nodes):
            if t.left[i] < 0:
                continue
            f = int(t.feat[i])
            F = max(F, f + 1)
            if t.is_cat[i] and t.cat_left[i] is not None:
                card[f] = max(card.get(f, 0), int(np.asarray(t.cat_left[i]).size))
            else:
                thr.setdefault(f, set()).add(as_f32(t.thr[i]))
    return F, thr, card


def edge_rows(forest, n, seed=0, F=None):
    """[F, n] float32 score matrix in the style of hand_rows: Gaussian numeric
    rows, uniform level codes in the categorical ones, and about a third of
    every row overwritten (at seeded positions) with the edges of the rule:
    every threshold of the forest on that feature, the f32 next to it on
    either side, +-inf, +-0.0 and NaN; in a categorical row -1, -0.5,
    0 .. card-1, 2.7, card, card + 3, +-3e9, +inf and NaN.  A row holds each of
    its edge values at least once when n allows (n >= their number)."""
    Fu, thr, card = _features(forest)
    F = Fu if F is None else F
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(F, n)).astype(np.float32)
    for f in range(F):
        sp = []
        for v in sorted(thr.get(f, ())):
            v = np.float32(v)
            sp += [v, np.nextafter(v, np.float32(-INF)), np.nextafter(v, np.float32(INF))]
        if f in card:
            c = card[f]
            X[f] = rng.integers(0, c, n).astype(np.float32)
            sp += [-1.0, -0.5, *range(c), 2.7, c, c + 3, 3e9, -3e9, INF, NAN]
        else:
            sp += [INF, -INF, -0.0, 0.0, NAN]
        sp = np.asarray(sp, dtype=np.float32)
        k = min(n, max(sp.size, n // 3))
        pos = rng.permutation(n)[:k]
        X[f, pos] = np.resize(sp[rng.permutation(sp.size)], k)
    return X


THR7 = (-1.5, -0.8, -0.25, 0.0, 0.1, 0.6, 1.3)


def _random_spec(rng, depth, F, cards):
    if depth == 0 or rng.random() < 0.15:
        return float(rng.normal())
    f = int(rng.integers(0, F))
    c = cards.get(f, 0)
    cut = [int(v) for v in rng.integers(0, 2, c)] if c else float(rng.choice(THR7))
    return (f, cut, bool(rng.integers(0, 2)), _random_spec(rng, depth - 1, F, cards),
            _random_spec(rng, depth - 1, F, cards))


def random_tree(rng, depth, F, cards):
    """A random full-ish tree (a node above the depth limit is a leaf with
    probability 0.15; the root always splits): thresholds from THR7, cards =
    {feature: levels} makes those features categorical."""
    spec = _random_spec(rng, depth, F, cards)
    while not isinstance(spec, tuple):
        spec = _random_spec(rng, depth, F, cards)
    return build_tree(spec)


def random_forest(seed, T, depth, F, cards, tclass=None):
    rng = np.random.default_rng(seed)
    return _forest([random_tree(rng, depth, F, cards) for _ in range(T)], tclass)


def threshold_rows(forest, n, seed=0, F=None, cards=None):
    """[F, n] float32: numeric rows drawn from THR7 (x == thr on a large share
    of the visits of a random_forest) with a few NaN; categorical rows hold
    codes -1 .. card + 1 and NaN."""
    Fu, _, card = _features(forest)
    F = Fu if F is None else F
    card = card if cards is None else cards
    rng = np.random.default_rng(seed)
    X = rng.choice(np.asarray(THR7, dtype=np.float32), size=(F, n))
    for f, c in card.items():
        X[f] = rng.integers(-1, c + 2, n).astype(np.float32)
    X[rng.random((F, n)) < 0.05] = np.nan
    return X


LANE_F, LANE_CARDS = 66, {64: 5, 65: 12}
CHAIN_DEPTH = 64
CHAIN_DEEPEST_LEAF = 2 * CHAIN_DEPTH       # build_tree numbers a chain's leaf at level k 2k + 1, the last one 2d


def lane_forests():
    """{name: forest} for the lock-step walk of TW trees per thread: C is a
    64-deep chain (features 0 .. 63), S a stump (a root that is a leaf), D a
    random depth-3 tree over all 66 features (64 and 65 categorical), N a
    numeric-only one."""
    rng = np.random.default_rng(64)

    def C(seed):
        return chain_forest(CHAIN_DEPTH, seed=seed).trees[0]

    def S(v=0.25):
        return build_tree(v)

    def D():
        return random_tree(rng, 3, LANE_F, LANE_CARDS)

    def N_():
        return random_tree(rng, 3, 64, {})
    return {
        "lane_T1_chain": _forest([C(1)]),                                   # T < TW
        "lane_T1_stump": _forest([S()]),
        "lane_T2_stump_chain": _forest([S(), C(2)]),                        # stump first, next to the chain
        "lane_T3_chain_stump": _forest([C(3), S(), D()]),                   # stump last in the group of TW = 2
        "lane_T3_stumps": _forest([S(), S(-1.5), S(0.1)]),                  # while (live) never runs
        "lane_T4": _forest([D(), S(), C(4), D()]),
        "lane_T5": _forest([D(), D(), S(), D(), C(5)]),                     # chain alone in the tail group
        "lane_T7": _forest([C(6), D(), S(), S(), D(), D(), C(7)]),
        "lane_T8": _forest([S(), D(), D(), C(8), D(), D(), D(), S()]),      # TW = 4: stump first / last in a group
        "lane_T5_nocat": _forest([N_(), C(9), N_(), S(), N_()]),            # no categorical split: placeholder cat_bits
    }


def chain_trees(forest):
    """Indices of the 64-deep chains of a lane forest."""
    return [i for i, t in enumerate(forest.trees) if t.n_nodes == 2 * CHAIN_DEPTH + 1]


def lane_rows(forest, n, seed=0, F=LANE_F):
    """edge_rows plus rows planted for the chains.  A chain's thresholds sit
    near -1 and its left children are leaves, so a Gaussian row leaves it
    within some 30 levels; a row with +inf, or a value above every threshold,
    in features 0 .. 63 goes right at all 64 nodes while the stump or depth-3
    tree in the next lane ended long before.  Column 0 (the only one at
    n = 1), 255, 256 and the last one go all the way down; column 1 leaves a
    chain at level 0, column 2 at level 1, column 3 at level 62."""
    X = edge_rows(forest, n, seed=seed, F=F)
    d = CHAIN_DEPTH
    for c, v in ((0, INF), (255, 1e6), (256, INF), (n - 1, 1e6)):
        if 0 <= c < n:
            X[:d, c] = v
    for c, level in ((1, 0), (2, 1), (3, d - 2)):
        if c < n - 1:
            X[:level, c] = 1e6
            X[level, c] = -INF
    return X


CLASS_F, CLASS_CARDS = 8, {6: 4, 7: 9}


def class_forests():
    """{name: (forest, K)}: a class without a tree and consecutive trees of
    one class; the alternating two-class layout of binomial_double_trees; a
    shuffled tclass over 4 classes."""
    k4 = [0, 1, 2, 3, 0, 1, 2, 3, 0]
    np.random.default_rng(4).shuffle(k4)
    return {
        "class_K3_gap": (random_forest(31, 5, 3, CLASS_F, CLASS_CARDS, [2, 0, 0, 2, 2]), 3),
        "class_K2_alt": (random_forest(32, 6, 3, CLASS_F, CLASS_CARDS, [0, 1, 0, 1, 0, 1]), 2),
        "class_K4_shuffled": (random_forest(33, 9, 4, CLASS_F, CLASS_CARDS, k4), 4),
    }


# ------------------------------------------------------------------ case table
def _lane(name):
    return lane_forests()[name]


def _class(name):
    return class_forests()[name][0]


def _cases():
    """(name, forest factory, X factory, K): every forest once at 777 rows (four
    blocks of 256 threads, the last one ragged), the row counts 1, 255, 256
    and 257 spread over the forests."""
    out = []

    def add(name, fo_f, K, ns, rows=edge_rows, **kw):
        for n in ns:
            out.append((f"{name}_n{n}", fo_f, functools.partial(rows, n=n, seed=len(out) + 1, **kw), K))
    add("edge", edge_forest, 1, (777, 1, 255, 256, 257))
    extra = {"lane_T1_stump": (1,), "lane_T2_stump_chain": (256,), "lane_T3_stumps": (257,), "lane_T5": (255,),
             "lane_T8": (1,)}
    for name in lane_forests():
        add(name, functools.partial(_lane, name), 1, (777,) + extra.get(name, ()), rows=lane_rows, F=LANE_F)
    extra = {"class_K3_gap": (257,), "class_K2_alt": (1,), "class_K4_shuffled": (255,)}
    for name, (_, K) in class_forests().items():
        add(name, functools.partial(_class, name), K, (777,) + extra[name], F=CLASS_F)
    add("random_K1", functools.partial(random_forest, 41, 10, 5, CLASS_F, CLASS_CARDS), 1, (777, 256),
        rows=threshold_rows, F=CLASS_F, cards=CLASS_CARDS)
    add("random_K3", functools.partial(random_forest, 42, 9, 4, CLASS_F, CLASS_CARDS, [0, 1, 2] * 3), 3, (777,),
        rows=threshold_rows, F=CLASS_F, cards=CLASS_CARDS)
    return out


CASES = _cases()
CASE_NAMES = [c[0] for c in CASES]
# what forest_predict_worker.py scores under H2O3_PREDICT_TW = 1 and 4
WORKER_CASE_NAMES = [n for n in CASE_NAMES if n.startswith(("lane_", "class_", "edge_"))]

Reference = namedtuple("Reference", "forest X K oracle")


def inputs(name):
    """(forest, X [F, N] f32, K) of one case, built afresh (seeded)."""
    _, fo_f, x_f, K = CASES[CASE_NAMES.index(name)]
    fo = fo_f()
    return fo, x_f(fo), K


@functools.lru_cache(maxsize=None)
def reference(name):
    """Reference(forest, X [F, N] f32, K, Oracle) of one case, computed once
    per process and shared; the arrays are read-only."""
    fo, X, K = inputs(name)
    orc = oracle(fo, X, K)
    for a in (X, orc.sums, orc.leaf, orc.sums64):
        a.flags.writeable = False
    return Reference(fo, X, K, orc)


def same_trees(forest):
    """A fresh Forest over the same Tree objects: nothing packed yet."""
    return _forest(forest.trees, forest.tclass)
