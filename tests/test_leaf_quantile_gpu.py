"""The radix-select leaf quantile (ops/csrc/tree_quantile.hip through
ops/quantile_ops.py) against the rule in numpy float64: per leaf, the rows with
w > 0 stably sorted by the f32 residual, the first whose running weight reaches
q * total (clamped to the last), 0.0 for a leaf without weight."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 63, 64, 65, 257, 1000]     # chunk = 128: the last three span several work items
ZERO_LEAF, CONST_LEAF, PAIR_LEAF = 3, 4, 2
# negatives, both zeros, a denormal, the ends of the range, and keys that agree
# with 1.0 in their top 8 (1.5), 16 (1 + 2^-10) and 24 (1 + 2^-23) bits
VALS = np.array([-3e38, -2.5, -1.0000001, -1.0, -0.0, 0.0, 1e-40, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -10, 1.5, 3e38],
                dtype=np.float32)
QS = [0.5, 0.2, 0.9, 1e-9, 1.0]


def _layout():
    g = np.random.default_rng(5)
    n = sum(COUNTS)
    st = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
    ridx = g.permutation(n).astype(np.int32)
    f = g.choice(np.array([0.0, 0.5], dtype=np.float32), n)
    y = g.choice(VALS, n).astype(np.float32)
    y[ridx[st[CONST_LEAF]:st[CONST_LEAF] + COUNTS[CONST_LEAF]]] = 1.5
    f[ridx[st[CONST_LEAF]:st[CONST_LEAF] + COUNTS[CONST_LEAF]]] = 0.0
    y[ridx[st[PAIR_LEAF]:st[PAIR_LEAF] + 2]] = [1.5, -2.0]       # q = 0.5, unit weights: cw[0] == t, the lower one
    f[ridx[st[PAIR_LEAF]:st[PAIR_LEAF] + 2]] = 0.0
    w01 = (g.random(n) < 0.7).astype(np.float32)
    wdy = g.choice(np.array([0, 0.25, 0.5, 1, 2, 3], dtype=np.float32), n)
    for w in (w01, wdy):
        w[ridx[st[ZERO_LEAF]:st[ZERO_LEAF] + COUNTS[ZERO_LEAF]]] = 0
    return dict(ridx=ridx, y=y, f=f, st=st.tolist(), ct=COUNTS, w={"none": None, "mask": w01, "dyadic": wdy},
                bits={"none": 0, "mask": 0, "dyadic": 2}, wu=g.random(n).astype(np.float32))


LAY = _layout()


def reference(x, w, ridx, st, ct, q):
    out = np.zeros(len(st))
    for l, (s, c) in enumerate(zip(st, ct)):
        r = ridx[s:s + c]
        xs, ws = x[r], (np.ones(c) if w is None else w[r].astype(np.float64))
        xs, ws = xs[ws > 0], ws[ws > 0]
        if xs.size:
            o = np.argsort(xs, kind="stable")
            cw = np.cumsum(ws[o])
            out[l] = xs[o][min(int(np.searchsorted(cw, q * cw[-1])), xs.size - 1)]
    return out


def _dev(a):
    return None if a is None else torch.as_tensor(a, device="cuda")


def _state(ridx, w, st, ct, q, bits, mode=0, y=LAY["y"], f=LAY["f"]):
    from h2o3_amd.ops.quantile_ops import LeafQuantile
    return LeafQuantile(_dev(ridx), _dev(y), _dev(f), _dev(w), list(range(len(st))), st, ct, len(st), q, bits,
                        mode=mode, chunk=128)


def _solve(states):
    for k in range(4):
        h = sum(s.hist(k) for s in states)
        for s in states:
            s.select(k, h)
    return [s.values().cpu().numpy() for s in states]


@pytest.mark.parametrize("wk", ["none", "mask", "dyadic"])
@pytest.mark.parametrize("q", QS)
def test_kernel_is_the_rule(q, wk):
    L_ = LAY
    w = L_["w"][wk]
    want = reference(L_["y"] - L_["f"], w, L_["ridx"], L_["st"], L_["ct"], q)
    got, = _solve([_state(L_["ridx"], w, L_["st"], L_["ct"], q, L_["bits"][wk])])
    assert np.array_equal(got, want), (got, want)
    if wk != "none":
        assert got[ZERO_LEAF] == 0.0
    if wk == "none" and q == 0.5:
        assert got[PAIR_LEAF] == -2.0 and got[CONST_LEAF] == 1.5
    # two shards, each with its own segments over half of every leaf's rows
    ha = [c // 2 for c in L_["ct"]]
    sa = _state(L_["ridx"], w, L_["st"], ha, q, L_["bits"][wk])
    sb = _state(L_["ridx"], w, [s + h for s, h in zip(L_["st"], ha)], [c - h for c, h in zip(L_["ct"], ha)], q,
                L_["bits"][wk])
    for v in _solve([sa, sb]):
        assert np.array_equal(v, want)


@pytest.mark.parametrize("q", QS)
def test_abs_mode_one_segment_without_ridx(q):
    L_ = LAY
    n = L_["y"].size
    x = np.abs(L_["y"] - L_["f"])
    want = reference(x, L_["w"]["dyadic"], np.arange(n), [0], [n], q)
    got, = _solve([_state(None, L_["w"]["dyadic"], [0], [n], q, 2, mode=1)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("q", QS)
def test_general_weights_within_the_quantum_bound(q):
    from h2o3_amd.ops.quantile_ops import weight_scale_bits
    L_ = LAY
    w, x = L_["wu"], L_["y"] - L_["f"]
    S = weight_scale_bits(float(w.max()), w.size, False)
    got, = _solve([_state(L_["ridx"], w, L_["st"], L_["ct"], q, S)])
    for l, (s, c) in enumerate(zip(L_["st"], L_["ct"])):
        r = L_["ridx"][s:s + c]
        xs, ws = x[r], w[r].astype(np.float64)
        if ws.sum() == 0:
            assert got[l] == 0.0
            continue
        # every weight is rounded to the nearest quantum 2^-S: half a quantum per row at most
        e, t = c * 2.0 ** -(S + 1), q * ws.sum()
        assert got[l] in xs[ws > 0]
        assert ws[xs < got[l]].sum() - e < t <= ws[xs <= got[l]].sum() + e


# ---- through the estimator -------------------------------------------------------------------------------------

FAMS = {"laplace": {}, "quantile": dict(quantile_alpha=0.2), "huber": {}}
_FITS = {}


def _fit(monkeypatch, fam, weighted, switch):
    if (fam, weighted, switch) not in _FITS:
        from h2o3_amd.core.frame import H2OFrame
        from h2o3_amd.estimators import H2OGradientBoostingEstimator
        from h2o3_amd.models.tree.gbm import GbmSwitches
        from h2o3_amd.ops import quantile_ops
        g = np.random.default_rng(11)
        X = g.standard_normal((3000, 4))
        cols = {f"x{j}": X[:, j] for j in range(4)}
        cols["y"] = X[:, 0] - 0.7 * X[:, 1] + np.sin(2 * X[:, 2]) + 0.3 * g.standard_t(3, 3000)
        cols["w"] = g.choice([0, 0.25, 0.5, 1, 2, 3], 3000)
        fr = H2OFrame(cols)
        monkeypatch.setenv("H2O3_LEAF_QUANTILE", switch)
        calls, real = [], quantile_ops.leaf_wquantile
        monkeypatch.setattr(quantile_ops, "leaf_wquantile", lambda *a, **k: calls.append(1) or real(*a, **k))
        kw = dict(weights_column="w") if weighted else {}
        m = H2OGradientBoostingEstimator(ntrees=5, max_depth=4, seed=1, distribution=fam, **FAMS[fam], **kw)
        m.train(x=[f"x{j}" for j in range(4)], y="y", training_frame=fr)
        assert GbmSwitches.from_env().leaf_quantile is (switch == "1")
        assert len(calls) == (5 if switch == "1" else 0)       # one kernel selection per tree, or none
        _FITS[fam, weighted, switch] = (m._forest.trees, m.predict(fr).as_data_frame()["predict"].values,
                                        float(np.ptp(cols["y"])))
    return _FITS[fam, weighted, switch]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "dyadic"])
@pytest.mark.parametrize("fam", list(FAMS))
def test_models_equal_with_and_without_the_kernel(monkeypatch, fam, weighted):
    (t0, p0, R), (t1, p1, _) = _fit(monkeypatch, fam, weighted, "0"), _fit(monkeypatch, fam, weighted, "1")
    assert len(t0) == len(t1) == 5
    tol_p = 0.0
    for a, b in zip(t0, t1):
        for name in ("feat", "left", "right", "thr", "na_left", "weight"):
            assert list(getattr(a, name)) == list(getattr(b, name)), name
        va, vb = np.asarray(a.value), np.asarray(b.value)
        if fam != "huber":
            assert np.array_equal(va, vb)
            continue
        # huber: equal medians plus sum(w corr) / sum(w).  Both routes add the same n_leaf f64 terms
        # (the kernel route as exact f32 parts) in another order: each sum is off by at most
        # n_leaf eps sum|w corr|, and |corr| <= delta <= R = max y - min y, so after the division the
        # values differ by at most 2 n_leaf eps R; n_leaf <= cover / (smallest positive weight).
        # The bound is absolute: corr changes sign within a leaf, so the sum can cancel to a value far
        # below sum|w corr| and no bound relative to the leaf value follows from the rounding
        tol = 2 * np.finfo(np.float64).eps * (np.asarray(a.weight) / (0.25 if weighted else 1.0)) * R
        assert (np.abs(va - vb) <= tol).all(), np.abs(va - vb).max()
        tol_p += tol.max()
    if fam != "huber":
        assert np.array_equal(p0, p1)
    else:
        # scoring adds f32 leaf values: a value that moved within tol may round to the next f32
        assert (np.abs(p0 - p1) <= tol_p + 5 * np.finfo(np.float32).eps * np.abs(p0).max()).all()
