"""eif_lengths_kernel (ops/csrc/tree_eif.hip, through
ops.eif_ops.hyperplane_forest_lengths) against eif_common.oracle, a numpy walk
over the raw node lists: equal bits on every non-ambiguous row (eif_common
says what ambiguous means and caps how many rows may be).  The case table runs
with 1, 2 and 4 trees in flight per thread, with the LDS row tile on and off
where X is narrow enough for it, from fresh packs, with leaf ids and in split
tree ranges; then trained models, the memory the entry and predict may take,
and score_tree_interval's scoring history."""
import numpy as np
import pandas as pd
import pytest
import torch

from h2o3_amd.estimators import H2OExtendedIsolationForestEstimator
from h2o3_amd.models.tree.isofor import c_factor
from h2o3_amd.ops import eif_ops

from eif_common import CASE_NAMES, TILE_MAX_P, case_columns, compare, oracle, reference

pytestmark = pytest.mark.gpu

# every allowed trees-in-flight value, the row tile off and (where X fits) on
LAUNCHES = [(name, tw, tile) for name in CASE_NAMES for tw in eif_ops.TREES_IN_FLIGHT for tile in (False, True)
            if not tile or case_columns(name) <= TILE_MAX_P]
_packs = {}


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def _pack(name):
    if name not in _packs:
        _packs[name] = eif_ops.pack_hyperplane_forest(reference(name)[0])
    return _packs[name]


def _np(t):
    assert t.is_cuda
    return t.cpu().numpy()


def test_launch_list_covers_both_sides_of_the_tile_limit():
    assert eif_ops.TILE_MAX_P == TILE_MAX_P
    assert all(case_columns(c) == reference(c)[1].shape[1] for c in CASE_NAMES)
    wide = [c for c in CASE_NAMES if case_columns(c) > TILE_MAX_P]
    assert wide and all((c, tw, False) in LAUNCHES and (c, tw, True) not in LAUNCHES
                        for c in wide for tw in eif_ops.TREES_IN_FLIGHT)
    assert len(LAUNCHES) == 6 * len(CASE_NAMES) - 3 * len(wide)


@pytest.mark.parametrize("name,tw,tile", LAUNCHES)
def test_kernel_matches_oracle(name, tw, tile):
    trees, X, orc = reference(name)
    out, nodes = eif_ops.hyperplane_forest_lengths(_pack(name), _dev(X), node_out=True, plan=(tw, tile))
    assert tuple(nodes.shape) == (X.shape[0], len(trees))
    compare(orc, _np(out), _np(nodes))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fresh_pack_and_split_ranges(name):
    trees, X, orc = reference(name)
    T = len(trees)
    pack = eif_ops.pack_hyperplane_forest(trees)
    Xd = _dev(X)
    whole = eif_ops.hyperplane_forest_lengths(pack, Xd)
    compare(orc, _np(whole))
    acc = torch.zeros(X.shape[0], dtype=torch.float64, device="cuda")
    cuts = sorted({0, 1, T // 2, T})
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        got, nodes = eif_ops.hyperplane_forest_lengths(pack, Xd, a, b, out=acc, node_out=True)
        assert got is acc
        parts.append(nodes)
    assert torch.equal(acc, whole)                     # ranges give the bits of one call
    compare(orc, _np(acc), _np(torch.cat(parts, 1)))
    before = acc.clone()
    eif_ops.hyperplane_forest_lengths(pack, Xd, 1, 1, out=acc)
    assert torch.equal(acc, before)


def test_row_window_and_no_rows():
    trees, X, orc = reference("n777_P3_T12")
    pack = _pack("n777_P3_T12")
    Xd = _dev(X)
    win = Xd[256:513].contiguous()
    assert win.shape[0] == 257
    out, nodes = eif_ops.hyperplane_forest_lengths(pack, win, node_out=True)
    compare(orc._replace(sums=orc.sums[256:513], leaf=orc.leaf[256:513], ambiguous=orc.ambiguous[256:513]),
            _np(out), _np(nodes))
    with pytest.raises(ValueError):
        eif_ops.hyperplane_forest_lengths(pack, Xd[256:513, :2])
    out, nodes = eif_ops.hyperplane_forest_lengths(pack, Xd[:0], node_out=True)
    assert out.is_cuda and tuple(out.shape) == (0,) and tuple(nodes.shape) == (0, 12)


# ------------------------------------------------------------------ trained models
@pytest.fixture(scope="module")
def frame():
    """The frame of test_forest_predict_gpu.py's fixture without its responses:
    1500 rows, numeric columns with NAs, a 7-level categorical with NAs and a
    3-level one."""
    import h2o3_amd as h2o
    rng = np.random.default_rng(11)
    n = 1500
    A = rng.normal(size=(n, 5))
    A[rng.random(n) < 0.06, 1] = np.nan
    A[rng.random(n) < 0.03, 3] = np.nan
    df = pd.DataFrame(A, columns=[f"x{i}" for i in range(5)])
    df["c1"] = rng.choice(list("abcdefg"), n)
    df["c2"] = rng.choice(["u", "v", "w"], n)
    df.loc[rng.random(n) < 0.05, "c1"] = None
    df.loc[rng.random(n) < 0.04, "c2"] = None
    return h2o.H2OFrame(df)


def _train(frame, **kw):
    m = H2OExtendedIsolationForestEstimator(seed=3, **kw)
    m.train(training_frame=frame)
    return m


@pytest.mark.parametrize("ext", [0, 2, "P-1"])
def test_trained_model_matches_oracle_on_both_routes(frame, ext, monkeypatch):
    monkeypatch.delenv("H2O3_TREE_EIF", raising=False)
    T = 12
    if ext == "P-1":
        ext = int(_train(frame, ntrees=1, sample_size=8)._dinfo.expand(frame, pad=False)[0].shape[1]) - 1
        assert ext > 8                                 # the categoricals are one-hot columns
    m = _train(frame, ntrees=T, sample_size=256, extension_level=ext)
    X = m._dinfo.expand(frame, pad=False)[0]
    assert X.is_cuda and X.dtype == torch.float32
    orc = oracle(m._trees, X.cpu().numpy())
    ok = ~orc.ambiguous
    assert int((~ok).sum()) * 1000 <= ok.size
    want = (orc.sums / T).astype(np.float32)
    kernel = m.predict(frame).as_data_frame()["mean_length"].values.astype(np.float32)
    assert np.array_equal(kernel[ok], want[ok])
    monkeypatch.setenv("H2O3_TREE_EIF", "torch")
    dense = m.predict(frame).as_data_frame()["mean_length"].values.astype(np.float32)
    assert np.array_equal(dense[ok], want[ok])


def test_memory_of_the_entry_and_of_predict():
    """n = 200 000, P = 16.  The entry with `out` given allocates nothing (1 MiB
    of slack); predict peaks at no more than the design matrix's own peak E
    plus 64 bytes per row (the f64 total, length, score, the stacked pair and
    the two f32 columns), where the dense rule needs E + 24 * n * P."""
    import h2o3_amd as h2o
    n, P = 200_000, 16
    rng = np.random.default_rng(1)
    fr = h2o.H2OFrame(pd.DataFrame(rng.normal(size=(n, P)).astype(np.float32), columns=[f"x{i}" for i in range(P)]))
    m = H2OExtendedIsolationForestEstimator(ntrees=10, sample_size=64, extension_level=1, seed=1)
    m.train(training_frame=fr)
    X = m._dinfo.expand(fr, pad=False)[0]
    assert tuple(X.shape) == (n, P)
    pack = m._sparse_pack()
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    eif_ops.hyperplane_forest_lengths(pack, X, out=out)          # moves the tables to the device, once
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    eif_ops.hyperplane_forest_lengths(pack, X, out=out)
    torch.cuda.synchronize()
    print("entry: peak over base", torch.cuda.max_memory_allocated() - base)
    assert torch.cuda.max_memory_allocated() - base <= 1 << 20
    del X, out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    X = m._dinfo.expand(fr, pad=False)[0]
    torch.cuda.synchronize()
    E = torch.cuda.max_memory_allocated() - base
    del X
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pred = m.predict(fr)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("expand peak", E, "predict peak", peak, "allowed", E + 64 * n, "dense rule at least", E + 24 * n * P)
    assert pred.nrows == n
    assert peak <= E + 64 * n


def test_scoring_history_matches_oracle(frame, monkeypatch):
    monkeypatch.delenv("H2O3_TREE_EIF", raising=False)
    m = _train(frame, ntrees=10, sample_size=128, extension_level=2, score_tree_interval=4)
    sh = m.scoring_history()
    assert list(sh["number_of_trees"]) == [4, 8, 10]
    X = m._dinfo.expand(frame, pad=False)[0].cpu().numpy()
    for k, ln, sc in zip(sh["number_of_trees"], sh["mean_tree_path_length"], sh["mean_anomaly_score"]):
        orc = oracle(m._trees[:k], X)
        assert int(orc.ambiguous.sum()) * 1000 <= X.shape[0]
        ml = orc.sums / k
        np.testing.assert_allclose(ln, ml.mean(), rtol=1e-12)
        np.testing.assert_allclose(sc, np.power(2.0, -ml / c_factor(m._psi)).mean(), rtol=1e-12)
    assert sh["mean_tree_path_length"].iloc[-1] == m._training_metrics.get("mean_length")
    assert sh["mean_anomaly_score"].iloc[-1] == m._training_metrics.get("mean_score")
