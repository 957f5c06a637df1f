"""ops.eif_ops on the CPU: the sparse hyperplane-forest tables against the node
lists they were packed from, the torch twin of the scoring kernel against
eif_common.oracle (equal bits on every non-ambiguous row, see eif_common), and
what the Extended Isolation Forest estimator builds on them: predictions,
score_tree_interval's scoring history, save / load."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o3_amd as h2o
from h2o3_amd.estimators import H2OExtendedIsolationForestEstimator
from h2o3_amd.ops import eif_ops

from eif_common import CASE_NAMES, TILE_MAX_P, compare, oracle, reference


def test_tile_limit_is_the_one_the_cases_straddle():
    assert eif_ops.TILE_MAX_P == TILE_MAX_P
    assert eif_ops.launch_plan(TILE_MAX_P).tile and not eif_ops.launch_plan(TILE_MAX_P + 1).tile
    assert eif_ops.launch_plan(3, 4, False) == (4, False)
    with pytest.raises(ValueError):
        eif_ops.launch_plan(3, 3)
    with pytest.raises(ValueError):
        eif_ops.launch_plan(TILE_MAX_P + 1, 2, True)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pack_holds_the_nonzero_entries(name):
    trees, X, _ = reference(name)
    pack = eif_ops.pack_hyperplane_forest(trees)
    assert pack.hdr.dtype == np.int32 and pack.col.dtype == np.int32 and pack.np.dtype == np.float64
    assert pack.hdr.shape == (sum(len(t) for t in trees), 4) and pack.np.shape == (pack.col.shape[0], 2)
    assert (pack.np[:, 0] != 0).all()
    leaf_bytes = pack.hdr.view(np.float64)[:, 1]
    used = 0
    for t, tr in enumerate(trees):
        base = int(pack.roots[t])
        assert base == sum(len(u) for u in trees[:t])
        for i, (nv, pt, l, r, v, _) in enumerate(tr):
            h = pack.hdr[base + i]
            if l < 0:
                assert h[0] == -1 and leaf_bytes[base + i] == v and pack.value[base + i] == v
                continue
            nz = np.flatnonzero(nv)
            assert (h[0], h[1], h[2], h[3]) == (base + l, base + r, used, nz.size)
            e = slice(used, used + nz.size)
            assert np.array_equal(pack.col[e], nz) and (np.diff(pack.col[e]) > 0).all()
            assert np.array_equal(pack.np[e, 0], nv[nz]) and np.array_equal(pack.np[e, 1], pt[nz])
            used += nz.size
    assert used == pack.col.shape[0]
    assert pack.P <= X.shape[1]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cpu_twin_matches_oracle(name):
    trees, X, orc = reference(name)
    T = len(trees)
    pack = eif_ops.pack_hyperplane_forest(trees)
    Xt = torch.tensor(X)
    out, nodes = eif_ops.hyperplane_forest_lengths(pack, Xt, 0, T, node_out=True)
    compare(orc, out.numpy(), nodes.numpy())
    acc = torch.zeros(X.shape[0], dtype=torch.float64)
    assert eif_ops.hyperplane_forest_lengths(pack, Xt, 0, 1, out=acc) is acc
    _, tail = eif_ops.hyperplane_forest_lengths(pack, Xt, 1, T, out=acc, node_out=True)
    assert torch.equal(acc, out) and torch.equal(tail, nodes[:, 1:])
    before = acc.clone()
    _, none = eif_ops.hyperplane_forest_lengths(pack, Xt, 0, 0, out=acc, node_out=True)
    assert torch.equal(acc, before) and tuple(none.shape) == (X.shape[0], 0)


def test_cpu_twin_walks_in_row_chunks(monkeypatch):
    trees, X, orc = reference("n777_P3_T12")
    monkeypatch.setattr(eif_ops, "CPU_CHUNK_BYTES", 8 * 3 * 100)      # 100 rows at a time
    out = eif_ops.hyperplane_forest_lengths(eif_ops.pack_hyperplane_forest(trees), torch.tensor(X))
    compare(orc, out.numpy())


def test_entry_checks_its_arguments():
    trees, X, _ = reference("n63_P3_T5")
    pack = eif_ops.pack_hyperplane_forest(trees)
    Xt = torch.tensor(X)
    for bad in (lambda: eif_ops.hyperplane_forest_lengths(pack, Xt, 2, 1),
                lambda: eif_ops.hyperplane_forest_lengths(pack, Xt, 0, 6),
                lambda: eif_ops.hyperplane_forest_lengths(pack, Xt.double()),
                lambda: eif_ops.hyperplane_forest_lengths(pack, Xt[:, :2].contiguous()),
                lambda: eif_ops.hyperplane_forest_lengths(pack, Xt.T.contiguous().T),
                lambda: eif_ops.hyperplane_forest_lengths(pack, Xt, out=torch.zeros(5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ the estimator
NCOL = 5


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(400, NCOL))
    A[:12] += 4.0
    A[rng.random(A.shape) < 0.05] = np.nan
    return h2o.H2OFrame(pd.DataFrame(A, columns=[f"x{i}" for i in range(NCOL)]))


def _matrix(m, fr):
    return m._dinfo.expand(fr, pad=False)[0]


@pytest.mark.parametrize("sample_size", [2, 64])
@pytest.mark.parametrize("ext", [0, 1, NCOL - 1])
def test_trained_model_matches_oracle(frame, sample_size, ext):
    T = 8
    m = H2OExtendedIsolationForestEstimator(ntrees=T, sample_size=sample_size, extension_level=ext, seed=7)
    m.train(training_frame=frame)
    X = _matrix(m, frame)
    assert X.shape[1] == NCOL and len(m._trees) == T
    for tr in m._trees:
        assert all(np.count_nonzero(nd[0]) == ext + 1 for nd in tr if nd[2] >= 0)
    orc = oracle(m._trees, X.cpu().numpy())
    pack = eif_ops.pack_hyperplane_forest(m._trees)
    compare(orc, eif_ops.hyperplane_forest_lengths(pack, X.cpu().contiguous()).numpy())
    ml = m.predict(frame).as_data_frame()["mean_length"].values.astype(np.float32)
    ok = ~orc.ambiguous
    assert int((~ok).sum()) * 1000 <= ok.size
    assert np.array_equal(ml[ok], (orc.sums / T).astype(np.float32)[ok])


def test_scoring_history_walks_each_tree_once(frame, monkeypatch):
    seen = []
    real = H2OExtendedIsolationForestEstimator._add_lengths

    def spy(self, X, tot, t0, t1):
        seen.append((t0, t1))
        return real(self, X, tot, t0, t1)
    monkeypatch.setattr(H2OExtendedIsolationForestEstimator, "_add_lengths", spy)
    m = H2OExtendedIsolationForestEstimator(ntrees=10, sample_size=64, extension_level=1, seed=2, score_tree_interval=4)
    m.train(training_frame=frame)
    assert seen == [(0, 4), (4, 8), (8, 10)]
    sh = m.scoring_history()
    assert list(sh["number_of_trees"]) == [4, 8, 10]
    assert {"timestamp", "duration", "mean_tree_path_length", "mean_anomaly_score"} <= set(sh.columns)
    assert sh["mean_tree_path_length"].iloc[-1] == m._training_metrics.get("mean_length")
    assert sh["mean_anomaly_score"].iloc[-1] == m._training_metrics.get("mean_score")
    assert not any(isinstance(v, torch.Tensor) and v.numel() == frame.nrows for v in m.__dict__.values())
    # every entry is the mean over the trees grown so far
    X = _matrix(m, frame).cpu().numpy()
    for k, got in zip(sh["number_of_trees"], sh["mean_tree_path_length"]):
        orc = oracle(m._trees[:k], X)
        assert not orc.ambiguous.any()
        np.testing.assert_allclose(got, (orc.sums / k).mean(), rtol=1e-12)
    del seen[:]
    plain = H2OExtendedIsolationForestEstimator(ntrees=10, sample_size=64, extension_level=1, seed=2)
    plain.train(training_frame=frame)
    assert seen == [(0, 10)]
    assert len(plain.scoring_history()) == 0
    a, b = m.predict(frame).as_data_frame(), plain.predict(frame).as_data_frame()
    assert np.array_equal(a.values, b.values)
    assert plain._training_metrics.get("mean_length") == m._training_metrics.get("mean_length")


def test_save_and_load_predict_the_same(frame, tmp_path):
    m = H2OExtendedIsolationForestEstimator(ntrees=6, sample_size=64, extension_level=2, seed=4)
    m.train(training_frame=frame)
    want = m.predict(frame).as_data_frame()
    assert m._sparse_pack() is m._sparse_pack()
    back = h2o.load_model(h2o.save_model(m, str(tmp_path), force=True))
    assert "_eif_sparse" not in back.__dict__               # derived state is not saved
    assert np.array_equal(back.predict(frame).as_data_frame().values, want.values)
    assert back._sparse_pack().ntrees == 6
    # a forest that changes drops the derived pack
    back._trees = back._trees[:3]
    assert back._sparse_pack().ntrees == 3
