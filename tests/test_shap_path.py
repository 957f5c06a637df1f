"""Path-dependent TreeSHAP in leaf-path form (ops/shap_ops.path_shap_torch over
Forest.leaf_paths' el_zero) against the node recursion of models/tree/shap.py
and the 2^F cover-weighted Shapley enumeration, on CPU tensors."""
import numpy as np
import pytest
import torch

from shap_path_common import (build_tree, chain_forest, covers_by_share, covers_from_rows, enumerate_path_shap,
                              hand_forest, hand_rows)

from h2o3_amd.models.tree.shap import forest_contributions, forest_path_contributions
from h2o3_amd.models.tree.shared import Forest
from h2o3_amd.ops import shap_ops

dev = torch.device("cpu")


def _both(fo, Xn, F):
    X = torch.tensor(Xn)
    PT = fo.leaf_paths(dev)
    got = shap_ops.path_shap_torch(fo.pack(dev), PT, X, F)
    ref = forest_contributions(fo.trees, X, F)
    assert not torch.isnan(got).any() and not torch.isnan(ref).any()
    assert float(got[:, F].abs().max()) == 0.0            # the bias column is the caller's
    return got.numpy(), ref.numpy()


def _hand_counted():
    return covers_from_rows(hand_forest(), hand_rows(6, 3))


def test_leaf_table_zero_fractions():
    fo = _hand_counted()
    PT = fo.leaf_paths(dev)
    assert PT["el_zero"].dtype == torch.float64 and PT["el_zero"].shape == PT["el_feat"].shape
    assert fo.leaf_paths(dev) is PT                        # cached as before
    covers = np.concatenate([np.asarray(t.weight) for t in fo.trees])
    assert (covers == 0).sum() >= 2                        # zero-cover nodes are part of the case
    # per leaf the zero-fractions multiply to cover[leaf] / cover[root]
    off = PT["el_off"].tolist()
    z = PT["el_zero"].numpy()
    li = 0
    for t in fo.trees:
        for j in t.leaves():
            want = t.weight[j] / t.weight[0]
            np.testing.assert_allclose(np.prod(z[off[li]:off[li + 1]]), want, rtol=0, atol=1e-15)
            li += 1
    assert li == PT["L"]


def test_hand_forest_counted_covers_matches_recursion():
    """Zero-cover children, features repeated on a path, a categorical split,
    NaN and out-of-range codes."""
    fo = _hand_counted()
    got, ref = _both(fo, hand_rows(9, 1), 6)
    np.testing.assert_allclose(got[:, :6], ref[:, :6], rtol=0, atol=1e-12)
    full = forest_path_contributions(fo, torch.tensor(hand_rows(9, 1)), 6).numpy()
    np.testing.assert_allclose(full, ref, rtol=0, atol=1e-12)     # bias column included


def test_single_leaf_tree():
    fo = Forest()
    fo.add(build_tree(0.7), 0)
    fo.trees[0].weight = [5.0]
    got, ref = _both(fo, hand_rows(4, 1), 6)
    assert not got.any()
    info = {}
    full = forest_path_contributions(fo, torch.tensor(hand_rows(4, 1)), 6, info=info).numpy()
    np.testing.assert_allclose(full, ref, rtol=0, atol=1e-12)
    assert info == {"kernel": False, "why": "CPU tensors"}


def test_chain_of_32_elements():
    fo = covers_by_share(chain_forest(32, seed=4), left=0.4)
    assert fo.leaf_paths(dev)["max_path"] == 32
    g = torch.Generator().manual_seed(5)
    X = torch.randn(33, 40, generator=g)
    X[3, 0] = X[31, 1] = float("nan")
    got, ref = _both(fo, X.numpy(), 33)
    np.testing.assert_allclose(got[:, :33], ref[:, :33], rtol=0, atol=1e-12)


def test_all_ones_covers_as_they_stand():
    fo = hand_forest()
    got, ref = _both(fo, hand_rows(9, 2), 6)
    np.testing.assert_allclose(got[:, :6], ref[:, :6], rtol=0, atol=1e-12)
    scaled = shap_ops.path_shap_torch(fo.pack(dev), fo.leaf_paths(dev), torch.tensor(hand_rows(9, 2)), 6,
                                      vscale=0.25).numpy()
    np.testing.assert_allclose(scaled, 0.25 * got, rtol=0, atol=1e-12)


@pytest.mark.parametrize("covers", ["counted", "share"])
def test_matches_cover_weighted_enumeration(covers):
    fo = _hand_counted() if covers == "counted" else covers_by_share(hand_forest(), left=0.3)
    Xn = hand_rows(5, 1)
    got = forest_path_contributions(fo, torch.tensor(Xn), 6).numpy()
    want = np.stack([enumerate_path_shap(fo, Xn[:, r], 6) for r in range(Xn.shape[1])])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_cpu_result_says_why_and_checks_features():
    fo = covers_by_share(chain_forest(33, seed=4), left=0.4)
    X = torch.randn(34, 7, generator=torch.Generator().manual_seed(1))
    res = shap_ops.path_shap(fo.pack(dev), fo.leaf_paths(dev), X, 34)
    assert not res.kernel and res.why == "CPU tensors" and res.phi.shape == (7, 35)
    ref = forest_contributions(fo.trees, X, 34)
    np.testing.assert_allclose(res.phi[:, :34].numpy(), ref[:, :34].numpy(), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="splits on a feature"):
        shap_ops.path_shap(fo.pack(dev), fo.leaf_paths(dev), X[:20], 20)
