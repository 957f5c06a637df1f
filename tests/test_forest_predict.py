"""Forest scoring on the CPU (Forest.pack + Forest._predict_torch, the twin
of forest_predict_kernel) against forest_predict_common.oracle, a per-row walk
over the Tree lists that never reads pack(): exact (rtol = atol = 0), since
both add the same f32 leaf values in tree order.  This is what makes the
oracle and the case table trustworthy before a GPU is involved;
test_forest_predict_gpu.py runs the same table on the kernel."""
import numpy as np
import pytest
import torch

from forest_predict_common import (CASE_NAMES, CHAIN_DEEPEST_LEAF, assert_covered, chain_trees, edge_forest,
                                   edge_rows, lane_forests, leaf_sums, oracle, reference)

from h2o3_amd.models.tree.shared import Forest

# 1e300 overflows to +inf in pack()'s f32 cast, as the edge forest means it to
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered in cast:RuntimeWarning")


def _exact(got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    torch.testing.assert_close(got, torch.from_numpy(want.copy()), rtol=0, atol=0)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_torch_walk_matches_oracle(name):
    fo, X, K, orc = reference(name)
    Xt = torch.tensor(X)
    P = fo.pack("cpu")
    _exact(Forest._predict_torch(Xt, K, P), orc.sums)
    leaf = Forest._predict_torch(Xt, K, P, leaf=True)
    assert leaf.dtype == torch.int32
    assert torch.equal(leaf, torch.from_numpy(orc.leaf.copy()))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_upto_prefixes_match_oracle(name):
    fo, X, K, orc = reference(name)
    Xt = torch.tensor(X)
    for u in range(len(fo) + 1):
        _exact(fo.predict(Xt, K, upto=u), leaf_sums(fo, orc.leaf, K, 0, u)[0])
    u = len(fo) // 2
    assert torch.equal(fo.predict(Xt, K, upto=u, leaf=True), torch.from_numpy(orc.leaf[:, :u].copy()))
    _exact(fo.predict(Xt, K), orc.sums)                    # the full pack again after the prefixes


@pytest.mark.parametrize("name", CASE_NAMES)
def test_predict_range_matches_oracle(name):
    fo, X, K, orc = reference(name)
    Xt = torch.tensor(X)
    T = len(fo)
    for a, b in {(0, T), (0, 0), (T, T), (T // 2, T // 2), (0, T // 2), (T // 2, T), (1, T), (T - 1, T)}:
        if 0 <= a <= b:
            _exact(fo.predict_range(Xt, K, a, b), leaf_sums(fo, orc.leaf, K, a, b)[0])


def test_oracle_upto_is_a_prefix():
    fo, X, K, orc = reference("edge_n257")
    part = oracle(fo, X, K, upto=3)
    assert np.array_equal(part.leaf, orc.leaf[:, :3])
    assert np.array_equal(part.sums, leaf_sums(fo, orc.leaf, K, 0, 3)[0])


def test_edge_case_covers_every_decision_outcome():
    assert_covered(reference("edge_n777").oracle.record)
    fo = edge_forest()
    assert_covered(oracle(fo, edge_rows(fo, 777), 1).record)


# chains per lane forest; the two stump-only forests have none
LANE_CHAINS = {"lane_T1_chain": 1, "lane_T1_stump": 0, "lane_T2_stump_chain": 1, "lane_T3_chain_stump": 1,
               "lane_T3_stumps": 0, "lane_T4": 1, "lane_T5": 1, "lane_T7": 2, "lane_T8": 1, "lane_T5_nocat": 1}


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith("lane_")])
def test_lane_rows_walk_the_chains_to_the_end(name):
    """A condition on the inputs, from the oracle alone: in every 64-deep
    chain some row reaches the deepest leaf, 60 levels and more after the
    stump or depth-3 tree in the neighbouring lane ended, and (with more than
    one row) other rows leave it at levels 0, 1 and 62."""
    fo, X, _, orc = reference(name)
    chains = chain_trees(fo)
    assert len(chains) == LANE_CHAINS[name.rsplit("_n", 1)[0]]
    assert all(max(t.depth) <= 3 for i, t in enumerate(fo.trees) if i not in chains)
    for c in chains:
        ids = orc.leaf[:, c]
        deep = ids == CHAIN_DEEPEST_LEAF
        assert deep.any()
        if X.shape[1] > 1:
            assert {1, 3, 2 * 62 + 1} <= set(ids.tolist())
        stumps = [s for s in (c - 1, c + 1) if 0 <= s < len(fo) and fo.trees[s].n_nodes == 1]
        assert stumps or "stump" not in name               # lane_T2_stump_chain, lane_T3_chain_stump
        for s in stumps:                                   # the same rows sit in the root of the stump beside it
            assert not orc.leaf[deep, s].any()


def test_edge_rows_hold_thresholds_and_neighbours():
    fo = edge_forest()
    X = edge_rows(fo, 777)
    assert X.dtype == np.float32 and X.shape == (8, 777)
    with np.errstate(over="ignore", under="ignore"):
        for t in fo.trees:
            for i in range(t.n_nodes):
                if t.left[i] < 0 or (t.is_cat[i] and t.cat_left[i] is not None):
                    continue
                v = np.float32(t.thr[i])
                row = X[t.feat[i]]
                for w in (v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))):
                    assert (row.view(np.int32) == np.float32(w).view(np.int32)).any(), (t.feat[i], w)
    assert (X[3].view(np.uint32) == 0x80000000).any() and (X[3].view(np.uint32) == 0).any()   # -0.0 and 0.0


def test_pack_structure_of_edge_forest():
    """What pack() hands the kernel, decoded and compared with the Tree lists."""
    fo = edge_forest()
    P = fo.pack("cpu")
    node = P["node"].numpy()
    roots = P["roots"].numpy()
    assert node.dtype == np.int32 and node.shape == (sum(t.n_nodes for t in fo.trees), 4)
    assert roots.tolist() == np.cumsum([0] + [t.n_nodes for t in fo.trees])[:-1].tolist()
    assert P["tclass"].tolist() == fo.tclass and P["T"] == len(fo)
    bits = P["cat_bits"].numpy()
    nb = 0
    with np.errstate(over="ignore", under="ignore"):
        for t, base in zip(fo.trees, roots):
            for i in range(t.n_nodes):
                w, tb, l, r = (int(v) for v in node[base + i])
                j = base + i
                assert int(P["left"][j]) == l and int(P["right"][j]) == r
                assert np.float32(P["value"][j].item()) == np.float32(t.value[i])
                if t.left[i] < 0:
                    assert l == -1 and r == -1
                    continue
                assert l == base + t.left[i] and r == base + t.right[i]
                has_mask = bool(t.is_cat[i]) and t.cat_left[i] is not None
                assert w & 0x3FFFFFFF == t.feat[i] == int(P["feat"][j])
                assert (w >> 30) & 1 == int(bool(t.na_left[i])) == int(P["na_left"][j])
                assert (w < 0) == has_mask == (int(P["cat_off"][j]) >= 0)
                if has_mask:
                    m = np.asarray(t.cat_left[i]).reshape(-1)
                    # offsets increase in node order, disjoint, without gaps
                    assert int(P["cat_off"][j]) == nb and int(P["cat_len"][j]) == m.size
                    assert np.array_equal(bits[nb:nb + m.size], m)
                    nb += m.size
                else:
                    assert int(P["cat_len"][j]) == 0
                    want = np.float32(t.thr[i]).view(np.int32)
                    assert np.int32(tb) == want and P["thr"].numpy().view(np.int32)[j] == want
    assert nb == bits.size == 1 + 4 + 300 * 3 + 4
    # 1e300 is +inf, -1e-45 the smallest subnormal, -1e-46 is -0.0
    tbits = set(node[:, 1].view(np.uint32).tolist())
    assert {0x7F800000, 0x80000001, 0x80000000} <= tbits


def test_pack_without_categorical_split_has_placeholder_bits():
    fo = lane_forests()["lane_T5_nocat"]
    P = fo.pack("cpu")
    assert P["cat_bits"].numel() == 1 and bool((P["cat_off"] == -1).all()) and bool((P["cat_len"] == 0).all())
    assert bool((P["node"][:, 0] >= 0).all())
