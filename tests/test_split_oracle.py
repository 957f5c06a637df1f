"""The exact split oracle of split_common.py against the CPU users' path
(TreeGrower._find_splits_torch on a CPU device), and the case table's own
conditions.  Runs without a GPU; the HIP kernels meet the same oracle and the
same table in test_split_kernels_gpu.py.

A node the oracle does not split must come back with gain = -inf; its other
fields (feature, threshold, sums, mask) have no defined value on either path
and are not read by the growers, so only the gain is compared there.  No case
and no node is left out of a comparison."""
import numpy as np
import pytest
import torch

import split_common as sc

ALL = sorted(sc.CASES)


@pytest.mark.parametrize("name", ALL)
def test_case_meets_the_classification(name):
    """Every comparison of the rule is decided between identical operands or
    by a 1e-9 margin above the rounding bound (the oracle raises otherwise)."""
    res = sc.oracle(name)
    case = sc.CASES[name]
    Fl, n, Bs, _ = case.H.shape
    assert len(res.nodes) == n and all(len(r) == Fl for r in res.cols)
    for nd in res.nodes:
        for mw, _ in case.sel2:
            sc.select2_ok(case, nd, mw)
    if case.family == "int":
        assert np.all(case.H * 8 == np.round(case.H * 8)) and np.abs(case.H).sum() < 2.0 ** 40


def test_table_covers_the_shapes_and_edges():
    """Nothing is excluded, and the table holds what it is meant to hold."""
    assert ALL == sorted(sc.CASES) and len(ALL) == len(set(ALL))
    shp = {(c.H.shape[2] - 1, c.H.shape[1], c.H.shape[0], c.crit) for c in sc.CASES.values()}
    for B in (1, 2, 3, 63, 64, 65, 66, 128, 129, 255, 1000):
        assert {cr for (b, _, _, cr) in shp if b == B} == {0, 1}, B
    for Fl in (1, 3, 13, 64, 65, 130):
        assert {cr for (_, _, f, cr) in shp if f == Fl} == {0, 1}, Fl
    assert {n for (_, n, _, _) in shp} >= {1, 3, 5, 6}
    assert {(n * f) % 4 for (_, n, f, _) in shp} == {0, 1, 2, 3}
    nodes = lambda nm: sc.oracle(nm).nodes
    assert [(d.opt, d.t, d.gain) for d in nodes("tie_opt0_later_chunk")] == [(0, 67, 250)]
    assert [(d.opt, d.t) for d in nodes("tie_mirror_cross_lane")] == [(0, 70)]
    assert [(d.opt, d.t) for d in nodes("tie_three_chunks")] == [(0, 197)]
    for nm in ("tie_opt0_later_chunk", "tie_mirror_cross_lane", "tie_three_chunks", "int_empty_runs_se",
               "int_empty_runs_xgb", "na_vs_rest_ties_threshold", "identical_features_1_65", "identical_features_0_1"):
        assert sc.oracle(nm).ties > 0, nm
    assert nodes("na_vs_rest_wins")[0].opt == 2 and nodes("na_vs_rest_wins_xgb")[0].opt == 2
    assert (nodes("na_vs_rest_ties_threshold")[0].opt, nodes("na_vs_rest_ties_threshold")[0].t) == (0, 1)
    assert all(d.feat == 1 for d in nodes("identical_features_1_65"))
    assert all(d.feat == 0 for d in nodes("identical_features_0_1"))
    assert [d.gain is None for d in nodes("min_rows_boundary")] == [False, True]
    assert [d.gain is None for d in nodes("min_rows_boundary_xgb")] == [False, True]
    assert [d.gain is None for d in nodes("float32_equal_means")] == [True, False]
    for nm in ("msi_removes_only_candidate", "pure_node", "all_zero_se", "all_zero_xgb", "all_zero_xgb_lambda0"):
        assert all(d.gain is None for d in nodes(nm)), nm
    for nm in ("empty_node_between", "empty_node_between_xgb_lambda0", "node_all_masked_se", "node_all_masked_xgb",
               "xgb_zero_hessian_lambda0", "xgb_zero_hessian_lambda1"):
        assert [d.gain is None for d in nodes(nm)] == [False, True, False], nm
    assert all(d.gain is None for lam in (0.0, 0.5, 1.0) for a in (0.0, 0.25, 6.0)
               for d in nodes(f"xgb_l{lam}_a{a}_g10000.0"))
    assert nodes("bounds_winner_changes_column")[0].feat == 1 and nodes("bounds_winner_keeps_column")[0].feat == 0
    # monotone / bounds cases change the free result
    for tag in ("se", "xgb"):
        free = sc.oracle(f"bounds_none_ub1_{tag}").nodes
        assert any(a[:5] != b[:5] for a, b in zip(free, sc.oracle(f"bounds_two_sided_ub1_{tag}").nodes))
        assert any(a[:5] != b[:5] for a, b in zip(sc.oracle(f"bounds_two_sided_ub0_{tag}").nodes,
                                                  sc.oracle(f"bounds_two_sided_ub1_{tag}").nodes))
        assert any(a[:5] != b[:5] for a, b in zip(sc.oracle(f"monotone_inc_{tag}").nodes,
                                                  sc.oracle(f"monotone_dec_{tag}").nodes))
    c = sc.CASES["select2_min_w2"]
    oks = {(mw, tuple(sc.select2_ok(c, d, mw) for d in sc.oracle(c.name).nodes)) for mw, _ in c.sel2}
    assert len({o for _, o in oks}) >= 2


@pytest.mark.parametrize("name", ALL)
def test_oracle_matches_torch_cpu(name):
    case = sc.CASES[name]
    res = sc.oracle(name)
    gr, cm = sc.make_grower(case)
    out = gr._find_splits_torch(torch.as_tensor(case.H.copy()), cm, torch.as_tensor(case.wyy.copy()))
    for i, nd in enumerate(res.nodes):
        g = float(out["gain"][i])
        if nd.gain is None:
            assert g == -np.inf, (name, i, g)
            continue
        assert abs(g - float(nd.gain)) <= nd.gtol, (name, i, g, float(nd.gain), nd.gtol)
        assert (int(out["feat"][i]), int(out["t"][i]), int(out["opt"][i])) == (nd.feat, nd.t, nd.opt), (name, i)
        assert np.array_equal(out["mask"][i].numpy(), nd.mask), (name, i)
        for ch in range(2):
            assert abs(float(out["L"][i, ch]) - float(nd.L[ch])) <= sc.sum_tol(case, nd, nd.L[ch]), (name, i, ch)
