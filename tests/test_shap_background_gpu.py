"""ops/csrc/tree_shap.hip (baseline SHAP kernels) against the 2^F subset
enumeration, the torch implementation of the same rule, and the scoring
kernel's decisions (Forest.predict)."""
import numpy as np
import pandas as pd
import pytest
import torch

from shap_bg_common import chain_forest, enumerate_all, hand_forest, hand_rows

pytestmark = pytest.mark.gpu

# f64 atomic sums of O(1) leaf values (the tolerances of test_logit_hist_gpu.py)
RTOL, ATOL = 1e-10, 1e-9
N_TEST, N_BG = 777, 33


def _run(fo, X, Z, F, **kw):
    from h2o3_amd.ops import shap_ops
    dev = X.device
    return shap_ops.background_shap(fo.pack(dev), fo.leaf_paths(dev), X, Z, F, **kw)


def _torch_ref(fo, X, Z, F, **kw):
    from h2o3_amd.ops import shap_ops
    dev = X.device
    return shap_ops.background_shap_torch(fo.pack(dev), fo.leaf_paths(dev), X, Z, F, **kw)[0]


def test_hand_built_forest_matches_enumeration():
    fo = hand_forest()
    Xh, Zh = hand_rows(5, 1), hand_rows(4, 2)
    ref = enumerate_all(fo, Xh, Zh)
    X, Z = torch.tensor(Xh, device="cuda"), torch.tensor(Zh, device="cuda")
    res = _run(fo, X, Z, 6, per_reference=True)
    assert res.kernel and res.why is None
    np.testing.assert_allclose(res.phi.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    avg = _run(fo, X, Z, 6)
    assert avg.kernel
    np.testing.assert_allclose(avg.phi.cpu().numpy(), ref.reshape(5, 4, 7).mean(1), rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def gbm_case():
    """GBM (10 trees, depth 5) on numeric + categorical columns with NAs; the
    777 x 33 score matrices get NaN and out-of-range categorical codes in
    both frames; the torch implementation's results are computed once."""
    import h2o3_amd as h2o
    from h2o3_amd.estimators import H2OGradientBoostingEstimator
    rng = np.random.default_rng(11)
    n = 1500
    A = rng.normal(size=(n, 5))
    A[rng.random(n) < 0.06, 1] = np.nan
    df = pd.DataFrame(A, columns=[f"x{i}" for i in range(5)])
    df["c1"] = rng.choice(list("abcdefg"), n)
    df["c2"] = rng.choice(["u", "v", "w"], n)
    df.loc[rng.random(n) < 0.05, "c1"] = None
    df["y"] = (A[:, 0] + np.nan_to_num(A[:, 1]) * (df["c2"] == "u") - 0.7 * (df["c1"].isin(["a", "d"])) +
               0.5 * A[:, 2] * A[:, 3] + rng.normal(scale=0.2, size=n))
    fr = h2o.H2OFrame(df)
    x = [f"x{i}" for i in range(5)] + ["c1", "c2"]
    m = H2OGradientBoostingEstimator(ntrees=10, max_depth=5, seed=1, min_rows=5)
    m.train(x=x, y="y", training_frame=fr)
    M = m._score_matrix(fr).clone()
    assert M.is_cuda
    X = M[:, :N_TEST].contiguous()
    Z = M[:, N_TEST:N_TEST + N_BG].contiguous()
    for T in (X, Z):                       # categorical rows 5, 6: NaN, past the bitset, negative
        T[5, 0], T[5, 1], T[5, 2], T[6, 3], T[6, 4] = float("nan"), 40.0, -3.0, 3.0, float("nan")
        T[0, 5] = float("nan")
    fo = m._forest
    F = len(x)
    assert fo.leaf_paths(X.device)["L"] > 100
    ref = {pr: _torch_ref(fo, X, Z, F, per_reference=pr) for pr in (False, True)}
    return fo, X, Z, F, ref


@pytest.mark.parametrize("per_reference", [False, True])
def test_trained_gbm_matches_torch_default_scratch(gbm_case, per_reference):
    fo, X, Z, F, ref = gbm_case
    res = _run(fo, X, Z, F, per_reference=per_reference)
    assert res.kernel and (res.row_tiles, res.bg_tiles, res.tree_chunks) == (1, 1, 1)
    assert res.phi.shape == ((N_TEST * N_BG if per_reference else N_TEST), F + 1)
    np.testing.assert_allclose(res.phi.cpu().numpy(), ref[per_reference].cpu().numpy(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("per_reference", [False, True])
def test_trained_gbm_matches_torch_tiled(gbm_case, per_reference):
    """A scratch bound that holds one tree's masks for 256 + 33 rows: 4 row
    tiles (777 rows) and at least 3 tree chunks."""
    fo, X, Z, F, ref = gbm_case
    PT = fo.leaf_paths(X.device)
    budget = 4 * PT["max_tree_leaves"] * (256 + N_BG)
    res = _run(fo, X, Z, F, per_reference=per_reference, max_scratch_bytes=budget)
    assert res.kernel
    assert res.row_tiles >= 3 and res.tree_chunks >= 3, (res.row_tiles, res.tree_chunks)
    np.testing.assert_allclose(res.phi.cpu().numpy(), ref[per_reference].cpu().numpy(), rtol=RTOL, atol=ATOL)


def _sigmoid_scale(fx, fz):
    d = fx.view(-1, 1) - fz.view(1, -1)
    g = torch.sigmoid(fx).view(-1, 1) - torch.sigmoid(fz).view(1, -1)
    return torch.where(d == 0, torch.zeros_like(d), g / torch.where(d == 0, torch.ones_like(d), d))


@pytest.mark.parametrize("per_reference", [False, True])
def test_background_rows_tiled(gbm_case, per_reference):
    """A scratch bound below one tree's masks for 64 + 33 rows splits the
    background rows too (tiles of 9): the per-reference index and the pair
    factors' stride at a background offset."""
    fo, X, Z, F, ref = gbm_case
    PT = fo.leaf_paths(X.device)
    budget = 4 * PT["max_tree_leaves"] * (64 + 9)
    res = _run(fo, X, Z, F, per_reference=per_reference, max_scratch_bytes=budget)
    assert res.kernel and res.bg_tiles >= 3 and res.row_tiles >= 3, (res.row_tiles, res.bg_tiles)
    np.testing.assert_allclose(res.phi.cpu().numpy(), ref[per_reference].cpu().numpy(), rtol=RTOL, atol=ATOL)
    budget += 40 * 64 * 9                      # room for the pair factors of a 64 x 9 tile
    res = _run(fo, X, Z, F, per_reference=per_reference, pair_scale=_sigmoid_scale, max_scratch_bytes=budget)
    assert res.kernel and res.bg_tiles >= 3, res.bg_tiles
    want = _torch_ref(fo, X, Z, F, per_reference=per_reference, pair_scale=_sigmoid_scale)
    np.testing.assert_allclose(res.phi.cpu().numpy(), want.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_empty_test_shard(gbm_case):
    """No test rows (an empty shard of a multi-rank frame): empty output."""
    fo, X, Z, F, _ = gbm_case
    for pr in (False, True):
        res = _run(fo, X[:, :0].contiguous(), Z, F, per_reference=pr)
        assert res.kernel and res.phi.shape == (0, F + 1) and res.fz.shape == (N_BG,)


@pytest.mark.parametrize("F", [120, 320])
def test_many_features(F):
    """Averaged mode's other two launch forms: per-row LDS sums above 64 KiB
    (F = 120) and, past the LDS of a CU (F = 320), global f64 atomics.  The
    forest splits on features spread over 0 .. F-1."""
    from h2o3_amd.ops import _native
    lib = _native.get_lib("tree_shap", required=True)
    lds = lib.h2o_shap_lds_bytes(F)
    assert (64 << 10) < lds <= (160 << 10) if F == 120 else lds > (160 << 10)
    feats = [int(v) for v in np.linspace(0, F - 1, 20)]
    fo = chain_forest(20, seed=6, feats=feats)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(F, 130, generator=g)
    Z = torch.randn(F, 9, generator=g)
    X[feats[3], 0] = Z[feats[-1], 2] = float("nan")
    X, Z = X.cuda(), Z.cuda()
    for pr in (False, True):
        res = _run(fo, X, Z, F, per_reference=pr)
        assert res.kernel
        ref = _torch_ref(fo, X, Z, F, per_reference=pr)
        np.testing.assert_allclose(res.phi.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=ATOL)
    fx = fo.predict(X, 1)[:, 0].double()
    torch.testing.assert_close(_run(fo, X, Z, F).phi.sum(1), fx, rtol=0, atol=1e-5)


def test_pair_factors_match_torch(gbm_case):
    """output_space's per-pair factor is applied before averaging."""
    fo, X, Z, F, _ = gbm_case
    scale = _sigmoid_scale
    for pr in (False, True):
        res = _run(fo, X, Z, F, per_reference=pr, pair_scale=scale)
        ref = _torch_ref(fo, X, Z, F, per_reference=pr, pair_scale=scale)
        np.testing.assert_allclose(res.phi.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_efficiency_identity_against_forest_predict(gbm_case):
    """The SHAP kernels and the scoring kernel take the same decisions (NaN,
    out-of-range categorical codes included): per pair the contributions sum
    to f(x) - f(z) and the bias is f(z).  Forest.predict sums in f32: 1e-5."""
    fo, X, Z, F, _ = gbm_case
    fx = fo.predict(X, 1)[:, 0].double()
    fz = fo.predict(Z, 1)[:, 0].double()
    res = _run(fo, X, Z, F, per_reference=True)
    phi = res.phi.view(N_TEST, N_BG, F + 1)
    torch.testing.assert_close(phi[:, :, :F].sum(2), fx.view(-1, 1) - fz.view(1, -1), rtol=0, atol=1e-5)
    torch.testing.assert_close(phi[:, :, F], fz.view(1, -1).expand(N_TEST, N_BG), rtol=0, atol=1e-5)
    avg = _run(fo, X, Z, F).phi
    torch.testing.assert_close(avg.sum(1), fx, rtol=0, atol=1e-5)


@pytest.mark.parametrize("width", [32, 33])
def test_wide_paths(width):
    """A chain tree whose longest path has exactly 32 distinct features runs
    on the kernel (full mask 0xFFFFFFFF); with 33 the torch implementation
    runs and the result says why.  Both match the torch implementation."""
    fo = chain_forest(width, seed=4)
    F = width + 1
    g = torch.Generator().manual_seed(5)
    X = torch.randn(F, 70, generator=g)
    Z = torch.randn(F, 9, generator=g)
    X[3, 0] = X[31, 1] = Z[0, 2] = Z[width - 1, 3] = float("nan")
    X, Z = X.cuda(), Z.cuda()
    assert fo.leaf_paths(X.device)["max_path"] == width
    for pr in (False, True):
        res = _run(fo, X, Z, F, per_reference=pr)
        if width <= 32:
            assert res.kernel and res.why is None
        else:
            assert not res.kernel and "33 distinct features" in res.why
        ref = _torch_ref(fo, X, Z, F, per_reference=pr)
        np.testing.assert_allclose(res.phi.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=ATOL)
    # efficiency through the deepest leaf too (its full mask is all 32 bits)
    fx = fo.predict(X, 1)[:, 0].double()
    torch.testing.assert_close(_run(fo, X, Z, F).phi.sum(1), fx, rtol=0, atol=1e-5)
