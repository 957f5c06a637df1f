"""ops/csrc/dl_shap.hip (the DeepSHAP pair kernel) against deep_shap_torch in
f64 on the same f32 weights, under forced tiling, for a net too wide for LDS,
and end to end through the Deep Learning and Stacked Ensemble estimators.

Tolerance of a case: 8 x max(d_ref, 2^-23 max|phi_ref|), where d_ref is the
largest difference between deep_shap_torch run in f32 and in f64 on that case
(both on the CPU, never from the kernel); the factor 8 covers the different
accumulation order of the MFMA tiles."""
import numpy as np
import pytest
import torch

from shap_baseline_common import X_COLS, dl_link_score, make_df, rand_net, rand_rows, train_dl, train_ensemble

pytestmark = pytest.mark.gpu

WIDTHS = [[7, 20, 9, 1], [33, 17, 1], [16, 16, 16, 16, 1]]
SHAPES = [(17, 1), (17, 5), (17, 33), (1, 70), (0, 5)]
ACTS = ["tanh", "rectifier", "exprectifier"]


def _sigmoid_scale():
    from h2o3_amd.models.shap_baseline import _pair_scale
    return _pair_scale(torch.sigmoid)


def _refs(net32, X32, Z32, per_reference, pair_scale):
    """(f64 reference phi, tolerance, d_ref) from the two CPU runs of the torch rule."""
    from h2o3_amd.ops import dl_shap_ops
    kw = dict(per_reference=per_reference, pair_scale=pair_scale, out_b=net32[4])
    r32 = dl_shap_ops.deep_shap_torch(*net32[:4], X32, Z32, **kw).phi
    r64 = dl_shap_ops.deep_shap_torch(*net32[:4], X32.double(), Z32.double(), **kw).phi
    d_ref = float((r32 - r64).abs().max()) if r64.numel() else 0.0
    top = float(r64.abs().max()) if r64.numel() else 0.0
    return r64, 8 * max(d_ref, 2.0 ** -23 * top), d_ref


def _to(net, dev):
    layers, acts, scales, out_w, out_b = net
    return [(W.to(dev), b.to(dev)) for W, b in layers], acts, scales, out_w.to(dev), out_b


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}xB{s[1]}")
@pytest.mark.parametrize("wi", range(len(WIDTHS)), ids=lambda i: "-".join(map(str, WIDTHS[i])))
def test_kernel_matches_the_torch_rule(wi, shape):
    from h2o3_amd.ops import dl_shap_ops
    widths = WIDTHS[wi]
    N, B = shape
    act = ACTS[(wi + N + B) % 3]
    net = rand_net(widths, act, [0.8, 0.9, 0.7], seed=20 + wi, dtype=torch.float32)
    X, Z = rand_rows(N, B, widths[0], seed=30 + B, dtype=torch.float32)
    gnet = _to(net, "cuda")
    for per_reference in (True, False):
        for ps in (None, _sigmoid_scale()):
            ref, tol, d_ref = _refs(net, X, Z, per_reference, ps)
            res = dl_shap_ops.deep_shap(*gnet[:4], X.cuda(), Z.cuda(), per_reference=per_reference, pair_scale=ps,
                                        out_b=gnet[4], use_native=True)
            assert res.kernel and res.why is None
            got = res.phi.cpu()
            assert got.shape == ref.shape == ((N * B if per_reference else N), widths[0] + 1)
            err = float((got - ref).abs().max()) if got.numel() else 0.0
            print(f"dl_shap case widths={widths} act={act} N={N} B={B} per_ref={int(per_reference)} "
                  f"scale={int(ps is not None)} err={err:.3e} d_ref={d_ref:.3e} tol={tol:.3e}")
            assert err <= tol


@pytest.mark.parametrize("N,B", [(50, 70), (50, 33)])
def test_forced_tiling_and_repeats_are_bit_identical(N, B):
    """50 x 70 runs on tiles of 16 background rows, 50 x 33 on tiles of 16
    test rows; either way a slice of the sum is 16 background rows, so a tiny
    budget (several row tiles and background tiles) changes no bit."""
    from h2o3_amd.ops import dl_shap_ops
    net = _to(rand_net([7, 20, 9, 1], "tanh", [0.8, 0.9], seed=41, dtype=torch.float32), "cuda")
    X, Z = (t.cuda() for t in rand_rows(N, B, 7, seed=42, dtype=torch.float32))
    for ps, budget in ((None, 1024), (_sigmoid_scale(), 16384)):
        run = lambda **kw: dl_shap_ops.deep_shap(*net[:4], X, Z, pair_scale=ps, out_b=net[4], use_native=True, **kw)
        one = run()
        assert one.kernel and (one.row_tiles, one.bg_tiles) == (1, 1)
        assert torch.equal(run().phi, one.phi)
        tiled = run(max_scratch_bytes=budget)
        assert tiled.kernel and tiled.row_tiles > 1 and tiled.bg_tiles > 1
        assert torch.equal(tiled.phi, one.phi)


def test_net_too_wide_for_lds_takes_the_torch_rule():
    from h2o3_amd.ops import dl_shap_ops
    widths = [40, 3000, 1]
    assert not dl_shap_ops.dl_shap_fits(widths)
    net = _to(rand_net(widths, "rectifier", [0.9], seed=51, dtype=torch.float32), "cuda")
    X, Z = (t.cuda() for t in rand_rows(9, 4, 40, seed=52, dtype=torch.float32))
    res = dl_shap_ops.deep_shap(*net[:4], X, Z, out_b=net[4])
    assert not res.kernel and "LDS" in res.why
    ref = dl_shap_ops.deep_shap_torch(*net[:4], X, Z, out_b=net[4])
    assert torch.equal(res.phi, ref.phi)
    with pytest.raises(ValueError, match="cannot run"):
        dl_shap_ops.deep_shap(*net[:4], X, Z, out_b=net[4], use_native=True)


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def frames():
    import h2o3_amd as h2o
    return h2o.H2OFrame(make_df()), h2o.H2OFrame(make_df(9, seed=5)), h2o.H2OFrame(make_df(12, seed=8))


def _cpu_net(m):
    from h2o3_amd.models.shap_baseline import _dl_net
    layers, acts, scales, out_w, out_b, linkinv = _dl_net(m)
    return ([(W.detach().cpu(), b.detach().cpu()) for W, b in layers], acts, scales, out_w.detach().cpu(), out_b), \
        linkinv


@pytest.mark.parametrize("y", ["yb", "y"])
def test_trained_deep_learning_on_the_device(frames, y):
    """The estimator's frames against the f64 torch rule on CPU copies of the
    trained weights and design matrices."""
    from h2o3_amd.models.shap_baseline import _pair_scale
    fr, bg, te = frames
    m = train_dl(fr, y)
    assert m._layers[0].W.is_cuda
    names = list(m._dinfo.coef_names)
    P = len(names)
    net, linkinv = _cpu_net(m)
    X, Z = m._design(te)[0].cpu(), m._design(bg)[0].cpu()
    for output_space in (False, True):
        ps = _pair_scale(linkinv) if output_space else None
        ref, tol, d_ref = _refs(net, X, Z, True, ps)
        per = m.predict_contributions(te, background_frame=bg, output_per_reference=True, output_space=output_space)
        assert m._last_shap.kernel and m._last_shap.why is None
        got = per.as_data_frame()[names].values.astype(np.float64)
        err = np.abs(got - ref[:, :P].numpy()).max()
        print(f"dl_shap end-to-end {y} output_space={int(output_space)} err={err:.3e} d_ref={d_ref:.3e} tol={tol:.3e}")
        assert err <= tol
        avg = m.predict_contributions(te, background_frame=bg, output_space=output_space).as_data_frame()
        assert np.abs(avg[names].values - ref[:, :P].view(te.nrows, bg.nrows, P).mean(1).numpy()).max() <= tol
    fx = dl_link_score(m, te)
    avg = m.predict_contributions(te, background_frame=bg).as_data_frame()
    np.testing.assert_allclose(avg[names].values.sum(1) + avg["BiasTerm"].values, fx, rtol=0,
                               atol=2e-5 * max(1.0, np.abs(fx).max()))


def test_stacked_ensemble_on_the_device(frames, monkeypatch):
    """The ensemble with its DL base model on the kernel against the same
    ensemble on the torch rule in f32 (itself d_ref away from the f64 rule):
    they differ by the DL base model's error times |beta_dl|
    (metalearner_transform NONE: du / dp = 1), plus the f32 rounding of the
    frame columns."""
    import h2o3_amd as h2o
    from h2o3_amd.models.shap_baseline import _meta_coefs, _pair_scale
    from h2o3_amd.ops import dl_shap_ops
    fr, bg, te = frames
    se = train_ensemble(fr, "yb", "NONE")
    dl = se._base[2]
    net, linkinv = _cpu_net(dl)
    _, tol_dl, d_ref = _refs(net, dl._design(te)[0].cpu(), dl._design(bg)[0].cpu(), True, _pair_scale(linkinv))
    beta_dl = abs(_meta_coefs(se)[0][2])
    monkeypatch.setattr(dl_shap_ops, "NATIVE_DEFAULT", True)
    got = se.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    monkeypatch.setattr(dl_shap_ops, "NATIVE_DEFAULT", False)
    ref = se.predict_contributions(te, background_frame=bg, output_per_reference=True).as_data_frame()
    cols = X_COLS + ["BiasTerm"]
    err = np.abs(got[cols].values - ref[cols].values).max()
    tol = beta_dl * (tol_dl + d_ref) + 2.0 ** -22 * np.abs(ref[cols].values).max()
    print(f"dl_shap ensemble err={err:.3e} beta_dl={beta_dl:.3e} d_ref={d_ref:.3e} tol={tol:.3e}")
    assert err <= tol
    lv = lambda f: h2o.H2OFrame.from_vecs(*se._level_one(se._base, f, use_cv=False))
    ex, ez = se._meta._predict_link(lv(te)).cpu().numpy(), se._meta._predict_link(lv(bg)).cpu().numpy()
    sums = got[X_COLS].values.sum(1).reshape(te.nrows, bg.nrows)
    np.testing.assert_allclose(sums, ex[:, None] - ez[None, :], rtol=0, atol=1e-4 * max(1.0, np.abs(ex).max()))
