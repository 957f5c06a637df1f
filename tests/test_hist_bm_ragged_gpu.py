"""Ragged last feature group of hist_bm_kernel (dense lanes, H2O3_HIST_BM_RAGGED)
vs the full-width mapping (bit for bit) and the fp64 torch reference."""
import functools

import numpy as np
import pytest
import torch

from test_tree_kernels_gpu import _binned, _need_gpu

pytestmark = pytest.mark.gpu

N = 30000
# (start, count): 1, 6, 7, 8 and 13 rows are the partial waves of the 7- and
# 12-row mappings, 9000 rows span several work items (2048 rows each: the
# reduce merges the partials of one node), the last one starts at an odd position
SEGS = [(0, 1), (1, 6), (7, 7), (14, 8), (22, 13), (36, 9000), (9037, 5001)]
# F -> lanes per row of the last group: 1, 2, 6, 9, 12, 13 (full-width mapping), no tail
FS = [65, 70, 88, 100, 110, 116, 128]


@functools.lru_cache(maxsize=None)
def _bd(F):
    return _binned(n=N, F=F, nbins=255, cats=False)[0]


def _payload(F, layout):
    """(mode, pack, va, vb for the kernel, va, vb for the reference).  Every
    weight is a multiple of 1/4 in [0, 2], so the fixed-point entries of the
    count layout are small multiples of a power of two and their f64 sums are
    exact in any order: the f64-atomic flush (H2O3_HIST_BM_RED=0) is then
    reproducible bit for bit, as the packed layout's always is (integers
    below 2^40 times a power of two)."""
    g = torch.Generator(device="cuda").manual_seed(F)
    va = torch.randn(N, generator=g, device="cuda")
    if layout == "pack_vb":          # MODE 0 packed, 0/1 weight vector (30 % zero-weight rows)
        vb = (torch.rand(N, generator=g, device="cuda") < 0.7).to(torch.float32)
        return 0, True, va, vb, va, vb
    if layout == "pack_nan":         # MODE 0 packed, no weight vector: NaN response = zero-weight row
        dead = torch.rand(N, generator=g, device="cuda") < 0.1
        vk = va.clone()
        vk[dead] = float("nan")
        return 0, True, vk, None, va, (~dead).to(torch.float32)
    vb = torch.randint(0, 9, (N,), generator=g, device="cuda").to(torch.float32) / 4   # MODE 2, 1/9 zero weights
    return 2, False, va, vb, va, vb


@pytest.mark.parametrize("layout", ["pack_vb", "pack_nan", "count"])
@pytest.mark.parametrize("F", FS)
def test_hist_bm_ragged_matches_full_width_and_reference(F, layout, monkeypatch):
    _need_gpu()
    monkeypatch.setenv("H2O3_HIST_BM", "1")
    from h2o3_amd.ops import tree_ops
    bd = _bd(F)
    assert tree_ops.bm_groups(bd.F, bd.Fp, bd.Bs, True) == (2, 64)
    mode, pack, va, vb, va_ref, vb_ref = _payload(F, layout)
    ridx = torch.randperm(N, generator=torch.Generator(device="cuda").manual_seed(F + 1), device="cuda").to(torch.int32)
    starts, counts = [s for s, _ in SEGS], [c for _, c in SEGS]
    vmax = tree_ops.channel_max(va, vb, mode)
    h_ref, w_ref = tree_ops.hist_build(bd, ridx, va_ref, vb_ref, mode, starts, counts, len(SEGS), use_native=False,
                                       want_wyy=True)
    for posv in (False, True):
        if posv:    # position-ordered payloads: entry p belongs to row ridx[p]
            r = ridx.long()
            pa, pb = va[r].contiguous(), (vb[r].contiguous() if vb is not None else None)
        else:
            pa, pb = va, vb
        for red in ("1", "0"):
            monkeypatch.setenv("H2O3_HIST_BM_RED", red)
            out = {}
            for rag in ("1", "0"):
                monkeypatch.setenv("H2O3_HIST_BM_RAGGED", rag)
                out[rag] = tree_ops.hist_build(bd, ridx, pa, pb, mode, starts, counts, len(SEGS), use_native=True,
                                               unit_w=pack, vmax=vmax, posv=posv, want_wyy=True)
            (h1, w1), (h0, w0) = out["1"], out["0"]
            err = float((h1 - h_ref).abs().max())
            print(f"F={F} {layout} posv={posv} red={red}: equal={torch.equal(h1, h0)} max|h - ref|={err:.3g}")
            assert torch.equal(h1, h0)
            torch.testing.assert_close(h1, h_ref, rtol=1e-5, atol=1e-4)
            if mode == 0:
                torch.testing.assert_close(w1, w_ref, rtol=1e-5, atol=1e-3)
                torch.testing.assert_close(w0, w_ref, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("rag", ["2", "3", "4"])
def test_hist_bm_alternative_tail_mappings(rag, monkeypatch):
    """The other measured tail mappings (slot stride = lanes per row; 8 codes
    per lane; full width with the padding atomics masked) stay selectable for
    the microbenchmark: same bits as the full-width mapping."""
    _need_gpu()
    monkeypatch.setenv("H2O3_HIST_BM", "1")
    from h2o3_amd.ops import tree_ops
    starts, counts = [s for s, _ in SEGS], [c for _, c in SEGS]
    for F in (70, 100, 110):
        bd = _bd(F)
        mode, pack, va, vb, _, _ = _payload(F, "pack_nan")
        ridx = torch.randperm(N, generator=torch.Generator(device="cuda").manual_seed(F + 1),
                              device="cuda").to(torch.int32)
        vmax = tree_ops.channel_max(va, vb, mode)
        out = {}
        for r in ("0", rag):
            monkeypatch.setenv("H2O3_HIST_BM_RAGGED", r)
            out[r] = tree_ops.hist_build(bd, ridx, va, vb, mode, starts, counts, len(SEGS), use_native=True,
                                         unit_w=pack, vmax=vmax)
        assert torch.equal(out[rag], out["0"])


# root_leaf: no split leaves 15 000 rows on both sides, the root stays the only
# leaf and its rows are read back through row-id buffer 0 (depth 3: odd parity)
DT_CASES = {"depth3": (3, {}), "depth1": (1, {}), "root_leaf": (3, dict(min_rows=15000.0))}


@pytest.mark.parametrize("case", list(DT_CASES))
def test_devtree_same_forest_with_switches(case, monkeypatch):
    """Bernoulli GBM on the device-resident tree: H2O3_DEV_ROOT_IDENT (root
    kernels without row ids, no iota) and H2O3_HIST_BM_RAGGED, each 1 and 0
    (read at construction, before the graph is captured), grow identical tree
    records and predictions."""
    _need_gpu()
    from test_leaf_gather_gpu import _fit, _frame
    max_depth, kw = DT_CASES[case]
    fr, names = _frame(20_003, 100, "bernoulli", seed=31)
    res = {}
    for ident, rag in (("1", "1"), ("0", "0"), ("1", "0"), ("0", "1")):
        monkeypatch.setenv("H2O3_DEV_ROOT_IDENT", ident)
        monkeypatch.setenv("H2O3_HIST_BM_RAGGED", rag)
        drv, forest, pred = _fit(monkeypatch, fr, names, True, ntrees=3, max_depth=max_depth, **kw)
        dt = getattr(drv, "_devtree", None)
        assert dt is not None, getattr(drv, "_devtree_why", None)
        assert dt.graph is not None
        assert dt.ragged == int(rag) and (dt.n_fg, dt.G) == (2, 64)
        assert dt.root_ident == (ident == "1" and max_depth >= 2)   # depth 1: the leaf gather reads ridx[0]
        res[ident, rag] = (forest, pred)
    fa, pa = res["0", "0"]
    assert len(fa.trees) == 3
    assert max(int(np.asarray(t.depth).max()) for t in fa.trees) == (0 if case == "root_leaf" else max_depth)
    # The splits come from the histograms (integer LDS sums: no switch changes
    # a bit).  The leaf values come from f64 atomic sums per node over the
    # partition work items: at depth 3 every last-level node is ONE item, so
    # the values are reproducible bit for bit; at depth 1 the root's 20 003
    # rows are several items whose sums arrive in no fixed order, in any
    # configuration (two runs of one configuration differ in the last bit).
    # (likewise a root that stays a leaf).  There: k items reordered move a sum by <= k * 2^-53 * sum|z| <= 3 * 1.1e-16
    # * 20003 = 7e-12 against denominators sum p(1-p) ~ 5e3, times the 0.1
    # learning rate: |dvalue| < 1e-15; predictions are f32 (ulp 1.2e-7 below 1).
    exact = case == "depth3"
    for key, (fb, pb) in res.items():
        assert len(fb.trees) == 3
        for ta, tb in zip(fa.trees, fb.trees):
            for k in ("feat", "left", "right", "na_left", "thr", "weight"):
                np.testing.assert_array_equal(np.asarray(getattr(ta, k)), np.asarray(getattr(tb, k)),
                                              err_msg=f"{key} {k}")
            va, vb = np.asarray(ta.value), np.asarray(tb.value)
            print(key, "max |dvalue|", float(np.abs(va - vb).max()), "max |dpred|", float(np.abs(pa - pb).max()))
            if exact:
                np.testing.assert_array_equal(va, vb, err_msg=f"{key} value")
            else:
                np.testing.assert_allclose(va, vb, rtol=0, atol=1e-15, err_msg=f"{key} value")
        if exact:
            np.testing.assert_array_equal(pa, pb, err_msg=str(key))
        else:
            np.testing.assert_allclose(pa, pb, rtol=0, atol=1.2e-7, err_msg=str(key))
