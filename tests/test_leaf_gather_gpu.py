"""Leaf gather and the uncompacted last level of the device-resident tree.

The per-row leaf values come back in row order by a gather over the sorted
leaf segments (tree_hist.hip lg_*_kernel) instead of leaf_scatter_kernel's
random stores, and the last level is not compacted: its leaves are read
through the go-left flag words of level D-1 (leaf_flag_sums_kernel for the
sums, flag segments in the gather).  The values are copies, so the kernel
tests compare `dbuf` with torch.equal against the scatter; the device tree is
compared with the level loop of engine.py, which keeps the scatter and the
compacted last level.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RS, OK, ST, CT = 16, 10, 13, 14


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _level(h):
    return int(np.floor(np.log2(h + 1)))


def _frontier(D, early):
    """Leaves of a depth-D tree, left to right: the `early` heap nodes plus
    every level-D node that is not below one of them."""
    def below(h):
        while h > 0:
            h = (h - 1) >> 1
            if h in early:
                return True
        return False
    first = (1 << D) - 1
    leaves = list(early) + [h for h in range(first, 2 * first + 1) if not below(h)]
    return sorted(leaves, key=lambda h: (h + 1 - (1 << _level(h))) / (1 << _level(h)))


class _Case:
    """Host-built end state of one tree: `assign[row]` = index into `leaves`.
    compacted: every leaf's sorted rows, leaves left to right (the level loop /
    H2O3_DEV_LAST_LEVEL=0 layout).  uncompacted: splitting nodes of level D-1
    keep their rows ascending, children told apart by the flag bits."""

    def __init__(self, N, D, leaves, assign, seed=0):
        from h2o3_amd.models.tree import devtree
        self.N, self.D, self.nh = N, D, (1 << (D + 1)) - 1
        self.lh, _ = devtree._libs()
        dev = torch.device("cuda")
        g = np.random.default_rng(seed)
        rows = [np.nonzero(assign == k)[0].astype(np.int32) for k in range(len(leaves))]
        rec = np.zeros((self.nh, RS))
        start = 0
        for h, r in zip(leaves, rows):
            rec[h, ST], rec[h, CT] = start, r.size
            a = h
            while a > 0:
                a = (a - 1) >> 1
                if rec[a, OK] == 0:
                    rec[a, OK], rec[a, ST] = 1.0, start
                rec[a, CT] += r.size
            start += r.size
        assert start == N
        ridx_c = np.concatenate(rows) if rows else np.zeros(0, np.int32)
        ridx_u = ridx_c.copy()
        self.left = np.zeros(N, dtype=bool)          # by position in the uncompacted order
        by_heap = dict(zip(leaves, rows))
        p0 = (1 << (D - 1)) - 1
        for h in range(p0, 2 * p0 + 1):
            if rec[h, OK] > 0:
                s, c = int(rec[h, ST]), int(rec[h, CT])
                u = np.sort(ridx_c[s:s + c])
                ridx_u[s:s + c] = u
                self.left[s:s + c] = np.isin(u, by_heap[2 * h + 1])
        self.rec_h = rec
        self.rec = torch.from_numpy(rec.reshape(-1).copy()).to(dev)
        self.ridx_c = torch.from_numpy(ridx_c).to(dev)
        self.ridx_u = torch.from_numpy(ridx_u).to(dev)
        self.vals = torch.from_numpy(g.standard_normal(self.nh).astype(np.float32)).to(dev)
        self.leaves, self.rows, self.assign = leaves, rows, assign
        # flag words of level D-1 exactly as the device tree lays them out
        n = 1 << (D - 1)
        self.chunk_p = 4096
        self.cap_p = (1 << D) + N // self.chunk_p + 1
        self.pwork = torch.zeros(self.cap_p * 4, dtype=torch.int32, device=dev)
        self.fbase = torch.zeros(self.cap_p, dtype=torch.int32, device=dev)
        self.slot_wb = torch.zeros(n, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)
        P = devtree._ptr
        devtree._ck(self.lh.h2o_dt_items2(0, P(self.rec[p0 * RS:]), n, D, 0, self.chunk_p, self.cap_p, P(self.pwork),
                                          P(self.fbase), P(self.slot_wb), P(self.counts), devtree._stream()),
                    "dt_items2")
        wb = self.slot_wb.cpu().numpy()
        fl = np.zeros(N // 64 + self.cap_p + 1, dtype=np.uint64)
        for i in range(n):
            s, c = int(rec[p0 + i, ST]), int(rec[p0 + i, CT])
            if c > 0:
                bits = np.zeros(-(-c // 64) * 64, dtype=np.uint8)
                bits[:c] = self.left[s:s + c]
                fl[wb[i]:wb[i] + bits.size // 64] = np.packbits(bits, bitorder="little").view(np.uint64)
        self.flags = torch.from_numpy(fl.view(np.int64)).to(dev)

    def scatter(self):
        """dbuf of leaf_scatter_kernel on the compacted layout (pre-filled with
        a marker so rows nobody writes would show)."""
        from h2o3_amd.models.tree import devtree
        P, s = devtree._ptr, devtree._stream()
        cap_l = self.nh + self.N // 65536 + 1
        lwork = torch.zeros(cap_l * 4, dtype=torch.int32, device="cuda")
        d = torch.full((self.N,), -7.0, dtype=torch.float32, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        devtree._ck(self.lh.h2o_dt_items(2, P(self.rec), self.nh, self.D, 0, 65536, cap_l, P(lwork), None,
                                         P(counts), s), "dt_items")
        devtree._ck(self.lh.h2o_leaf_scatter_dev(P(self.ridx_c), P(lwork), cap_l, P(self.vals), P(d), P(counts), s),
                    "leaf_scatter_dev")
        return d

    def gather(self, last, R=None):
        from h2o3_amd.models.tree import devtree
        lg = devtree.LeafGather(self.lh, self.N, self.D, torch.device("cuda"), R=R)
        d = torch.full((self.N,), -7.0, dtype=torch.float32, device="cuda")
        if last:
            lg.run(self.rec, self.ridx_u, self.vals, d, self.flags, self.slot_wb)
        else:
            lg.run(self.rec, self.ridx_c, self.vals, d)
        torch.cuda.synchronize()
        return d

    def check(self, R=None):
        ref = self.scatter()
        host = np.empty(self.N, dtype=np.float32)
        v = self.vals.cpu().numpy()
        for h, r in zip(self.leaves, self.rows):
            host[r] = v[h]
        assert np.array_equal(ref.cpu().numpy(), host)
        assert torch.equal(self.gather(False, R), ref)
        assert torch.equal(self.gather(True, R), ref)


def _rows_per_block():
    from h2o3_amd.models.tree import devtree
    return devtree.gather_rows(1)


@pytest.mark.parametrize("n", ["1", "R", "R+1", "100003"])
def test_gather_sizes(n):
    _need_gpu()
    R = _rows_per_block()
    N = {"1": 1, "R": R, "R+1": R + 1, "100003": 100_003}[n]
    leaves = _frontier(3, [3])
    g = np.random.default_rng(N)
    _Case(N, 3, leaves, g.integers(0, len(leaves), N)).check()


def test_gather_256_leaves_skewed_empty_and_one_block():
    """One leaf holds 90 % of the rows, leaves 3..9 are empty, and leaf 20's
    rows all lie inside the second row block."""
    _need_gpu()
    R = _rows_per_block()
    N, D = 100_003, 8
    assert N > 2 * R
    leaves = _frontier(D, [])
    g = np.random.default_rng(1)
    others = np.array([k for k in range(256) if k not in (100, 20) and not 3 <= k <= 9])
    assign = np.where(g.random(N) < 0.9, 100, g.choice(others, N))
    assign[R + 11:R + 61] = 20
    cs = _Case(N, D, leaves, assign)
    assert cs.rows[100].size > 0.85 * N and all(cs.rows[k].size == 0 for k in range(3, 10))
    assert cs.rows[20].size == 50
    cs.check()


def test_gather_depth11_sparse_blocks():
    """2048 leaves on 50 000 rows: most row blocks miss most leaves."""
    _need_gpu()
    N, D = 50_000, 11
    leaves = _frontier(D, [])
    g = np.random.default_rng(2)
    # contiguous-ish leaves (rows of a leaf cluster in one block) + a random part
    assign = np.where(g.random(N) < 0.7, (np.arange(N) * 2048) // N, g.integers(0, 2048, N))
    _Case(N, D, leaves, assign).check()
    _Case(N, D, leaves, assign).check(R=1024)


def test_gather_early_leaves_and_flag_segments():
    """Early leaves at levels 1, 2 and 3 next to flag segments of level D-1
    whose counts are not multiples of 64; one flag segment all left, one all
    right."""
    _need_gpu()
    N, D = 100_003, 5
    leaves = _frontier(D, [1, 5, 13])
    assert [_level(h) for h in leaves[:3]] == [1, 2, 3] and len(leaves) == 7
    g = np.random.default_rng(3)
    assign = g.choice(7, N, p=[0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1])
    cs = _Case(N, D, leaves, assign)
    assert any(int(cs.rec_h[h, CT]) % 64 for h in (29, 30))
    cs.check()
    # node 29: every row goes left; node 30: every row goes right
    assign2 = assign.copy()
    assign2[assign2 == 4] = 3
    assign2[assign2 == 5] = 6
    cs = _Case(N, D, leaves, assign2)
    assert cs.rows[4].size == 0 and cs.rows[5].size == 0 and cs.rows[3].size % 64 and cs.rows[6].size % 64
    cs.check()
    cs.check(R=256)


@pytest.mark.parametrize("mode", [0, 1])
def test_last_level_sums(mode):
    """Sums of the level-D leaves from the level-(D-1) payload and the flag
    words against an f64 host sum of the same payload and flags:
    |s - ref| <= n 2^-52 sum|z| per leaf (n-term f64 sum); NaN rows carry no
    weight.  A non-splitting slot of level D-1 contributes nothing."""
    _need_gpu()
    from h2o3_amd.models.tree import devtree
    N, D = 100_003, 5
    leaves = _frontier(D, [3, 20])          # 20: a leaf of level D-1 inside the partition's item list
    g = np.random.default_rng(4 + mode)
    assign = g.integers(0, len(leaves), N)
    cs = _Case(N, D, leaves, assign)
    z = (g.random(N) * 1.98 - 0.99).astype(np.float32)
    z[g.random(N) < 0.05] = np.nan
    zp = torch.from_numpy(z).cuda()
    sums = torch.zeros(cs.nh * 2, dtype=torch.float64, device="cuda")
    P = devtree._ptr
    p0 = (1 << (D - 1)) - 1
    devtree._ck(cs.lh.h2o_leaf_flag_sums_dev(P(zp), P(cs.pwork), P(cs.fbase), cs.cap_p, P(cs.flags),
                                             P(cs.rec[p0 * RS:]), D, mode, P(sums), P(cs.counts),
                                             devtree._stream()), "leaf_flag_sums_dev")
    got = sums.cpu().numpy().reshape(cs.nh, 2)
    ref = np.zeros((cs.nh, 2))
    bound = np.zeros(cs.nh)
    zd = z.astype(np.float64)
    for h in range(p0, 2 * p0 + 1):
        if cs.rec_h[h, OK] > 0:
            s, c = int(cs.rec_h[h, ST]), int(cs.rec_h[h, CT])
            for child, sel in ((2 * h + 1, cs.left[s:s + c]), (2 * h + 2, ~cs.left[s:s + c])):
                zz = zd[s:s + c][sel]
                zz = zz[~np.isnan(zz)]
                az = np.abs(zz)
                ref[child] = [zz.sum(), (az * (1.0 - az)).sum() if mode == 1 else zz.size]
                bound[child] = zz.size * 2.0 ** -52 * az.sum()
    assert np.count_nonzero(ref[:, 1]) >= 8
    err = np.abs(got - ref).max(axis=1)
    print("max err / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


# ------------------------------------------------------------ device tree
def _frame(n, F, family, seed=0, na=0.0, steps=False):
    import h2o3_amd
    from h2o3_amd.core.frame import H2OFrame
    h2o3_amd.init(verbose=False)
    g = np.random.default_rng(seed)
    X = g.standard_normal((n, F)).astype(np.float32)
    if na:
        X[g.random((n, F)) < na] = np.nan
    Xz = np.nan_to_num(X)
    if steps:
        # a small group (x0 > 1, ~16 %) split off at the root, two balanced
        # splits below the rest
        eta = np.where(Xz[:, 0] > 1.0, 3.0, 1.0 * np.sign(Xz[:, 1]) + 0.6 * np.sign(Xz[:, 2]) - 2.0)
    else:
        eta = Xz[:, 0] - 0.7 * Xz[:, 1] + 0.5 * np.sin(2 * Xz[:, 2]) * Xz[:, 3]
    cols = {f"x{j}": X[:, j] for j in range(F)}
    if family == "bernoulli":
        cols["y"] = (g.random(n) < 1 / (1 + np.exp(-eta))).astype(int)
    else:
        cols["y"] = eta + 0.3 * g.standard_normal(n)
    fr = H2OFrame(cols)
    if family == "bernoulli":
        fr["y"] = fr["y"].asfactor()
    return fr, [f"x{j}" for j in range(F)]


def _fit(monkeypatch, fr, names, dev_tree, ntrees=5, gather="1", last="1", **kw):
    from h2o3_amd.models.base import TrainSpec
    from h2o3_amd.models.tree.gbm import GBMDriver, H2OGradientBoostingEstimator
    monkeypatch.setenv("H2O3_DEV_TREE", "1" if dev_tree else "0")
    monkeypatch.setenv("H2O3_LEAF_GATHER", gather)
    monkeypatch.setenv("H2O3_DEV_LAST_LEVEL", last)
    est = H2OGradientBoostingEstimator(ntrees=ntrees, seed=7, ignore_const_cols=False, histogram_type="QuantilesGlobal",
                                       nbins=255, **kw)
    spec = TrainSpec(fr, names, "y")
    est._spec = spec
    drv = GBMDriver(est, spec)
    for _ in range(ntrees):
        drv.step()
    return drv, drv.forest, drv.predictions().detach().cpu().numpy()


def _same_trees(fa, fb):
    assert len(fa.trees) == len(fb.trees)
    for ta, tb in zip(fa.trees, fb.trees):
        assert ta.n_nodes == tb.n_nodes
        np.testing.assert_array_equal(np.asarray(ta.feat), np.asarray(tb.feat))
        np.testing.assert_array_equal(np.asarray(ta.left), np.asarray(tb.left))
        np.testing.assert_array_equal(np.asarray(ta.right), np.asarray(tb.right))
        np.testing.assert_array_equal(np.asarray(ta.na_left), np.asarray(tb.na_left))
        np.testing.assert_allclose(np.asarray(ta.thr), np.asarray(tb.thr))
        np.testing.assert_allclose(np.asarray(ta.value), np.asarray(tb.value), rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(np.asarray(ta.weight), np.asarray(tb.weight), rtol=1e-9)


CASES = {
    "depth1": ("bernoulli", dict(max_depth=1), {}),
    "early_leaf": ("bernoulli", dict(max_depth=3, min_rows=20000.0), dict(steps=True)),
    "na": ("bernoulli", dict(max_depth=5), dict(na=0.03)),
    "sample_rate": ("bernoulli", dict(max_depth=5, sample_rate=0.8), {}),
    "gaussian": ("gaussian", dict(max_depth=4), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_devtree_gather_matches_level_loop(monkeypatch, case):
    _need_gpu()
    family, kw, fkw = CASES[case]
    fr, names = _frame(200_000, 16, family, seed=21, **fkw)
    d1, f1, p1 = _fit(monkeypatch, fr, names, True, **kw)
    dt = getattr(d1, "_devtree", None)
    assert dt is not None, getattr(d1, "_devtree_why", None)
    assert dt.gather and dt.last_level
    if family == "bernoulli":
        assert dt.graph is not None
    d0, f0, p0 = _fit(monkeypatch, fr, names, False, **kw)
    assert getattr(d0, "_devtree", None) is None
    if case == "early_leaf":
        # one level-1 node is a leaf while its sibling splits down to the last level
        t = f1.trees[0]
        dl = np.asarray(t.depth)[np.asarray(t.left) < 0]
        assert dl.min() == 1 and dl.max() == 3
    _same_trees(f1, f0)
    np.testing.assert_allclose(p1, p0, rtol=1e-5, atol=1e-6)


def test_switches_off_same_forest(monkeypatch):
    """H2O3_LEAF_GATHER=0 H2O3_DEV_LAST_LEVEL=0 (scatter, compacted last level)
    grows the forest of the default path."""
    _need_gpu()
    fr, names = _frame(200_000, 16, "bernoulli", seed=22)
    d1, f1, p1 = _fit(monkeypatch, fr, names, True, max_depth=5)
    d0, f0, p0 = _fit(monkeypatch, fr, names, True, gather="0", last="0", max_depth=5)
    assert d1._devtree.gather and d1._devtree.last_level
    assert not d0._devtree.gather and not d0._devtree.last_level
    _same_trees(f1, f0)
    np.testing.assert_allclose(p1, p0, rtol=1e-5, atol=1e-6)
