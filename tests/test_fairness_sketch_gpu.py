"""ops/csrc/fairness.hip grouped score sketch against its definition in torch
(fairness_ops.group_sketch_torch) on the same device tensors.

The counts are integers, so `cnt` and `cm` must be equal; the two f64 loss
sums are atomic sums in arrival order and are compared with the tolerance
tests/test_logit_hist_gpu.py uses for the same kind of sum."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 1 << 10


def _inputs(n, G, kind="random", dtype=torch.float64, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "constant":
        p = torch.full((n,), 0.31, dtype=torch.float64, device="cuda")
    elif kind == "few":
        p = torch.sigmoid(torch.randint(-3, 4, (n,), generator=g, device="cuda").double())
    else:
        p = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    y = (torch.rand(n, generator=g, device="cuda") < 0.3).to(torch.int32)
    grp = torch.randint(0, G, (n,), generator=g, device="cuda", dtype=torch.int32)
    return p.to(dtype), y, grp


def _check(res, ref, chunks=None):
    cnt, cm, sums = ref
    assert res.kernel is True and res.why is None
    assert res.cnt.dtype == torch.int64 and res.cm.dtype == torch.int64
    assert torch.equal(res.cnt, cnt)
    assert torch.equal(res.cm, cm)
    torch.testing.assert_close(res.sums, sums, rtol=1e-10, atol=1e-9)
    if chunks is not None:
        assert res.chunks == chunks


def test_constant_score_one_group():
    """Maximal contention: one key per class."""
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(70_001, 1, "constant")
    res = fo.group_sketch(p, y, g, 1, 0.25, nb=NB)
    _check(res, fo.group_sketch_torch(p, y, g, 1, 0.25, nb=NB), chunks=1)
    assert int(res.cnt.sum()) == 70_001 and int((res.cnt > 0).sum()) == 2
    assert res.cm[0].tolist() == [int((y == 1).sum()), int((y == 0).sum()), 0, 0]


def test_few_scores_three_groups():
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(70_001, 3, "few")
    assert torch.unique(p).numel() == 7
    res = fo.group_sketch(p, y, g, 3, 0.5, nb=1 << 18)
    _check(res, fo.group_sketch_torch(p, y, g, 3, 0.5, nb=1 << 18))
    assert int(res.cm.sum()) == 70_001


@pytest.mark.parametrize("extra", [0, 1])
def test_many_groups_both_sides_of_the_lds_switch(extra):
    from h2o3_amd.ops import fairness_ops as fo
    G = fo.LDS_GROUPS + extra
    p, y, g = _inputs(50_000, G, "random")
    g[:G] = torch.arange(G, dtype=torch.int32, device="cuda")          # every group occupied, the last one too
    res = fo.group_sketch(p, y, g, G, 0.4, nb=NB)
    _check(res, fo.group_sketch_torch(p, y, g, G, 0.4, nb=NB), chunks=1)
    assert int((res.cm.sum(1) > 0).sum()) == G


def test_grid_stride_with_three_blocks():
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(5_000, 4, "random")
    res = fo.group_sketch(p, y, g, 4, 0.6, nb=NB, max_blocks=3)
    _check(res, fo.group_sketch_torch(p, y, g, 4, 0.6, nb=NB))
    assert int(res.cm.sum()) == 5_000


def test_row_filter_and_guard_buffers():
    """NaN scores, NA and foreign response codes, NA and out-of-range groups
    are skipped, and nothing is written around the three outputs."""
    from h2o3_amd.ops import fairness_ops as fo
    n, G, pad = 20_011, 5, 4096
    p, y, g = _inputs(n, G, "random")
    p[::97] = float("nan")
    y[::101] = -1
    y[::103] = 2
    g[::89] = -1
    g[::83] = G + 3
    i = torch.arange(n, device="cuda")
    keep = (i % 97 != 0) & (i % 101 != 0) & (i % 103 != 0) & (i % 89 != 0) & (i % 83 != 0)
    ref = fo.group_sketch_torch(p[keep], y[keep], g[keep], G, 0.5, nb=NB)
    assert int(ref[1].sum()) == int(keep.sum()) < n
    # the oracle's own filter gives the same on all rows
    own = fo.group_sketch_torch(p, y, g, G, 0.5, nb=NB)
    assert torch.equal(ref[0], own[0]) and torch.equal(ref[1], own[1])
    torch.testing.assert_close(ref[2], own[2], rtol=1e-10, atol=1e-9)     # torch's own f64 atomics reorder too
    # one allocation: guard | cnt | guard | cm | guard | sums | guard (8-byte cells)
    sizes = [G * 2 * NB, G * 4, G * 2]
    buf = torch.zeros(sum(sizes) + 4 * pad, dtype=torch.int64, device="cuda")
    offs = [pad, 2 * pad + sizes[0], 3 * pad + sizes[0] + sizes[1]]
    views = [buf[offs[0]:offs[0] + sizes[0]].view(G, 2, NB), buf[offs[1]:offs[1] + sizes[1]].view(G, 4),
             buf[offs[2]:offs[2] + sizes[2]].view(torch.float64).view(G, 2)]
    res = fo.group_sketch(p, y, g, G, 0.5, nb=NB, out=tuple(views))
    assert res.cnt.data_ptr() == views[0].data_ptr() and res.sums.data_ptr() == views[2].data_ptr()
    _check(res, ref)
    guard = torch.ones_like(buf, dtype=torch.bool)
    for o, s in zip(offs, sizes):
        guard[o:o + s] = False
    assert int(guard.sum()) == 4 * pad and not bool(buf[guard].any())


def test_flip_and_the_row_on_the_threshold():
    from h2o3_amd.ops import fairness_ops as fo
    n, G = 30_001, 3
    p, y, g = _inputs(n, G, "random")
    thr = 0.4375
    p[7], y[7], g[7] = thr, 1, 2
    plain = fo.group_sketch(p, y, g, G, thr, nb=NB)
    flipped = fo.group_sketch(p, y, g, G, thr, flip=True, nb=NB)
    _check(plain, fo.group_sketch_torch(p, y, g, G, thr, nb=NB))
    _check(flipped, fo.group_sketch_torch(p, y, g, G, thr, flip=True, nb=NB))
    # flipping swaps the classes and the selection: tp <-> tn, fp <-> fn
    assert torch.equal(flipped.cm, plain.cm[:, [2, 3, 0, 1]])
    # the row with p1 == thr and y = 1: selected as it stands (a tp of group 2); flipped it is y' = 0 and not
    # selected (a tn)
    p2 = p.clone()
    p2[7] = float("nan")
    without = fo.group_sketch(p2, y, g, G, thr, nb=NB)
    without_f = fo.group_sketch(p2, y, g, G, thr, flip=True, nb=NB)
    assert (plain.cm - without.cm).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]]
    assert (flipped.cm - without_f.cm).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("flip", [False, True])
def test_score_dtypes(dtype, flip):
    """f32 scores are read as they are and widened in the kernel."""
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(40_003, 6, "random", dtype=dtype)
    thr = float(p[11])                                                  # a threshold some row sits on, in either dtype
    res = fo.group_sketch(p, y.to(torch.int64), g.to(torch.int64), 6, thr, flip=flip, nb=1 << 18)
    _check(res, fo.group_sketch_torch(p, y, g, 6, thr, flip=flip, nb=1 << 18))


def test_chunked_launches_equal_one_launch():
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(30_000, 5, "random")
    one = fo.group_sketch(p, y, g, 5, 0.5, nb=NB)
    two = fo.group_sketch(p, y, g, 5, 0.5, nb=NB, max_bytes=3 * 2 * NB * 8)   # 3 groups per launch
    assert one.chunks == 1 and two.chunks == 2
    assert torch.equal(one.cnt, two.cnt) and torch.equal(one.cm, two.cm)
    torch.testing.assert_close(one.sums, two.sums, rtol=1e-10, atol=1e-9)
    _check(two, fo.group_sketch_torch(p, y, g, 5, 0.5, nb=NB))


def test_counts_that_do_not_fit_the_device_are_a_value_error(monkeypatch):
    """max_bytes bounds a launch, not the allocation of cnt."""
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = _inputs(1_000, 5, "random")
    real = torch.zeros

    def zeros(shape, **kw):                 # the allocator refuses the counts, as it does past the free memory
        if isinstance(shape, tuple) and shape == (5, 2, 1 << 18):
            raise torch.cuda.OutOfMemoryError("HIP out of memory")
        return real(shape, **kw)
    monkeypatch.setattr(fo.torch, "zeros", zeros)
    with pytest.raises(ValueError, match=r"G = 5 groups .* need %d bytes" % (5 * 2 * (1 << 18) * 8)):
        fo.group_sketch(p, y, g, 5, 0.5, max_bytes=1 << 20)
    monkeypatch.undo()
    assert fo.group_sketch(p, y, g, 5, 0.5, max_bytes=1 << 20).chunks == 5


def test_cpu_tensors_take_the_torch_path():
    from h2o3_amd.ops import fairness_ops as fo
    p, y, g = (t.cpu() for t in _inputs(1_000, 2, "random"))
    res = fo.group_sketch(p, y, g, 2, 0.5, nb=NB)
    assert res.kernel is False and res.why == "CPU tensors" and int(res.cm.sum()) == 1_000
