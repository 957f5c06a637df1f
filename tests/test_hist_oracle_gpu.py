"""The histogram kernels of ops/csrc/tree_hist.hip against the exact float64
oracle of hist_common.py, entrywise within the bound derived there (equality
where every contribution is exactly representable), on constant, two-valued
and ramp code columns at the group borders, payloads at the channel maximum
and segments of one, two and five work items -- the edges of the fixed-point
scales -- and tree_ops.hist_build_dev (child_work_kernel) against a plain
loop over a hand-written split record.

What these tests found.  With the two-pass flush (H2O3_HIST_BM_RED=1, the
default) hist_bm_reduce_kernel summed the partial images of up to 32 work
items of a node in one int64.  One item may reach 2^62 (2048 rows of the
channel maximum in one bin at scale 2^51), so the 4096-row node of the +max
cases summed to 2^63, which wraps: the reduce now hands its running sum to
the f64 histogram before an add that would wrap."""
import numpy as np
import pytest
import torch

import hist_common as hc
from h2o3_amd.ops import tree_ops

pytestmark = pytest.mark.gpu


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _worst(H, ref, bnd, name):
    err = np.abs(H - ref)
    bad = ~(err <= bnd)
    ratio = float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)))
    print(f"RATIO {name} {ratio:.4f}")
    if bad.any():
        over = np.where(bad, np.where(np.isnan(err), np.inf, err - bnd), -np.inf)
        f, s, b, c = np.unravel_index(int(np.argmax(over)), H.shape)
        pytest.fail(f"{name}: {int(bad.sum())} entries outside the bound; worst (feature {f}, slot {s}, bin {b}, "
                    f"channel {c}): kernel {H[f, s, b, c]!r}, oracle {ref[f, s, b, c]!r}, bound {bnd[f, s, b, c]!r}")


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_hist_build_matches_oracle(monkeypatch, name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    case = hc.build(name)
    hc.set_env(monkeypatch, case.env)
    plan = hc.plan_of(case)
    assert (plan.kernel, plan.width, plan.pack, plan.chunk) == case.expect + (hc.CHUNK,)
    orc, bnd, exact, skipped = hc.expected(name)
    sf = hc.s_floor(case.vmax, plan.chunk, plan.pack)
    s0, s1, _ = plan.scales(case.vmax)
    assert (plan.pack or s0 >= sf[0]) and (case.mode == 2 or s1 >= sf[1])
    bd = hc.make_bd(case.codes, case.Bs, case.code_bytes, "cuda")
    S = len(case.counts)
    H, wyy = tree_ops.hist_build(bd, _cuda(case.ridx), _cuda(case.va), _cuda(case.vb), case.mode, case.starts,
                                 case.counts, S, use_native=True, vmax=list(case.vmax), want_wyy=True,
                                 posv=case.posv, unit_w=case.unit_w, need_mask=_cuda(case.need_mask))
    torch.cuda.synchronize()
    H = H.cpu().numpy()
    ref, bnd = orc.H.copy(), bnd.copy()
    for c, ex in enumerate(exact):
        if ex:
            bnd[..., c] = 0.0
    if skipped is not None:
        ref[skipped] = 0.0          # groups with no needed feature stay exactly zero
        bnd[skipped] = 0.0
    _worst(H, ref, bnd, name)
    if case.mode == 0 and skipped is None:
        w = wyy.cpu().numpy()
        tol = hc.wyy_tol(orc, case.has_w)
        assert np.all(np.abs(w - orc.wyy) <= tol), (name, w.tolist(), orc.wyy.tolist())


# --------------------------------------------------------------------------- hist_build_dev
COLS = (1, 3, 4, 5)      # ok, nleft, wl, wr of a record of stride 7


def _frame(F, Bs, n, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, Bs, (n, F))
    codes[:, 0] = 0
    codes[:, F - 1] = Bs - 1
    ridx = rng.permutation(n).astype(np.int32)
    va = rng.standard_normal(n).astype(np.float32)
    vb = rng.random(n).astype(np.float32)
    vmax = [float(vb.max()), float(np.abs((va * vb).astype(np.float64)).max())]
    return codes, ridx, va, vb, vmax


def _record(nodes):
    """nodes: (count, ok, nleft, wl, wr) -> rec [n, 7] f64, starts, counts."""
    rec = np.full((len(nodes), 7), -7.0)
    counts = [x[0] for x in nodes]
    starts = [int(v) for v in np.cumsum([0] + counts[:-1])]
    for i, (_, ok, nl, wl, wr) in enumerate(nodes):
        rec[i, list(COLS)] = (ok, nl, wl, wr)
    return rec, starts, counts


# ok = 0 nodes between splitting ones; a lighter right child of 2049 rows and a lighter left child of
# 2048; a tie of the weights (the left child builds); nleft = 0 and nleft = count: pairs without work
_NODES_EDGES = [(5000, 1, 2048, 10.0, 30.0), (100, 0, 50, 1.0, 2.0), (5000, 1, 2951, 30.0, 20.0),
                (1000, 1, 400, 5.0, 5.0), (541, 0, 0, 0.0, 0.0), (2000, 1, 0, 0.0, 9.0), (2000, 1, 2000, 9.0, 0.0),
                (3900, 1, 1, 0.5, 40.0)]


def _nodes_many():
    """1030 nodes of 3..18 rows: child_work_kernel takes a second round of its 1024-thread loop."""
    rng = np.random.default_rng(11)
    out = []
    for i in range(1030):
        ct = 3 + i % 16
        wl, wr = (1.0, 1.0) if i % 7 == 0 else (float(rng.random()), float(rng.random()))
        out.append((ct, 0 if i % 3 == 0 else 1, int(rng.integers(0, ct + 1)), wl, wr))
    return out


@pytest.mark.parametrize("kernel", ["bm", "quad"])
@pytest.mark.parametrize("which", ["edges", "many"])
def test_hist_build_dev_matches_loop_and_oracle(monkeypatch, which, kernel):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hc.set_env(monkeypatch, {} if kernel == "bm" else {"H2O3_HIST_BM": "0"})
    nodes = _NODES_EDGES if which == "edges" else _nodes_many()
    F, Bs = (37, 256) if which == "edges" else (13, 8)
    rec, starts, counts = _record(nodes)
    n_rows = int(sum(counts))
    codes, ridx, va, vb, vmax = _frame(F, Bs, n_rows, 5)
    bd = hc.make_bd(codes, Bs, 1, "cuda")
    plan = tree_ops.hist_plan(bd, 0, False, (n_rows + 1) // 2)
    assert (plan.kernel, plan.width, plan.chunk) == (kernel, 16, hc.CHUNK)
    build, der, par, items, segs = hc.child_work_expected(rec, COLS, starts, counts, plan.chunk)
    n = len(nodes)
    out = tree_ops.hist_build_dev(bd, _cuda(ridx), _cuda(va), _cuda(vb), 0, _cuda(rec), COLS, starts, counts,
                                  list(vmax))
    assert out is not None
    Hb, wyy, slots, cnts = out
    torch.cuda.synchronize()
    k = len(par)
    assert cnts.cpu().tolist() == [k, len(items)]
    sl = slots.cpu().numpy()
    assert sl[:k].tolist() == build and sl[n:n + k].tolist() == der and sl[2 * n:2 * n + k].tolist() == par
    # the work items precede the slots in the buffer hist_build_dev allocates
    work = slots._base[:4 * len(items)].cpu().numpy().reshape(-1, 4)
    assert work.tolist() == [list(x) for x in items]
    c_st = [s for s, _ in segs] + [0] * (n - k)
    c_ct = [c for _, c in segs] + [0] * (n - k)      # slots past the pairs stay zero
    orc = hc.hist_oracle(codes, ridx, va, vb, 0, c_st, c_ct, Bs, False)
    bnd = hc.bound(orc, 0, hc.s_floor(vmax, plan.chunk, False), False, True)
    _worst(Hb.cpu().numpy(), orc.H, bnd, f"hist_build_dev-{which}-{kernel}")
    assert np.all(np.abs(wyy.cpu().numpy() - orc.wyy) <= hc.wyy_tol(orc, True))
