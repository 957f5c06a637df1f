"""The histogram oracle of hist_common.py checked on the CPU: against a
triple-loop sum, against the torch path the project already relies on, and --
for every case the GPU test runs -- against a numpy emulation of a correct
fixed-point kernel, which must land inside the derived bound (and be equal
where the case claims equality).  The last one is the proof that the inputs
and the bound are fair to a correct kernel."""
import numpy as np
import pytest
import torch

import hist_common as hc
from h2o3_amd.ops import tree_ops


def _tiny(mode, weights, nan, posv, seed=0):
    rng = np.random.default_rng(seed)
    n, F, Bs = 60, 3, 5
    codes = rng.integers(0, Bs, (n, F))
    ridx = rng.permutation(n).astype(np.int32)
    va = rng.standard_normal(n).astype(np.float32)
    vb = rng.random(n).astype(np.float32) if (weights or mode == 1) else None
    if vb is not None and mode != 1:
        vb[rng.random(n) < 0.2] = 0.0
    if nan:
        va[rng.random(n) < 0.2] = np.nan
    return codes, ridx, va, vb, [0, 7, 7, 30], [7, 0, 23, 30], Bs


@pytest.mark.parametrize("posv", [False, True])
@pytest.mark.parametrize("mode,weights,nan", [(0, False, False), (0, False, True), (0, True, False), (1, True, False),
                                              (2, True, False), (2, False, False)])
def test_oracle_matches_brute_force(mode, weights, nan, posv):
    codes, ridx, va, vb, starts, counts, Bs = _tiny(mode, weights, nan, posv)
    orc = hc.hist_oracle(codes, ridx, va, vb, mode, starts, counts, Bs, posv)
    F, C = codes.shape[1], hc.channels(mode)
    H = np.zeros((F, len(starts), Bs, C))
    wyy = np.zeros(len(starts))
    for s, (st, ct) in enumerate(zip(starts, counts)):
        for p in range(st, st + ct):
            r = int(ridx[p])
            i = p if posv else r
            a = float(va[i])
            b = None if vb is None else float(vb[i])
            if mode == 0:
                w = b if b is not None else (0.0 if a != a else 1.0)
                if w == 0.0:
                    continue
                v = (w, w * a)
                wyy[s] += w * a * a
            elif mode == 1:
                v = (a, b)
            else:
                v = (1.0 if b is None else b,)
            for f in range(F):
                for c in range(C):
                    H[f, s, codes[r, f], c] += v[c]
    assert np.allclose(orc.H, H, rtol=1e-13, atol=1e-13)
    assert np.allclose(orc.wyy, wyy, rtol=1e-13, atol=1e-13)
    assert np.all(orc.N >= 0) and np.all(orc.A >= np.abs(orc.H) - 1e-12)


@pytest.mark.parametrize("posv", [False, True])
@pytest.mark.parametrize("mode,weights", [(0, False), (0, True), (1, True), (2, True), (2, False)])
def test_oracle_matches_torch_path(mode, weights, posv):
    rng = np.random.default_rng(3)
    n, F, Bs = 700, 6, 9
    codes = rng.integers(0, Bs, (n, F))
    ridx = rng.permutation(n).astype(np.int32)
    va = rng.standard_normal(n).astype(np.float32)
    vb = rng.random(n).astype(np.float32) if weights else None
    starts, counts = [0, 1, 300], [1, 299, 400]
    bd = hc.make_bd(codes, Bs, 1)
    t = torch.from_numpy
    out = tree_ops.hist_build(bd, t(ridx), t(va), None if vb is None else t(vb), mode, starts, counts, 3,
                              use_native=False, want_wyy=True, posv=posv)
    orc = hc.hist_oracle(codes, ridx, va, vb, mode, starts, counts, Bs, posv)
    # the torch path forms w*y in fp32: one fp32 rounding per term
    tol = 2.0 ** -23 * orc.A + 1e-12
    assert np.all(np.abs(out[0].numpy() - orc.H) <= tol)
    if mode == 0:
        assert np.allclose(out[1].numpy(), orc.wyy, rtol=1e-12)


@pytest.mark.parametrize("layout", sorted(hc.LAYOUTS))
def test_plan_of_every_case(monkeypatch, layout):
    names = [n for n, c in hc.CASES.items() if c[0] == layout]
    assert names
    for name in names:
        case = hc.build(name)
        hc.set_env(monkeypatch, case.env)
        plan = hc.plan_of(case)
        assert (plan.kernel, plan.width, plan.pack) == case.expect, name
        assert plan.chunk == hc.CHUNK, name
        assert hc.padded_width(case.F, case.code_bytes) >= plan.n_fg * plan.width or plan.kernel in ("pk", "flat")


@pytest.mark.parametrize("layout", sorted(hc.LAYOUTS))
def test_every_gpu_case_is_satisfiable(monkeypatch, layout):
    seen = set()
    for name, c in hc.CASES.items():
        # the launch switches change neither the inputs' kind nor the scales: one emulation per payload
        key = c[:4] + (c[6],)
        if c[0] != layout or key in seen:
            continue
        seen.add(key)
        case = hc.build(name)
        hc.set_env(monkeypatch, case.env)
        plan = hc.plan_of(case)
        orc, bnd, exact, _ = hc.expected(name)
        s0, s1, bq = plan.scales(case.vmax)
        sf = hc.s_floor(case.vmax, plan.chunk, plan.pack)
        assert s0 >= sf[0] or plan.pack, name
        assert s1 >= sf[1] or case.mode == 2, name
        H = hc.emulate(case, plan)
        err = np.abs(H - orc.H)
        assert np.all(err <= bnd), (name, float((err - bnd).max()))
        for ch, ex in enumerate(exact):
            if ex:
                assert np.array_equal(H[..., ch], orc.H[..., ch]), (name, ch)


@pytest.mark.parametrize("name", [n for n in hc.EDGE_CASES if n.endswith("-row")])
def test_edge_cases_sit_on_the_reduce_edge(monkeypatch, name):
    """Two work items of one node, every row in one bin at the channel maximum: each item sums to at
    most 2^62, the node to 2^63 or more -- past int64."""
    case = hc.build(name)
    hc.set_env(monkeypatch, case.env)
    plan = hc.plan_of(case)
    _, stats = hc.emulate(case, plan, want_items=True)
    assert all(st[0] <= 2 ** 62 for st in stats)
    assert stats[0][1] >= 2 ** 63


@pytest.mark.parametrize("name", [n for n in hc.PACK_MAX_CASES if hc.CASES[n][2] == "none" and n.endswith("-row")])
def test_packed_field_is_filled(monkeypatch, name):
    case = hc.build(name)
    hc.set_env(monkeypatch, case.env)
    plan = hc.plan_of(case)
    _, _, bq = plan.scales(case.vmax)
    assert plan.chunk * (2 * bq + 1) < 2 ** 40
    _, stats = hc.emulate(case, plan, want_items=True)
    assert stats[1][0] >= 2 ** 39
