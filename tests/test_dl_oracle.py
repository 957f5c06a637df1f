"""The fp64 oracle of the fused MLP step (tests/dl_oracle_common.py) checked
where no GPU is at hand: against the project's CPU step pieces
(use_native=False) in float32-vs-fp64 tolerance, and the conditions of the
GPU test that depend on the reference alone.  This is a check of the oracle,
not of the kernels."""
import pytest
import torch

from h2o3_amd.ops import dl_ops

import dl_oracle_common as oc

def _cpu_unfused(c, s):
    """One step's A, dZ, dW, db from the CPU pieces of dl_ops in float32."""
    nl = len(c.Ws)
    seed = c.seeds[s]
    idx = c.idxs[s]
    a = c.X.index_select(0, idx)
    a = a * dl_ops.keep_mask((seed + 0x5bd1e995) & ((1 << 64) - 1), c.B, a.shape[1], c.in_drop, "cpu")
    A, Z = [a], []
    for l in range(nl - 1):
        z = A[l] @ c.Ws[l].t()
        A.append(dl_ops.fwd(z, c.bs[l], c.acts[l], c.drops[l], seed=seed + 7919 * (l + 1), train=True,
                            use_native=False))
        Z.append(z)
    zo = A[-1] @ c.Ws[-1].t()
    ww = None if c.w is None else c.w.index_select(0, idx)
    _, dz, _ = dl_ops.softmax(zo, c.bs[-1], c.y.index_select(0, idx), ww, c.inv_n,
                              loss="quadratic" if c.out_kind == 1 else "crossentropy", use_native=False)
    dZ, dW, db = [None] * nl, [None] * nl, [None] * nl
    dZ[-1], db[-1] = dz, dz.sum(0)
    for l in range(nl - 1, -1, -1):
        dW[l] = dZ[l].t() @ A[l]
        if l > 0:
            dA = dZ[l] @ c.Ws[l]
            dZ[l - 1], db[l - 1] = dl_ops.bwd(dA, A[l], Z[l - 1], c.acts[l - 1], c.drops[l - 1],
                                              seed=seed + 7919 * l, use_native=False)
    return dict(A=A, dZ=dZ, dW=dW, db=db)


@pytest.mark.parametrize("name", ["ragged_tanh", "eight_layers"])
def test_oracle_grads_match_cpu_unfused(name):
    c = oc.make_case(name)
    for s in range(oc.STEPS):
        got = _cpu_unfused(c, s)
        relu_on = [got["A"][l + 1] > 0 if act == "rectifier" else None for l, act in enumerate(c.acts)]
        ref = oc.oracle_grads(c.Ws, c.bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind,
                              c.inv_n, c.seeds[s], relu_on=relu_on)
        assert ref.fragile <= oc.FRAGILE_CAP * max(ref.nrelu, 1)
        r32 = oc.oracle_grads(c.Ws, c.bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind,
                              c.inv_n, c.seeds[s], dtype=torch.float32, on_fixed=ref.on)
        # the tolerance of the GPU test: float32 sums in another order than the yardstick's
        for q, (ek, e32) in oc.grad_errors(got, ref, r32).items():
            assert ek <= oc.tau(e32), (s, q, ek, e32)
        # the scales are scales: the reference itself lies within them
        for q in ("A", "dZ", "dW", "db"):
            for l in range(len(c.Ws)):
                assert bool((getattr(ref, q)[l].abs() <= getattr(ref, "S_" + q)[l] * (1 + 1e-12)).all()), (q, l)


@pytest.mark.parametrize("I", oc.UPDATE_WIDTHS)
@pytest.mark.parametrize("kind", oc.UPDATE_KINDS)
def test_oracle_update_matches_cpu(kind, I):
    """oracle_update against dl_ops.update(use_native=False) on the inputs of
    the GPU update test, and that test's max_w2 margin on the reference."""
    for s, (res, (rel, above, below)) in enumerate(oc.run_update_case(oc.update_case(kind, I), "cpu",
                                                                      use_native=False)):
        assert rel > oc.MAXW2_MARGIN and above > 0 and below > 0, (s, rel, above, below)
        for k, (bad, worst) in res.items():
            assert bad == 0, (s, k, bad, worst)
        assert ("ada.g2" in res) == (kind == "adadelta") and ("mom" in res) == (kind != "adadelta")


@pytest.mark.parametrize("name", oc.CASES)
def test_reference_conditions(name):
    """What the GPU test relies on and the reference alone decides: the share
    of fragile rectifier units and the max_w2 margin with rows on both sides."""
    c = oc.make_case(name)
    assert dl_ops.mlp_fits(list(c.widths))
    for s, st in enumerate(oc.reference_run(c)):
        assert st.ref.fragile <= oc.FRAGILE_CAP * max(st.ref.nrelu, 1), (s, st.ref.fragile, st.ref.nrelu)
        if c.max_w2:
            above = below = 0
            for r2, m in st.r2s:
                rel, a, b = oc.maxw2_margin(r2, m)
                assert rel > oc.MAXW2_MARGIN, (s, rel)
                above, below = above + a, below + b
            assert above > 0 and below > 0, (s, above, below)
