"""The fused MLP training step (dl.hip dl_mlp_fb_kernel / dl_mlp_dw_kernel /
dl_mlp_upd_kernel through dl_ops.mlp_step) and the unfused per-row update
(dl_update_kernel through dl_ops.update) against the fp64 oracle of
tests/dl_oracle_common.py.

Each fused case runs two consecutive steps; after each one
 (a) the step's raw A, dZ, dW, db (left in `bufs`) are compared entry by
     entry with oracle_grads on the weights before the step:
     |delta| <= tau * S, tau = min(TAU_M * e32, 2^-13) (see dl_oracle_common.TAU_M);
 (b) the weights, biases and optimiser state after the step are compared
     with oracle_update fed the kernel's own dW / db, so the optimiser is
     judged apart from the gradient, at a relative tolerance with no fixed
     absolute floor.
"""
import pytest
import torch

from h2o3_amd.ops import _native, dl_ops

import dl_oracle_common as oc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", oc.CASES)
def test_fused_step_matches_fp64_oracle(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = oc.make_case(name)
    assert dl_ops.mlp_fits(list(c.widths))
    steps = oc.run_fused_case(c)
    assert "libdl.so" in " ".join(_native.loaded_libs())
    nl = len(c.Ws)
    for s, st in enumerate(steps):
        ref = st.ref
        # fragile rectifier units: few enough that adopting the kernel's side of zero hides nothing
        assert ref.fragile <= oc.FRAGILE_CAP * max(ref.nrelu, 1), (s, ref.fragile, ref.nrelu)
        # dropout masks, apart from the arithmetic: A is zero exactly where the hash drops the unit
        for l, act in enumerate(c.acts):
            if act in ("tanh", "exprectifier"):
                assert torch.equal(st.got["A"][l + 1] == 0, ~ref.keep[l]), (s, l)
        if c.seed_dev0 is not None:
            assert st.sd_after == st.sd_expected, (s, st.sd_after, st.sd_expected)
        # (a) gradients
        errs = oc.grad_errors(st.got, ref, st.r32)
        for q, (ek, e32) in errs.items():
            print(f"RHO {name} step{s} {q}: err={ek:.3e} e32={e32:.3e} rho={ek / e32:.3f}")
        for q, (ek, e32) in errs.items():
            assert ek <= oc.tau(e32) <= oc.TAU_CAP, (s, q, ek, e32, ek / e32)
        # (b) update, from the kernel's own gradients
        above = below = 0
        for l in range(nl):
            p = c.ups[s][l]
            res, r2 = oc.check_update(st.after[l], st.snap[l], st.got["dW"][l], st.got["db"][l], p)
            if c.max_w2:
                rel, a, b = oc.maxw2_margin(r2, p.max_w2)
                assert rel > oc.MAXW2_MARGIN, (s, l, rel)
                above, below = above + a, below + b
            for k, (bad, worst) in res.items():
                print(f"UPD {name} step{s} layer{l} {k}: bad={bad} worst={worst:.3f} of the bound")
                assert bad == 0, (s, l, k, bad, worst)
            assert ("ada.g2" in res) == bool(p.ada) and ("mom" in res) == (not p.ada and p.has_momenta)
        if c.max_w2:
            assert above > 0 and below > 0, (s, above, below)


@pytest.mark.parametrize("I", oc.UPDATE_WIDTHS)
@pytest.mark.parametrize("kind", oc.UPDATE_KINDS)
def test_update_kernel_matches_fp64_oracle(kind, I):
    """dl_update_kernel (U = 300): three steps, W, b and the optimiser state
    compared with oracle_update after each one."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for s, (res, (rel, above, below)) in enumerate(oc.run_update_case(oc.update_case(kind, I), "cuda")):
        assert rel > oc.MAXW2_MARGIN and above > 0 and below > 0, (s, rel, above, below)
        for k, (bad, worst) in res.items():
            print(f"UPD update_{kind}_{I} step{s} {k}: bad={bad} worst={worst:.3f} of the bound")
            assert bad == 0, (s, k, bad, worst)
        assert ("ada.g2" in res) == (kind == "adadelta") and ("mom" in res) == (kind != "adadelta")
    assert "libdl.so" in " ".join(_native.loaded_libs())
