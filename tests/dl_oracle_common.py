"""fp64 oracle of the fused MLP training step (dl.hip dl_mlp_fb_kernel /
dl_mlp_dw_kernel / dl_mlp_upd_kernel, reached through dl_ops.mlp_step) and of
the per-row update (dl_update_kernel, dl_ops.update).

Plain torch on the CPU.  The only thing taken from dl_ops is keep_mask (the
definition of the dropout hash) and the UpdateParams record; no forward,
backward, update or softmax of the project is called here.

oracle_grads  forward under autograd in fp64, the output gradient set by hand
              from the formulas of the output layers, pushed back with
              torch.autograd.grad; returns A_l, dZ_l, dW_l, db_l per layer and
              the scale S of each entry's rounding error (the same sum with
              every term replaced by its absolute value).
oracle_update the per-neuron-row bprop tail of Neurons.java in fp64.

The cases of the GPU test live here too, so that what depends on the
reference alone (the share of fragile rectifier units, the max_w2 margin) is
checked without a GPU.
"""
from types import SimpleNamespace

import torch

from h2o3_amd.ops import dl_ops

_M = (1 << 64) - 1
F64 = torch.float64

# a rectifier pre-activation this close to zero (relative to its error scale
# S_A) may land on either side of it in float32: 64 ulp of the scale
FRAGILE = 64 * 2.0 ** -24
FRAGILE_CAP = 1e-4          # largest share of fragile entries among a case's rectifier pre-activations
MAXW2_MARGIN = 1e-4         # no row's squared norm this close (relative) to max_w2
TAU_CAP = 2.0 ** -13        # one of 531 rows missing from a sum shows at ~2e-3 S: tau stays far below
E32_FLOOR = 2.0 ** -24      # the yardstick is never below one float32 rounding of the scale

# Gradient tolerance tau = min(TAU_M * e32, TAU_CAP), where e32 is the worst
# |delta| / S of the same oracle graph evaluated in float32 torch on the CPU
# (floored at 2^-24), per case, step and quantity.  e32 is a maximum over all
# entries and so is led by the few whose gradient cancels to far below its
# scale; it moves by a factor of two or three with the CPU's summation order.
# rho = kernel error / e32 measured on an MI355X, the worse of the two steps:
#
#   case                A      dZ     dW     db
#   ragged_tanh         1.23   1.14   0.66   0.58
#   wide_relu           1.21   1.04   1.15   1.50
#   one_layer           0.00   0.82   1.26   1.56
#   eight_layers        2.77   0.74   0.64   1.42
#   regression_elu      1.00   1.48   0.44   0.68
#   momentum_nesterov   0.93   1.00   1.24   3.29
#   momentum_plain      0.93   1.00   1.24   3.29
#   device_seed         1.69   0.94   0.92   1.27
#
# (the 3.29 is 3.3 float32 roundings of db against an e32 at its floor.)
# TAU_M is the smallest power of two >= 4 * max rho = 13.2; the 4 covers the
# other summation order (4-deep MFMA k-steps, 8-wave folds) and __expf in the
# softmax.  The largest kernel error measured is 7.8e-6 S (eight_layers dZ),
# the largest tau before the cap 16 * 1.05e-5 = 1.7e-4 (the same entry; its
# e32 is 4.3e-6 with another CPU's summation order), so there the cap is the
# tolerance.
TAU_M = 16


def tau(e32):
    return min(TAU_M * e32, TAU_CAP)


# Update tolerance: |delta| <= UPD_RTOL |ref| + 1e-3 median|ref| per tensor.
# An updated value is a chain of fewer than 20 float32 roundings per element
# on top of a 64-lane (or 256-thread) sum of at most 600 squares; 64 ulp of
# float32 bounds that with room for the other summation order.  The absolute
# term is for entries that cancel (w - rate * grad near zero).
UPD_RTOL = 2.0 ** -18
UPD_ATOL_MEDIAN = 1e-3


def lcg(s: int) -> int:
    """One step of the device step seed (dl_lcg)."""
    return (s * 6364136223846793005 + 1442695040888963407) & _M


def _f32(x) -> float:
    """The float32 value the kernels receive for a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _ratio(delta, S):
    """max |delta| / S over the entries; an entry with S = 0 must match exactly."""
    delta = delta.abs().to(F64)
    S = S.to(F64)
    r = torch.where(S > 0, delta / S.clamp_min(1e-300), torch.where(delta > 0, float("inf"), 0.0).to(F64))
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------- gradients
def oracle_grads(Ws, bs, X, idx, y, w, acts, drops, in_drop, out_kind, inv_n, seed, relu_on=None,
                 dtype=F64, on_fixed=None):
    """Reference forward + backward of one step.

    Ws / bs: float32 weights [U, I] and biases per layer; X [n, P]; idx [B]
    int64 or None (the first B = len(X) rows); y labels (int64, out_kind 0 / 1)
    or float32 targets (out_kind 2), w row weights or None -- both indexed by
    the gathered row, as X is; acts / drops per hidden layer.
    relu_on: per hidden layer None or a bool [B, U] with the kernel's A > 0;
    it decides `on` for the fragile rectifier entries of kept units only.
    dtype / on_fixed: the same graph in another precision with every
    rectifier decision given (the float32 yardstick).
    """
    nl = len(Ws)
    B = int(idx.shape[0]) if idx is not None else int(X.shape[0])
    src = idx if idx is not None else torch.arange(B)
    seed = int(seed) & _M
    Wp = [W.detach().cpu().to(dtype).requires_grad_(True) for W in Ws]
    bp = [b.detach().cpu().to(dtype).requires_grad_(True) for b in bs]
    a = X.cpu().index_select(0, src).to(dtype)
    a = a * dl_ops.keep_mask((seed + 0x5bd1e995) & _M, B, a.shape[1], in_drop, "cpu")
    A, S_A, zs, dacts, keeps, ons = [a], [a.abs()], [], [], [], []
    fragile = nrelu = 0
    z_out = S_z = None
    for l in range(nl):
        z = a @ Wp[l].t() + bp[l]
        sz = a.detach().abs() @ Wp[l].detach().abs().t() + bp[l].detach().abs()
        if l == nl - 1:
            z_out, S_z = z, sz
            break
        U = z.shape[1]
        keep = dl_ops.keep_mask((seed + 7919 * (l + 1)) & _M, B, U, drops[l], "cpu")
        zd = z.detach()
        on = None
        if acts[l] == "tanh":
            h = torch.tanh(z)
            dact = 1 - h.detach() ** 2
        elif acts[l] == "exprectifier":
            h = torch.where(z > 0, z, torch.expm1(z))
            dact = torch.where(zd > 0, torch.ones_like(zd), h.detach() + 1)
        elif acts[l] == "linear":
            h = z
            dact = torch.ones_like(zd)
        elif acts[l] == "rectifier":
            if on_fixed is not None:
                on = on_fixed[l]
            else:
                on = zd > 0
                frag = (zd.abs() < FRAGILE * sz) & keep
                nrelu += zd.numel()
                fragile += int(frag.sum())
                if relu_on is not None and relu_on[l] is not None:
                    on = torch.where(frag, relu_on[l].cpu(), on)
            h = z * on
            dact = on.to(dtype)
        else:
            raise ValueError(acts[l])
        a = h * keep
        zs.append(z)
        dacts.append(dact)
        keeps.append(keep)
        ons.append(on)
        A.append(a.detach())
        S_A.append(sz)
    # output gradient dE/dnet, from the detached logits
    zo = z_out.detach()
    wr = torch.ones(B, dtype=dtype) if w is None else w.cpu().index_select(0, src).to(dtype)
    scale = (wr * _f32(inv_n)).view(-1, 1)
    if out_kind < 2:
        t = y.cpu().index_select(0, src).to(torch.int64)
        scale = torch.where((t < 0).view(-1, 1), torch.zeros_like(scale), scale)
        p = torch.softmax(zo, 1)
        T = torch.zeros_like(p)
        valid = t >= 0
        T[valid, t[valid]] = 1.0
        g0 = (p - T) if out_kind == 0 else (p - T) * (1 - p) * p
        g = g0 * scale
        # p_k moves by at most 2 p_k max_j |dz_j|, and carries its own rounding
        S_out = (g0.abs() + p * (1 + S_z.max(1, keepdim=True).values)) * scale
    else:
        yv = y.cpu().reshape(-1).index_select(0, src).to(dtype).view(-1, 1)
        g = 2 * (zo - yv) * scale
        S_out = 2 * (S_z + yv.abs()) * scale
    grads = torch.autograd.grad(z_out, Wp + bp + zs, grad_outputs=g)
    dW, db = list(grads[:nl]), list(grads[nl:2 * nl])
    dZ = list(grads[2 * nl:]) + [g]
    S_dZ = [None] * (nl - 1) + [S_out]
    for l in range(nl - 2, -1, -1):
        S_dZ[l] = (dZ[l + 1].abs() @ Wp[l + 1].detach().abs()) * dacts[l].abs() * keeps[l]
    S_dW = [dZ[l].abs().t() @ A[l].abs() for l in range(nl)]
    S_db = [dZ[l].abs().sum(0) for l in range(nl)]
    return SimpleNamespace(A=A, dZ=dZ, dW=dW, db=db, S_A=S_A, S_dZ=S_dZ, S_dW=S_dW, S_db=S_db, on=ons, keep=keeps,
                           fragile=fragile, nrelu=nrelu)


def grad_errors(got, ref, r32):
    """Per quantity: (worst |got - ref| / S, e32 = worst |r32 - ref| / S floored
    at 2^-24), over every layer and entry.  got: object or dict with lists A,
    dZ, dW, db of float32 tensors."""
    out = {}
    for q in ("A", "dZ", "dW", "db"):
        S = getattr(ref, "S_" + q)
        gq = got[q] if isinstance(got, dict) else getattr(got, q)
        ek = max(_ratio(gq[l].detach().cpu().to(F64) - getattr(ref, q)[l], S[l]) for l in range(len(S)))
        e32 = max(_ratio(getattr(r32, q)[l].to(F64) - getattr(ref, q)[l], S[l]) for l in range(len(S)))
        out[q] = (ek, max(e32, E32_FLOOR))
    return out


# ---------------------------------------------------------------- update
def oracle_update(W, b, dW, db, state, p):
    """The per-row bprop tail of Neurons.java in fp64: gradient + L1 / L2,
    ADADELTA on (E[dx^2], E[g^2]) or momentum (plain / Nesterov), the max_w2
    rescale after the weight pass, the bias update with the row's mean squared
    weight gradient.  state: dict with ada [U, I, 2], ada_b [U, 2], mom, mom_b
    (missing or None: zeros).  Returns (W, b, state, r2) in fp64; r2 is each
    row's squared norm before the rescale."""
    rho, eps, rate, mu, l1, l2 = (_f32(v) for v in (p.rho, p.eps, p.rate, p.momentum, p.l1, p.l2))
    max_w2 = _f32(p.max_w2) if p.max_w2 is not None and p.max_w2 < 3.0e38 else float("inf")
    W, b, dW, db = (t.detach().cpu().to(F64) for t in (W, b, dW, db))
    U, I = W.shape
    st = {k: (v.detach().cpu().to(F64) if v is not None else None) for k, v in (state or {}).items()}
    ada = st.get("ada") if st.get("ada") is not None else torch.zeros((U, I, 2), dtype=F64)
    ada_b = st.get("ada_b") if st.get("ada_b") is not None else torch.zeros((U, 2), dtype=F64)
    mom = st.get("mom") if st.get("mom") is not None else torch.zeros((U, I), dtype=F64)
    mom_b = st.get("mom_b") if st.get("mom_b") is not None else torch.zeros(U, dtype=F64)
    new = {"ada": ada.clone(), "ada_b": ada_b.clone(), "mom": mom.clone() if p.has_momenta else None,
           "mom_b": mom_b.clone() if p.has_momenta else None}
    g = dW + torch.sign(W) * l1 + W * l2
    msq = None
    if p.ada:
        e_dx, e_g = ada[..., 0], ada[..., 1]
        gg = g * g
        e_g = rho * e_g + (1 - rho) * gg
        r = torch.sqrt((e_dx + eps) / (e_g + eps))
        new["ada"] = torch.stack([rho * e_dx + (1 - rho) * r * r * gg, e_g], 2)
        nW = W - r * g
        msq = gg.sum(1) / max(I, 1)
    elif not p.nesterov:
        step = -rate * g
        nW = W + step
        if p.has_momenta:
            nW = nW + mu * mom
            new["mom"] = step
    else:
        d = -g
        if p.has_momenta:
            d = mom * mu + d
            new["mom"] = d
        nW = W + rate * d
    r2 = (nW * nW).sum(1)
    over = r2 > max_w2
    nW = torch.where(over.view(-1, 1), nW * torch.sqrt(max_w2 / r2.clamp_min(1e-300)).view(-1, 1), nW)
    gb = db + torch.sign(b) * l1 + b * l2
    if p.ada:
        e_g = rho * ada_b[:, 1] + (1 - rho) * msq
        r = torch.sqrt((ada_b[:, 0] + eps) / (e_g + eps))
        new["ada_b"] = torch.stack([rho * ada_b[:, 0] + (1 - rho) * r * r * msq, e_g], 1)
        nb = b - r * gb
    elif not p.nesterov:
        step = -rate * gb
        nb = b + step
        if p.has_momenta:
            nb = nb + mu * mom_b
            new["mom_b"] = step
    else:
        d = -gb
        if p.has_momenta:
            d = mom_b * mu + d
            new["mom_b"] = d
        nb = b + rate * d
    return nW, nb, new, r2


def update_mismatch(got, ref):
    """Entries of `got` outside UPD_RTOL |ref| + UPD_ATOL_MEDIAN median|ref|,
    and the worst excess ratio |delta| / bound."""
    ref = ref.to(F64)
    got = got.detach().cpu().to(F64)
    bound = UPD_RTOL * ref.abs() + UPD_ATOL_MEDIAN * float(ref.abs().median())
    d = (got - ref).abs()
    bad = int((d > bound).sum())
    worst = float(torch.where(bound > 0, d / bound.clamp_min(1e-300),
                              torch.where(d > 0, float("inf"), 0.0).to(F64)).max())
    return bad, worst


def check_update(layer_after, snap, dW, db, p, names=None):
    """Compare one layer's post-step W, b and optimiser state with
    oracle_update on the snapshot; returns ({name: (bad, worst)}, r2)."""
    W0, b0, st0 = snap
    nW, nb, nst, r2 = oracle_update(W0, b0, dW, db, st0, p)
    res = {"W": update_mismatch(layer_after.W, nW), "b": update_mismatch(layer_after.b, nb)}
    if p.ada:
        # E[dx^2] and E[g^2] live on different scales: each against its own median
        for k in ("ada", "ada_b"):
            for ch, nm in enumerate(("dx2", "g2")):
                res[f"{k}.{nm}"] = update_mismatch(layer_after.state[k][..., ch], nst[k][..., ch])
    elif p.has_momenta:
        for k in ("mom", "mom_b"):
            res[k] = update_mismatch(layer_after.state[k], nst[k])
    return res, r2


def maxw2_margin(r2, max_w2):
    """(smallest relative distance of a row's r2 to max_w2, rows above, rows below)."""
    m = _f32(max_w2)
    rel = ((r2 - m).abs() / m)
    return float(rel.min()), int((r2 > m).sum()), int((r2 <= m).sum())


def snapshot(layers):
    return [(L.W.detach().cpu().clone(), L.b.detach().cpu().clone(),
             {k: (v.detach().cpu().clone() if v is not None else None) for k, v in L.state.items()})
            for L in layers]


# ---------------------------------------------------------------- cases
def glorot(g, U, I):
    lim = (6.0 / (I + U)) ** 0.5
    return ((torch.rand((U, I), generator=g) * 2 - 1) * lim).to(torch.float32)


CASES = ("ragged_tanh", "wide_relu", "one_layer", "eight_layers", "regression_elu", "momentum_nesterov",
         "momentum_plain", "device_seed")
STEPS = 2

# data seed of each case, picked on the CPU from the reference alone so that
# the fragile share stays under FRAGILE_CAP and no row sits within
# MAXW2_MARGIN of max_w2 in either step (test_dl_oracle.py asserts both); for
# wide_relu, eight_layers and regression_elu the one of seeds 0..39 whose
# float32 yardstick e32 is smallest (the best-conditioned data: an entry whose
# gradient cancels to far below its scale carries the error of the layers
# behind it, and e32 with it)
DATA_SEED = {"ragged_tanh": 0, "wide_relu": 11, "one_layer": 0, "eight_layers": 33, "regression_elu": 21,
             "momentum_nesterov": 0, "momentum_plain": 0, "device_seed": 0}


def make_case(name):
    """Everything one case needs, as CPU tensors: widths, B, Ws, bs, X, idxs
    (one per step, None = the first B rows), y, w, acts, drops, in_drop,
    out_kind, ups (per step, per layer), seeds (per step), seed_dev0."""
    g = torch.Generator().manual_seed(1000 + DATA_SEED[name])
    c = SimpleNamespace(name=name, n=1000, in_drop=0.0, out_kind=0, w=None, seed_dev0=None, max_w2=False,
                        up=dict(ada=True))
    if name in ("ragged_tanh", "device_seed"):
        c.widths, c.B = (13, 37, 19, 5), 333 if name == "ragged_tanh" else 48
        c.acts, c.drops, c.in_drop = ["tanh", "tanh"], [0.2, 0.3], 0.1
        c.up = dict(ada=True, l1=1e-4, l2=1e-3)
        c.max_w2 = True
        if name == "device_seed":
            c.seed_dev0 = 0x123456789ABCDEF
    elif name == "wide_relu":
        c.widths, c.B = (100, 260, 200, 2), 531
        c.acts, c.drops = ["rectifier", "rectifier"], [0.5, 0.5]
    elif name == "one_layer":
        c.widths, c.B, c.n = (24, 3), 7, 7
        c.acts, c.drops = [], []
    elif name == "eight_layers":
        c.widths, c.B = (5, 17, 16, 15, 33, 4, 1, 20, 64), 100
        c.acts = ["tanh", "rectifier", "exprectifier", "linear", "tanh", "exprectifier", "rectifier"]
        c.drops = [0.1, 0.0, 0.0, 0.2, 0.0, 0.0, 0.0]
        c.out_kind = 1
    elif name == "regression_elu":
        c.widths, c.B = (24, 50, 1), 100
        c.acts, c.drops = ["exprectifier"], [0.0]
        c.out_kind = 2
    elif name in ("momentum_nesterov", "momentum_plain"):
        c.widths, c.B = (32, 64, 32, 3), 256
        c.acts, c.drops = ["rectifier", "rectifier"], [0.0, 0.0]
        c.up = dict(ada=False, rate=0.01, momentum=0.9, has_momenta=True, nesterov=name == "momentum_nesterov")
        c.max_w2 = True
    else:
        raise KeyError(name)
    nl = len(c.widths) - 1
    K = c.widths[-1]
    c.X = torch.randn((c.n, c.widths[0]), generator=g)
    c.Ws = [glorot(g, c.widths[l + 1], c.widths[l]) for l in range(nl)]
    c.bs = [0.1 * torch.randn(c.widths[l + 1], generator=g) for l in range(nl)]
    if c.out_kind < 2:
        c.y = torch.randint(0, K, (c.n,), generator=g)
        if name in ("ragged_tanh", "device_seed"):
            c.y[::11] = -1
    else:
        c.y = torch.randn(c.n, generator=g)
    if name in ("ragged_tanh", "device_seed", "regression_elu"):
        c.w = torch.rand(c.n, generator=g) + 0.5
    c.idxs = [None if name == "one_layer" else torch.randint(0, c.n, (c.B,), generator=g) for _ in range(STEPS)]
    c.seeds = [77 + 1000003 * s for s in range(STEPS)]
    c.inv_n = 1.0 / c.B
    # max_w2 of layer l at step s: the expected squared row norm of a
    # Glorot-uniform row, 2 I / (I + U), lowered by 3% per step so that the
    # rows rescaled onto it in one step are clear of it in the next
    c.ups = [[dl_ops.UpdateParams(max_w2=(2.0 * c.widths[l] / (c.widths[l] + c.widths[l + 1]) * 0.97 ** s
                                          if c.max_w2 else float("inf")), **c.up)
              for l in range(nl)] for s in range(STEPS)]
    return c


def step_seed(c, s, seed_dev_before):
    """The seed the masks of step s are drawn with."""
    if c.seed_dev0 is None:
        return c.seeds[s]
    return (c.seeds[s] + lcg(seed_dev_before)) & _M


def reference_run(c):
    """The two steps of a case on the reference alone (the weights of step 2
    are the fp64 update of step 1 rounded to float32).  Returns per step the
    oracle result, its float32 twin and the r2 / max_w2 pairs."""
    nl = len(c.Ws)
    Ws, bs = [W.clone() for W in c.Ws], [b.clone() for b in c.bs]
    states = [{} for _ in range(nl)]
    sd = c.seed_dev0
    out = []
    for s in range(STEPS):
        seed = step_seed(c, s, sd)
        if sd is not None:
            sd = lcg(sd)
        ref = oracle_grads(Ws, bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind, c.inv_n, seed)
        r32 = oracle_grads(Ws, bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind, c.inv_n, seed,
                           dtype=torch.float32, on_fixed=ref.on)
        r2s = []
        for l in range(nl):
            nW, nb, nst, r2 = oracle_update(Ws[l], bs[l], ref.dW[l].float(), ref.db[l].float(), states[l],
                                            c.ups[s][l])
            Ws[l], bs[l] = nW.float(), nb.float()
            states[l] = {k: (v.float() if v is not None else None) for k, v in nst.items()}
            r2s.append((r2, c.ups[s][l].max_w2))
        out.append(SimpleNamespace(ref=ref, r32=r32, r2s=r2s))
    return out


# ---------------------------------------------------------------- the kernel side
def run_fused_case(c, dev="cuda"):
    """The two steps of a case through dl_ops.mlp_step.  Per step: the
    snapshot before it, the kernel's raw A / dZ / dW / db, the layers after
    it, and the oracle (fp64 and its float32 twin) on the snapshot."""
    nl = len(c.Ws)
    layers = [SimpleNamespace(W=W.clone().to(dev), b=b.clone().to(dev), state={}) for W, b in zip(c.Ws, c.bs)]
    X, y = c.X.to(dev), c.y.to(dev)
    w = None if c.w is None else c.w.to(dev)
    seed_dev = None
    if c.seed_dev0 is not None:
        seed_dev = torch.tensor([dl_ops._i64(c.seed_dev0)], dtype=torch.int64, device=dev)
    bufs, sd, out = {}, c.seed_dev0, []
    for s in range(STEPS):
        snap = snapshot(layers)
        idx = None if c.idxs[s] is None else c.idxs[s].to(dev)
        dl_ops.mlp_step(X, idx, y, w, layers, c.acts, c.drops, c.in_drop, c.out_kind, c.inv_n, c.ups[s],
                        seed=c.seeds[s], seed_dev=seed_dev, advance=seed_dev is not None, bufs=bufs)
        torch.cuda.synchronize()
        seed = step_seed(c, s, sd)
        sd_after = None
        if sd is not None:
            sd = lcg(sd)
            sd_after = int(seed_dev.item()) & _M
        got = {q: [t.detach().cpu().clone() for t in bufs[q]] for q in ("A", "dZ", "dW", "db")}
        after = [SimpleNamespace(W=W, b=b, state=st) for W, b, st in snapshot(layers)]
        relu_on = [got["A"][l + 1] > 0 if act == "rectifier" else None for l, act in enumerate(c.acts)]
        Ws, bs = [t[0] for t in snap], [t[1] for t in snap]
        ref = oracle_grads(Ws, bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind, c.inv_n, seed,
                           relu_on=relu_on)
        r32 = oracle_grads(Ws, bs, c.X, c.idxs[s], c.y, c.w, c.acts, c.drops, c.in_drop, c.out_kind, c.inv_n, seed,
                           dtype=torch.float32, on_fixed=ref.on)
        out.append(SimpleNamespace(snap=snap, got=got, after=after, ref=ref, r32=r32, seed=seed, sd_expected=sd,
                                   sd_after=sd_after))
    assert nl == len(layers)
    return out


UPDATE_KINDS = ("adadelta", "nesterov", "plain")
UPDATE_WIDTHS = (129, 600)      # 600: a thread of dl_update_kernel's 256 handles more than one column


# picked on the CPU so that no row sits within MAXW2_MARGIN of max_w2 in any step
UPDATE_SEED = {("adadelta", 129): 10, ("adadelta", 600): 5, ("nesterov", 129): 13, ("nesterov", 600): 8,
               ("plain", 129): 13, ("plain", 600): 5}


def update_case(kind, I, U=300, steps=3):
    """Inputs of the dl_ops.update tests: Glorot W [U, I], small b, per step a
    gradient and the UpdateParams (max_w2 as in make_case)."""
    g = torch.Generator().manual_seed(UPDATE_SEED[kind, I])
    t0 = 2.0 * I / (I + U)
    kw = dict(ada=True) if kind == "adadelta" else dict(ada=False, rate=0.01, momentum=0.9, has_momenta=True,
                                                        nesterov=kind == "nesterov")
    return SimpleNamespace(W=glorot(g, U, I), b=0.1 * torch.randn(U, generator=g),
                           ps=[dl_ops.UpdateParams(l1=1e-4, l2=1e-3, max_w2=t0 * 0.97 ** s, **kw)
                               for s in range(steps)],
                           dWs=[0.01 * torch.randn((U, I), generator=g) for _ in range(steps)],
                           dbs=[0.01 * torch.randn(U, generator=g) for _ in range(steps)])


def run_update_case(uc, dev, use_native=None):
    """Three dl_ops.update steps on `dev`; per step ({tensor: (bad, worst)},
    (closest relative distance to max_w2, rows above, rows below))."""
    L = SimpleNamespace(W=uc.W.clone().to(dev), b=uc.b.clone().to(dev), state={})
    out = []
    for p, dW, db in zip(uc.ps, uc.dWs, uc.dbs):
        snap = snapshot([L])[0]
        dl_ops.update(L.W, dW.to(dev), L.b, db.to(dev), L.state, p, use_native=use_native)
        if L.W.device.type == "cuda":
            torch.cuda.synchronize()
        res, r2 = check_update(L, snap, dW, db, p)
        out.append((res, maxw2_margin(r2, p.max_w2)))
    return out
