"""DeepSHAP (rescale rule) of a dense MLP against background rows.

`deep_shap` dispatches to libdl_shap.so (csrc/dl_shap.hip) for f32 tensors on
a GPU; `deep_shap_torch` is the same rule in torch, in the dtype of its
inputs, vectorised over (test row, background row) pairs.  It runs on CPU
tensors, for maxout layers and for networks wider than the kernel's LDS plan,
and is the kernel tests' second oracle.

The network: hidden layer l has W_l [U_l * k, U_{l-1}] and b_l [U_l * k]
(k = 2 for maxout: unit u owns rows 2u, 2u + 1), an activation and a test-time
scale s_l (1 - hidden_dropout_ratio); the explained scalar is
f = out_w . A_L + out_b with A_l = s_l act(a_l), a_l = A_{l-1} W_l^T + b_l.

The rule, for test row x and background row z: the multiplier on A_L is out_w;
going down, g_l = s_l (act(a_l(x)) - act(a_l(z))) / (a_l(x) - a_l(z)), or
s_l act'((a_l(x) + a_l(z)) / 2) where the two differ by less than 1e-6, and
M_{l-1} = (M_l * g_l) W_l; phi_i = M_0,i (x_i - z_i).  A maxout unit's two
pieces each get their exact two-player Shapley share of max(a1, a2) between x
and z, divided by the piece's own difference (0 where that is 0).  Per pair
the contributions sum to f(x) - f(z) (exactly for piecewise-linear units, to
rounding otherwise); the bias term is f(z).
"""
from __future__ import annotations

import ctypes

import torch

from . import _native, dl_ops
from ._native import check, ptr as _ptr, stream as _stream
from .shap_ops import ShapResult

EPS = 1e-6                      # |a(x) - a(z)| below which the derivative is used
KERNEL_ACTS = ("tanh", "rectifier", "exprectifier")
MAX_LAYERS = 8
LDS_BYTES = 160 * 1024
_ROW_TILE_CAP = 1 << 19
# whether the kernel runs by default on GPU tensors (use_native=None): it is
# faster than the torch rule at both shapes of profiles/dl_shap_mb.txt
# (10k x 100: 2.4x, 1 x 10k: 1.2x)
NATIVE_DEFAULT = True
_cv, _ci = ctypes.c_void_p, ctypes.c_int


class DeepShapResult(ShapResult):
    """ShapResult of `deep_shap`: phi [N, P+1] (averaged) or [N*B, P+1] (per
    reference, test row major) f64 with the bias term f(z) last; fz [B] and
    fx [N] the f64 link-space scores; kernel / why / row_tiles / bg_tiles as
    in ShapResult."""
    __slots__ = ("fx",)

    def __init__(self, phi, fx, fz, kernel, why=None, row_tiles=0, bg_tiles=0):
        super().__init__(phi, fz, kernel, why, row_tiles, bg_tiles, 0)
        self.fx = fx


# ------------------------------------------------------------------ forward
def _forward(layers, acts, scales, out_w, out_b, X, native):
    """Pre-activations (bias included) of every hidden layer and the f64 score
    f, by the scoring forward's own ops (dl_ops.gemm + dl_ops.fwd)."""
    A, pre = X, []
    for (W, b), act, s in zip(layers, acts, scales):
        Zl = dl_ops.gemm(A, W.t()) if native else A @ W.t()
        A = dl_ops.fwd(Zl, b, act, 0.0, train=False, test_scale=float(s), use_native=native)
        pre.append(Zl)
    f = A.to(torch.float64) @ out_w.to(torch.float64).view(-1) + float(out_b)
    return pre, f


def _act(act, a):
    if act == "tanh":
        return torch.tanh(a)
    if act == "rectifier":
        return torch.relu(a)
    if act == "exprectifier":
        return torch.where(a > 0, a, torch.expm1(a))
    if act == "linear":
        return a
    raise ValueError(f"deep_shap: unknown activation {act}")


def _dact(act, a):
    if act == "tanh":
        return 1 - torch.tanh(a) ** 2
    if act == "rectifier":
        return (a > 0).to(a.dtype)
    if act == "exprectifier":
        return torch.where(a > 0, torch.ones_like(a), torch.exp(a))
    return torch.ones_like(a)


def _gain(act, ax, az, s):
    d = ax - az
    small = d.abs() < EPS
    sec = (_act(act, ax) - _act(act, az)) / torch.where(small, torch.ones_like(d), d)
    return s * torch.where(small, _dact(act, 0.5 * (ax + az)), sec)


def _maxout_gain(ax, az, s):
    """[n, B, 2U] multipliers of the two pieces of every maxout unit."""
    n, B = ax.shape[0], az.shape[1]
    x = ax.reshape(n, 1, -1, 2)
    z = az.reshape(1, B, -1, 2)
    x1, x2, z1, z2 = x[..., 0], x[..., 1], z[..., 0], z[..., 1]
    mz, mx = torch.maximum(z1, z2), torch.maximum(x1, x2)
    p1 = 0.5 * ((torch.maximum(x1, z2) - mz) + (mx - torch.maximum(z1, x2)))
    p2 = 0.5 * ((torch.maximum(z1, x2) - mz) + (mx - torch.maximum(x1, z2)))
    out = []
    for p, d in ((p1, x1 - z1), (p2, x2 - z2)):
        out.append(torch.where(d == 0, torch.zeros_like(p), p / torch.where(d == 0, torch.ones_like(d), d)))
    return s * torch.stack(out, 3).reshape(n, B, -1)


def _check(layers, acts, scales, out_w, X, Z):
    if len(layers) < 1 or not (len(layers) == len(acts) == len(scales)):
        raise ValueError("deep_shap: layers, acts and scales must have one entry per hidden layer")
    if int(Z.shape[0]) == 0:
        raise ValueError("deep_shap: the background frame has no rows")
    fin = int(X.shape[1])
    if int(Z.shape[1]) != fin:
        raise ValueError("deep_shap: X and Z must both be [rows, inputs]")
    for (W, b), act in zip(layers, acts):
        k = 2 if act == "maxout" else 1
        if int(W.shape[1]) != fin or int(W.shape[0]) % k or int(b.numel()) != int(W.shape[0]):
            raise ValueError("deep_shap: layer shapes do not chain")
        fin = int(W.shape[0]) // k
    if int(out_w.numel()) != fin:
        raise ValueError("deep_shap: out_w must have one weight per unit of the last hidden layer")


def _finish(phi, fx, fz, N, B, P, per_reference):
    if per_reference:
        phi.view(N, B, P + 1)[:, :, P] = fz.view(1, B)
    else:
        phi[:, :P] /= B
        phi[:, P] = fz.mean()
    return phi


# ------------------------------------------------------------------ torch
def deep_shap_torch(layers, acts, scales, out_w, X, Z, per_reference=False, pair_scale=None,
                    max_scratch_bytes=1 << 30, out_b=0.0) -> DeepShapResult:
    """The rule above in torch, in X's dtype (f64 for the oracle).  Test rows
    are chunked so that one [rows, B, widest layer] tensor stays within a
    quarter of max_scratch_bytes."""
    _check(layers, acts, scales, out_w, X, Z)
    dt, dev = X.dtype, X.device
    layers = [(W.to(dt), b.to(dt)) for W, b in layers]
    out_w = out_w.to(dt).view(-1)
    Z = Z.to(dt)
    N, B, P = int(X.shape[0]), int(Z.shape[0]), int(X.shape[1])
    pre_x, fx = _forward(layers, acts, scales, out_w, out_b, X, False)
    pre_z, fz = _forward(layers, acts, scales, out_w, out_b, Z, False)
    S = pair_scale(fx, fz) if pair_scale is not None else None
    phi = torch.zeros((N * B if per_reference else N, P + 1), dtype=torch.float64, device=dev)
    widest = max([P] + [int(W.shape[0]) for W, _ in layers])
    step = max(1, int(max_scratch_bytes) // 4 // max(1, B * widest * X.element_size()))
    for r0 in range(0, N, step):
        r1 = min(N, r0 + step)
        n = r1 - r0
        M = out_w.view(1, 1, -1).expand(n, B, -1)
        for l in range(len(layers) - 1, -1, -1):
            ax, az = pre_x[l][r0:r1].unsqueeze(1), pre_z[l].unsqueeze(0)
            if acts[l] == "maxout":
                G = M.repeat_interleave(2, dim=2) * _maxout_gain(ax, az, float(scales[l]))
            else:
                G = M * _gain(acts[l], ax, az, float(scales[l]))
            M = G @ layers[l][0]
        c = (M * (X[r0:r1].unsqueeze(1) - Z.unsqueeze(0))).to(torch.float64)
        if S is not None:
            c = c * S[r0:r1].to(torch.float64).unsqueeze(2)
        if per_reference:
            phi.view(N, B, P + 1)[r0:r1, :, :P] = c
        else:
            phi[r0:r1, :P] = c.sum(1)
    return DeepShapResult(_finish(phi, fx, fz, N, B, P, per_reference), fx, fz, False, "torch rule")


# ------------------------------------------------------------------ kernel
def _lib():
    return _native.get_lib("dl_shap", required=True)


def dl_shap_lds_bytes(widths) -> int:
    """LDS bytes of the pair kernel's plan for widths = [inputs, hidden
    units ..., 1]: a 16-row tile of the inputs, of the slice sum and of every
    hidden layer's pre-activations, plus two multiplier buffers of the widest
    hidden layer (rows padded to a multiple of 16 floats, + 4)."""
    pad = [((int(w) + 15) // 16) * 16 + 4 for w in widths[:-1]]
    return 4 * 16 * (sum(pad) + pad[0] + 2 * max(pad[1:]))


def dl_shap_fits(widths) -> bool:
    """The kernel takes up to 8 hidden layers whose plan fits 160 KiB of LDS."""
    nl = len(widths) - 2
    return 1 <= nl <= MAX_LAYERS and int(widths[-1]) == 1 and dl_shap_lds_bytes(widths) <= LDS_BYTES


def _plan(N, B, P, chunk, max_scratch_bytes, with_scale, per_reference):
    """Row tile (a multiple of 16) and background tile (a multiple of the
    kernel's slice) whose scratch fits the budget: the f32 slice sums
    [bt / chunk, rt, P] (averaged mode) and, with pair factors, the [rt, bt]
    f64 temporaries of computing them (counted as five) plus their f32 copy."""
    budget = int(max_scratch_bytes)

    def cost(rt, bt):
        c = 0 if per_reference else 4 * (-(-bt // chunk)) * rt * P
        return c + (44 * rt * bt if with_scale else 0)
    bt = min(-(-B // chunk) * chunk, 65535 * chunk)
    while bt > chunk and cost(16, bt) > budget:
        bt = max(chunk, (bt // 2 + chunk - 1) // chunk * chunk)
    if cost(16, bt) > budget:
        raise ValueError(f"max_scratch_bytes={budget} cannot hold the scratch of 16 rows against {bt} "
                         f"background rows: {cost(16, bt)} bytes")
    rt = min(max(16, -(-N // 16) * 16), _ROW_TILE_CAP)
    while rt > 16 and cost(rt, bt) > budget:
        rt = max(16, (rt // 2 + 15) // 16 * 16)
    return rt, bt


def deep_shap(layers, acts, scales, out_w, X, Z, per_reference=False, pair_scale=None,
              max_scratch_bytes=1 << 30, out_b=0.0, use_native=None, timing=None) -> DeepShapResult:
    """Contributions of the P inputs (+ bias term) to f for the test rows X
    [N, P] against the background rows Z [B, P].

    layers         [(W_l, b_l)] of the hidden layers, bottom up
    acts / scales  their activations ("tanh", "rectifier", "exprectifier",
                   "maxout") and test-time scales
    out_w, out_b   the output unit: f = out_w . A_L + out_b
    per_reference  one output row per (test row, background row) pair instead
                   of the mean over the background rows
    pair_scale     optional (fx [N] f64, fz [B] f64) -> [N, B] factor on each
                   pair's contributions (output_space); applied before averaging
    max_scratch_bytes  bound on the scratch; rows and background rows are tiled
    use_native     None: the kernel where it applies (f32 GPU tensors, no
                   maxout, a plan that fits LDS) if NATIVE_DEFAULT; True / False
                   force the choice (True raises where the kernel cannot run)
    timing         optional dict: gets "pairs_ms", the pair stage's device time
    """
    _check(layers, acts, scales, out_w, X, Z)
    widths = [int(X.shape[1])] + [int(W.shape[0]) // (2 if a == "maxout" else 1)
                                   for (W, _), a in zip(layers, acts)] + [1]
    why = None
    if X.device.type != "cuda":
        why = "CPU tensors"
    elif any(a not in KERNEL_ACTS for a in acts):
        why = "the kernel has no " + ", ".join(sorted({a for a in acts if a not in KERNEL_ACTS})) + " units"
    elif X.dtype != torch.float32:
        why = f"{X.dtype} inputs, the kernel is f32"
    elif not dl_shap_fits(widths):
        why = f"widths {widths} need {dl_shap_lds_bytes(widths)} bytes of LDS, the kernel has {LDS_BYTES}" \
            if len(widths) - 2 <= MAX_LAYERS else f"{len(widths) - 2} hidden layers, the kernel takes {MAX_LAYERS}"
    if use_native and why is not None:
        raise ValueError(f"deep_shap: the kernel cannot run: {why}")
    if why is None and (use_native is False or (use_native is None and not NATIVE_DEFAULT)):
        why = "use_native=False" if use_native is False else "the torch rule is the default (use_native=True)"
    if why is not None:
        res = deep_shap_torch(layers, acts, scales, out_w, X, Z, per_reference, pair_scale, max_scratch_bytes, out_b)
        res.why = why
        return res
    lib = _lib()
    dev = X.device
    f32 = lambda t: t.to(torch.float32).contiguous()
    layers = [(f32(W), f32(b)) for W, b in layers]
    out_w = f32(out_w.view(-1))
    X, Z = f32(X), f32(Z)
    N, B, P = int(X.shape[0]), int(Z.shape[0]), int(X.shape[1])
    pre_x, fx = _forward(layers, acts, scales, out_w, out_b, X, True)
    pre_z, fz = _forward(layers, acts, scales, out_w, out_b, Z, True)
    nl = len(layers)
    chunk = int(lib.h2o_dl_shap_chunk())
    rt, bt = _plan(N, B, P, chunk, max_scratch_bytes, pair_scale is not None, per_reference)
    # few test rows: tiles of 16 background rows looping over the test rows pad
    # less than tiles of 16 test rows (decided from the totals, not the tiling)
    swap = N * (-(-B // 16) * 16) < (-(-N // 16) * 16) * B
    phi = torch.zeros((N * B if per_reference else N, P + 1), dtype=torch.float64, device=dev)
    partial = None
    if not per_reference and N > 0:
        partial = torch.empty(-(-bt // chunk) * min(rt, N) * P, dtype=torch.float32, device=dev)
    wid = (_ci * (nl + 1))(*widths[:-1])
    actc = (_ci * nl)(*[dl_ops.ACT[a] for a in acts])
    scc = (ctypes.c_float * nl)(*[float(s) for s in scales])
    Wp = (_cv * nl)(*[W.data_ptr() for W, _ in layers])
    stream = _stream()
    ev = None
    if timing is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    row_tiles = bg_tiles = 0
    for r0 in range(0, N, rt):
        nr = min(rt, N - r0)
        row_tiles += 1
        bg_tiles = 0
        pxp = (_cv * nl)(*[p.data_ptr() + 4 * r0 * p.shape[1] for p in pre_x])
        for b0 in range(0, B, bt):
            nb = min(bt, B - b0)
            bg_tiles += 1
            S = None
            if pair_scale is not None:
                S = pair_scale(fx[r0:r0 + nr], fz[b0:b0 + nb]).to(torch.float32).contiguous()
                assert S.shape == (nr, nb)
            pzp = (_cv * nl)(*[p.data_ptr() + 4 * b0 * p.shape[1] for p in pre_z])
            rc = lib.h2o_dl_shap_pairs(nl, wid, actc, scc, Wp, pxp, pzp, _cv(X.data_ptr() + 4 * r0 * P),
                                       _cv(Z.data_ptr() + 4 * b0 * P), _ptr(out_w), _ptr(S), nr, nb,
                                       _ptr(partial), _ptr(phi), r0, b0, B, 1 if per_reference else 0,
                                       1 if swap else 0, stream)
            check(rc, "h2o_dl_shap_pairs")
    if ev is not None:
        ev[1].record()
        torch.cuda.synchronize()
        timing["pairs_ms"] = ev[0].elapsed_time(ev[1])
    return DeepShapResult(_finish(phi, fx, fz, N, B, P, per_reference), fx, fz, True, None, row_tiles, bg_tiles)
