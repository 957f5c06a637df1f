"""Baseline (interventional) SHAP of a packed forest against background rows.

`background_shap` dispatches to libtree_shap.so (csrc/tree_shap.hip) on a GPU
device; `background_shap_torch` is the same rule in torch, vectorised over
(test row, background row) pairs with a loop over leaves.  It runs on CPU
tensors, scores forests whose paths are too wide for the kernel's 32-bit masks,
and is the kernel tests' second oracle.

The rule, for test row x, background row z and a leaf of value v whose
root-to-leaf conditions are grouped by feature into m path elements: with
okx[e] / okz[e] = "x / z satisfies every condition of element e", the leaf
contributes only when every element holds for x or for z; then with
A = okx & ~okz (a elements) and B = okz & ~okx (b elements) each feature of A
gets +v (a-1)! b! / (a+b)! and each feature of B gets -v a! (b-1)! / (a+b)!.
Per pair the contributions sum to f(x) - f(z); the bias term is f(z).

`path_shap` / `path_shap_torch` (end of the file) are path-dependent TreeSHAP,
predict_contributions without a background frame, over the same leaf table:
node covers take the place of the background rows.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import torch

from . import _native
from ._native import check as _check, ptr as _ptr, stream as _stream

MAX_PATH = 32                 # path elements a uint32 mask holds
_ROW_TILE_CAP = 32768         # test rows per tile (bounds the per-tile scratch)


class ShapResult:
    """Result of `background_shap` (and of `path_shap`: fz None, bg_tiles 0,
    bias column left at zero).

    phi          [N, F+1] (averaged) or [N*B, F+1] (per reference, ordered by
                 test row then background row) f64; last column = bias term
    kernel       True when the HIP kernels produced it
    why          why the torch implementation ran instead (None on the kernel)
    fz           [B] f64 tree score (times vscale) of every background row
    row_tiles / bg_tiles / tree_chunks   how the kernel run was tiled
    """
    __slots__ = ("phi", "fz", "kernel", "why", "row_tiles", "bg_tiles", "tree_chunks")

    def __init__(self, phi, fz, kernel, why=None, row_tiles=0, bg_tiles=0, tree_chunks=0):
        self.phi, self.fz, self.kernel, self.why = phi, fz, kernel, why
        self.row_tiles, self.bg_tiles, self.tree_chunks = row_tiles, bg_tiles, tree_chunks


_weight_tables: dict = {}


def weight_table(n: int, device) -> torch.Tensor:
    """W[a, b] = (a-1)! b! / (a+b)! for 1 <= a, a + b <= n (else 0), [n+1, n+1]
    f64, built once per (n, device).  The negative side's a! (b-1)! / (a+b)!
    is W[b, a]."""
    key = (n, str(device))
    if key not in _weight_tables:
        _weight_tables[key] = _build_weight_table(n, device)
    return _weight_tables[key]


def _build_weight_table(n, device):
    W = [[0.0] * (n + 1) for _ in range(n + 1)]
    for a in range(1, n + 1):
        for b in range(0, n + 1 - a):
            W[a][b] = float(Fraction(math.factorial(a - 1) * math.factorial(b), math.factorial(a + b)))
    return torch.tensor(W, dtype=torch.float64, device=device)


# ------------------------------------------------------------------ torch
def _go_left(P, nd, X):
    """forest_predict_kernel's decision for packed nodes nd [C] on every
    column of X [F, n]: bool [C, n]."""
    x = X[P["feat"][nd].long()]
    isn = torch.isnan(x)
    nal = (P["na_left"][nd] != 0).view(-1, 1).expand_as(x)
    co = P["cat_off"][nd].long().view(-1, 1)
    cl = P["cat_len"][nd].long().view(-1, 1)
    code = torch.nan_to_num(x, nan=-1.0).clamp(-1.0, 1073741824.0).long()   # (int)x, saturated
    inr = (code >= 0) & (code < cl)
    nb = P["cat_bits"].numel()
    bit = P["cat_bits"][(co + code).clamp(0, nb - 1)] != 0
    go_cat = torch.where(isn | ~inr, nal, bit)
    go_num = torch.where(isn, nal, x < P["thr"][nd].view(-1, 1))
    return torch.where(co >= 0, go_cat, go_num)


def _leaf_ok(P, PT, host, l, X):
    """[m, n] bool: element e of leaf l holds for column (row) r of X."""
    el_off, cond_off = host
    e0, e1 = el_off[l], el_off[l + 1]
    c0, c1 = cond_off[e0], cond_off[e1]
    ok = _go_left(P, PT["cond_node"][c0:c1].long(), X) == (PT["cond_left"][c0:c1] != 0).view(-1, 1)
    out = torch.empty((e1 - e0, X.shape[1]), dtype=torch.bool, device=X.device)
    for e in range(e0, e1):
        out[e - e0] = ok[cond_off[e] - c0:cond_off[e + 1] - c0].all(0)
    return out


def background_shap_torch(P, PT, X, Z, F, per_reference=False, vscale=1.0, tree_class=0, pair_scale=None):
    """The rule above in torch.  Returns (phi, fz) as in ShapResult."""
    dev = X.device
    X = X.to(torch.float32)
    Z = Z.to(torch.float32)
    N, B = X.shape[1], Z.shape[1]
    host = (PT["el_off"].tolist(), PT["cond_off"].tolist())
    cls = PT["leaf_cls"].tolist()
    val = PT["leaf_val"].tolist()
    leaves = [l for l in range(PT["L"]) if cls[l] == tree_class]
    W = weight_table(max(PT["max_path"], 1), dev)
    fx = torch.zeros(N, dtype=torch.float64, device=dev)
    fz = torch.zeros(B, dtype=torch.float64, device=dev)
    for l in leaves:                          # link-space scores (bias term, pair_scale)
        fz += float(vscale) * val[l] * _leaf_ok(P, PT, host, l, Z).all(0).to(torch.float64)
        if pair_scale is not None:
            fx += float(vscale) * val[l] * _leaf_ok(P, PT, host, l, X).all(0).to(torch.float64)
    S = pair_scale(fx, fz) if pair_scale is not None else None      # [N, B]
    phi = torch.zeros((N, B, F + 1) if per_reference else (N, F + 1), dtype=torch.float64, device=dev)
    for l in leaves:
        e0 = host[0][l]
        m = host[0][l + 1] - e0
        if m == 0:
            continue
        okx = _leaf_ok(P, PT, host, l, X).unsqueeze(2)          # [m, N, 1]
        okz = _leaf_ok(P, PT, host, l, Z).unsqueeze(1)          # [m, 1, B]
        valid = (okx | okz).all(0)                               # [N, B]
        A = okx & ~okz
        Bm = okz & ~okx
        a = A.sum(0)
        b = Bm.sum(0)
        v = float(vscale) * val[l] * valid.to(torch.float64)
        if S is not None:
            v = v * S
        wa = v * W[a, b]
        wb = v * W[b, a]
        feats = PT["el_feat"][e0:e0 + m].tolist()
        for e, f in enumerate(feats):
            c = wa * A[e] - wb * Bm[e]
            if per_reference:
                phi[:, :, f] += c
            else:
                phi[:, f] += c.sum(1)
    if per_reference:
        phi[:, :, F] = fz.view(1, B)
        return phi.reshape(N * B, F + 1), fz
    phi[:, :F] /= B
    phi[:, F] = fz.mean()
    return phi, fz


# ------------------------------------------------------------------ kernel
def _plan(PT, N, B, max_scratch_bytes, with_scale):
    """Row tile, background tile and tree chunks whose scratch (uint32 masks
    [leaves, rows] for both frames, plus the f64 pair factors and the
    [rows, background rows] temporaries of computing them, counted as five f64
    matrices) fits the budget.  The smallest chunk is one whole tree."""
    lmin = max(1, PT["max_tree_leaves"])
    budget = int(max_scratch_bytes)
    pair_bytes = 5 * 8

    def cost(leaves, rt, bt):
        return 4 * leaves * (rt + bt) + (pair_bytes * rt * bt if with_scale else 0)
    bt = B
    while bt > 1 and cost(lmin, 64, bt) > budget:
        bt = (bt + 1) // 2
    if cost(lmin, 64, bt) > budget:
        raise ValueError(f"max_scratch_bytes={budget} cannot hold the masks of one tree ({lmin} leaves) "
                         f"for 64 rows: {cost(lmin, 64, bt)} bytes")
    rt = min(max(64, -(-N // 64) * 64), _ROW_TILE_CAP)      # N = 0 (an empty shard): no tile is run
    while rt > 64 and cost(lmin, rt, bt) > budget:
        rt = max(64, (rt // 2 + 63) // 64 * 64)
    per_leaf = 4 * (rt + bt)
    lc = max(lmin, (budget - (pair_bytes * rt * bt if with_scale else 0)) // per_leaf)
    off = PT["tree_leaf_off"]
    chunks, start = [], 0
    for t in range(1, len(off)):
        if off[t] - off[start] > lc:          # tree t-1 does not fit any more
            chunks.append((off[start], off[t - 1]))
            start = t - 1
    chunks.append((off[start], off[-1]))
    return rt, bt, [c for c in chunks if c[1] > c[0]]


def background_shap(P, PT, X, Z, F, per_reference=False, vscale=1.0, tree_class=0, pair_scale=None,
                    max_scratch_bytes=1 << 30, timing=None) -> ShapResult:
    """Contributions of the F features (+ bias term) for the test rows X
    [F, N] against the background rows Z [F, B], both column-major float32.

    P, PT          Forest.pack() and Forest.leaf_paths() on X's device
    per_reference  one output row per (test row, background row) pair instead
                   of the mean over the background rows
    vscale         factor on every leaf value (DRF: 1 / ntrees)
    tree_class     only trees of this class are scored
    pair_scale     optional (fx [N] f64, fz [B] f64) -> [N, B] f64 factor on
                   each pair's contributions, given the link-space tree scores
                   (output_space); applied before averaging
    max_scratch_bytes  bound on the mask scratch; rows and trees are tiled to fit
    timing         optional dict: gets "masks_ms" / "pairs_ms", the two stages'
                   device time from stream events (synchronises at the end)
    """
    N, B = int(X.shape[1]), int(Z.shape[1])
    if B == 0:
        raise ValueError("background_shap: the background frame has no rows")
    if int(X.shape[0]) != int(Z.shape[0]) or int(X.shape[0]) < F:
        raise ValueError("background_shap: X and Z must both be [F, rows]")
    if PT["max_feat"] >= F:
        raise ValueError("background_shap: the forest splits on a feature the matrices do not have")
    why = None
    if X.device.type != "cuda":
        why = "CPU tensors"
    elif PT["max_path"] > MAX_PATH:
        why = f"a path has {PT['max_path']} distinct features, the kernel's masks hold {MAX_PATH}"
    if why is not None:
        phi, fz = background_shap_torch(P, PT, X, Z, F, per_reference, vscale, tree_class, pair_scale)
        return ShapResult(phi, fz, False, why)
    lib = _native.get_lib("tree_shap", required=True)
    dev = X.device
    X = X.contiguous().to(torch.float32)
    Z = Z.contiguous().to(torch.float32)
    stream = _stream()
    W = weight_table(MAX_PATH, dev)
    L = PT["L"]
    tree_args = (_ptr(P["node"]), _ptr(P["cat_off"]), _ptr(P["cat_len"]), _ptr(P["cat_bits"]),
                 _ptr(PT["el_off"]), _ptr(PT["el_feat"]), _ptr(PT["cond_off"]), _ptr(PT["cond_node"]),
                 _ptr(PT["cond_left"]), _ptr(PT["leaf_val"]), _ptr(PT["leaf_cls"]), int(tree_class))

    def masks(M, c0, n, l0, l1, mask, score):
        # rows [c0, c0 + n) of the column-major matrix M, leaves [l0, l1)
        base = ctypes.c_void_p(M.data_ptr() + 4 * c0)
        rc = lib.h2o_shap_masks(base, M.shape[1], n, *tree_args, l0, l1, _ptr(mask), _ptr(score),
                                float(vscale), stream)
        _check(rc, "h2o_shap_masks")

    # link-space scores: the bias term, and the pair factors' inputs
    fz = torch.zeros(B, dtype=torch.float64, device=dev)
    masks(Z, 0, B, 0, L, None, fz)
    fx = None
    if pair_scale is not None:
        fx = torch.zeros(N, dtype=torch.float64, device=dev)
        masks(X, 0, N, 0, L, None, fx)
    rt, bt, chunks = _plan(PT, N, B, max_scratch_bytes, pair_scale is not None)
    phi = torch.zeros((N * B if per_reference else N, F + 1), dtype=torch.float64, device=dev)
    lmax = max(c[1] - c[0] for c in chunks) if chunks else 0
    MX = torch.empty(lmax * rt, dtype=torch.int32, device=dev)
    MZ = torch.empty(lmax * bt, dtype=torch.int32, device=dev)
    row_tiles = bg_tiles = 0
    events = []

    def mark():
        if timing is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e
    for r0 in range(0, N, rt):
        nr = min(rt, N - r0)
        row_tiles += 1
        bg_tiles = 0
        for b0 in range(0, B, bt):
            nb = min(bt, B - b0)
            bg_tiles += 1
            S = None
            if pair_scale is not None:
                S = pair_scale(fx[r0:r0 + nr], fz[b0:b0 + nb]).to(torch.float64).contiguous()
                assert S.shape == (nr, nb)
            for l0, l1 in chunks:
                e0 = mark()
                masks(X, r0, nr, l0, l1, MX, None)
                masks(Z, b0, nb, l0, l1, MZ, None)
                e1 = mark()
                rc = lib.h2o_shap_pairs(_ptr(MX), nr, _ptr(MZ), nb, _ptr(PT["el_off"]), _ptr(PT["el_feat"]),
                                        _ptr(PT["leaf_val"]), _ptr(PT["leaf_cls"]), int(tree_class), l0, l1,
                                        _ptr(W), _ptr(S), float(vscale), _ptr(phi), r0, b0, B, F,
                                        1 if per_reference else 0, stream)
                _check(rc, "h2o_shap_pairs")
                events.append((e0, e1, mark()))
    if per_reference:
        phi.view(N, B, F + 1)[:, :, F] = fz.view(1, B)
    else:
        phi[:, :F] /= B
        phi[:, F] = fz.mean()
    if timing is not None:
        torch.cuda.synchronize()
        timing["masks_ms"] = sum(a.elapsed_time(b) for a, b, _ in events)
        timing["pairs_ms"] = sum(b.elapsed_time(c) for _, b, c in events)
    return ShapResult(phi, fz, True, None, row_tiles, bg_tiles, len(chunks))


# ------------------------------------------------------------------ path-dependent TreeSHAP
_path_tables: dict = {}


def path_coef_table(device) -> torch.Tensor:
    """C[k, i] = i! (k-1-i)! / k! for i < k <= 32 (else 0), [33, 32] f64: the
    Shapley weight of a coalition of i of the other k-1 path elements.  Built
    once per device."""
    key = str(device)
    if key not in _path_tables:
        C = [[0.0] * MAX_PATH for _ in range(MAX_PATH + 1)]
        for k in range(1, MAX_PATH + 1):
            for i in range(k):
                C[k][i] = float(Fraction(math.factorial(i) * math.factorial(k - 1 - i), math.factorial(k)))
        _path_tables[key] = torch.tensor(C, dtype=torch.float64, device=device)
    return _path_tables[key]


def path_shap_torch(P, PT, X, F, vscale=1.0, tree_class=0):
    """Path-dependent TreeSHAP (Lundberg et al., Algorithm 2) over leaf paths
    in torch, vectorised over rows with a loop over leaves.  Returns phi
    [N, F+1] f64 with the bias column left at zero.

    For a leaf of value v with k path elements, element e has the feature
    d_e, the one-fraction o_e in {0, 1} ("the row satisfies every condition
    of the element") and the zero-fraction z_e = PT["el_zero"].  EXTEND
    builds the path weights w[0..k] one element at a time; per element the
    UNWOUND-SUM of models/tree/shap.py (_unwound_sum, both branches) times
    (o_e - z_e) * v goes to column d_e."""
    dev = X.device
    X = X.to(torch.float32)
    N = X.shape[1]
    host = (PT["el_off"].tolist(), PT["cond_off"].tolist())
    cls = PT["leaf_cls"].tolist()
    val = PT["leaf_val"].tolist()
    phi = torch.zeros((N, F + 1), dtype=torch.float64, device=dev)
    for l in range(PT["L"]):
        e0 = host[0][l]
        k = host[0][l + 1] - e0
        if cls[l] != tree_class or k == 0:
            continue
        O = _leaf_ok(P, PT, host, l, X).to(torch.float64)             # [k, N]
        Z = PT["el_zero"][e0:e0 + k].view(k, 1)
        idx = torch.arange(k + 1, dtype=torch.float64, device=dev).view(-1, 1)
        w = torch.zeros((k + 1, N), dtype=torch.float64, device=dev)
        w[0] = 1.0
        for d in range(1, k + 1):                                      # EXTEND with element d-1
            up = torch.zeros_like(w)
            up[1:] = w[:-1] * (idx[1:] / (d + 1))                      # w[i] (i+1)/(d+1) into w[i+1]
            w = Z[d - 1] * w * ((d - idx).clamp(min=0.0) / (d + 1)) + O[d - 1] * up
        nz = O != 0
        zok = Z != 0
        zsafe = torch.where(zok, Z, torch.ones_like(Z))
        nxt = w[k].expand(k, N).clone()
        total = torch.zeros((k, N), dtype=torch.float64, device=dev)
        for i in range(k - 1, -1, -1):                                 # UNWOUND-SUM of every element at once
            tmp = nxt * (k + 1) / (i + 1)
            t_zero = torch.where(zok, (w[i] / zsafe) / ((k - i) / (k + 1)), torch.zeros_like(tmp))
            total = total + torch.where(nz, tmp, t_zero)
            nxt = torch.where(nz, w[i] - tmp * Z * ((k - i) / (k + 1)), nxt)
        c = total * (O - Z) * (float(vscale) * val[l])
        phi.index_add_(1, PT["el_feat"][e0:e0 + k].long(), c.t())
    return phi


def path_shap(P, PT, X, F, vscale=1.0, tree_class=0, max_scratch_bytes=1 << 30, timing=None) -> ShapResult:
    """Path-dependent TreeSHAP contributions of the F features for the rows X
    [F, N] (column-major float32): phi [N, F+1] f64 whose bias column is left
    at zero for the caller (it does not depend on the rows).

    P, PT          Forest.pack() and Forest.leaf_paths() on X's device
    vscale         factor on every leaf value (DRF: 1 / ntrees)
    tree_class     only trees of this class are scored
    max_scratch_bytes  bound on the mask scratch; rows and trees are tiled to fit
    timing         optional dict: gets "masks_ms" / "path_ms", the two stages'
                   device time from stream events (synchronises at the end)

    On a GPU: shap_mask_kernel for the one-fractions, then shap_path_kernel
    (csrc/tree_shap.hip).  `path_shap_torch` runs for CPU tensors and for
    paths wider than the kernel's masks; the result then says why."""
    N = int(X.shape[1])
    if int(X.shape[0]) < F:
        raise ValueError("path_shap: X must be [F, rows]")
    if PT["max_feat"] >= F:
        raise ValueError("path_shap: the forest splits on a feature the matrix does not have")
    why = None
    if X.device.type != "cuda":
        why = "CPU tensors"
    elif PT["max_path"] > MAX_PATH:
        why = f"a path has {PT['max_path']} distinct features, the kernel's masks hold {MAX_PATH}"
    if why is not None:
        return ShapResult(path_shap_torch(P, PT, X, F, vscale, tree_class), None, False, why)
    lib = _native.get_lib("tree_shap", required=True)
    dev = X.device
    X = X.contiguous().to(torch.float32)
    stream = _stream()
    C = path_coef_table(dev)
    rt, _, chunks = _plan(PT, N, 0, max_scratch_bytes, False)
    phi = torch.zeros((N, F + 1), dtype=torch.float64, device=dev)
    lmax = max(c[1] - c[0] for c in chunks) if chunks else 0
    MX = torch.empty(lmax * rt, dtype=torch.int32, device=dev)
    row_tiles = 0
    events = []

    def mark():
        if timing is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e
    for r0 in range(0, N, rt):
        nr = min(rt, N - r0)
        row_tiles += 1
        base = ctypes.c_void_p(X.data_ptr() + 4 * r0)
        for l0, l1 in chunks:
            e0 = mark()
            rc = lib.h2o_shap_masks(base, X.shape[1], nr, _ptr(P["node"]), _ptr(P["cat_off"]), _ptr(P["cat_len"]),
                                    _ptr(P["cat_bits"]), _ptr(PT["el_off"]), _ptr(PT["el_feat"]),
                                    _ptr(PT["cond_off"]), _ptr(PT["cond_node"]), _ptr(PT["cond_left"]),
                                    _ptr(PT["leaf_val"]), _ptr(PT["leaf_cls"]), int(tree_class), l0, l1, _ptr(MX),
                                    _ptr(None), float(vscale), stream)
            _check(rc, "h2o_shap_masks")
            e1 = mark()
            rc = lib.h2o_shap_path(_ptr(MX), nr, _ptr(PT["el_off"]), _ptr(PT["el_feat"]), _ptr(PT["el_zero"]),
                                   _ptr(PT["leaf_val"]), _ptr(PT["leaf_cls"]), int(tree_class), l0, l1, _ptr(C),
                                   float(vscale), _ptr(phi), r0, F, stream)
            _check(rc, "h2o_shap_path")
            events.append((e0, e1, mark()))
    if timing is not None:
        torch.cuda.synchronize()
        timing["masks_ms"] = sum(a.elapsed_time(b) for a, b, _ in events)
        timing["path_ms"] = sum(b.elapsed_time(c) for _, b, c in events)
    return ShapResult(phi, None, True, None, row_tiles, 0, len(chunks))
