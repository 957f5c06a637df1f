"""Word2Vec hierarchical-softmax mini-batch step.

One *example* is a target word c and n_in >= 0 input words (skip-gram: one;
CBOW: the window words its mask allows, n_in = 0 does nothing).  From the
tables as they stand at the start of the batch:

    h      = mean of syn0[inputs]
    dot_l  = syn1[point[c][l]] . h                        for l < len(c)
    valid  = |dot_l| < 6
    g_l    = ((1 - code[c][l]) - sigmoid(dot_l)) * lr * valid
    neu1e  = sum_l g_l * syn1[point[c][l]]
    c1[node] = valid (example, l) entries of the batch on that node
    c0[word] = (example, input slot) entries on that word
    syn1[node] += sum g * h  / max(1, c1[node] / 8)
    syn0[word] += sum neu1e  / max(1, c0[word] / 8)

`hsm_step_torch` is that rule in torch ops, in the dtype of syn0 / syn1 (so
on f64 copies it is the oracle of the kernel tests).  `hsm_step` routes f32
GPU tables with d <= 512 to csrc/w2v.hip (one call = counter memset + three
kernels) and everything else -- CPU tensors, wider vectors, H2O3_W2V=torch --
to `hsm_step_torch`.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np
import torch

from . import _native
from ._native import check as _check, ptr as _ptr, stream as _stream

MAX_EXP = 6.0            # WordVectorTrainer.MAX_EXP
MAX_D = 512              # widest vector the kernel holds in registers (8 per lane)
LDS_BYTES = 64 * 1024    # hot-node cache of a workgroup: two workgroups fit a CU
MAX_HOT = 2048

Plan = namedtuple("Plan", "hot threads grid")


def launch_plan(B, d, nodes, cus, hot=None, threads=None, grid=None) -> Plan:
    """The kernel launch for a batch of B examples: `hot` top Huffman nodes
    cached in LDS, threads per workgroup (one wave per example), `grid`
    workgroups that each walk ceil(B / grid) consecutive examples.  Explicit
    values override the defaults and are checked."""
    cap = min(int(nodes), LDS_BYTES // (4 * (int(d) + 1)), MAX_HOT)
    hot = cap if hot is None else int(hot)
    if not 0 <= hot <= cap:
        raise ValueError(f"hot nodes must be in [0, {cap}] at d = {d}, got {hot}")
    threads = 512 if threads is None else int(threads)
    if threads % 64 or not 64 <= threads <= 1024:
        raise ValueError(f"threads must be a multiple of 64 in [64, 1024], got {threads}")
    # 8 waves, two workgroups per CU (~32 examples each at B = 16384, 256 CUs): the fastest of
    # 4 or 8 waves x 1, 2, 4 per CU at both measured shapes (profiles/w2v_hsm_mb.txt)
    grid = max(1, min(-(-int(B) // (threads // 64)), 2 * int(cus))) if grid is None else int(grid)
    if grid < 1:
        raise ValueError(f"grid must be positive, got {grid}")
    return Plan(hot, threads, grid)


class HuffmanTables:
    """The Huffman tree of a vocabulary, in both layouts.

    Ragged, for the kernel: len [V] int32, point [V, L] int32, code [V, L]
    int8 (entries past len are 0 and never read).  Padded, for the torch rule:
    pt_t [V, L] int64 (0 past the end) and code_t [V, L] f32 (-1 past the end).
    nodes = rows of syn1 = max(V - 1, 1)."""

    def __init__(self, codes, points, device):
        V = len(codes)
        self.V, self.nodes = V, max(V - 1, 1)
        self.L = L = max(1, max(len(c) for c in codes))
        ln = np.array([len(c) for c in codes], dtype=np.int32)
        inside = np.arange(L)[None, :] < ln[:, None]
        code = np.zeros((V, L), dtype=np.int8)
        point = np.zeros((V, L), dtype=np.int32)
        code[inside] = np.fromiter((b for c in codes for b in c), dtype=np.int8, count=int(ln.sum()))
        point[inside] = np.fromiter((q for p in points for q in p), dtype=np.int32, count=int(ln.sum()))
        self.len = torch.from_numpy(ln).to(device)
        self.code = torch.from_numpy(code).to(device)
        self.point = torch.from_numpy(point).to(device)
        self.pt_t = self.point.long()
        self.code_t = torch.where(torch.from_numpy(inside).to(device), self.code.float(),
                                  torch.full((), -1.0, device=device))


class Scratch:
    """Temporaries of the kernel route for batches up to B examples, made once
    per training: g [B, L], neu1e [B, d] f32 and the c1 | c0 counters."""

    def __init__(self, B, d, tb, device):
        self.B = int(B)
        self.g = torch.empty((self.B, tb.L), dtype=torch.float32, device=device)
        self.neu1e = torch.empty((self.B, int(d)), dtype=torch.float32, device=device)
        self.counts = torch.empty(tb.nodes + tb.V, dtype=torch.int32, device=device)


def route(syn0) -> str:
    """"hip" or "torch": where hsm_step sends these tables."""
    if (syn0.device.type == "cuda" and syn0.dtype == torch.float32 and syn0.shape[1] <= MAX_D
            and os.environ.get("H2O3_W2V", "").lower() != "torch"):
        return "hip"
    return "torch"


def hsm_step_torch(syn0, syn1, tb, c, w_in, mask, lr):
    """The rule in torch ops, updating syn0 / syn1 in place.  c [b] targets;
    skip-gram: w_in [b], mask None; CBOW: w_in [b, W] and mask [b, W] bool.
    Returns dot [b, L] (entries past a word's code length are meaningless)."""
    pts, cds = tb.pt_t[c], tb.code_t[c]
    if mask is not None:
        m = mask
        bag = m.sum(1)
        ctxw = w_in                                          # [b, 2w]
        h = (syn0[ctxw] * m.unsqueeze(2)).sum(1) / bag.clamp_min(1).unsqueeze(1)
        S1 = syn1[pts]
        dot = (S1 * h.unsqueeze(1)).sum(2)
        valid = (cds >= 0) & (bag > 0).view(-1, 1) & (dot.abs() < MAX_EXP)
        gsc = ((1 - cds) - torch.sigmoid(dot)) * lr * valid
        neu1e = (gsc.unsqueeze(2) * S1).sum(1)
        pv = pts[valid]
        c1 = (torch.bincount(pv, minlength=syn1.shape[0]).to(h.dtype) / 8).clamp_min(1)
        syn1.index_add_(0, pv, (gsc.unsqueeze(2) * h.unsqueeze(1))[valid] / c1[pv].unsqueeze(1))
        wi = ctxw[m]
        upd = neu1e.unsqueeze(1).expand(-1, m.shape[1], -1)[m]
        c0 = (torch.bincount(wi, minlength=syn0.shape[0]).to(h.dtype) / 8).clamp_min(1)
        syn0.index_add_(0, wi, upd / c0[wi].unsqueeze(1))
        return dot
    h = syn0[w_in]             # [b, d]
    S1 = syn1[pts]             # [b, L, d]
    dot = (S1 * h.unsqueeze(1)).sum(2)
    # hierarchicalSoftmaxSG skips nodes with |f| >= MAX_EXP (6)
    valid = (cds >= 0) & (dot.abs() < MAX_EXP)
    f_ = torch.sigmoid(dot)
    gsc = ((1 - cds) - f_) * lr * valid
    neu1e = (gsc.unsqueeze(2) * S1).sum(1)
    # batched Hogwild: rows hit several times in one batch get the
    # sum of at most ~8 of their updates (a plain sum overshoots for frequent words)
    pv = pts[valid]
    c1 = (torch.bincount(pv, minlength=syn1.shape[0]).to(h.dtype) / 8).clamp_min(1)
    syn1.index_add_(0, pv, (gsc.unsqueeze(2) * h.unsqueeze(1))[valid] / c1[pv].unsqueeze(1))
    c0 = (torch.bincount(w_in, minlength=syn0.shape[0]).to(h.dtype) / 8).clamp_min(1)
    syn0.index_add_(0, w_in, neu1e / c0[w_in].unsqueeze(1))
    return dot


_CU = {}


def _cu_count(dev):
    if dev not in _CU:
        _CU[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _CU[dev]


def hsm_step(syn0, syn1, tb, c, w_in, mask, lr, scratch=None, plan=None):
    """One mini-batch step in place on syn0 [V, d] / syn1 [nodes, d]; arguments
    as hsm_step_torch.  On the kernel route `scratch` (a Scratch of at least
    this batch; allocated when not given) holds every temporary and `plan`
    (hot, threads, grid; None entries default) overrides launch_plan.  Returns
    the route taken."""
    if route(syn0) == "torch":
        hsm_step_torch(syn0, syn1, tb, c, w_in, mask, lr)
        return "torch"
    V, d = int(syn0.shape[0]), int(syn0.shape[1])
    B = int(c.shape[0])
    if B == 0:
        return "hip"
    W = 1 if w_in.dim() == 1 else int(w_in.shape[1])
    if (syn1.dtype != torch.float32 or tuple(syn1.shape) != (tb.nodes, d) or V != tb.V
            or not (syn0.is_contiguous() and syn1.is_contiguous())):
        raise ValueError("hsm_step: syn0 [V, d] and syn1 [nodes, d] must be contiguous f32 tables of this tree")
    if c.dtype != torch.int64 or w_in.dtype != torch.int64 or w_in.numel() != B * W:
        raise ValueError("hsm_step: c [b] and w_in [b] / [b, W] must be int64")
    if mask is not None and (mask.dtype != torch.bool or tuple(mask.shape) != tuple(w_in.shape) or W == 0):
        raise ValueError("hsm_step: mask must be a bool tensor of w_in's shape")
    if scratch is None:
        scratch = Scratch(B, d, tb, syn0.device)
    if scratch.B < B or scratch.neu1e.shape[1] != d or scratch.g.shape[1] != tb.L:
        raise ValueError("hsm_step: scratch is smaller than the batch")
    plan = launch_plan(B, d, tb.nodes, _cu_count(syn0.device), *(plan or ()))
    c, w_in = c.contiguous(), w_in.contiguous()
    mask = None if mask is None else mask.contiguous()
    lib = _native.get_lib("w2v", required=True)
    rc = lib.h2o_w2v_hsm_step(_ptr(syn0), _ptr(syn1), V, tb.nodes, d, _ptr(tb.len), _ptr(tb.point), _ptr(tb.code),
                              tb.L, _ptr(c), _ptr(w_in), _ptr(mask), B, W, float(lr), _ptr(scratch.g),
                              _ptr(scratch.neu1e), _ptr(scratch.counts), plan.hot, plan.threads, plan.grid,
                              _stream())
    _check(rc, "h2o_w2v_hsm_step")
    return "hip"
