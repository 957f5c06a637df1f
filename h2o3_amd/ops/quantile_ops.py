"""Segmented weighted quantiles on the GPU: libtree_quantile.so
(csrc/tree_quantile.hip), an exact MSD radix selection over the rows of each
leaf segment, 8 key bits per pass.

The rule: among the rows of a segment with w > 0, ordered by the f32 value
x = y - f, the first whose running weight reaches q * (total weight), the last
such row if rounding leaves none; 0.0 for a segment without weight.  Weights
are summed as int64 fixed point (w * 2^scale_bits, see `weight_scale_bits`),
so the result does not depend on chunking, on the order of the atomics or on
how the rows are spread over ranks: the ranks add their [L, 256] tables, four
times, and every rank takes the same decisions from the sum.

Nothing here runs on CPU tensors: the torch / numpy functions of
models/tree/gbm.py remain the CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _native
from ._native import check, ptr as _ptr, stream as _stream
from .tree_ops import _h2d, make_work
from ..parallel import collectives as coll

PASSES = 4     # 8 bits each over the 32-bit key


def _lib():
    return _native.get_lib("tree_quantile", required=True)


def weight_scale_bits(max_w, n_global, unit):
    """S of the fixed-point weights: 0 when every weight is 0 or 1 (`unit`),
    else the largest S <= 40 with max_w * n_global * 2^S < 2^62, so that no sum
    of quanta over all rows of all ranks leaves int64."""
    if unit:
        return 0
    top = float(max_w) * max(float(n_global), 1.0)
    if not top > 0 or not math.isfinite(top):
        return 0
    return max(0, min(40, 62 - math.frexp(top)[1]))    # top < 2^exponent


class LeafQuantile:
    """The selection state of one rank: position-ordered keys and fixed-point
    weights (written once, at construction, by the only kernel that gathers)
    and per leaf the key prefix chosen so far, the weight below it and the
    total weight.

    ridx    i32 positions -> rows, or None (position = row)
    y, f, w f32 by row; f None: x = y; w None: unit weights
    mode    1: |x|
    """

    def __init__(self, ridx, y, f, w, leaf_ids, starts, counts, n_leaves, q, scale_bits, mode=0, chunk=65536):
        dev = y.device
        if dev.type != "cuda":
            raise ValueError("LeafQuantile: device tensors only (models/tree/gbm.py holds the CPU path)")
        self.lib = _lib()
        self.L, self.q, self.S = int(n_leaves), float(q), int(scale_bits)
        items = make_work(starts, counts, leaf_ids, chunk)
        self.n_work = len(items)
        self.work = _h2d(items, dev) if self.n_work else None
        npos = int((items[:, 1] + items[:, 2]).max()) if self.n_work else 0
        self.key_pos = torch.empty(npos, dtype=torch.int32, device=dev)      # u32 bits
        self.wq_pos = torch.empty(npos, dtype=torch.int64, device=dev)
        self.prefix = torch.zeros(self.L, dtype=torch.int32, device=dev)     # u32 bits
        self.cum = torch.zeros(self.L, dtype=torch.int64, device=dev)
        self.wtot = torch.zeros(self.L, dtype=torch.int64, device=dev)
        self.out = torch.zeros(self.L, dtype=torch.float64, device=dev)
        if self.n_work:
            if int(items[:, 0].min()) < 0 or int(items[:, 0].max()) >= self.L:
                raise ValueError("LeafQuantile: leaf id outside [0, n_leaves)")
            y, f, w = (None if t is None else t.to(torch.float32).contiguous() for t in (y, f, w))
            nrow = npos if ridx is None else int(y.numel())
            if y.numel() < nrow or any(t is not None and t.numel() < y.numel() for t in (f, w)) or \
                    (ridx is not None and ridx.numel() < npos):
                raise ValueError("LeafQuantile: y / f / w / ridx shorter than the segments")
            check(self.lib.h2o_lq_keys(_ptr(ridx), _ptr(y), _ptr(f), _ptr(w), _ptr(self.work), self.n_work, int(mode),
                                       float(2.0 ** self.S), _ptr(self.key_pos), _ptr(self.wq_pos), _stream()),
                  "h2o_lq_keys")

    def hist(self, k):
        """This rank's [L, 256] i64 table of pass k."""
        h = torch.zeros((self.L, 256), dtype=torch.int64, device=self.out.device)
        if self.n_work:
            check(self.lib.h2o_lq_hist(_ptr(self.key_pos), _ptr(self.wq_pos), _ptr(self.work), self.n_work,
                                       _ptr(self.prefix), int(k), _ptr(h), _stream()), "h2o_lq_hist")
        return h

    def select(self, k, hist):
        """Advance every leaf by the 8 bits of pass k, decided from `hist`
        (the sum of the ranks' tables)."""
        if tuple(hist.shape) != (self.L, 256) or hist.dtype != torch.int64 or not hist.is_contiguous():
            raise ValueError("LeafQuantile.select: hist is a contiguous [L, 256] int64 table")
        check(self.lib.h2o_lq_select(_ptr(hist), self.L, int(k), self.q, float(2.0 ** -self.S), _ptr(self.prefix),
                                     _ptr(self.cum), _ptr(self.wtot), _ptr(self.out), _stream()), "h2o_lq_select")

    def values(self):
        """[L] f64 on the device (after the last pass)."""
        return self.out


def _run(s):
    for k in range(PASSES):
        h = s.hist(k)
        coll.allreduce_(h)
        s.select(k, h)
    return s.values()


def leaf_wquantile(ridx, y, f, w, leaf_ids, starts, counts, n_leaves, q, scale_bits, mode=0, chunk=65536):
    """Weighted q-quantile of y - f within every leaf segment of ridx, over
    all ranks -> [n_leaves] f64 on the device, the same bits on every rank."""
    return _run(LeafQuantile(ridx, y, f, w, leaf_ids, starts, counts, n_leaves, q, scale_bits, mode, chunk))


def global_wquantile(y, f, w, q, scale_bits, mode=0, chunk=65536):
    """Weighted q-quantile of y - f (f None: of y; mode 1: of |y - f|) over all
    rows of all ranks -> float."""
    return float(_run(LeafQuantile(None, y, f, w, [0], [0], [int(y.numel())], 1, q, scale_bits, mode, chunk))[0])
