"""Grouped binomial score sketch: the primitive under the fairness tables
(models/fairness.py).

`group_sketch` dispatches to libfairness.so (csrc/fairness.hip) on a GPU
device; `group_sketch_torch` is the definition in torch (`torch.bincount` on
the combined key plus masked sums).  It runs on CPU tensors and is the kernel
tests' oracle.

The definition: over the rows with a non-NaN score p1, a response code y in
{0, 1} and a group id g in [0, G) -- every other row is skipped --

    cnt[g, y', b]  rows per group, class and logit bin b of p' (i64)
    cm[g]          tp, fp, tn, fn at `thr`, favourable class positive (i64)
    sums[g]        sum of logloss, sum of squared error (f64)

with y' = y, p' = p1, selected = (p1 >= thr); with `flip` the favourable class
is code 0: y' = 1 - y, p' = 1 - p1, selected = !(p1 >= thr).  The score is
widened to f64 before anything is computed from it.  Every row counts 1: the
counts are exact and the same from run to run.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from ._native import check, ptr as _ptr, stream as _stream

LDS_GROUPS = 512              # groups whose per-group cells accumulate in LDS (FS_LDS_GROUPS of the kernel)
_c_void = ctypes.c_void_p


class SketchResult:
    """Result of `group_sketch`.

    cnt     [G, 2, nb] i64
    cm      [G, 4] i64: tp, fp, tn, fn
    sums    [G, 2] f64: sum of logloss, sum of squared error
    kernel  True when the HIP kernel produced it
    why     why the torch implementation ran instead (None on the kernel)
    chunks  launches (ranges of groups) the kernel run took
    """
    __slots__ = ("cnt", "cm", "sums", "kernel", "why", "chunks")

    def __init__(self, cnt, cm, sums, kernel, why=None, chunks=0):
        self.cnt, self.cm, self.sums, self.kernel, self.why, self.chunks = cnt, cm, sums, kernel, why, chunks


def _lib():
    lib = _native.get_lib("fairness", required=True)
    if lib.h2o_fairness_lds_groups() != LDS_GROUPS:
        raise RuntimeError("libfairness.so was built with another LDS_GROUPS than fairness_ops.py states")
    return lib


def _check(p1, y, g, G, nb):
    p1, y, g = p1.reshape(-1), y.reshape(-1), g.reshape(-1)
    if y.numel() != p1.numel() or g.numel() != p1.numel():
        raise ValueError("group_sketch: p1 / y / g lengths differ")
    if p1.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"group_sketch: p1 must be float32 or float64, got {p1.dtype}")
    if y.is_floating_point() or g.is_floating_point():
        raise ValueError("group_sketch: y and g are integer codes")
    if G < 0 or nb <= 0:
        raise ValueError("group_sketch: G >= 0 and nb > 0")
    return p1, y, g


def group_sketch_torch(p1, y, g, G, thr, flip=False, nb=1 << 18):
    """The definition above in torch: (cnt, cm, sums)."""
    from ..models.metrics import _logit_bins
    G, nb = int(G), int(nb)
    p1, y, g = _check(p1, y, g, G, nb)
    p = p1.to(torch.float64)
    ok = ~torch.isnan(p) & ((y == 0) | (y == 1)) & (g >= 0) & (g < G)
    p, y, g = p[ok], y[ok].to(torch.int64), g[ok].to(torch.int64)
    sel = p >= float(thr)
    if flip:
        y, p, sel = 1 - y, 1.0 - p, ~sel
    pos = y == 1
    cnt = torch.bincount((g * 2 + y) * nb + _logit_bins(p, nb), minlength=G * 2 * nb).view(G, 2, nb)
    cell = torch.where(pos, torch.where(sel, 0, 3), torch.where(sel, 1, 2))
    cm = torch.bincount(g * 4 + cell, minlength=G * 4).view(G, 4)
    pc = p.clamp(1e-15, 1 - 1e-15)
    ll = -torch.where(pos, pc.log(), (1 - pc).log())
    se = (y.to(torch.float64) - p) ** 2
    sums = torch.zeros((G, 2), dtype=torch.float64, device=p.device)
    sums.index_add_(0, g, torch.stack([ll, se], 1))
    return cnt, cm, sums


def group_sketch(p1, y, g, G, thr, flip=False, nb=1 << 18, max_bytes=1 << 30, max_blocks=None,
                 out=None) -> SketchResult:
    """The sketch of the module docstring for p1 [n] (f32 or f64, read as it
    is: no f64 copy), y [n] and g [n] integer codes.

    G          number of groups; ids outside [0, G) are skipped
    max_bytes  the most bytes of `cnt` one launch covers: when G * 2 * nb * 8
               exceeds it the groups go in ranges, one launch each, every
               launch filling its slice of the outputs.  It bounds what one
               launch addresses, not the allocation: the whole [G, 2, nb]
               i64 `cnt` (4 MiB per group at nb = 2^18) is one tensor, and a
               G whose counts the device cannot allocate is a ValueError
    max_blocks cap on the blocks of a launch (None: the kernel's own)
    out        (cnt, cm, sums) to accumulate into instead of fresh zeros:
               contiguous tensors of the result's shapes and dtypes on p1's
               device

    On a GPU: group_sketch_kernel (csrc/fairness.hip).  CPU tensors take
    `group_sketch_torch`; the result then says why."""
    G, nb = int(G), int(nb)
    p1, y, g = _check(p1, y, g, G, nb)
    dev = p1.device
    if out is not None:
        cnt, cm, sums = out
        for t, shape, dt in ((cnt, (G, 2, nb), torch.int64), (cm, (G, 4), torch.int64),
                             (sums, (G, 2), torch.float64)):
            if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError(f"group_sketch: out needs a contiguous {dt} tensor of shape {shape} on {dev}")
    if dev.type != "cuda":
        res = group_sketch_torch(p1, y, g, G, thr, flip, nb)
        if out is not None:
            for t, r in zip(out, res):
                t += r
            res = out
        return SketchResult(*res, False, "CPU tensors")
    if out is None:
        try:
            cnt = torch.zeros((G, 2, nb), dtype=torch.int64, device=dev)
        except torch.cuda.OutOfMemoryError as e:
            raise ValueError(f"group_sketch: G = {G} groups x 2 x {nb} bins need {G * 2 * nb * 8} bytes for the "
                             f"counts, more than {dev} has free: fewer intersections or a smaller nb") from e
        cm = torch.zeros((G, 4), dtype=torch.int64, device=dev)
        sums = torch.zeros((G, 2), dtype=torch.float64, device=dev)
    n = p1.numel()
    if n == 0 or G == 0:
        return SketchResult(cnt, cm, sums, True, None, 0)
    lib = _lib()
    p1 = p1.contiguous()
    # wider codes are narrowed after the filter, so none wraps into range
    if y.dtype != torch.int32:
        y = torch.where((y == 0) | (y == 1), y, -1)
    if g.dtype != torch.int32:
        g = torch.where((g >= 0) & (g < G), g, -1)
    y = y.to(device=dev, dtype=torch.int32).contiguous()
    g = g.to(device=dev, dtype=torch.int32).contiguous()
    per = max(1, int(max_bytes) // (2 * nb * 8))
    stream = _stream()
    chunks = 0
    for g0 in range(0, G, per):
        gc = min(per, G - g0)
        rc = lib.h2o_group_sketch(_ptr(p1), 1 if p1.dtype == torch.float64 else 0, _ptr(y), _ptr(g), n, nb, g0, gc,
                                  float(thr), 1 if flip else 0, _c_void(cnt.data_ptr() + 8 * g0 * 2 * nb),
                                  _c_void(cm.data_ptr() + 8 * g0 * 4), _c_void(sums.data_ptr() + 8 * g0 * 2),
                                  int(max_blocks) if max_blocks else 0, stream)
        check(rc, "h2o_group_sketch")
        chunks += 1
    return SketchResult(cnt, cm, sums, True, None, chunks)
