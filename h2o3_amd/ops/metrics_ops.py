"""Aggregations on the HIP kernels of ops/csrc/metrics.hip: the binomial
logit histogram plus the logloss / MSE / response sums in one pass, and
grouped f64 sums, both with wave-aggregated atomics (hex/AUC2.java AUCBuilder, ModelMetricsBinomial
MetricBuilderBinomial)."""
from __future__ import annotations


import torch

from . import _native
from ._native import check as _check, ptr as _ptr, stream as _stream


def _lib():
    return _native.get_lib("metrics", required=False)


def available(t) -> bool:
    return t.is_cuda and _lib() is not None


def logit_hist(y, p1, w, nb):
    """One f64 buffer [2 nb + 5] = (positive bins, negative bins, sum w,
    sum w*logloss, sum w*(y-p)^2, sum w*y, row count) over the rows where
    neither y nor p1 is NaN.  Not yet reduced over ranks."""
    lib = _lib()
    if lib is None:
        raise RuntimeError("metrics HIP library missing")
    n = p1.numel()
    p1 = p1.reshape(-1).to(torch.float64).contiguous()
    y = y.reshape(-1).to(device=p1.device, dtype=torch.float64).contiguous()
    if y.numel() != n or (w is not None and w.numel() != n):
        raise ValueError("logit_hist: y / p1 / w lengths differ")
    w = None if w is None else w.reshape(-1).to(device=p1.device, dtype=torch.float64).contiguous()
    buf = torch.zeros(2 * nb + 5, dtype=torch.float64, device=p1.device)
    _check(lib.h2o_logit_hist(_ptr(p1), _ptr(y), _ptr(w), n, nb, _ptr(buf), _ptr(buf[2 * nb:]), _stream()),
           "h2o_logit_hist")
    return buf


_OPS = {"sum": (0, 0.0), "min": (1, float("inf")), "max": (2, float("-inf"))}


def group_reduce(idx, vals, nbins, op="sum"):
    """f64 [nbins, C] sums / minima / maxima of vals [n, C] by idx (rows
    outside [0, nbins) skipped; empty groups hold 0 / +inf / -inf), on the
    device."""
    lib = _lib()
    if lib is None:
        raise RuntimeError("metrics HIP library missing")
    code, fill = _OPS[op]
    v = vals.to(torch.float64).contiguous()
    idx = idx.reshape(-1).to(device=v.device, dtype=torch.int64).contiguous()
    n, C = v.shape
    if idx.numel() != n:
        raise ValueError("group_reduce: idx / vals lengths differ")
    out = torch.full((nbins, C), fill, dtype=torch.float64, device=v.device)
    if n == 0 or nbins == 0 or C == 0:
        return out
    _check(lib.h2o_group_reduce(_ptr(idx), _ptr(v), n, C, nbins, code, _ptr(out), _stream()), "h2o_group_reduce")
    return out


def group_sum(idx, vals, nbins):
    return group_reduce(idx, vals, nbins, "sum")
