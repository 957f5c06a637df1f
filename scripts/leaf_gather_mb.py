"""Microbenchmark: leaf gather (lg_*_kernel) against leaf_scatter_kernel.

Builds the end state of a synthetic tree on the GPU -- a stable partition of
N rows into 2^D leaves (every leaf's rows ascending), and the same tree with
the last level left uncompacted (level-(D-1) order + go-left flag words) --
and times, with device events, the scatter, the gather on the compacted
layout and the gather on the uncompacted layout, for a sweep of the gather's
rows per workgroup R.  Useful bytes: 4 N of ridx in, 4 N of dbuf out.

    python scripts/leaf_gather_mb.py [--rows 100000000,12500000] [--depths 8,11]
                                     [--R 2048,4096,8192,16384] [--iters 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from h2o3_amd.models.tree import devtree  # noqa: E402

RS, OK, ST, CT = devtree.RS, devtree.OK, devtree.ST, devtree.CT


def build(N, D, skew, seed=0):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nl = 1 << D
    leaf = torch.randint(0, nl, (N,), device=dev, generator=g, dtype=torch.int32)
    if skew:   # one leaf holds 90 % of the rows
        leaf = torch.where(torch.rand(N, device=dev, generator=g) < 0.9, torch.full_like(leaf, nl // 3), leaf)
    cnt = torch.bincount(leaf, minlength=nl).cpu().numpy().astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    nh = (1 << (D + 1)) - 1
    rec = np.zeros((nh, RS))
    first = nl - 1
    rec[first:, ST], rec[first:, CT] = start, cnt
    for h in range(first - 1, -1, -1):
        rec[h, OK] = 1.0
        rec[h, ST] = rec[2 * h + 1, ST]
        rec[h, CT] = rec[2 * h + 1, CT] + rec[2 * h + 2, CT]
    ridx_c = torch.argsort(leaf, stable=True).to(torch.int32)
    par = leaf >> 1
    ridx_u = torch.argsort(par, stable=True).to(torch.int32)
    # flag words of level D-1: slot i's words start at wb[i]; bit q % 64 of word q / 64 = row q goes left
    p0 = (1 << (D - 1)) - 1
    pc = rec[p0:first, CT].astype(np.int64)
    ps = rec[p0:first, ST].astype(np.int64)
    wb = np.concatenate([[0], np.cumsum((pc + 63) // 64)[:-1]])
    lu = leaf[ridx_u.long()]
    slot = (lu >> 1).long()
    q = torch.arange(N, device=dev) - torch.from_numpy(ps).to(dev)[slot]
    word = torch.from_numpy(wb).to(dev)[slot] + (q >> 6)
    bit = ((lu & 1) == 0).long() << (q & 63)
    flags = torch.zeros(N // 64 + nl + 2, dtype=torch.int64, device=dev)
    flags.index_add_(0, word, bit)
    del lu, slot, q, word, bit, par, leaf
    vals = torch.randn(nh, device=dev)
    return dict(rec=torch.from_numpy(rec.reshape(-1).copy()).to(dev), ridx_c=ridx_c, ridx_u=ridx_u, flags=flags,
                slot_wb=torch.from_numpy(wb.astype(np.int32)).to(dev), vals=vals, nh=nh)


def timed(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000000,12500000")
    ap.add_argument("--depths", default="8,11")
    ap.add_argument("--R", default="2048,4096,8192,16384")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    lh, _ = devtree._libs()
    P, ck = devtree._ptr, devtree._ck
    for N in [int(x) for x in a.rows.split(",")]:
        for D in [int(x) for x in a.depths.split(",")]:
            for skew in (0, 1):
                c = build(N, D, skew)
                nh = c["nh"]
                gb = 8.0 * N / 1e9
                cap_l = nh + N // 65536 + 1
                lwork = torch.zeros(cap_l * 4, dtype=torch.int32, device="cuda")
                counts = torch.zeros(2, dtype=torch.int32, device="cuda")
                d_s = torch.zeros(N, device="cuda")
                ck(lh.h2o_dt_items(2, P(c["rec"]), nh, D, 0, 65536, cap_l, P(lwork), None, P(counts),
                                   devtree._stream()), "dt_items")

                def scatter():
                    ck(lh.h2o_leaf_scatter_dev(P(c["ridx_c"]), P(lwork), cap_l, P(c["vals"]), P(d_s), P(counts),
                                               devtree._stream()), "scatter")
                med, mn = timed(scatter, a.iters)
                tag = f"rows={N} leaves={1 << D} skew={skew}"
                print(f"{tag} scatter            ms={med:.3f} min={mn:.3f} useful_TBps={gb / med:.2f}", flush=True)
                for R in [int(x) for x in a.R.split(",")]:
                    lg = devtree.LeafGather(lh, N, D, torch.device("cuda"), R=R)
                    for last in (0, 1):
                        d_g = torch.full((N,), -7.0, device="cuda")
                        if last:
                            fn = lambda: lg.run(c["rec"], c["ridx_u"], c["vals"], d_g, c["flags"], c["slot_wb"])  # noqa
                        else:
                            fn = lambda: lg.run(c["rec"], c["ridx_c"], c["vals"], d_g)  # noqa
                        med, mn = timed(fn, a.iters)
                        same = bool(torch.equal(d_g, d_s))
                        print(f"{tag} gather R={R:<5d} last={last} ms={med:.3f} min={mn:.3f} "
                              f"useful_TBps={gb / med:.2f} equal={same}", flush=True)
                        del d_g
                    del lg
                del c, d_s
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
