"""K-Means kernels (ops/csrc/kmeans.hip) against an independent float64 oracle
at small shapes, exact ties and un-centred data.

Oracle: plain numpy float64 from the f32 values the kernels see, distances as
sum_c (x_ic - c_jc)^2 (no |x|^2 - 2 x.c + |c|^2 expansion), arg-min with the
lowest index on ties; sums / weights / within-SS / changed from a GIVEN
assignment.  Checker: `check_pass` / `check_xv`; every tolerance is derived
from the unit roundoff u = 2^-24 of f32 and the inputs (docstrings below),
none is fitted to what a kernel returns.

Every case runs on the CPU route (`torch`, unmarked) and, on a GPU, on every
device route of cluster_ops.lloyd_pass / cluster_ops.xv that serves its shape.
"""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from h2o3_amd.ops import cluster_ops  # noqa: E402

U = 2.0 ** -24          # unit roundoff of f32 (round to nearest)
U64 = 2.0 ** -53        # unit roundoff of f64: the oracle's own sums and the kernels' f64 partials


# ------------------------------------------------------------------ oracle
def _f64(t):
    """The f32 values a kernel sees, as float64 numpy."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().to(torch.float32).numpy()
    return np.asarray(t, dtype=np.float32).astype(np.float64)


def _i64(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(np.int64)


class Oracle:
    """D[i, j] = sum_c (x_ic - c_jc)^2 in f64, ref = argmin_j D (lowest index
    on ties), and the per-distance error bound of an f32 kernel

        E[i, j] = (P + 8) u (|x_i|^2 + 2 sum_c |x_ic c_jc| + |c_j|^2).

    Derivation.  A kernel forms d2 = fl(xsq + fl(cn - 2 dot)).  dot is an f32
    dot product of P exact f32 products: in any summation order its error
    is at most P u sum|x c| (Higham, Accuracy and Stability, 3.1: gamma_P).
    xsq is an f32 sum of P rounded squares: (P + 1) u |x|^2.  cn is |c|^2 of
    the f64 centres rounded once to f32 (u |c|^2) while the dot product uses
    the centres rounded to f32 (2 u |c|^2 on |c|^2): 3 u |c|^2.  The two
    final additions round once each, at most 2 u (|x|^2 + 2 sum|x c| +
    |c|^2).  Every coefficient is at most P + 8."""

    def __init__(self, X, C):
        X, C = _f64(X), _f64(C)
        self.X, self.C = X, C
        N, P = X.shape
        k = C.shape[0]
        D = np.empty((N, k))
        for j in range(k):
            D[:, j] = ((X - C[j]) ** 2).sum(1)
        self.D = D
        self.ref = D.argmin(1)
        self.E = (P + 8) * U * ((X * X).sum(1)[:, None] + 2.0 * (np.abs(X) @ np.abs(C).T) + (C * C).sum(1)[None, :])

    def clear_share(self):
        """Share of rows whose f64 gap between the closest and the second
        closest centre exceeds E[1st] + E[2nd]: only there does the regret
        check pin the assignment to one centre."""
        N, k = self.D.shape
        if k < 2:
            return 1.0
        o = np.argsort(self.D, axis=1, kind="stable")[:, :2]
        r = np.arange(N)
        gap = self.D[r, o[:, 1]] - self.D[r, o[:, 0]]
        return float((gap > self.E[r, o[:, 0]] + self.E[r, o[:, 1]]).mean())


def stats_from(X, w, assign_old, assign, dmin, k):
    """f64 statistics of a GIVEN assignment and GIVEN per-row distances."""
    X = _f64(X)
    N, P = X.shape
    wd = np.ones(N) if w is None else _f64(w)
    sums = np.zeros((k, P))
    np.add.at(sums, assign, X * wd[:, None])
    weights = np.bincount(assign, weights=wd, minlength=k)
    withinss = np.bincount(assign, weights=wd * np.asarray(dmin, dtype=np.float64), minlength=k)
    changed = 0 if assign_old is None else int((_i64(assign_old) != assign).sum())
    return types.SimpleNamespace(sums=sums, weights=weights, withinss=withinss, changed=changed)


def _ratio(err, bound, what):
    """max err / bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), f"{what}: non-finite result"
    z = bound <= 0
    assert not (err[z] > 0).any(), f"{what}: error {err[z].max() if z.any() else 0} where the bound is exactly 0"
    r = float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0
    i = int(np.argmax(np.where(z, 0, err / np.where(z, 1, bound)))) if err.size else 0
    assert r <= 1.0, f"{what}: error / bound = {r:.4g} (flat index {i}, error {err.flat[i]:.6g}, bound {bound.flat[i]:.6g})"
    return r


def check_pass(X, C, w, assign_old, got_assign, got_dmin, stats, *, xabs_max=None, sums="f32", exact=False,
               orc=None):
    """One Lloyd pass against the oracle; returns the worst error / bound per
    quantity.  X, C, w: what the kernel was given (rounded to f32 here);
    assign_old: the previous assignment (None: none given); stats: an object
    with sums [k, P], weights [k], withinss [k], changed (None: assignment-only
    pass).  sums: "f32" or "fx" (64-bit fixed point, needs xabs_max).
    exact=True (integer lattice: every f32 product and sum is exact) demands
    got == ref and dmin == D with no tolerance.

    Assignment (no row excluded): the kernel's arg-min is exact on its own
    f32 distances d, |d_ij - D_ij| <= E_ij, so d[got] <= d[ref] gives
        regret_i = D[i, got_i] - D[i, ref_i] <= E[i, got_i] + E[i, ref_i].
    dmin: |dmin_i - D[i, got_i]| <= E[i, got_i] + u D[i, got_i] (one more
    rounding where a route stores an f64 distance as f32), dmin >= 0.

    weights, withinss: against f64 sums over the kernel's OWN assignment and
    its OWN dmin.  A cluster of n_c rows sums n_c f32 terms (each product
    w d2 rounded once) with at most n_c - 1 f32 additions per 64-row tile
    before the f64 fold: (n_c + 2) u sum|term|.
    sums, f32 route: the same count ((n_c + 2) u sum_{i in c} |w_i x_ic|):
    one rounding of w x, at most n_c - 1 f32 additions in the private
    copies and their fold.
    sums, fixed point: each term is fl(fl(w x) fx) rounded to an integer:
    2 u |w x| + 0.5 / fx, and 0.5 / fx <= xabs_max 64 ntiles 2^-63 for any
    grid (no workgroup holds more than 64 ntiles rows, and the scale keeps
    a workgroup's |sum| below 2^62): per term 2 u |w x| + xabs_max 64 ntiles 2^-63.
    (Two roundings to nearest err by at most u / (1 + u) each, and
    (1 + u / (1 + u))^2 - 1 < 2 u, so no second-order term is missing.)
    Every sum bound also carries the f64 roundoff of this reference and of
    the kernels' f64 partials, (2 n_c + ntiles + 2) 2^-53 sum|term|.
    Clusters without (weighted) rows have bound 0: exact zeros.
    changed counts every row whose assignment differs from assign_old,
    whatever its weight, exactly."""
    orc = orc or Oracle(X, C)
    Xd, D, E, ref = orc.X, orc.D, orc.E, orc.ref
    N, P = Xd.shape
    k = D.shape[1]
    r = np.arange(N)
    got = _i64(got_assign)
    out = {}
    assert got.shape == (N,) and (got >= 0).all() and (got < k).all(), "assign: index out of range"
    if exact:
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, f"assign: {bad.size} rows differ from the lowest-index arg-min, first row {bad[:1]}"
    regret = D[r, got] - D[r, ref]
    out["regret"] = _ratio(regret, E[r, got] + E[r, ref], "regret")
    if got_dmin is not None:
        dm = np.asarray(got_dmin.detach().cpu().numpy() if isinstance(got_dmin, torch.Tensor) else got_dmin,
                        dtype=np.float64)
        assert (dm >= 0).all(), "dmin: negative distance"
        Dg = D[r, got]
        if exact:
            assert (dm == Dg).all(), "dmin: not exact on the integer lattice"
        out["dmin"] = _ratio(np.abs(dm - Dg), E[r, got] + U * Dg, "dmin")
    if stats is None:
        return out
    assert got_dmin is not None
    want = stats_from(Xd, w, assign_old, got, dm, k)

    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
    assert float(stats.changed) == want.changed, f"changed: {float(stats.changed)} != {want.changed}"
    wd = np.ones(N) if w is None else _f64(w)
    n_c = np.bincount(got, minlength=k).astype(np.float64)
    ntiles = (N + 63) // 64
    f64c = (2 * n_c + ntiles + 2) * U64
    aw = np.bincount(got, weights=np.abs(wd), minlength=k)
    out["weights"] = _ratio(np.abs(host(stats.weights) - want.weights), ((n_c + 2) * U + f64c) * aw, "weights")
    ass = np.bincount(got, weights=np.abs(wd) * dm, minlength=k)
    out["withinss"] = _ratio(np.abs(host(stats.withinss) - want.withinss), ((n_c + 2) * U + f64c) * ass, "withinss")
    asum = np.zeros((k, P))
    np.add.at(asum, got, np.abs(Xd * wd[:, None]))
    if sums == "fx":
        assert xabs_max is not None
        bound = 2 * U * asum + (n_c * (float(xabs_max) * 64 * ntiles * 2.0 ** -63))[:, None] + f64c[:, None] * asum
        bound[n_c == 0] = 0.0
    else:
        bound = ((n_c + 2) * U + f64c)[:, None] * asum
    got_sums = host(stats.sums).reshape(k, P)
    out["sums"] = _ratio(np.abs(got_sums - want.sums), bound, "sums")
    return out


def check_xv(X, V, out):
    """out = X @ V on the f32 matrix cores: |out_ij - ref_ij| <= (P + 2) u
    sum_c |x_ic v_cj| -- P exact products, P - 1 f32 additions in any order
    (gamma_P), and V rounded to f32 is what both sides see."""
    Xd, Vd = _f64(X), _f64(V)
    ref = np.zeros((Xd.shape[0], Vd.shape[1]))
    for c in range(Xd.shape[1]):
        ref += Xd[:, c:c + 1] * Vd[c:c + 1, :]
    bound = (Xd.shape[1] + 2) * U * (np.abs(Xd) @ np.abs(Vd))
    got = np.asarray(out.detach().cpu().numpy() if isinstance(out, torch.Tensor) else out, dtype=np.float64)
    assert got.shape == ref.shape, "xv: shape"
    return {"xv": _ratio(np.abs(got - ref), bound, "xv")}


# ------------------------------------------------------------------ cases
class Case(types.SimpleNamespace):
    pass


def _case(name, N, P, k, kind="random", weights="none", old="none", n_groups=None, idle=False, colscale=False):
    return Case(name=name, N=N, P=P, k=k, kind=kind, weights=weights, old=old, n_groups=n_groups, idle=idle,
                colscale=colscale)


# (P, k): every MAXNV bucket of ka_launch (P16 / 16 -> 2, 3, 4, 5, 6, 7, 8, 12, 16), MAXV 4 / 8 / 16, vpr
# 64 / 128 / 256, P % 16 != 0, lane groups without columns (P = 4, 20); every KT bucket of ka_dispatch
# (2, 4, 6, 8, 12, 16; 1 in xv) and of km_kt (1, 2, 4, 8, 16), on both sides of each bucket edge
_SHAPES = [(4, 1), (4, 2), (4, 15), (4, 256), (16, 16), (16, 17), (16, 193), (20, 32), (20, 33), (20, 129),
           (36, 64), (36, 65), (52, 96), (52, 97), (64, 128), (64, 256), (68, 192), (68, 2), (96, 129), (96, 16),
           (100, 65), (100, 128), (128, 97), (128, 17), (132, 96), (132, 33), (192, 64), (192, 15), (196, 33),
           (196, 64), (256, 32), (256, 1)]
_WEIGHTS = ["none", "zeros", "zero_cluster", "mixed"]
_OLD = ["none", "partly"]

CASES = []
for _i, (_P, _k) in enumerate(_SHAPES):
    CASES.append(_case(f"shape-P{_P}-k{_k}", 300 if _i % 2 else 257, _P, _k, weights=_WEIGHTS[_i % 4],
                       old=_OLD[(_i // 4) % 2]))
# small N: a short only tile, a wave whose second 16-row tile lies past N, workgroups without a tile
for _N in (1, 15, 16, 17, 31, 33, 63, 64, 65, 129):
    CASES.append(_case(f"rows-N{_N}", _N, 20, 33, weights="zeros" if _N > 16 else "none"))
for _N in (1, 17, 65):
    CASES.append(_case(f"rows-k5-N{_N}", _N, 16, 5))
# 36 tiles per workgroup and fewer: two folds of KM_FOLD = 16 tiles of the f32 private sums plus a remainder
for _g in (1, 2, 3):
    CASES.append(_case(f"tiles36-g{_g}", 64 * 35 + 5, 20, 5, weights="mixed", old="partly", n_groups=_g))
# idle workgroups (n_groups = ntiles + 3) contribute exact zeros
CASES.append(_case("idle-groups", 200, 20, 5, weights="zeros", idle=True))
CASES.append(_case("idle-groups-k40", 200, 36, 40, idle=True))
# integer lattice: exact arithmetic, duplicate centres, equidistant rows
CASES.append(_case("lattice-dups", 200, 16, 64, kind="lattice_dups", weights="zeros", old="partly"))
CASES.append(_case("lattice-axes", 120, 16, 32, kind="lattice_axes"))
CASES.append(_case("lattice-axes-P64", 150, 64, 128, kind="lattice_axes", weights="mixed"))
# fixed-point headroom: same-sign data, one cluster, default grid and a single workgroup
CASES.append(_case("headroom", 2245, 4, 1, kind="headroom"))
CASES.append(_case("headroom-g1", 2245, 4, 1, kind="headroom", n_groups=1))
# column scales 1e-3 and 1e3 in one matrix
CASES.append(_case("colscale", 300, 20, 5, weights="mixed", colscale=True))
CASES.append(_case("colscale-k40", 257, 52, 40, colscale=True, old="partly"))
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES) <= 60


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and oracle of a case, built once and shared (never modified)."""
    c = CASE_BY_NAME[name]
    rng = np.random.RandomState(1000 + CASES.index(c))
    N, P, k = c.N, c.P, c.k
    if c.kind == "random":
        C = rng.randn(k, P)
        lab = rng.randint(0, k, N)
        X = np.where((rng.rand(N) < 0.75)[:, None], C[lab] + 0.5 * rng.randn(N, P), rng.randn(N, P))
        if c.colscale:
            s = np.where(np.arange(P) % 2 == 0, 1e-3, 1e3)
            X, C = X * s, C * s
    elif c.kind == "headroom":
        X = np.full((N, P), 3.0)
        C = np.full((k, P), 3.0)
    elif c.kind == "lattice_dups":
        C = rng.randint(-8, 9, (k, P)).astype(np.float64)
        C[9] = C[2]                      # duplicates within one 16-chunk
        C[20] = C[4]                     # across chunks: j, j + 16, j + 48
        C[52] = C[4]
        X = rng.randint(-8, 9, (N, P)).astype(np.float64)
        X[0], X[1], X[2] = C[2], C[4], C[52]
        # rows equidistant from two chosen centres: their midpoint where it is an integer vector
        a, b = C[30].copy(), C[47].copy()
        odd = (a + b) % 2 != 0
        b[odd] += np.where(b[odd] < 8, 1, -1)
        C[47] = b
        X[3] = (a + b) / 2
        X[4] = (C[2] + C[4]) // 2
    elif c.kind == "lattice_axes":
        h = k // 2
        C = np.zeros((k, P))
        for j in range(h):
            C[j, j % P] = 2.0 * (1 + j // P)       # +2 e_i (then +4 e_i, ...)
            C[h + j, j % P] = -2.0 * (1 + j // P)
        X = rng.randint(-3, 4, (N, P)).astype(np.float64)
        X[0] = 0.0                                 # every +-2 e_i at distance 4
        X[1] = 0.0
        X[1, :2] = 1.0                             # equidistant from 2 e_0 and 2 e_1
        X[2] = 0.0
        X[2, P - 1] = 1.0
    else:
        raise AssertionError(c.kind)
    X32 = torch.tensor(X, dtype=torch.float32)
    C64 = torch.tensor(C, dtype=torch.float64)
    orc = Oracle(X32, C64)
    if c.weights == "none":
        w = None
    elif c.weights == "zeros":
        w = rng.rand(N)
        w[::3] = 0.0
    elif c.weights == "zero_cluster":
        w = rng.rand(N) + 0.5
        w[orc.ref == orc.ref[0]] = 0.0             # one non-empty cluster of weight 0
    else:
        w = np.where(rng.rand(N) < 0.5, 1e-3, 1e3)
    w32 = None if w is None else torch.tensor(w, dtype=torch.float32)
    if c.old == "none":
        old = np.full(N, -1)
    else:
        old = orc.ref.copy()
        old[::2] = (old[::2] + 1) % max(k, 2)      # partly equal (k = 1: index 1 never comes back)
    return types.SimpleNamespace(case=c, X=X32, C=C64, w=w32, old=torch.tensor(old, dtype=torch.int32), orc=orc)


def _lattice(c):
    return c.kind.startswith("lattice")


# ------------------------------------------------------------------ routes
ROUTES = ("fused-f32", "fused-fx", "split-wave", "split-lloyd", "assign-only")
LDS_MAX = 160 * 1024


def _wave_fits(P, k):
    """LDS of the wave assignment kernel (ka_dispatch): padded centres + |c|^2."""
    P16, KP = (P + 15) & ~15, ((k + 15) // 16) * 16
    return (KP * (P16 + 4) + KP) * 4 <= LDS_MAX


def _sums_fits(P, k):
    """LDS of kmeans_sums_kernel (km_sums_lds_bytes)."""
    return k * P * 8 + 2 * k * 8 + 2 * 2 * 64 * 4 <= LDS_MAX


def route_serves(route, c, lib):
    """Whether lloyd_pass takes `route` for the case: the library's own k limit
    (h2o_kmeans_max_k) and, for the split path, the two LDS limits."""
    if route == "xv":
        return c.kind == "random" and c.n_groups is None and not c.idle and _wave_fits(c.P, c.k)
    acc = 0 if route == "assign-only" else 1
    if c.k > int(lib.h2o_kmeans_max_k(c.P, acc)):
        return False
    if route.startswith("split"):
        return c.n_groups is None and not c.idle and _sums_fits(c.P, c.k) and \
            (route == "split-lloyd" or _wave_fits(c.P, c.k))
    return True


def _buckets(c):
    kt = (c.k + 15) // 16
    nv = ((c.P + 15) & ~15) // 16
    ka = next(b for b in (1, 2, 4, 6, 8, 12, 16) if kt <= b)
    return dict(ka_kt=max(ka, 2), ka_kt_xv=ka, maxnv=next(b for b in (2, 3, 4, 5, 6, 7, 8, 12, 16) if nv <= b),
                km_kt=next(b for b in (1, 2, 4, 8, 16) if kt <= b), maxv=4 if c.P <= 64 else 8 if c.P <= 128 else 16)


def _kmeans_lib():
    from h2o3_amd.ops import _native
    lib = _native.get_lib("kmeans")
    assert lib is not None, "libkmeans.so is not built"
    return lib


def test_cases_cover_every_dispatch_bucket():
    """Every template bucket of the three dispatch ladders is reached by at
    least one case on each route that can reach it (plain integers; the k
    limits are the library's)."""
    lib = _kmeans_lib()
    hit = {r: {"ka_kt": set(), "maxnv": set(), "km_kt": set(), "maxv": set()} for r in ROUTES + ("xv",)}
    for c in CASES:
        b = _buckets(c)
        for r in ROUTES + ("xv",):
            if not route_serves(r, c, lib):
                continue
            if r in ("split-wave", "xv"):
                hit[r]["ka_kt"].add(b["ka_kt_xv"] if r == "xv" else b["ka_kt"])
                hit[r]["maxnv"].add(b["maxnv"])
            if r != "xv" and r != "split-wave":
                hit[r]["km_kt"].add(b["km_kt"])
                hit[r]["maxv"].add(b["maxv"])
    assert hit["split-wave"]["ka_kt"] == {2, 4, 6, 8, 12, 16}
    assert hit["xv"]["ka_kt"] == {1, 2, 4, 6, 8, 12, 16}
    for r in ("split-wave", "xv"):
        assert hit[r]["maxnv"] == {2, 3, 4, 5, 6, 7, 8, 12, 16}, r
    for r in ("fused-f32", "fused-fx", "split-lloyd", "assign-only"):
        assert hit[r]["km_kt"] == {1, 2, 4, 8, 16}, r
        assert hit[r]["maxv"] == {4, 8, 16}, r
    # both sum layouts of the fused kernel under a scale
    fx = {bool(lib.h2o_kmeans_fused_fixed_point(c.k, c.P)) for c in CASES if route_serves("fused-fx", c, lib)}
    assert fx == {True, False}


def _report(route, name, ratios, share=None):
    print("KM_ORACLE " + json.dumps(dict(route=route, case=name, clear=share, **ratios)))


def run_route(route, ref, dev, monkeypatch):
    """One pass of a case on a route -> (assign, dmin, stats, sums kind, xabs_max)."""
    c = ref.case
    X = ref.X.to(dev)
    w = None if ref.w is None else ref.w.to(dev)
    a = ref.old.clone().to(dev)
    dmin = torch.full((c.N,), -1.0, dtype=torch.float32, device=dev)
    xa, kind, kw = None, "f32", {}
    monkeypatch.delenv("H2O3_KM_ASSIGN", raising=False)
    monkeypatch.setenv("H2O3_KM_SPLIT", "1" if route.startswith("split") else "0")
    if route == "split-lloyd":
        monkeypatch.setenv("H2O3_KM_ASSIGN", "lloyd")
    if route != "torch":
        lib = _kmeans_lib()
        assert cluster_ops.native_ok(X, c.k, route != "assign-only")
        if c.n_groups is not None:
            kw["n_groups"] = c.n_groups
        if c.idle:
            kw["n_groups"] = (c.N + 63) // 64 + 3
        if route in ("fused-fx", "split-wave", "split-lloyd"):
            xa = cluster_ops.abs_bound(X, w)
            kind = "fx" if route != "fused-fx" or lib.h2o_kmeans_fused_fixed_point(c.k, c.P) else "f32"
        if route.startswith("split"):
            assert int(lib.h2o_kmeans_sums_resident_per_cu(c.k, c.P)) >= 1
            if route == "split-wave":
                assert int(lib.h2o_kmeans_assign_resident_per_cu(c.k, c.P, 0)) >= 1
    if route == "assign-only":
        st = cluster_ops.lloyd_pass(X, ref.C, None, a, accumulate=False, dmin=dmin, **kw)
        assert st is None
    else:
        st = cluster_ops.lloyd_pass(X, ref.C, w, a, dmin=dmin, xabs_max=xa, **kw)
    if dev != "cpu":
        torch.cuda.synchronize()
    return a, dmin, st, kind, xa


def _check_route(route, ref, dev, monkeypatch):
    c = ref.case
    if c.kind == "random":
        # the regret check is not vacuous: most rows have an f64 gap between the two closest centres
        # above E[1st] + E[2nd], so only one centre passes there
        assert ref.orc.clear_share() >= 0.9
    a, dmin, st, kind, xa = run_route(route, ref, dev, monkeypatch)
    ratios = check_pass(ref.X, ref.C, ref.w, ref.old, a, dmin, st, xabs_max=xa, sums=kind, exact=_lattice(c),
                        orc=ref.orc)
    _report(route, c.name, ratios, ref.orc.clear_share())
    if st is not None:
        # previous assignment equal to the answer: nothing changes, same statistics
        ref2 = types.SimpleNamespace(**{**ref.__dict__, "old": a.cpu()})
        a2, _, st2, _, _ = run_route(route, ref2, dev, monkeypatch)
        assert bool((a2.cpu() == a.cpu()).all()) and float(st2.changed) == 0
    return a.cpu()


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_torch_route(name, monkeypatch):
    _check_route("torch", reference(name), "cpu", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_device_routes(name, monkeypatch):
    """Every device route that serves the case, each against the oracle; the
    routes agree with each other bit for bit on the assignment."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from h2o3_amd.ops import _native
    ref = reference(name)
    lib = _kmeans_lib()
    got = {}
    for route in ROUTES:
        if route_serves(route, ref.case, lib):
            got[route] = _check_route(route, ref, "cuda", monkeypatch)
    assert "fused-f32" in got and "assign-only" in got
    assert "libkmeans.so" in " ".join(_native.loaded_libs())
    first = got["fused-f32"]
    for route, a in got.items():
        assert bool((a == first).all()), f"{route} and fused-f32 assign differently"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES if route_serves("xv", c, None)])
def test_xv_route(name):
    """cluster_ops.xv (skinny-GEMM mode of kmeans_assign_kernel, KT = 1 included)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ref = reference(name)
    c = ref.case
    assert int(_kmeans_lib().h2o_kmeans_assign_resident_per_cu(c.k, c.P, 1)) >= 1
    V = ref.C.T.contiguous()
    out = cluster_ops.xv(ref.X.cuda(), V.cuda(), min_rows=0)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32, "xv did not run the HIP kernel"
    _report("xv", c.name, check_xv(ref.X, V, out))


# ------------------------------------------------------------------ one-tile wave kernel
ONE_TILE_CASES = ("shape-P36-k64", "shape-P52-k96", "shape-P100-k128", "shape-P68-k192", "shape-P64-k256",
                  "lattice-dups", "rows-N17")


def _one_tile_child():
    """Child process body (H2O3_KM_RT=1 is read once per process): the
    split-wave route on one case per KT in {4, 6, 8, 12, 16}."""
    assert os.environ.get("H2O3_KM_RT") == "1"
    mp = pytest.MonkeyPatch()
    try:
        assert {_buckets(CASE_BY_NAME[n])["ka_kt"] for n in ONE_TILE_CASES} == {4, 6, 8, 12, 16}
        lib = _kmeans_lib()
        for n in ONE_TILE_CASES:
            ref = reference(n)
            assert route_serves("split-wave", ref.case, lib), n
            a = _check_route("split-wave", ref, "cuda", mp)
            b = _check_route("split-lloyd", ref, "cuda", mp)
            assert bool((a == b).all()), n
    finally:
        mp.undo()


@pytest.mark.gpu
def test_one_tile_wave_kernel_in_child_process():
    """kmeans_assign_kernel at KT >= 4 (H2O3_KM_RT=1) through the same checker,
    in one fresh child process."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, H2O3_KM_RT="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-tile-child"], env=env,
                         capture_output=True, text=True, timeout=120)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("KM_ORACLE") >= 2 * len(ONE_TILE_CASES)


# ------------------------------------------------------------------ checker self-test
def _exact_results(ref, assign=None, D=None):
    """What a perfect kernel returns for the case (f64), for a given assignment."""
    orc = ref.orc
    D = orc.D if D is None else D
    assign = orc.ref.copy() if assign is None else assign
    dmin = D[np.arange(len(assign)), assign].copy()
    return assign, dmin, stats_from(ref.X, ref.w, ref.old, assign, dmin, D.shape[1])


def _checked(ref, assign, dmin, st, **kw):
    return check_pass(ref.X, ref.C, ref.w, ref.old, assign, dmin, st, exact=_lattice(ref.case), orc=ref.orc, **kw)


def test_checker_accepts_the_oracle_and_rejects_wrong_results():
    ref = reference("shape-P20-k33")
    orc = ref.orc
    N, k = orc.D.shape
    r = np.arange(N)
    a, dmin, st = _exact_results(ref)
    out = _checked(ref, a, dmin, st)
    assert max(out.values()) <= 1e-6
    # a row moved to its second-closest centre where the gap exceeds the bound
    o = np.argsort(orc.D, axis=1, kind="stable")
    gap = orc.D[r, o[:, 1]] - orc.D[r, o[:, 0]] - orc.E[r, o[:, 0]] - orc.E[r, o[:, 1]]
    i = int(np.argmax(gap > 0))
    assert gap[i] > 0
    a2 = a.copy()
    a2[i] = o[i, 1]
    with pytest.raises(AssertionError, match="regret"):
        _checked(ref, *_exact_results(ref, a2))
    # sums with one row left out / one row in the wrong cluster
    i = int(np.argmax(np.abs(orc.X).min(1) * (1 if ref.w is None else _f64(ref.w))))
    for wrong in (a[i], (a[i] + 1) % k):
        s2 = types.SimpleNamespace(**{**st.__dict__, "sums": st.sums.copy()})
        s2.sums[a[i]] -= orc.X[i] * (1 if ref.w is None else _f64(ref.w)[i])
        if wrong != a[i]:
            s2.sums[wrong] += orc.X[i] * (1 if ref.w is None else _f64(ref.w)[i])
        for kind in ("f32", "fx"):
            with pytest.raises(AssertionError, match="sums"):
                _checked(ref, a, dmin, s2, sums=kind, xabs_max=cluster_ops.abs_bound(ref.X, ref.w))
    # the last real column dropped from the distances
    Dm = Oracle(ref.X[:, :-1], ref.C[:, :-1]).D
    with pytest.raises(AssertionError, match="regret|dmin"):
        _checked(ref, *_exact_results(ref, Dm.argmin(1), Dm))
    # changed off by one
    s2 = types.SimpleNamespace(**{**st.__dict__, "changed": st.changed + 1})
    with pytest.raises(AssertionError, match="changed"):
        _checked(ref, a, dmin, s2)
    # dmin of one row moved by twice its bound (its statistics follow it: only the dmin check can object)
    for sign in (1.0, -1.0):
        i = int(np.argmax(dmin))
        d2 = dmin.copy()
        d2[i] += sign * 2 * (orc.E[i, a[i]] + U * dmin[i])
        with pytest.raises(AssertionError, match="dmin"):
            _checked(ref, a, d2, stats_from(ref.X, ref.w, ref.old, a, d2, k))
    # weights / within-SS of one row lost
    i = int(np.argmax((1 if ref.w is None else _f64(ref.w)) * dmin))
    s2 = types.SimpleNamespace(**{**st.__dict__, "withinss": st.withinss.copy()})
    s2.withinss[a[i]] -= (1 if ref.w is None else _f64(ref.w)[i]) * dmin[i]
    with pytest.raises(AssertionError, match="withinss"):
        _checked(ref, a, dmin, s2)


def test_checker_rejects_a_tie_resolved_to_the_higher_index():
    for name, row, hi in (("lattice-dups", 0, 9), ("lattice-dups", 1, 20), ("lattice-dups", 1, 52),
                          ("lattice-axes", 0, 1), ("lattice-axes", 1, 1)):
        ref = reference(name)
        a, dmin, st = _exact_results(ref)
        _checked(ref, a, dmin, st)
        assert ref.orc.D[row, hi] == ref.orc.D[row, a[row]] and hi > a[row]
        a2 = a.copy()
        a2[row] = hi
        # the distances are equal, so only the exact arg-min rule can object
        with pytest.raises(AssertionError, match="assign"):
            _checked(ref, *_exact_results(ref, a2))


def test_xv_checker_rejects_a_neighbouring_column():
    ref = reference("shape-P20-k33")
    V = ref.C.T.contiguous()
    out = ref.X.double() @ V.to(torch.float32).double()
    assert check_xv(ref.X, V, out)["xv"] <= 1e-6
    bad = out.clone()
    bad[7, 11] = out[7, 12]
    with pytest.raises(AssertionError, match="xv"):
        check_xv(ref.X, V, bad)


def test_lattice_cases_hold_the_ties_they_claim():
    orc = reference("lattice-dups").orc
    assert (orc.D[0, [2, 9]] == 0).all() and (orc.D[1, [4, 20, 52]] == 0).all() and orc.ref[1] == 4
    assert orc.D[3, 30] == orc.D[3, 47]
    orc = reference("lattice-axes").orc
    assert (orc.D[0] == 4).all() and orc.ref[0] == 0
    assert orc.D[1, 0] == orc.D[1, 1] == orc.D[1].min() and orc.ref[1] == 0


# ------------------------------------------------------------------ model: un-centred data
def _lloyd_f64(Xn, cats, L, C0n, C0c, iters):
    """Reference Lloyd iteration in f64: squared euclidean on the numeric
    columns as sum (x - c)^2, 0/1 mismatch on the categorical one, centres =
    mean / most frequent level; stops like the model (fewer than max(1,
    1e-4 N) rows changed, or `iters`)."""
    N = Xn.shape[0]
    Cn, Cc = C0n.copy(), None if cats is None else C0c.copy()
    a = np.full(N, -1)
    for _ in range(iters):
        D = ((Xn[:, None, :] - Cn[None]) ** 2).sum(2)
        if cats is not None:
            D = D + (cats[:, None] != Cc[None, :])
        new = D.argmin(1)
        changed = int((new != a).sum())
        a = new
        for j in range(Cn.shape[0]):
            if (a == j).any():
                Cn[j] = Xn[a == j].mean(0)
                if cats is not None:
                    Cc[j] = np.bincount(cats[a == j], minlength=L).argmax()
        if changed < max(1.0, N * 1e-4):
            break
    return a, Cn, Cc


_MODEL = [("cpu", 0.0, False), ("cpu", 1e3, False), ("cpu", 1e4, False), ("cpu", 1e4, True), ("cpu", 1e6, False)]
_MODEL_PARAMS = [pytest.param(*m, id=f"{m[0]}-off{m[1]:g}{'-cat' if m[2] else ''}") for m in _MODEL] + \
    [pytest.param("cuda", m[1], m[2], id=f"cuda-off{m[1]:g}{'-cat' if m[2] else ''}", marks=pytest.mark.gpu)
     for m in _MODEL]


@pytest.mark.parametrize("dev,off,cat", _MODEL_PARAMS)
def test_model_is_invariant_to_the_data_offset(dev, off, cat, monkeypatch):
    """standardize=False on blobs shifted by `off` in every column: sizes,
    centres, within-SS, totss and predictions equal an f64 Lloyd iteration
    with distances as sum (x - c)^2, whatever the offset."""
    from h2o3_amd.core.frame import H2OFrame
    from h2o3_amd.core.vec import make_enum, make_numeric
    from h2o3_amd.estimators import H2OKMeansEstimator
    from h2o3_amd.parallel import cloud
    if dev == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    if dev == "cpu":
        monkeypatch.setitem(cloud._state, "device", torch.device("cpu"))
    rng = np.random.RandomState(17)
    N, P, k = 4096, 8, 4
    cen = rng.randn(k, P) * 6.0
    lab = rng.randint(0, k, N)
    Xn = cen[lab] + rng.randn(N, P) + off
    cols = [f"x{i}" for i in range(P)]
    cats = None
    levels = ["p", "q", "r"]
    if cat:
        cats = np.where(rng.rand(N) < 0.8, lab % 3, rng.randint(0, 3, N))

    def frame(num, codes):
        # float64 columns: the frame's default f32 storage would quantise 1e6 + x to 1/16 before the
        # model sees it, and the reference below is built from the f64 values
        vecs = [make_numeric(num[:, i], dtype=torch.float64) for i in range(P)]
        if codes is not None:
            vecs.append(make_enum(np.asarray(codes, dtype=np.int32), levels))
        return H2OFrame.from_vecs(vecs, cols + (["g"] if codes is not None else []))
    fr = frame(Xn, cats)
    up = frame(cen + 0.5 + off, None if cats is None else np.arange(k) % 3)
    m = H2OKMeansEstimator(k=k, standardize=False, user_points=up, max_iterations=10)
    m.train(training_frame=fr)
    a, Cn, Cc = _lloyd_f64(Xn, cats, 3, cen + 0.5 + off, None if cats is None else np.arange(k) % 3, 10)
    # metrics: distances of the rows to the final centres, assignment by those centres
    D = ((Xn[:, None, :] - Cn[None]) ** 2).sum(2)
    if cat:
        D = D + (cats[:, None] != Cc[None, :])
    af = D.argmin(1)
    assert m.size() == np.bincount(af, minlength=k).tolist()
    got_c = m.centers()
    names = m._dinfo.x
    num = np.array([[row[names.index(c)] for c in cols] for row in got_c], dtype=np.float64)
    np.testing.assert_allclose(num, Cn, rtol=0, atol=1e-6 * max(1.0, off))
    if cat:
        assert [row[names.index("g")] for row in got_c] == [levels[j] for j in Cc]
    within = np.bincount(af, weights=D[np.arange(N), af], minlength=k)
    np.testing.assert_allclose(m.withinss(), within, rtol=1e-4)
    mu = Xn.mean(0)
    totss = ((Xn - mu) ** 2).sum()
    if cat:
        totss += (cats != np.bincount(cats, minlength=3).argmax()).sum()
    np.testing.assert_allclose(m.totss(), totss, rtol=1e-5)
    np.testing.assert_allclose(m.betweenss(), m.totss() - m.tot_withinss(), rtol=1e-9)
    pred = m.predict(fr).as_data_frame()["predict"].values
    assert (pred == af).all()
    # centers_std stays in the space of the raw inputs
    cs = np.array(m.centers_std())[:, m._dinfo.n_cat_expanded:]
    np.testing.assert_allclose(cs, Cn, rtol=0, atol=1e-6 * max(1.0, off))


if __name__ == "__main__" and "--one-tile-child" in sys.argv:
    _one_tile_child()
