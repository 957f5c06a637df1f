"""Exact oracle, derived error bound and case table for the histogram kernels
of ops/csrc/tree_hist.hip (hist_bm_kernel + hist_bm_reduce_kernel,
hist_quad_kernel, hist_build_kernel flat and packed, child_work_kernel).

Inputs never pass through binning: a case is a plain numpy code matrix
codes[n, F] with integers in [0, Bs), a row permutation, segments and fp32
payloads.  `make_bd` lays the matrix out the way bin_frame_tensors documents
it ([n, Fp] row-major, uint8 / int16, Fp a multiple of 16 bytes and of 128
bytes once wider than 64, padding columns = NA code Bs - 1); the oracle reads
the numpy matrix only.

Oracle.  `hist_oracle` sums the exact float64 values of the fp32 inputs with
numpy only.  A float64 bincount of n terms would itself err by up to
n 2^-53 sum|v|, more than the kernels are allowed, so every value is split
as v = hi + lo with hi on a grid of 2^-26 times the channel's power-of-two
ceiling: the hi sums are exact in float64 (n < 2^13 terms of 27 bits), the lo
sums carry at most n^2 2^-80 of the ceiling, and one final add rounds once.

Bound (entrywise, `bound`), derived from the number formats and the launch
geometry, never from a kernel's output:
  N * 0.5 / s_floor     one round-to-nearest per non-zero row entry at the
                        fixed-point scale s >= s_floor;
  2^-24 * sum|w*y|      channel 1 of mode 0 with a weight vector whose fp32
                        product w*y is inexact (the kernels form it in fp32);
  2^-50 * sum|v|        integer -> double conversions and the f64 adds across
                        work items.
s_floor comes from chunk (tree_ops.hist_plan) and the vmax handed to the
kernel: unpacked s >= 2^61 / (vmax chunk) (the largest power of two with
chunk values of vmax below 2^62 is more than half of 2^62 / (vmax chunk));
packed response s1 >= 2^37 / (vmax chunk) (chunk (2 bq + 1) < 2^40 with one
bit of floor).  A channel is compared with EQUALITY (`exact`) when every row
entry is an integer at s_floor and all integer sums fit 53 bits: then no step
of a correct kernel rounds.  Packed counts are always exact.

The per-slot sum of w*y*y is returned exactly; `wyy_tol` is 2^-40 relative,
plus 2^-24 sum|w*y*y| only where a weight vector makes the fp32 product w*y
inexact (the kernels multiply that fp32 channel value by y in f64, the same
term the histogram bound grants channel 1).

NaN responses: the bin-major and grouped-lane kernels take a NaN response as
a zero-weight row (the engine hands them NaN-masked payloads); the flat /
packed wide-code kernel is never given one, so those layouts carry no NaN.
"""
import math
import types
from functools import lru_cache

import numpy as np
import torch

from h2o3_amd.ops import tree_ops

CHUNK = 2048
# segments over a random permutation: 1, chunk - 1, chunk, chunk + 1 rows, an
# empty segment, two and five work items, and a segment of zero-weight rows;
# starts 1, 6145, 10241 and 19241 are odd
SEG_COUNTS = [1, 2047, 2048, 2049, 0, 4096, 9000, 300]
SEG_STARTS = [int(x) for x in np.cumsum([0] + SEG_COUNTS[:-1])]
N_ROWS = int(sum(SEG_COUNTS))
ZERO_SEG = len(SEG_COUNTS) - 1
HIST_ENV = ("H2O3_HIST_BM", "H2O3_HIST_KERNEL", "H2O3_HIST_PACK", "H2O3_HIST_BIG", "H2O3_HIST_TB",
            "H2O3_HIST_CHUNK", "H2O3_HIST_FGL", "H2O3_HIST_FGW", "H2O3_HIST_BM_RAGGED", "H2O3_HIST_BM_RED",
            "H2O3_HIST_BM_LW", "H2O3_HIST_LW")


def set_env(monkeypatch, env):
    for k in HIST_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def channels(mode):
    return 1 if mode == 2 else 2


def padded_width(F, code_bytes):
    align = 16 // code_bytes
    Fp = -(-F // align) * align
    if Fp * code_bytes > 64:
        Fp = -(-(Fp * code_bytes) // 128) * 128 // code_bytes
    return Fp


def make_bd(codes, Bs, code_bytes, dev="cpu"):
    n, F = codes.shape
    Fp = padded_width(F, code_bytes)
    full = np.full((n, Fp), Bs - 1, dtype=np.uint8 if code_bytes == 1 else np.int16)
    full[:, :F] = codes
    return types.SimpleNamespace(F=F, Fp=Fp, Bs=Bs, code_bytes=code_bytes, codes=torch.from_numpy(full).to(dev),
                                 codes_col=None, nrows_local=n)


# --------------------------------------------------------------------------- oracle
def _rows(ridx, va, vb, mode, st, ct, posv):
    """(rows, channel values [C][m] f64, y f64 or None) of the rows of one segment that contribute."""
    pos = np.arange(st, st + ct)
    r = ridx[pos].astype(np.int64)
    vi = pos if posv else r
    f64 = np.float64
    if mode == 0:
        y = va[vi].astype(f64)
        w = (~np.isnan(y)).astype(f64) if vb is None else vb[vi].astype(f64)
        keep = w != 0
        r, w, y = r[keep], w[keep], y[keep]
        return r, [w, w * y], y
    if mode == 1:
        return r, [va[vi].astype(f64), vb[vi].astype(f64)], None
    w = np.ones(ct, f64) if vb is None else vb[vi].astype(f64)
    return r[w != 0], [w[w != 0]], None


def _exact_bincount(idx, v, size):
    """sum of v per index, exact up to one final rounding (see the module docstring)."""
    m = float(np.max(np.abs(v))) if v.size else 0.0
    if m == 0.0:
        return np.zeros(size)
    g = 2.0 ** (math.ceil(math.log2(m)) - 26)
    hi = np.rint(v / g) * g
    return np.bincount(idx, weights=hi, minlength=size) + np.bincount(idx, weights=v - hi, minlength=size)


class Oracle(types.SimpleNamespace):
    """H, A = sum|v|, N = non-zero row entries: [F, n_slots, Bs, C]; wyy, wyy_abs: [n_slots];
    inexact_prod: some fp32 product w*y of mode 0 is inexact."""


def hist_oracle(codes, ridx, va, vb, mode, starts, counts, Bs, posv):
    n, F = codes.shape
    S, C = len(starts), channels(mode)
    H = np.zeros((F, S, Bs, C))
    A = np.zeros((F, S, Bs, C))
    N = np.zeros((F, S, Bs, C))
    wyy = np.zeros(S)
    wyy_abs = np.zeros(S)
    inexact = False
    foff = (np.arange(F, dtype=np.int64) * Bs)[None, :]
    for s, (st, ct) in enumerate(zip(starts, counts)):
        if ct <= 0:
            continue
        r, ch, y = _rows(ridx, va, vb, mode, st, ct, posv)
        if r.size == 0:
            continue
        idx = (codes[r].astype(np.int64) + foff).reshape(-1)
        for c, v in enumerate(ch):
            vv = np.repeat(v, F)
            H[:, s, :, c] = _exact_bincount(idx, vv, F * Bs).reshape(F, Bs)
            A[:, s, :, c] = _exact_bincount(idx, np.abs(vv), F * Bs).reshape(F, Bs)
            N[:, s, :, c] = np.bincount(idx, weights=(vv != 0).astype(np.float64), minlength=F * Bs).reshape(F, Bs)
        if mode == 0:
            t = ch[1] * y
            wyy[s] = _exact_bincount(np.zeros(t.size, np.int64), t, 1)[0]
            wyy_abs[s] = np.abs(t).sum()
            inexact = inexact or bool(np.any(ch[1].astype(np.float32).astype(np.float64) != ch[1]))
    return Oracle(H=H, A=A, N=N, wyy=wyy, wyy_abs=wyy_abs, inexact_prod=inexact)


def s_floor(vmax, chunk, pack):
    """Least fixed-point scales (s0, s1) a correct launch may use, from the geometry alone."""
    f = [2.0 ** 61 / (max(v, 1e-30) * chunk) for v in vmax]
    if pack:
        f[1] = 2.0 ** 37 / (max(vmax[1], 1e-30) * chunk)
    return f


def bound(orc, mode, sf, pack, has_w):
    C = channels(mode)
    b = np.zeros_like(orc.H)
    for c in range(C):
        b[..., c] = orc.N[..., c] * 0.5 / sf[c] + 2.0 ** -50 * orc.A[..., c]
    if mode == 0 and has_w and orc.inexact_prod:
        b[..., 1] += 2.0 ** -24 * orc.A[..., 1]
    if pack:
        b[..., 0] = 0.0
    return b


def wyy_tol(orc, has_w):
    t = 2.0 ** -40 * np.abs(orc.wyy)
    if has_w and orc.inexact_prod:
        t = t + 2.0 ** -24 * orc.wyy_abs
    return t


def _low_bit(v):
    """Exponent of the lowest set bit over the non-zero entries of v (f64), or None."""
    v = v[v != 0]
    if v.size == 0:
        return None
    m, e = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(mi.shape, np.int64)
    for k in (32, 16, 8, 4, 2, 1):
        z = (mi & ((1 << k) - 1)) == 0
        tz += np.where(z, k, 0)
        mi = np.where(z, mi >> k, mi)
    return int(np.min(e.astype(np.int64) - 53 + tz))


# --------------------------------------------------------------------------- cases
# name -> F, Bs, code_bytes, mode, unit_w, env, expected (kernel, width, pack).  The widths follow
# tree_ops.bm_groups / quad_groups / feature_group by hand: F = 37 pads to Fp = 48, two groups of 32
# would read past the row, so its two-channel layout is 3 x 16; F = 100 (Fp 128) gives 4 x 32.
_Q = {"H2O3_HIST_BM": "0"}
LAYOUTS = {
    "bm64_pack_F65": (65, 256, 1, 0, True, {}, ("bm", 64, True)),
    "bm64_pack_F100": (100, 256, 1, 0, True, {}, ("bm", 64, True)),
    "bm64_pack_F128": (128, 256, 1, 0, True, {}, ("bm", 64, True)),
    "bm64_pack_Bs20_F65": (65, 20, 1, 0, True, {}, ("bm", 64, True)),
    "bm64_m2_F65": (65, 256, 1, 2, False, {}, ("bm", 64, False)),
    "bm64_m2_F100": (100, 256, 1, 2, False, {}, ("bm", 64, False)),
    "bm64_m2_F128": (128, 256, 1, 2, False, {}, ("bm", 64, False)),
    "bm32_m0_F100": (100, 256, 1, 0, False, {}, ("bm", 32, False)),
    "bm32_m1_F100": (100, 256, 1, 1, False, {}, ("bm", 32, False)),
    "bm16_m0_F37": (37, 256, 1, 0, False, {}, ("bm", 16, False)),
    "bm16_m1_F37": (37, 256, 1, 1, False, {}, ("bm", 16, False)),
    "bm16_m0_F13": (13, 256, 1, 0, False, {}, ("bm", 16, False)),
    "bm16_pack_F13": (13, 256, 1, 0, True, {}, ("bm", 16, True)),
    "quad_pack_F100": (100, 256, 1, 0, True, _Q, ("quad", 36, True)),
    "quad_m0_F100": (100, 256, 1, 0, False, _Q, ("quad", 16, False)),
    "quad_m1_Bs20_F37": (37, 20, 1, 1, False, _Q, ("quad", 40, False)),
    "quad_pack_Bs8_F13": (13, 8, 1, 0, True, _Q, ("quad", 16, True)),
    "quad_m2_Bs8_F13": (13, 8, 1, 2, False, _Q, ("quad", 16, False)),
    "pk_Bs304_F70": (70, 304, 2, 0, True, {}, ("pk", 14, True)),
    "flat2_m1_Bs304_F70": (70, 304, 2, 1, False, {}, ("flat", 14, False)),
    "flat1_m0_F37": (37, 256, 1, 0, False, {"H2O3_HIST_KERNEL": "old"}, ("flat", 19, False)),
}
# one sweep of the launch switches per bin-major / grouped-lane layout
_BM_ENVS = [{"H2O3_HIST_BM_RED": "0"}, {"H2O3_HIST_BM_LW": "1"}, {"H2O3_HIST_BM_RAGGED": "1"},
            {"H2O3_HIST_BM_RED": "0", "H2O3_HIST_BM_LW": "1"}, {"H2O3_HIST_BM_RED": "0", "H2O3_HIST_BM_RAGGED": "1"}]
_QUAD_ENVS = [{"H2O3_HIST_LW": "2"}]

# (payload, weights, posv) per kind of layout.  Mode 1: (payload of g, payload of h, posv); mode 2:
# the payload is the weight vector itself.
_V_PACK = [("+max1", "none", 0), ("+max4", "w01", 0), ("+max.25", "nan", 0), ("-max", "none", 0), ("alt", "w01", 0),
           ("below", "none", 0), ("outlier", "nan", 0), ("randn", "none", 0), ("randn", "nan", 0), ("randn", "w01", 0),
           ("grid34", "none", 0), ("randn", "w01", 1), ("+max1", "nan", 1)]
_V_M0 = [("+max1", "ones", 0), ("+max4", "twos", 0), ("+max.25", "none", 0), ("-max", "ones", 0), ("-max", "twos", 0),
         ("alt", "quarter", 0), ("below", "ones", 0), ("outlier", "rand", 0), ("randn", "rand", 0), ("randn", "nan", 0),
         ("randn", "quarter", 0), ("grid34", "ones", 0), ("grid34", "none", 0), ("randn", "rand", 1),
         ("+max1", "twos", 1)]
_V_M1 = [("+max1", "+max4", 0), ("-max", "-max", 0), ("+max.25", "-max", 0), ("alt", "alt", 0), ("below", "+max.25", 0),
         ("outlier", "randn", 0), ("randn", "randn", 0), ("grid34", "grid34", 0), ("randn", "outlier", 1),
         ("+max1", "-max", 1)]
_V_M2 = [("+max1", None, 0), ("+max4", None, 0), ("+max.25", None, 0), ("-max", None, 0), ("alt", None, 0),
         ("below", None, 0), ("outlier", None, 0), ("rand", None, 0), ("quarter", None, 0), ("grid34", None, 0),
         ("none", None, 0), ("rand", None, 1), ("+max1", None, 1)]


# layouts that differ from a fully swept one in F or Bs only: the edge payload, a random one, one
# position-ordered, and the switches
_LITE = {"bm64_pack_F65", "bm64_pack_F128", "bm64_m2_F65", "bm64_m2_F128", "bm64_pack_Bs20_F65", "bm16_m1_F37",
         "bm16_pack_F13"}


def _first_random(var):
    return [v for v in var if v[0] in ("randn", "rand")][0]


def _case_table():
    t = {}
    for lname, (F, Bs, cb, mode, unit_w, env, expect) in LAYOUTS.items():
        var = _V_PACK if expect[2] else _V_M0 if mode == 0 else _V_M1 if mode == 1 else _V_M2
        nan_ok = expect[0] in ("bm", "quad")
        k = 0
        if lname in _LITE:
            var = [var[0], _first_random(var), var[-1]]
        for a, b, posv in var:
            if b == "nan" and not nan_ok:
                b = "none"
            t[f"{lname}-{a}-{b}-{'pos' if posv else 'row'}"] = (lname, a, b, posv, env, k % 5, False)
            k += 1
        envs = _BM_ENVS if expect[0] == "bm" else _QUAD_ENVS if expect[0] == "quad" else []
        # the switches run on the reduce-edge payload and on a random one
        for e in envs:
            tag = ",".join(f"{x[10:]}={y}" for x, y in e.items())
            for a, b, posv in (var[0], _first_random(var)):
                t[f"{lname}-{a}-{b}-{tag}"] = (lname, a, b, posv, dict(env, **e), k % 5, False)
                k += 1
    for lname in ("bm64_pack_F100", "quad_m0_F100"):
        a, b, posv = ("randn", "w01", 0) if LAYOUTS[lname][4] else ("randn", "rand", 0)
        t[f"{lname}-{a}-{b}-need"] = (lname, a, b, posv, LAYOUTS[lname][5], 0, True)
    return t


CASES = _case_table()
# unpacked layouts on the reduce edge: every row of a node in one bin at the channel maximum
EDGE_CASES = sorted(n for n, c in CASES.items() if not LAYOUTS[c[0]][6][2] and c[1] in ("+max1", "+max4", "+max.25")
                    and not c[6])
PACK_MAX_CASES = sorted(n for n, c in CASES.items() if LAYOUTS[c[0]][6][2] and c[1].startswith("+max"))


def _adversarial_columns(F, width):
    cols = {0, F - 1}
    for g in range(width, F, width):
        cols.update((g - 1, g))
    return sorted(cols)


def _codes(F, Bs, width, rot, rng):
    """Random codes; constant / two-valued / ramp columns at features 0, F - 1 and both sides of every
    group border, the five distributions rotated over those columns by `rot`."""
    n = N_ROWS
    codes = rng.integers(0, Bs, size=(n, F), dtype=np.int64)
    row = np.arange(n)
    dist = [np.zeros(n, np.int64), np.full(n, Bs - 2), np.full(n, Bs - 1), np.where(row % 2 == 0, 0, Bs - 2),
            row % (Bs - 1)]
    for i, c in enumerate(_adversarial_columns(F, width)):
        codes[:, c] = dist[(i + rot) % 5]
    return codes


def _grid(vmax, pack):
    """0.75 steps of the one power-of-two scale in [s_floor, 2 s_floor): round-to-nearest errs by a
    quarter step per row, truncation by three quarters, and vmax = 1.0625 keeps s within 1.07 s_floor."""
    sf = (2.0 ** 37 if pack else 2.0 ** 61) / (vmax * CHUNK)
    return 0.75 / 2.0 ** math.ceil(math.log2(sf))


def _payload(kind, rng, pack, wmax=1.0):
    """(values f32 [n] in row order, nominal channel maximum or None = take the data's)."""
    n = N_ROWS
    row = np.arange(n)
    f32 = np.float32
    if kind.startswith("+max"):
        m = float(kind[4:])
        return np.full(n, m, f32), m
    if kind == "-max":
        return np.full(n, -1.0, f32), 1.0
    if kind == "alt":
        return np.where(row % 2 == 0, 1.0, -1.0).astype(f32), 1.0
    if kind == "below":
        return np.full(n, np.nextafter(f32(1.0), f32(0.0)), f32), 1.0
    if kind == "outlier":
        v = (1e-3 * (0.5 + rng.random(n))).astype(f32)
        v[n // 2] = 2.0 ** 20
        return v, 2.0 ** 20
    if kind == "grid34":
        v = np.full(n, _grid(1.0625 * wmax, pack) / wmax, f32)
        v[n // 2] = 1.0625
        return v, 1.0625
    if kind == "randn":
        return rng.standard_normal(n).astype(f32), None
    if kind == "rand":
        return rng.random(n).astype(f32), None
    if kind == "quarter":
        return (rng.integers(0, 9, n) / 4.0).astype(f32), 2.0
    raise KeyError(kind)


def _weights(kind, rng):
    n = N_ROWS
    if kind in ("none", "nan"):
        return None
    if kind == "w01":
        return (rng.random(n) < 0.7).astype(np.float32)
    if kind == "ones":
        return np.ones(n, np.float32)
    if kind == "twos":
        return np.full(n, 2.0, np.float32)
    if kind == "quarter":
        return (rng.integers(0, 9, n) / 4.0).astype(np.float32)
    if kind == "rand":
        return rng.random(n).astype(np.float32)
    raise KeyError(kind)


@lru_cache(maxsize=4)
def build(name):
    """The inputs of one case: codes [n, F], ridx, va / vb as handed to hist_build (row or position
    order), vmax, segments, need_mask."""
    lname, a, b, posv, env, rot, need = CASES[name]
    F, Bs, cb, mode, unit_w, _, expect = LAYOUTS[lname]
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    rng = np.random.default_rng(seed)
    n = N_ROWS
    codes = _codes(F, Bs, expect[1], rot, rng)
    ridx = rng.permutation(n).astype(np.int32)
    zrows = ridx[SEG_STARTS[ZERO_SEG]: SEG_STARTS[ZERO_SEG] + SEG_COUNTS[ZERO_SEG]]
    pack = expect[2]
    if mode == 0:
        vb = _weights(b, rng)
        wmax = 1.0 if vb is None else float(np.max(np.abs(vb)))
        va, ym = _payload(a, rng, pack, wmax)
        if vb is not None:
            vb[zrows] = 0.0
            if b == "w01" and expect[0] in ("bm", "quad"):
                va[vb == 0] = np.nan            # the engine's NaN-masked response under a 0/1 vector
        if b == "nan":
            va[rng.random(n) < 0.1] = np.nan
            va[zrows] = np.nan
        prod = np.abs((va if vb is None else va * vb)[~np.isnan(va)].astype(np.float64))
        m1 = float(prod.max()) if prod.size else 0.0
        vmax = [wmax, max(m1, ym * wmax) if ym is not None else m1]
    elif mode == 1:
        va, m0 = _payload(a, rng, pack)
        vb, m1 = _payload(b, rng, pack)
        va[zrows] = 0.0
        vb[zrows] = 0.0
        vmax = [m0 if m0 is not None else float(np.abs(va).max()), m1 if m1 is not None else float(np.abs(vb).max())]
    else:
        va = np.zeros(n, np.float32)
        if a == "none":
            vb, vmax = None, [1.0, 1.0]
        else:
            vb, m0 = _payload(a, rng, pack)
            vb[zrows] = 0.0
            m0 = m0 if m0 is not None else float(np.abs(vb).max())
            vmax = [m0, m0]
    if posv:
        va = va[ridx]
        vb = None if vb is None else vb[ridx]
    need_mask = None
    if need:
        # one needed feature in every other group, the groups alternating with the slot
        S, width = len(SEG_COUNTS), expect[1]
        need_mask = np.zeros((S, F), bool)
        for s in range(S):
            for g in range(-(-F // width)):
                if (s + g) % 2 == 0:
                    need_mask[s, min(F - 1, g * width + (3 * s) % width)] = True
    return types.SimpleNamespace(name=name, layout=lname, F=F, Bs=Bs, code_bytes=cb, mode=mode, unit_w=unit_w,
                                 env=env, expect=expect, codes=codes, ridx=ridx, va=va, vb=vb, vmax=vmax,
                                 posv=bool(posv), starts=SEG_STARTS, counts=SEG_COUNTS, need_mask=need_mask,
                                 has_w=mode == 0 and vb is not None)


def plan_of(case):
    """The launch plan hist_build takes for the case (its environment switches must be set)."""
    bd = make_bd(case.codes[:8], case.Bs, case.code_bytes)
    return tree_ops.hist_plan(bd, case.mode, case.unit_w, int(sum(case.counts)))


@lru_cache(maxsize=4)
def expected(name):
    """(oracle, bound, exact [C] bools, expected zero mask of need_mask or None) of a case."""
    case = build(name)
    orc = hist_oracle(case.codes, case.ridx, case.va, case.vb, case.mode, case.starts, case.counts, case.Bs,
                      case.posv)
    pack = case.expect[2]
    sf = s_floor(case.vmax, CHUNK, pack)
    bnd = bound(orc, case.mode, sf, pack, case.has_w)
    exact = []
    for c in range(channels(case.mode)):
        if pack and c == 0:
            exact.append(True)
            continue
        vals = _channel_values(case, c)
        lb = _low_bit(vals)
        prod_ok = not (c == 1 and case.has_w and orc.inexact_prod)
        exact.append(lb is None or (prod_ok and 2.0 ** lb * sf[c] >= 1.0 and
                                    float(orc.A[..., c].max()) / 2.0 ** lb < 2.0 ** 53))
    skipped = None
    if case.need_mask is not None:
        width = case.expect[1]
        ng = -(-case.F // width)
        gneed = np.zeros((len(case.counts), ng * width), bool)
        gneed[:, :case.F] = case.need_mask
        gneed = gneed.reshape(len(case.counts), ng, width).any(2)               # [S, ng]
        skipped = ~np.repeat(gneed, width, axis=1)[:, :case.F].T                # [F, S]
    return orc, bnd, exact, skipped


def _channel_values(case, c):
    """Exact f64 row values of channel c over all rows that contribute."""
    out = []
    for st, ct in zip(case.starts, case.counts):
        if ct > 0:
            out.append(_rows(case.ridx, case.va, case.vb, case.mode, st, ct, case.posv)[1][c])
    return np.concatenate(out)


# --------------------------------------------------------------------------- a correct kernel, emulated
def emulate(case, plan, want_items=False):
    """What a correct fixed-point kernel returns for the case: rint(fl32(w*y) * s), ties to even, at the
    scales of plan.scales; int64 sums per work item, unbounded Python integers per node, one correctly
    rounded conversion.  want_items: also (largest |item sum|, largest |node sum|) per channel as
    Python integers (unpacked) or the largest packed response field."""
    s0, s1, bq = plan.scales(case.vmax)
    sc = [s0, s1]
    F, Bs, mode = case.F, case.Bs, case.mode
    C, S = channels(mode), len(case.starts)
    H = np.zeros((F, S, Bs, C))
    foff = (np.arange(F, dtype=np.int64) * Bs)[None, :]
    stats = [[0, 0] for _ in range(C)]
    f32 = np.float32
    for s, (st, ct) in enumerate(zip(case.starts, case.counts)):
        if ct <= 0:
            continue
        pos = np.arange(st, st + ct)
        r = case.ridx[pos].astype(np.int64)
        vi = pos if case.posv else r
        if mode == 0:
            y = case.va[vi]
            w = (~np.isnan(y)).astype(f32) if case.vb is None else case.vb[vi]
            keep = w != 0
            pos, r, w, y = pos[keep], r[keep], w[keep], y[keep]
            ch = [w, (w * y).astype(f32)]
            if plan.pack:
                ch = [w, y]
        elif mode == 1:
            ch = [case.va[vi], case.vb[vi]]
        else:
            w = np.ones(ct, f32) if case.vb is None else case.vb[vi]
            pos, r, w = pos[w != 0], r[w != 0], w[w != 0]
            ch = [w]
        if r.size == 0:
            continue
        item = (pos - st) // plan.chunk
        n_it = int(item.max()) + 1
        idx = (item[:, None] * (F * Bs) + case.codes[r].astype(np.int64) + foff).reshape(-1)
        for c in range(C):
            if plan.pack and c == 0:
                H[:, s, :, 0] = np.bincount(idx % (F * Bs), minlength=F * Bs).reshape(F, Bs)
                continue
            q = np.rint(ch[c].astype(np.float64) * sc[c])
            assert np.all(np.abs(q) <= 2.0 ** 51)
            if plan.pack:
                q = q + bq
                assert np.all(q >= 0)
            qi = np.repeat(q.astype(np.int64), F)
            lo = qi & ((1 << 26) - 1)
            hi = qi >> 26
            sz = n_it * F * Bs
            # two 26-bit halves: float64 bincounts of fewer than 2^13 terms each are exact
            il = np.bincount(idx, weights=lo.astype(np.float64), minlength=sz).astype(np.int64)
            ih = np.bincount(idx, weights=hi.astype(np.float64), minlength=sz).astype(np.int64)
            assert np.all(np.abs(ih) <= 2 ** 36)                      # |item sum| <= 2^62: fits int64
            it = (ih << 26) + il                                      # int64 per work item
            it = it.reshape(n_it, F * Bs)
            if plan.pack:
                assert int(it.max()) < 2 ** 40                        # the field does not carry into the count
                cnt = np.bincount(idx, minlength=sz).reshape(n_it, F * Bs)
                stats[c][0] = max(stats[c][0], int(it.max()))
                node = (it - cnt * bq).sum(0)
                H[:, s, :, c] = (node.astype(np.float64) / sc[c]).reshape(F, Bs)
                continue
            stats[c][0] = max(stats[c][0], int(np.abs(it).max()))
            if np.abs(it.astype(np.float64)).sum(0).max() < 2.0 ** 62:
                node = it.sum(0)                                      # fits int64
                stats[c][1] = max(stats[c][1], int(np.abs(node).max()))
                H[:, s, :, c] = (node.astype(np.float64) / sc[c]).reshape(F, Bs)
            else:
                node = it.astype(object).sum(0)                       # Python integers
                stats[c][1] = max(stats[c][1], max(abs(int(x)) for x in node))
                H[:, s, :, c] = (np.array([float(int(x)) for x in node]) / sc[c]).reshape(F, Bs)
    return (H, stats) if want_items else H


# --------------------------------------------------------------------------- device work list
def child_work_expected(rec, cols, starts, counts, chunk):
    """slots (build | der | par), #pairs, work items of tree_ops.hist_build_dev by a plain loop over
    the split record, and the (start, count) of every pair's built child."""
    ok_c, nl_c, wl_c, wr_c = cols
    n = len(starts)
    build, der, par, items, segs = [], [], [], [], []
    for i in range(n):
        if not rec[i, ok_c] > 0:
            continue
        j = len(par)
        nl = int(rec[i, nl_c])
        left = rec[i, wl_c] <= rec[i, wr_c]
        st, ct = (starts[i], nl) if left else (starts[i] + nl, counts[i] - nl)
        build.append(2 * j + (0 if left else 1))
        der.append(2 * j + (1 if left else 0))
        par.append(i)
        segs.append((st, ct))
        k = 0
        while k * chunk < ct:
            items.append((j, st + k * chunk, min(chunk, ct - k * chunk), k))
            k += 1
    return build, der, par, items, segs
