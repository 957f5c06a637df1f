"""Shared pieces of the split search tests (test_split_oracle.py and
test_split_kernels_gpu.py): an exact per-threshold oracle of the numeric
split search and the case table both files run.

The oracle is written from the header comments of ops/csrc/tree_split.hip and
DTree.findBestSplitPoint's rule, in plain Python over fractions.Fraction.
Every f64 is an exact Fraction, so sums, scores and gains are exact numbers,
not "higher precision".  It imports nothing from the tree engine.

Layout: H [Fl][n][Bs][2] f64, B = Bs - 1 non-NA bins, the NA bin is B.
Channels are (w, wy) for the squared-error criterion (crit 0) and (g, h) for
the second-order one (crit 1).  Candidates of one (node, feature) column in
index order k = 0 .. 2(B-1):
    k <  B-1        opt 0, t = k          left = bins <= t, NA right
    k <  2(B-1)     opt 1, t = k - (B-1)  left = bins <= t plus NA
    k == 2(B-1)     opt 2, t = 0          left = every non-NA bin, right = NA
opt 1 and opt 2 exist only when the column has NAs.  The column keeps the
first candidate of the largest gain (strict > in index order), the node the
first column of the largest gain (strict > in feature order).

Squared error: score(w, wy) = wy^2 / w (0 when w <= 0); a candidate is valid
when both children weigh >= min_rows and > 0 and float32(ly / lw) !=
float32(ry / rw) (f64 division); has_na = nw > 0; se_before = max(wyy - sT,
0), a node with se_before <= 0 does not split; a candidate is kept only if
gain > se_before * msi.
Second order: g is soft-thresholded by alpha, score = g^2 / (h + lambda),
gain = 0.5 (sL + sR - sT) - gamma kept only if > 0; valid when both child
hessians are >= max(min_rows, 1e-12); has_na = h_na > 0 or g_na != 0.
Monotone columns compare the child predictions (ly / lw, -g / (h + lambda)):
+1 rejects pl > pr, -1 rejects pl < pr.  Node bounds [lo, hi] apply to the
column's best candidate only: a child prediction outside them vetoes the
split (use_bounds 0) or costs w (c - p)^2 (0.5 (h + lambda) (c - p)^2) per
clamped child.

Classification.  Discrete outputs are compared with tolerance zero, so the
oracle raises CaseError unless every comparison the rule makes (arg-max
steps, gain > threshold, min_rows, the monotone order, the bound clamps,
min_w2) is decided either between operands the f64 code computes identically
or by a relative margin >= 1e-9 in exact arithmetic that also exceeds the
rounding bound below.  An exact tie of gains is accepted only between
candidates with the same (lw, ly, rw, ry): the same partition reached
through empty bins or through another NA option.  In the integer family the
mirrored partition (children swapped: NA-left at t = 0 over an empty bin 0
against NA-vs-rest, say) is accepted too, because sL + sR is the same f64
whichever child comes first.  In the float family the mirrored tie would be
decided by the rounding of two differently ordered sums, so the float
histograms keep bins 0 and B - 1 occupied and the oracle raises on it.  No
case is excluded.

Rounding bound (first order, u = 2^-53).  Any sum the f64 code forms over a
column adds at most B terms, in any order: |err| <= B u sum|terms| =: e_c per
channel c.  A right child is a difference of two such sums, so scores are
propagated with 2 e_c:
    squared error   ds = |2 wy / w| 2e_y + (wy / w)^2 2e_w + 2u |s|
    second order    dG = 2e_g + u |G|,  D = h + lambda,
                    ds = |2 G / D| dG + (G / D)^2 (2e_h + u |D|) + 2u |s|
    gain            dg = 2 (dsL + dsR + dsT) + 4u (|sL| + |sR| + |sT|)
(the factor 2 in dg covers second-order terms; 4u the final adds, the halving
and - gamma).  A clamped child adds d(a (c - p)^2) = 2 a |c - p| dp +
(c - p)^2 da + 4u a (c - p)^2 with dp = (2e_y + |p| 2e_w) / |w| + u |p|.
Sums of the float family are compared to 2 e_c + u |x|.  Every tolerance is
capped by 1e-9 (1 + |reference|), the rtol = atol of the older split tests.
In the integer family (small integer weights, responses in multiples of
1/8, totals < 2^40) every sum is exact and sums are compared with tolerance
zero."""
import functools
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np

U = 2.0 ** -53
MARGIN = Fr(1, 10 ** 9)
INF = float("inf")
SENTINEL = -12345.5

Case = namedtuple("Case", "name family crit H wyy ok mono min_rows msi lam alpha gamma bnd use_bounds f0 sel2")
# sel2: tuple of (min_w2, stride) runs of split_select2
Col = namedtuple("Col", "gain k opt t L R gtol stol")        # gain None = no split
Node = namedtuple("Node", "gain feat k opt t L R T gtol stol mask naw")
Result = namedtuple("Result", "cols nodes ties")


class CaseError(AssertionError):
    """A case of the table breaks a condition of the classification."""


def _cap(tol, ref):
    return min(tol, 1e-9 * (1.0 + abs(float(ref))))


def _gt(a, b, what, slack=0.0, tie_ok=False):
    """a > b in exact arithmetic; raises unless the f64 code decides it the same way."""
    if a == b:
        if not tie_ok:
            raise CaseError(f"{what}: exact tie {float(a)!r}")
        return False
    d = abs(a - b)
    if d < MARGIN * max(abs(a), abs(b)) or float(d) <= slack:
        raise CaseError(f"{what}: margin {float(d):.3e} between {float(a)!r} and {float(b)!r} (slack {slack:.3e})")
    return a > b


def _soft(g, alpha):
    if alpha > 0:
        m = max(abs(g) - alpha, Fr(0))
        return m if g >= 0 else -m
    return g


class _Column:
    """One (node, feature) histogram in exact arithmetic."""

    def __init__(self, case, node, f):
        self.c = case
        h = case.H[f, node]
        self.B = B = h.shape[0] - 1
        self.a = [Fr(float(v)) for v in h[:, 0]]
        self.b = [Fr(float(v)) for v in h[:, 1]]
        self.ea = B * U * float(np.abs(h[:, 0]).sum())
        self.eb = B * U * float(np.abs(h[:, 1]).sum())
        if case.family == "int":
            self.ea = self.eb = 0.0
        self.lam, self.alpha, self.gamma = Fr(case.lam), Fr(case.alpha), Fr(case.gamma)
        self.mono = 0.0 if case.mono is None else float(case.mono[f])
        self.what = f"{case.name} node {node} feature {f}"

    def score(self, a, b):
        """(score, rounding bound) of channel sums (a, b); None when undefined."""
        if self.c.crit == 1:
            if self.alpha > 0 and self.c.family != "int" and abs(a) != self.alpha:
                _gt(abs(a), self.alpha, self.what + " alpha")
            G = _soft(a, self.alpha)
            D = b + self.lam
            if D == 0:
                return None, 0.0
            s = G * G / D
            fG, fD, fs = float(G), float(D), float(s)
            dG = 2 * self.ea + U * abs(fG)
            return s, abs(2 * fG / fD) * dG + (fG / fD) ** 2 * (2 * self.eb + U * abs(fD)) + 2 * U * abs(fs)
        if a <= 0:
            return Fr(0), 0.0
        s = b * b / a
        fa, fb = float(a), float(b)
        return s, abs(2 * fb / fa) * 2 * self.eb + (fb / fa) ** 2 * 2 * self.ea + 2 * U * abs(float(s))

    def pred(self, a, b):
        return -a / (b + self.lam) if self.c.crit == 1 else b / a

    def _ge_min(self, w, what):
        mr = Fr(self.c.min_rows)
        if self.c.crit == 1:
            mr = max(mr, Fr(1e-12))
        if w == mr:
            if self.c.family != "int":
                raise CaseError(f"{what}: weight equals min_rows in the float family")
            return True
        if self.c.family != "int" and abs(w - mr) < MARGIN * max(abs(w), mr):
            raise CaseError(f"{what}: weight within 1e-9 of min_rows")
        return w > mr

    def valid(self, la, lb, ra, rb, what):
        if self.c.crit == 1:
            if not (self._ge_min(lb, what) and self._ge_min(rb, what)):
                return False
        else:
            if not (la > 0 and ra > 0 and self._ge_min(la, what) and self._ge_min(ra, what)):
                return False
            pl, pr = float(lb) / float(la), float(rb) / float(ra)
            if self.c.family != "int" and abs(pl - pr) <= 2.0 ** -20 * max(abs(pl), abs(pr)):
                raise CaseError(f"{what}: child means too close for the float32 test in the float family")
            with np.errstate(over="ignore", under="ignore"):
                if np.float32(pl) == np.float32(pr):
                    return False
        if self.mono != 0:
            pl, pr = self.pred(la, lb), self.pred(ra, rb)
            if pl != pr and self.c.family != "int":
                _gt(pl, pr, what + " monotone")
            if (self.mono > 0 and pl > pr) or (self.mono < 0 and pl < pr):
                return False
        return True

    def solve(self, wyy, lo, hi, T0):
        """Best candidate of the column (Col); T0 = the node totals (feature 0)."""
        c, B, a, b = self.c, self.B, self.a, self.b
        none = Col(None, 0, 0, 0, (Fr(0), Fr(0)), (Fr(0), Fr(0)), 0.0, 0.0)
        ta, tb = sum(a[:B], Fr(0)), sum(b[:B], Fr(0))
        na, nb = a[B], b[B]
        Ta, Tb = ta + na, tb + nb
        sT, dT = self.score(Ta, Tb)
        if sT is None:
            return none, 0
        has_na = (nb > 0 or na != 0) if c.crit == 1 else na > 0
        thr, thr_slack = Fr(0), 0.0
        if c.crit == 0:
            w = Fr(float(wyy))
            if w == sT:
                # decided between identical operands only if the f64 score is exact
                if c.family != "int" or (Ta > 0 and Fr(float(Tb) * float(Tb) / float(Ta)) != sT):
                    raise CaseError(f"{self.what}: wyy ties with an inexact node score")
                return none, 0
            if not _gt(w, sT, self.what + " se_before", slack=dT):
                return none, 0
            thr = (w - sT) * Fr(float(c.msi))
            thr_slack = dT * float(c.msi)
        nt = B - 1
        best, ties = None, 0
        ca, cb = Fr(0), Fr(0)
        pre = []
        for t in range(nt):
            ca += a[t]
            cb += b[t]
            pre.append((ca, cb))
        for k in range(2 * nt + 1):
            if k < nt:
                opt, t = 0, k
                la, lb = pre[t]
                ra, rb = ta - la + na, tb - lb + nb
            elif k < 2 * nt:
                opt, t = 1, k - nt
                if not has_na:
                    continue
                la, lb = pre[t][0] + na, pre[t][1] + nb
                ra, rb = ta - pre[t][0], tb - pre[t][1]
            else:
                opt, t = 2, 0
                if not has_na:
                    continue
                la, lb, ra, rb = ta, tb, na, nb
            what = f"{self.what} k {k}"
            if not self.valid(la, lb, ra, rb, what):
                continue
            (sL, dL), (sR, dR) = self.score(la, lb), self.score(ra, rb)
            g = sL + sR - sT
            gtol = 2 * (dL + dR + dT) + 4 * U * (abs(float(sL)) + abs(float(sR)) + abs(float(sT)))
            if c.crit == 1:
                g = g / 2 - self.gamma
                gtol = 0.5 * gtol + 2 * U * abs(float(g))
            if c.family == "int" and g == thr and sL == 0 and sR == 0 and sT == 0 and self.gamma == 0:
                continue                                  # 0 > 0 between exact zeros
            if not _gt(g, thr, what + " threshold", slack=gtol + thr_slack):
                continue
            part = (la, lb, ra, rb)
            if best is not None:
                if g == best[0]:
                    swapped = (ra, rb, la, lb) == best[6] and c.family == "int"
                    if part != best[6] and not swapped:
                        raise CaseError(f"{what}: gain ties with k {best[1]} on another partition")
                    ties += 1
                    continue
                if not _gt(g, best[0], what + f" vs k {best[1]}", slack=gtol + best[4]):
                    continue
            best = (g, k, opt, t, gtol, (sL, sR), part)
        if best is None:
            return none, ties
        g, k, opt, t, gtol, _, (la, lb, ra, rb) = best
        stol = max(2 * self.ea, 2 * self.eb)
        # node bounds on the column's best candidate; the right child is the node total minus the left
        if lo is not None and (lo > -INF or hi < INF):
            ra, rb = Ta - la, Tb - lb
            if c.crit == 1:
                al, ar = (lb + self.lam) / 2, (rb + self.lam) / 2
            else:
                al, ar = la, ra
            pen, dpen, viol = Fr(0), 0.0, False
            for (wa, wb, aa) in ((la, lb, al), (ra, rb, ar)):
                p = self.pred(wa, wb)
                cl = p
                if lo > -INF and p != Fr(lo) and _gt(Fr(lo), p, self.what + " lower bound"):
                    cl = Fr(lo)
                if hi < INF and cl != Fr(hi) and _gt(cl, Fr(hi), self.what + " upper bound"):
                    cl = Fr(hi)
                if cl != p:
                    viol = True
                    d = float(abs(cl - p))
                    den = abs(float(wb + self.lam if c.crit == 1 else wa))
                    ep, ew = (self.ea, self.eb) if c.crit == 1 else (self.eb, self.ea)
                    dp = (2 * ep + abs(float(p)) * 2 * ew) / den + U * abs(float(p))
                    pen += aa * (cl - p) ** 2
                    dpen += 2 * float(aa) * d * dp + d * d * 2 * ew + 4 * U * float(aa) * d * d
            if viol:
                if not c.use_bounds:
                    return none, ties
                g -= pen
                gtol += 2 * dpen + 2 * U * abs(float(g))
        return Col(g, k, opt, t, (la, lb), (ra, rb), _cap(gtol, g), stol), ties


def _mask(Bs, opt, t):
    B = Bs - 1
    m = np.zeros(Bs, dtype=np.uint8)
    m[:B] = 1 if opt == 2 else (np.arange(B) <= t)
    m[B] = 1 if opt == 1 else 0
    return m


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Result(cols [n][Fl] of Col, nodes [n] of Node, number of accepted exact ties)."""
    c = CASES[name]
    Fl, n, Bs, _ = c.H.shape
    cols, nodes, ties = [], [], 0
    for node in range(n):
        h0 = c.H[0, node]
        T0 = (sum((Fr(float(v)) for v in h0[:, 0]), Fr(0)), sum((Fr(float(v)) for v in h0[:, 1]), Fr(0)))
        tstol = 0.0 if c.family == "int" else 2 * (Bs - 1) * U * float(np.abs(h0).sum(0).max())
        lo, hi = (None, None) if c.bnd is None else (float(c.bnd[node, 0]), float(c.bnd[node, 1]))
        row, best, bf = [], None, 0
        for f in range(Fl):
            if not c.ok[node, f]:
                row.append(Col(None, 0, 0, 0, (Fr(0), Fr(0)), (Fr(0), Fr(0)), 0.0, 0.0))
                continue
            col, tk = _Column(c, node, f).solve(c.wyy[node], lo, hi, T0)
            ties += tk
            row.append(col)
            if col.gain is None:
                continue
            if best is not None:
                if col.gain == best.gain:
                    if (col.L, col.R) != (best.L, best.R):
                        raise CaseError(f"{name} node {node}: features {bf} and {f} tie on different splits")
                    ties += 1
                    continue
                if not _gt(col.gain, best.gain, f"{name} node {node} feature {f} vs {bf}", slack=col.gtol + best.gtol):
                    continue
            best, bf = col, f
        cols.append(row)
        naw = float(c.H[bf if best is not None else 0, node, Bs - 1, 0])
        if best is None:
            nodes.append(Node(None, c.f0, 0, 0, 0, (Fr(0), Fr(0)), T0, T0, 0.0, tstol, None, naw))
        else:
            R = (T0[0] - best.L[0], T0[1] - best.L[1])
            nodes.append(Node(best.gain, bf + c.f0, best.k, best.opt, best.t, best.L, R, T0, best.gtol, best.stol + tstol,
                              _mask(Bs, best.opt, best.t), naw))
    return Result(cols, nodes, ties)


def make_grower(case, device="cpu"):
    """(TreeGrower, column mask) over a small all-numeric BinnedData with the
    case's parameters; the split search never reads the rows."""
    import torch
    from h2o3_amd.models.tree.binning import BinnedData
    from h2o3_amd.models.tree.engine import GrowParams, TreeGrower
    Fl, n, Bs, _ = case.H.shape
    F = case.f0 + Fl
    bd = BinnedData()
    bd.codes = torch.zeros((4, F), dtype=torch.uint8, device=device)
    bd.F = bd.Fp = F
    bd.Bs = Bs
    bd.na_code = Bs - 1
    bd.nbins = [Bs - 1] * F
    bd.is_cat = [False] * F
    bd.names = [f"f{j}" for j in range(F)]
    bd.nrows_local = 4
    mono = np.zeros(F)
    if case.mono is not None:
        mono[case.f0:] = case.mono
    p = GrowParams(criterion="xgb" if case.crit == 1 else "se", min_rows=case.min_rows,
                   min_split_improvement=case.msi, reg_lambda=case.lam, reg_alpha=case.alpha, gamma=case.gamma,
                   monotone=mono, use_bounds=bool(case.use_bounds))
    gr = TreeGrower(bd, p)
    assert gr.W == 1 and gr.dev.type == torch.device(device).type
    gr.f0 = case.f0
    if case.bnd is not None:
        gr._bnd, gr._bnd_off = torch.as_tensor(case.bnd.copy()).to(device), 0
    cm = torch.zeros((n, F), dtype=torch.bool)
    cm[:, case.f0:] = torch.as_tensor(case.ok.copy()).bool()
    return gr, cm


def select2_ok(case, node_res, min_w2):
    """ok flag of split_select2: a finite gain and node weight >= min_w2 (min_w2 < 0: no test)."""
    if node_res.gain is None:
        return False
    if min_w2 < 0:
        return True
    w, m = node_res.T[0], Fr(float(min_w2))
    if w == m:
        if case.family != "int":
            raise CaseError(f"{case.name}: node weight equals min_w2 in the float family")
        return True
    if case.family != "int" and abs(w - m) < MARGIN * max(abs(w), abs(m)):
        raise CaseError(f"{case.name}: node weight within 1e-9 of min_w2")
    return w > m


def sum_tol(case, node_res, ref):
    """Tolerance of a channel sum of the winner (0 in the integer family)."""
    if case.family == "int":
        return 0.0
    return _cap(node_res.stol + U * abs(float(ref)), ref)


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
CASES = {}
_DEFAULT_STRIDES = (12, 13, 16)


def _add(name, family, crit, H, wyy=None, ok=None, mono=None, min_rows=1.0, msi=1e-5, lam=1.0, alpha=0.0, gamma=0.0,
         bnd=None, use_bounds=1, f0=0, sel2=None):
    H = np.ascontiguousarray(H, dtype=np.float64)
    Fl, n, Bs, _ = H.shape
    if wyy is None:
        wyy = H[0].sum(1)[:, 0] * 10.0 + 1.0 if crit == 0 else np.zeros(n)
    wyy = np.ascontiguousarray(np.broadcast_to(np.asarray(wyy, dtype=np.float64), (n,)))
    ok = np.ones((n, Fl), dtype=np.uint8) if ok is None else np.ascontiguousarray(ok, dtype=np.uint8)
    if mono is not None:
        mono = np.ascontiguousarray(mono, dtype=np.float32)
    if bnd is not None:
        bnd = np.ascontiguousarray(bnd, dtype=np.float64)
    if sel2 is None:
        mw = 2.0 * min_rows if crit == 0 else -1.0
        sel2 = tuple((mw, s) for s in _DEFAULT_STRIDES)
    assert name not in CASES, name
    for arr in (H, wyy, ok):
        arr.setflags(write=False)
    CASES[name] = Case(name, family, crit, H, wyy, ok, mono, float(min_rows), float(msi), float(lam), float(alpha),
                       float(gamma), bnd, int(use_bounds), int(f0), tuple(sel2))


def _float_hist(seed, Fl, n, B, crit, zero=0.3, na_empty=0.3):
    """Seeded random f64 histograms like the older split tests: w in [0, 50),
    signed wy = (u - 0.3) w (positive h), some bins zeroed, some NA bins empty."""
    r = np.random.RandomState(seed)
    H = r.rand(Fl, n, B + 1, 2) * 50
    if crit == 0:
        H[..., 1] = (r.rand(Fl, n, B + 1) - 0.3) * H[..., 0]
    else:
        H[..., 0] = (r.rand(Fl, n, B + 1) - 0.45) * 40
    keep = r.rand(Fl, n, B, 1) >= zero
    keep[:, :, 0] = keep[:, :, B - 1] = True               # see "ties" in the module docstring
    H[..., :B, :] *= keep
    H[..., B, :] *= (r.rand(Fl, n, 1) >= na_empty)
    return H


def _int_hist(seed, Fl, n, B, crit, zero=0.4, na_empty=0.3, wmax=6, vmax=40):
    """Integer family: w (h) small non-negative integers, wy (g) multiples of 1/8."""
    r = np.random.RandomState(seed)
    H = np.zeros((Fl, n, B + 1, 2))
    w = r.randint(0, wmax, (Fl, n, B + 1)).astype(np.float64)
    v = r.randint(-vmax, vmax + 1, (Fl, n, B + 1)) / 8.0
    keep = r.rand(Fl, n, B + 1) >= zero
    keep[..., B] = r.rand(Fl, n) >= na_empty
    w *= keep
    if crit == 0:
        H[..., 0], H[..., 1] = w, v * w
    else:
        H[..., 0], H[..., 1] = v * keep, w
    return H


def _mask_some(seed, n, Fl):
    ok = np.ones((n, Fl), dtype=np.uint8)
    if n * Fl > 1:
        r = np.random.RandomState(seed)
        ok[r.randint(n), r.randint(Fl)] = 0
    return ok


def _bins(B, entries, na=(0, 0)):
    """[1][1][B + 1][2] histogram with the given {bin: (c0, c1)} and NA bin."""
    H = np.zeros((1, 1, B + 1, 2))
    for b, v in entries.items():
        H[0, 0, b] = v
    H[0, 0, B] = na
    return H


def _build():
    # --- shapes: every B of the chunk / last-lane / multi-chunk paths, n * Fl of every remainder mod 4
    shapes = [(1, 3, 3), (2, 5, 3), (3, 6, 13), (63, 1, 3), (64, 3, 3), (65, 5, 3), (66, 1, 1), (128, 6, 1),
              (129, 3, 3), (255, 5, 1), (1000, 1, 3)]
    for i, (B, n, Fl) in enumerate(shapes):
        for crit in (0, 1):
            tag = "se" if crit == 0 else "xgb"
            _add(f"float_B{B}_n{n}_F{Fl}_{tag}", "float", crit, _float_hist(100 + 2 * i + crit, Fl, n, B, crit),
                 ok=_mask_some(i, n, Fl), min_rows=5.0)
            if B <= 255:
                _add(f"int_B{B}_n{n}_F{Fl}_{tag}", "int", crit, _int_hist(200 + 2 * i + crit, Fl, n, B, crit),
                     ok=_mask_some(50 + i, n, Fl), min_rows=2.0)
    for i, (Fl, n, B) in enumerate([(13, 5, 9), (64, 1, 6), (65, 3, 5), (130, 1, 5), (130, 3, 4), (3, 1, 20)]):
        for crit in (0, 1):
            tag = "se" if crit == 0 else "xgb"
            _add(f"float_F{Fl}_n{n}_B{B}_{tag}", "float", crit, _float_hist(300 + 2 * i + crit, Fl, n, B, crit),
                 ok=_mask_some(70 + i, n, Fl), min_rows=5.0)
    # --- the in-lane tie: {bin 3 + NA | rest} is opt 1 at t = 3..66 and opt 0 at t = 67..99; k = 67 wins
    tie = _bins(129, {3: (10, 0), 67: (10, 20), 100: (10, 100)}, na=(10, 20))
    _add("tie_opt0_later_chunk", "int", 0, tie, wyy=1e6, min_rows=20.0)
    # its mirror: opt 0 at t = 70..74 sits alone in its lanes, opt 1 at t = 10..69 in earlier lanes
    _add("tie_mirror_cross_lane", "int", 0, _bins(129, {10: (10, 0), 70: (10, 20), 75: (10, 100)}, na=(10, 20)),
         wyy=1e6, min_rows=20.0)
    # the same tie for the second-order criterion (g, h)
    _add("tie_opt0_later_chunk_xgb", "int", 1, _bins(129, {3: (0, 10), 67: (-20, 10), 100: (-100, 10)}, na=(-20, 10)),
         min_rows=20.0, lam=0.0)
    # a tie three chunks apart in the same lane (5 and 197 = 3 * 64 + 5) at B = 255
    _add("tie_three_chunks", "int", 0, _bins(255, {5: (10, 0), 197: (10, 20), 230: (10, 100)}, na=(10, 20)),
         wyy=1e6, min_rows=20.0)
    # --- runs of empty bins across the 64 / 128 boundaries, integer sums (ties are exact in any order)
    for crit in (0, 1):
        H = _int_hist(401 + crit, 3, 3, 200, crit, zero=0.0, na_empty=0.0)
        for lo_, hi_ in ((50, 80), (120, 140), (190, 200)):
            H[:, :, lo_:hi_] = 0
        H[1, :, 60:135] = 0
        _add(f"int_empty_runs_{'se' if crit == 0 else 'xgb'}", "int", crit, H, min_rows=3.0)
    # --- NA vs rest
    na_h = np.zeros((1, 1, 6, 2))
    na_h[0, 0, :5] = (5, 5)
    na_h[0, 0, 5] = (10, 100)
    _add("na_vs_rest_wins", "int", 0, na_h, wyy=1e5)
    na_t = na_h.copy()
    na_t[0, 0, 2:5] = 0                                    # trailing empty bins: opt 0 at t = 1 is the same split
    _add("na_vs_rest_ties_threshold", "int", 0, na_t, wyy=1e5)
    _add("na_vs_rest_wins_xgb", "int", 1, na_h[..., ::-1] * np.array([-1.0, 1.0]), lam=0.5)
    # --- identical feature histograms: the lower feature wins
    for nm, (fa, fb), Fl in (("1_65", (1, 65), 130), ("0_1", (0, 1), 3)):
        H = _int_hist(411, Fl, 3, 6, 0, wmax=3, vmax=5)     # weak columns
        H[fa] = H[fb] = _int_hist(412, 1, 3, 6, 0, zero=0.0, na_empty=0.0)[0]
        _add(f"identical_features_{nm}", "int", 0, H, wyy=1e5)
    # --- no NA
    H = _int_hist(421, 3, 3, 10, 0)
    H[:, :, 10] = 0
    _add("no_na_se", "int", 0, H)
    H = _int_hist(422, 3, 3, 10, 1)
    H[:, :, 10] = 0
    _add("no_na_xgb_g0_h0", "int", 1, H)
    H = H.copy()
    H[:, :, 10, 0] = [[-3.5, 1.625, 0.0]] * 3               # g != 0, h = 0: has_na, but no NA-vs-rest
    _add("no_na_xgb_g_without_h", "int", 1, H)
    # --- min_rows boundary: left child exactly at min_rows (node 0) and one below (node 1)
    H = np.zeros((1, 2, 5, 2))
    H[0, 0, :4] = [(7, 0), (0, 0), (9, 27), (4, 12)]
    H[0, 1, :4] = [(6, 0), (0, 0), (9, 27), (4, 12)]
    _add("min_rows_boundary", "int", 0, H, wyy=1e4, min_rows=7.0)
    _add("min_rows_boundary_xgb", "int", 1, H[..., ::-1] * np.array([-1.0, 1.0]), min_rows=7.0)
    # --- min_split_improvement
    _add("msi_zero", "int", 0, _int_hist(431, 3, 3, 10, 0), msi=0.0)
    _add("msi_removes_only_candidate", "int", 0, tie, wyy=1e6, min_rows=20.0, msi=0.01)
    # --- (float)pl == (float)pr with unequal f64 means: 3 vs 3 + 2^-24 (node 0); 3 vs 3.25 splits (node 1)
    H = np.zeros((1, 2, 4, 2))
    H[0, 0, :2] = [(4, 12), (2 ** 21, 3 * 2 ** 21 + 0.125)]
    H[0, 1, :2] = [(4, 12), (2 ** 21, 3.25 * 2 ** 21)]
    _add("float32_equal_means", "int", 0, H, wyy=1e9, msi=0.0)
    # --- pure node (wyy == sT), all-zero histogram, all features masked for one node
    _add("pure_node", "int", 0, tie, wyy=490.0, min_rows=1.0)
    _add("all_zero_se", "int", 0, np.zeros((3, 3, 9, 2)), wyy=0.0)
    _add("all_zero_xgb", "int", 1, np.zeros((3, 3, 9, 2)))
    _add("all_zero_xgb_lambda0", "int", 1, np.zeros((3, 3, 9, 2)), lam=0.0)
    H = _int_hist(441, 3, 3, 9, 0)
    H[:, 1] = 0                                            # an empty node between two live ones
    _add("empty_node_between", "int", 0, H, wyy=[100.0, 0.0, 100.0])
    H = _int_hist(442, 3, 3, 9, 1)
    H[:, 1] = 0
    _add("empty_node_between_xgb_lambda0", "int", 1, H, lam=0.0, min_rows=0.0)
    ok = np.ones((3, 5), dtype=np.uint8)
    ok[1] = 0
    for crit in (0, 1):
        _add(f"node_all_masked_{'se' if crit == 0 else 'xgb'}", "int", crit, _int_hist(451 + crit, 5, 3, 9, crit), ok=ok)
    # --- f0 = 5
    for crit in (0, 1):
        _add(f"f0_5_{'se' if crit == 0 else 'xgb'}", "int", crit, _int_hist(461 + crit, 7, 3, 9, crit), f0=5)
    _add("f0_5_float", "float", 0, _float_hist(463, 7, 5, 20, 0), f0=5, min_rows=5.0)
    # --- second-order parameters
    Hx = _int_hist(471, 3, 3, 8, 1, zero=0.2)
    for lam in (0.0, 0.5, 1.0):
        for alpha in (0.0, 0.25, 6.0):
            for gamma in (0.0, 0.125, 1e4):
                _add(f"xgb_l{lam}_a{alpha}_g{gamma}", "int", 1, Hx, lam=lam, alpha=alpha, gamma=gamma, min_rows=0.0)
    H = Hx.copy()
    H[:, 1, :, 1] = 0                                      # node 1: zero total hessian, g left in place
    _add("xgb_zero_hessian_lambda0", "int", 1, H, lam=0.0, min_rows=0.0)
    _add("xgb_zero_hessian_lambda1", "int", 1, H, lam=1.0, min_rows=0.0)
    _add("xgb_float_params", "float", 1, _float_hist(472, 3, 5, 40, 1), lam=0.5, gamma=0.125, min_rows=0.0)
    # --- monotone constraints on columns whose best free split violates the order
    for crit in (0, 1):
        tag = "se" if crit == 0 else "xgb"
        Hm = _int_hist(481 + crit, 4, 3, 12, crit, zero=0.1)
        for sgn in (1.0, -1.0):
            _add(f"monotone_{'inc' if sgn > 0 else 'dec'}_{tag}", "int", crit, Hm, mono=[sgn, 0.0, -sgn, sgn])
        _add(f"monotone_float_{tag}", "float", crit, _float_hist(483 + crit, 4, 5, 70, crit), mono=[1, 0, -1, -1],
             min_rows=5.0)
    # gamma < 0 (outside XGBoost's range) keeps candidates of negative raw gain: the only ones whose child
    # order can depend on lambda (ab(x - y)^2 > lambda (ax^2 + by^2) fixes the order of every positive gain)
    # Here -g / (h + 1) = 1.5 < 2 is increasing, -g / h = 3 > 2.22 is not; raw gain -1.795.
    _add("monotone_negative_gamma_xgb", "int", 1, _bins(2, {0: (-3, 1), 1: (-20, 9)}), mono=[1],
         lam=1.0, gamma=-50.0, min_rows=0.0)
    # --- node bounds
    for crit in (0, 1):
        tag = "se" if crit == 0 else "xgb"
        Hb = _int_hist(491 + crit, 4, 6, 12, crit, zero=0.1)
        none = np.array([[-INF, INF]] * 6)
        one = np.array([[-INF, INF], [-0.25, INF], [-INF, 0.5], [0.125, INF], [-INF, -0.125], [-INF, INF]])
        two = np.array([[-INF, INF], [-0.25, 0.25], [0.0, 0.5], [-1.0, 1.0], [0.125, 0.375], [-8.0, 8.0]])
        for nm, bnd in (("none", none), ("one_sided", one), ("two_sided", two)):
            for ub in (0, 1):
                _add(f"bounds_{nm}_ub{ub}_{tag}", "int", crit, Hb, bnd=bnd, use_bounds=ub, mono=[1, 0, -1, 0])
        _add(f"bounds_float_{tag}", "float", crit, _float_hist(493 + crit, 4, 6, 70, crit),
             bnd=np.array([[-INF, INF], [-0.1, 0.1], [0.05, INF], [-INF, 0.02], [-1.0, 1.0], [0.2, 0.3]]),
             mono=[1, 0, -1, 0], min_rows=5.0)
    # the winner changes column after the penalty: column 0 (means -10 and 40/9) has the free gain
    # 200 + 3200/9 - 180 = 375.6 but its left mean lies below lo = 0 and pays 2 * 10^2 = 200; column 1
    # (means 0 and 6, gain 180) is inside the bounds and wins.  With lo = -5 column 0 pays 50 and stays.
    H = np.zeros((2, 1, 4, 2))
    H[0, 0, :2] = [(2, -20), (18, 80)]
    H[1, 0, :2] = [(10, 0), (10, 60)]
    _add("bounds_winner_changes_column", "int", 0, H, wyy=1e4, bnd=[[0.0, INF]], use_bounds=1, sel2=((2.0, 13),))
    _add("bounds_winner_keeps_column", "int", 0, H, wyy=1e4, bnd=[[-5.0, INF]], use_bounds=1, sel2=((2.0, 13),))
    # --- split_select2: min_w2 at the node weight (ok), just above (not ok), negative (disabled)
    Hs = _int_hist(501, 3, 3, 9, 0, zero=0.1)
    Hs[:, 2] = Hs[:, 0]                                    # nodes 0 and 2 weigh the same
    wn = float(Hs[0, 0, :, 0].sum())
    _add("select2_min_w2", "int", 0, Hs, wyy=1e4,
         sel2=((wn, 12), (wn, 13), (wn, 16), (wn + 0.5, 13), (wn + 0.5, 16), (-1.0, 13), (-1.0, 12)))


_build()

# the single-feature numeric cases the pair kernel (h2o_cat_pairs, pcat = 0) can score: B <= 255, no bounds
PAIR_CASES = tuple(nm for nm, c in CASES.items()
                   if c.H.shape[0] == 1 and c.H.shape[2] - 1 <= 255 and c.bnd is None)
