"""Level-wise GPU tree growth shared by GBM, DRF, XGBoost and Uplift.

Reference: hex/tree/SharedTree.java (scoreAndBuildTrees / buildLayer),
hex/tree/DTree.java (UndecidedNode/DecidedNode, findBestSplitPoint at
DTree.java:984), hex/tree/ScoreBuildHistogram2.java.

Per tree, per level:
  1. histograms for the *smaller* child of every split (HIP LDS kernel,
     ops/csrc/tree_hist.hip); the larger sibling is parent - smaller
     (histogram subtraction — the reference builds every node from rows);
  2. multi-GPU: reduce_scatter over the feature dim, each rank scores the
     splits of its feature slice, candidates are all_gathered (small);
  3. vectorized split search over [node, feature, threshold, NA-direction]
     (squared-error criterion of the reference, or the second-order gain of
     XGBoost), categorical levels sorted by mean response -> bitset;
  4. stable GPU partition of each split node's row segment.
Leaves end up as contiguous segments of the row permutation, giving the
per-row leaf id for the leaf-value pass without any tree traversal.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from ...ops import _native, tree_ops
from ...ops._native import check, ptr, stream
from ...parallel import cloud
from ...parallel import collectives as coll
from ...utils.timer import phase
from .record import decode, rec_cols, weight_col

NEG_INF = float("-inf")


def _row_weight(S, mode):
    """Row weight of channel sums [..., C] (numpy or torch): the weight
    channel, plus the control group's under uplift."""
    return (S[:, 0] if mode != 1 else S[:, 1]) + (S[:, 2] if mode == 3 else 0.0)


def _clamp_mask(mode):
    """Channels a derived (parent minus built) sibling clamps at zero."""
    return {0: 0b1, 1: 0b0}.get(mode, (1 << tree_ops.channels(mode)) - 1)


@dataclass
class _Frontier:
    """The nodes of one level, in order (all share the depth)."""
    id: np.ndarray                 # tree node ids
    st: np.ndarray                 # row segments [st, st + ct) of ridx
    ct: np.ndarray
    tot: np.ndarray = None         # channel totals from the parent's split record (a last level builds no histograms)
    allow: torch.Tensor = None     # [n, F] features the node may still split on (interaction constraints)
    lo: np.ndarray = None          # monotone prediction bounds
    hi: np.ndarray = None
    p_build: np.ndarray = None     # of the node pairs: slot built from rows,
    p_der: np.ndarray = None       # slot derived as parent minus built,
    p_par: np.ndarray = None       # parent's slot in the previous level


@dataclass
class GrowParams:
    criterion: str = "se"          # "se" (H2O GBM/DRF) | "xgb" (second order)
    max_depth: int = 5
    min_rows: float = 10.0         # se: min weighted rows per child; xgb: min_child_weight
    min_split_improvement: float = 1e-5
    reg_lambda: float = 1.0
    reg_alpha: float = 0.0
    gamma: float = 0.0             # xgb min_split_loss
    max_leaves: int = 0            # 0 = unlimited
    monotone: np.ndarray | None = None  # [F] in {-1,0,1}
    col_sample_rate: float = 1.0   # per split (GBM) / mtries fraction
    mtries: int = -1               # DRF: features per node (-1 = all)
    col_sample_rate_change_per_level: float = 1.0
    tree_col_mask: np.ndarray | None = None  # [F] bool, per-tree sampling
    seed: int = 0
    hist_mem_budget: int = 8 << 30
    interaction_sets: list | None = None  # list of sets of feature ids
    leaf_budget_by_gain: bool = False   # max_leaves spent on the highest-gain nodes first (lossguide)
    use_bounds: bool = True        # monotone node bounds clamp (True) or veto (False) splits (GBMModel.java:84)


@dataclass
class Tree:
    """Host-side tree in BFS order (the per-node arrays feed scoring kernels,
    MOJO writer, SHAP and varimp)."""
    feat: list = field(default_factory=list)
    left: list = field(default_factory=list)
    right: list = field(default_factory=list)
    thr: list = field(default_factory=list)        # numeric: x < thr goes left
    na_left: list = field(default_factory=list)
    is_cat: list = field(default_factory=list)
    cat_left: list = field(default_factory=list)   # list of np.uint8 level masks (len = cardinality) or None
    value: list = field(default_factory=list)
    weight: list = field(default_factory=list)     # training cover (sum w or sum h)
    gain: list = field(default_factory=list)
    depth: list = field(default_factory=list)
    split_code: list = field(default_factory=list) # code threshold (numeric) for debugging

    def add_children(self, depth, wl, wr):
        """Append a (left, right) node pair per entry of wl / wr; returns the
        id of the first new node (pairs are consecutive)."""
        k = 2 * len(wl)
        base = len(self.feat)
        w = [0.0] * k
        w[0::2] = [float(x) for x in wl]
        w[1::2] = [float(x) for x in wr]
        self.feat += [-1] * k; self.left += [-1] * k; self.right += [-1] * k; self.thr += [0.0] * k
        self.na_left += [False] * k; self.is_cat += [False] * k; self.cat_left += [None] * k
        self.value += [0.0] * k; self.weight += w; self.gain += [0.0] * k
        self.depth += [depth] * k; self.split_code += [-1] * k
        return base

    def add_node(self, depth, weight):
        self.feat.append(-1); self.left.append(-1); self.right.append(-1); self.thr.append(0.0)
        self.na_left.append(False); self.is_cat.append(False); self.cat_left.append(None)
        self.value.append(0.0); self.weight.append(float(weight)); self.gain.append(0.0)
        self.depth.append(depth); self.split_code.append(-1)
        return len(self.feat) - 1

    @property
    def n_nodes(self):
        return len(self.feat)

    def is_leaf(self, i):
        return self.left[i] < 0

    def leaves(self):
        return np.nonzero(np.asarray(self.left, dtype=np.int64) < 0)[0].tolist()

    def max_depth(self):
        return int(np.max(np.asarray(self.depth))) if len(self.depth) else 0

    def to_arrays(self):
        return {k: np.asarray(getattr(self, k)) for k in ("feat", "left", "right", "thr", "na_left", "is_cat",
                                                          "value", "weight", "gain", "depth")}

    def predict_host(self, X: np.ndarray) -> np.ndarray:
        """Reference traversal on host (X: [n, F] float64, cats as codes)."""
        out = np.empty(X.shape[0])
        for r in range(X.shape[0]):
            i = 0
            while self.left[i] >= 0:
                x = X[r, self.feat[i]]
                if self.is_cat[i]:
                    m = self.cat_left[i]
                    if np.isnan(x) or int(x) >= len(m) or int(x) < 0:
                        go_left = self.na_left[i]
                    else:
                        go_left = bool(m[int(x)])
                elif np.isnan(x):
                    go_left = self.na_left[i]
                else:
                    go_left = x < self.thr[i]
                i = self.left[i] if go_left else self.right[i]
            out[r] = self.value[i]
        return out


class CatMasks:
    """Categorical level masks of a tree's nodes, stored as the per-level
    [k, Bs] uint8 mask matrices the split search produced plus (node, row,
    feature) indices: cat_masks[i] gives node i's level mask (None for a
    non-categorical node) on access.  Building the per-node arrays in the
    level loop cost ~10% of a depth-20 DRF tree's host time (10^4-10^5
    categorical splits per tree)."""

    def __init__(self, n, mats=(), feats=(), part=None, row=None, lvm=None):
        self.n = int(n)
        self.mats = list(mats)
        self.feats = list(feats)
        self.part = np.full(self.n, -1, dtype=np.int32) if part is None else part
        self.row = np.zeros(self.n, dtype=np.int32) if row is None else row
        self.lvm = dict(lvm or {})          # feature -> level index array into the mask row
        self.extra = {}                     # per-node overrides (assignments after construction)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        i = int(i)
        if i < 0:
            i += self.n
        if i in self.extra:
            return self.extra[i]
        p = int(self.part[i])
        if p < 0:
            return None
        r = int(self.row[i])
        return self.mats[p][r][self.lvm[int(self.feats[p][r])]]

    def __setitem__(self, i, v):
        self.extra[int(i)] = v

    def __iter__(self):
        for i in range(self.n):
            yield self[i]


class _TreeBuf:
    """Growable per-node numpy arrays for one tree under construction: the
    level loop records the splits of a whole level with vectorized
    assignments (the per-node Python bookkeeping cost seconds per tree at
    depth 20 / 10^5 nodes); to_tree() hands back the list-based Tree."""

    _FIELDS = (("feat", np.int64, -1), ("left", np.int64, -1), ("right", np.int64, -1), ("thr", np.float64, 0.0),
               ("na_left", bool, False), ("is_cat", bool, False), ("value", np.float64, 0.0),
               ("weight", np.float64, 0.0), ("gain", np.float64, 0.0), ("depth", np.int64, 0),
               ("split_code", np.int64, -1))

    def __init__(self, cap=256):
        self.n = 1                       # the root
        self.cap = cap
        for name, dt, fill in self._FIELDS:
            setattr(self, name, np.full(cap, fill, dtype=dt))
        self.cat_left = {}
        self.cat_parts = []                  # (node ids, features, [k, Bs] mask matrix) per level
        self.cat_lvm = {}

    def _grow(self, need):
        cap = self.cap
        while cap < need:
            cap *= 2
        if cap == self.cap:
            return
        for name, dt, fill in self._FIELDS:
            a = np.full(cap, fill, dtype=dt)
            a[:self.n] = getattr(self, name)[:self.n]
            setattr(self, name, a)
        self.cap = cap

    def add_children(self, depth, wl, wr):
        """(left, right) node pairs for every entry of wl / wr; returns the
        first new id (pairs are consecutive)."""
        k = 2 * len(wl)
        base = self.n
        self._grow(base + k)
        self.weight[base:base + k:2] = wl
        self.weight[base + 1:base + k:2] = wr
        self.depth[base:base + k] = depth
        self.n = base + k
        return base

    def to_tree(self):
        """Tree over numpy per-node arrays (copies; no per-node Python lists:
        the list conversion cost ~5 ms per depth-20 DRF tree).  Index,
        assignment and len() behave like the list form."""
        n = self.n
        t = Tree()
        for name, _, _ in self._FIELDS:
            setattr(t, name, getattr(self, name)[:n].copy())
        cm = CatMasks(n, lvm=self.cat_lvm)
        for nodes, feats, mat in self.cat_parts:
            cm.part[nodes] = len(cm.mats)
            cm.row[nodes] = np.arange(nodes.size, dtype=np.int32)
            cm.mats.append(mat)
            cm.feats.append(feats)
        for i, m in self.cat_left.items():
            cm.extra[i] = m
        t.cat_left = cm
        return t


class TreeGrower:
    """Grows one tree over a BinnedData with a given channel mode."""

    def __init__(self, bd, params: GrowParams):
        self.bd = bd
        self.p = params
        self.dev = bd.codes.device
        n = bd.nrows_local
        self.ridx = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.ridx2 = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.W = cloud.world()
        self.rank = cloud.rank()
        F = bd.F
        self.Fpad = ((F + self.W - 1) // self.W) * self.W
        self.Fl = self.Fpad // self.W
        self.f0 = self.rank * self.Fl
        self.is_cat_t = torch.tensor(bd.is_cat + [False] * (self.Fpad - F), dtype=torch.bool, device=self.dev)
        self.nbins_t = torch.tensor(bd.nbins + [0] * (self.Fpad - F), dtype=torch.int64, device=self.dev)
        mono = params.monotone if params.monotone is not None else np.zeros(F)
        self.mono_t = torch.tensor(list(mono) + [0] * (self.Fpad - F), dtype=torch.float64, device=self.dev)
        self.rng = np.random.RandomState(params.seed & 0x7FFFFFFF)
        if tree_ops.env("H2O3_HIST_BUDGET"):
            params.hist_mem_budget = int(os.environ["H2O3_HIST_BUDGET"])
        self.last_segs = None
        # per tree (_start_tree): number of the tree being grown (the first is 0), histogram scale,
        # the mode-0 response with 0/1 weights folded in as NaN and its [current, next] position-ordered
        # copies, categorical mask rows in flight to _mask_stage, look-ahead histograms of the next level
        self._tree_no = self._trees_grown = 0
        self._adaptive = self._unit_w = False
        self._stream_obj = self._vmax = self._va_eff = self._pos1 = self._mask_pend = self._la = self._last_wyy = None
        # per level (_start_level)
        self._level = self._depth = self._bnd_off = 0
        self._bnd = self._adapt_par = self._adapt_next = self._rng_par = self._rng_cur = None
        # lazy caches
        self._elig_dev, self._ok_cache = {}, {}
        self._ics_cache = self._qmask = self._is_cat_cpu = self._mono_f32 = self._nbins_t = None
        self._fcat_u8 = self._pw_t = self._cutmat = self._mask_stage = None
        self._d2h_ring, self._d2h_ev, self._d2h_k = [None, None], [None, None], 0

    # ------------------------------------------------------------------ hist
    def _hist_response(self, va, vb, mode, moved=False):
        """(va, vb, posv) a histogram kernel reads: the position-ordered
        payload when the tree keeps one, else the NaN-masked response, else the
        caller's channels.  moved=True reads the payload buffer the partition
        just wrote (_pos1[1]: the look-ahead runs before the buffers swap)."""
        if mode == 0 and self._pos1 is not None:
            # moved by the partition compaction: read coalesced, no row gather
            return self._pos1[1 if moved else 0], None, True
        if mode == 0 and self._va_eff is not None:
            return self._va_eff, None, False
        return va, vb, False

    def pos_payload(self):
        """The mode-0 response of the last grown tree in position order (the
        order of ridx), or None when the tree kept no such payload."""
        return self._pos1[0] if self._pos1 is not None else None

    def _build_hist(self, ridx, va, vb, mode, starts, counts, need_mask=None):
        if mode == 3:
            # uplift: treatment and control (w, w*y) histograms side by side
            with phase("tree.hist"):
                H1, _ = tree_ops.hist_build(self.bd, ridx, va, vb[0], 0, starts, counts, len(starts),
                                            vmax=self._vmax, posv=False, want_wyy=True)
                H2, _ = tree_ops.hist_build(self.bd, ridx, va, vb[1], 0, starts, counts, len(starts),
                                            vmax=self._vmax, posv=False, want_wyy=True)
            H = torch.cat([H1, H2], -1)
            self._last_wyy = None
            return self._rs_hist_wyy(H, None)[0] if self.W > 1 else H
        va, vb, posv = self._hist_response(va, vb, mode)
        with phase("tree.hist"), phase(f"tree.hist.L{self._level}"):
            H, wyy = tree_ops.hist_build(self.bd, ridx, va, vb, mode, starts, counts, len(starts), vmax=self._vmax,
                                         posv=posv, want_wyy=True, unit_w=self._unit_w, need_mask=need_mask)
        if self.W > 1:
            H, wyy = self._rs_hist_wyy(H, wyy)
        self._last_wyy = wyy
        return H  # [Fl, n, Bs, C]

    def _rs_hist_wyy(self, H, wyy):
        """Multi-GPU reduce of a level histogram [F, n, Bs, C]: reduce-scatter
        by feature (each rank keeps its Fl features), with the per-node w*y*y
        sums riding along -- every rank's chunk carries a copy of its local
        wyy, so the scattered chunk ends in the global sums: ONE collective
        per level instead of reduce_scatter + all_reduce."""
        W = self.W
        if self.Fpad > self.bd.F:
            H = torch.cat([H, torch.zeros((self.Fpad - self.bd.F,) + tuple(H.shape[1:]), dtype=H.dtype,
                                          device=H.device)], 0)
        if wyy is None:
            return coll.reduce_scatter_dim0(H), None
        n = wyy.numel()
        loc = H.shape[1:]
        buf = torch.cat([H.reshape(W, -1), wyy.to(H.dtype).view(1, n).expand(W, n)], 1)
        out = coll.reduce_scatter_dim0(buf).view(-1)
        chunk = out.numel() - n
        return out[:chunk].view((self.Fl,) + tuple(loc)), out[chunk:]

    def _hist_need(self, cm):
        """Per-node features whose histograms the split search reads: the
        sampled columns plus each rank's first local feature (node totals come
        from H[0]).  None = all (no column sampling / no GPU kernels)."""
        if self.dev.type != "cuda" or getattr(cm, "_all_true", False) or self.p.criterion.startswith("uplift") \
                or tree_ops.env("H2O3_HIST_NEED", "1") == "0":
            return None
        need = cm.to(self.dev, dtype=torch.bool).clone()
        for r in range(self.W):
            if r * self.Fl < self.bd.F:
                need[:, r * self.Fl] = True
        return need

    # ------------------------------------------------------------------ splits
    def _col_sel(self, n_nodes, depth):
        """Per-node sampled columns as a [n, k] int64 tensor of global feature
        ids in ascending order (k random eligible features per node: the k
        smallest of per-(node, feature) uniform keys, on the device when the
        data is -- deep DRF levels have 10^4+ nodes), or None when every
        eligible feature is scored.  Consumes the tree's RNG exactly like the
        mask path so both give the same samples."""
        p = self.p
        F = self.bd.F
        base = np.ones(F, dtype=bool) if p.tree_col_mask is None else p.tree_col_mask.astype(bool)
        k, n_elig = self._sample_k(depth)
        if k >= n_elig:
            return None
        elig = np.nonzero(base)[0]
        if self.dev.type == "cuda":
            # one HIP launch: per-node selection sampling, rows come out sorted
            # (was rand + top-k + gather + segmented sort, with a host sync)
            seed = int(self.rng.randint(0, 2 ** 31 - 1))
            el = self._elig_dev
            key = elig.tobytes()
            if key not in el:
                el.clear()
                el[key] = self._upload_elig(elig)
            return tree_ops.col_sample(n_nodes, el[key], k, seed)
        keys = self.rng.random_sample((n_nodes, len(elig)))
        sel = np.argpartition(keys, k - 1, axis=1)[:, :k]
        return torch.from_numpy(np.sort(elig[sel], axis=1))

    def _upload_elig(self, elig):
        """The eligible feature ids on the device without a host wait: a
        pageable H2D copy waits for the queued kernels (the look-ahead
        pipeline stalled once per tree, ~1 ms), so the ids go through the
        pinned upload ring (non-blocking) and a stream-ordered device copy
        that outlives the ring slot (the ids are cached for the tree)."""
        return tree_ops._h2d(elig.astype(np.int64), self.dev).clone()

    def _col_mask_allowed(self, allow, depth):
        """Per-node mask under interaction constraints, on the device: the
        branch's allowed features (BranchInteractionConstraints) intersected
        with the per-tree column mask, then column sampling among them
        (DTree.UndecidedNode.scoreCols samples from the columns that still have
        histograms): k smallest of per-(node, feature) uniform keys among each
        node's eligible features -- no per-node host loop."""
        p = self.p
        F = self.bd.F
        dev = allow.device
        base = torch.ones(F, dtype=torch.bool, device=dev) if p.tree_col_mask is None else \
            torch.as_tensor(p.tree_col_mask.astype(bool), device=dev)
        m = allow & base.view(1, -1)
        n = m.shape[0]
        rate = p.col_sample_rate * (p.col_sample_rate_change_per_level ** depth)
        if (p.mtries is not None and p.mtries > 0) or rate < 1.0:
            cnt = m.sum(1)
            if p.mtries is not None and p.mtries > 0:
                k = torch.full_like(cnt, int(p.mtries))
            else:
                k = torch.floor(rate * cnt.to(torch.float64) + 0.5).to(cnt.dtype).clamp(min=1)
            g = torch.Generator(device=dev)
            g.manual_seed(int(self.rng.randint(0, 2 ** 31 - 1)))
            keys = torch.rand((n, F), generator=g, device=dev)
            keys = torch.where(m, keys, torch.full_like(keys, 2.0))
            rank = torch.argsort(torch.argsort(keys, 1), 1)
            m = m & (rank < k.view(-1, 1))
        if self.Fpad > F:
            m = torch.cat([m, torch.zeros((n, self.Fpad - F), dtype=torch.bool, device=dev)], 1)
        m = m.contiguous()
        m._all_true = False
        return m

    def _col_mask(self, n_nodes, depth, sel=None, allow=None):
        """[n, Fpad] bool mask of features eligible per node."""
        p = self.p
        F = self.bd.F
        if allow is not None:
            return self._col_mask_allowed(allow, depth)
        if sel is None:
            sel = self._col_sel(n_nodes, depth)
        if sel is not None:
            m = torch.zeros((n_nodes, self.Fpad), dtype=torch.bool, device=sel.device)
            m.scatter_(1, sel, True)
            m._all_true = False
            return m
        base = np.ones(F, dtype=bool) if p.tree_col_mask is None else p.tree_col_mask.astype(bool)
        m = np.tile(base, (n_nodes, 1))
        all_true = bool(m.all())
        if self.Fpad > F:
            m = np.concatenate([m, np.zeros((n_nodes, self.Fpad - F), dtype=bool)], 1)
        t = torch.from_numpy(m)
        t._all_true = all_true
        return t

    def _interaction_map(self):
        """(allow [F, F] bool: features that may follow a split on f, root [F]
        bool) from GrowParams.interaction_sets, or None."""
        sets = self.p.interaction_sets
        if not sets:
            return None
        F = self.bd.F
        if self._ics_cache is not None:
            return self._ics_cache
        allow = np.zeros((F, F), dtype=bool)
        root = np.zeros(F, dtype=bool)
        for st in sets:
            idx = np.asarray(sorted(st), dtype=np.int64)
            root[idx] = True
            for f in idx:
                allow[f, idx] = True
        self._ics_cache = (allow, root)
        return self._ics_cache

    # ------------------------------------------------------------------ monotone node bounds
    def _bnd_dev(self, n):
        """[n, 2] f64 (lo, hi) prediction bounds of the frontier nodes being
        scored, or None when no node is bounded."""
        if self._bnd is None:
            return None
        return self._bnd[self._bnd_off:self._bnd_off + n]

    def _bound_cost(self, Lb, Rb, lo, hi):
        """(gain penalty of clamping the children's constants into [lo, hi],
        violated?) for left / right channel sums [..., C]."""
        p = self.p
        if p.criterion == "xgb":
            al, ar = Lb[..., 1] + p.reg_lambda, Rb[..., 1] + p.reg_lambda
            pl, pr = -Lb[..., 0] / al, -Rb[..., 0] / ar
            al, ar = 0.5 * al, 0.5 * ar
        else:
            al, ar = Lb[..., 0], Rb[..., 0]
            pl, pr = Lb[..., 1] / al.clamp_min(1e-300), Rb[..., 1] / ar.clamp_min(1e-300)
        cl, cr = torch.minimum(torch.maximum(pl, lo), hi), torch.minimum(torch.maximum(pr, lo), hi)
        viol = (cl != pl) | (cr != pr)
        return al * (cl - pl) ** 2 + ar * (cr - pr) ** 2, viol

    def _bound_winners(self, res):
        """Per-node check of already selected winners (categorical pair
        paths): clamp penalty or veto for splits outside the node bounds."""
        n = res["gain"].shape[0]
        bnd = self._bnd_dev(n)
        if bnd is None:
            return res
        pen, viol = self._bound_cost(res["L"].to(torch.float64), res["R"].to(torch.float64), bnd[:, 0], bnd[:, 1])
        g = res["gain"].to(torch.float64)
        g = torch.where(viol & torch.isfinite(g), g - pen if self.p.use_bounds else torch.full_like(g, NEG_INF), g)
        res = dict(res)
        res["gain"] = g
        return res

    def _child_bounds(self, lo, hi, f_s, cat_s, Lsel, Rsel, mode):
        """Constraints.withNewConstraint for the children of the split nodes:
        bounds at the midpoint of the (clamped) child predictions on
        increasing / decreasing columns, inherited otherwise."""
        p = self.p
        mono = np.asarray(p.monotone, dtype=np.float64)
        c = np.where(cat_s | (f_s >= mono.size), 0.0, mono[np.minimum(f_s, mono.size - 1)])
        if p.criterion == "xgb":
            pl = -Lsel[:, 0] / (Lsel[:, 1] + p.reg_lambda)
            pr = -Rsel[:, 0] / (Rsel[:, 1] + p.reg_lambda)
        else:
            pl = Lsel[:, 1] / np.maximum(Lsel[:, 0], 1e-300)
            pr = Rsel[:, 1] / np.maximum(Rsel[:, 0], 1e-300)
        mid = 0.5 * (np.clip(pl, lo, hi) + np.clip(pr, lo, hi))
        lo_l, hi_l, lo_r, hi_r = lo.copy(), hi.copy(), lo.copy(), hi.copy()
        inc, dec = c > 0, c < 0
        hi_l[inc] = np.minimum(hi[inc], mid[inc])
        lo_r[inc] = np.maximum(lo[inc], mid[inc])
        lo_l[dec] = np.maximum(lo[dec], mid[dec])
        hi_r[dec] = np.minimum(hi[dec], mid[dec])
        return np.stack([lo_l, lo_r], 1).reshape(-1), np.stack([hi_l, hi_r], 1).reshape(-1)

    # ------------------------------------------------------------------ adaptive bins
    _RR_TYPES = ("uniformadaptive", "uniformadaptive", "random", "quantilesglobal")

    def _tree_hist_type(self):
        """Histogram type of the tree being grown: RoundRobin cycles the
        reference's ROUND_ROBIN_CANDIDATES (AUTO counts as UniformAdaptive,
        SharedTreeModel.java:59) tree by tree."""
        ht = getattr(self.bd, "hist_type", "auto")
        if ht == "roundrobin":
            return self._RR_TYPES[(int(self.p.seed) + self._tree_no) % 4]
        return ht

    def _adapt_hist(self, H):
        """Per-node adaptive binning of the numeric features (reference
        UniformAdaptive / Random, DHistogram.java:366-386, DTree.java:337).  The
        level histogram is on the fixed fine grid of nbins_top_level cells; the
        reference re-bins each (node, column) into
        nb = max(nbins_top_level >> (depth - 1), nbins) uniform bins over the
        parent's observed range (_adapt_range).  Here each run of fine bins that falls into one coarse
        bin is folded into the run's LAST fine bin: every cumulative sum at an
        allowed boundary is unchanged and every other boundary repeats the sums
        of the previous allowed one, so any split search on the folded
        histogram picks only coarse boundaries (ties go to the lower code).
        Random draws the cut subset per (tree, level, node, feature); a
        RoundRobin tree on QuantilesGlobal keeps only the boundaries next to the
        global quantiles.  Categorical features and the NA bin are untouched."""
        ht = self._tree_hist_type()
        if ht not in ("uniformadaptive", "random", "quantilesglobal") or \
                getattr(self.bd, "hist_type", "auto") not in ("uniformadaptive", "random", "roundrobin"):
            return H
        Fl, n, Bs, C = H.shape
        B = Bs - 1
        depth = self._depth
        # bins per node: nbins_top_level at the root AND its children, halved per
        # level below (the reference fixture's splits, gbm_variable_importance.zip,
        # sit on 1024 / 512 / 256 / 128 cells of the parent's range at depths 1-4)
        nb = max(self.bd.nbins_top >> max(depth - 1, 0), self.bd.nbins_node)
        f0 = self.f0
        isnum = ~self.is_cat_t[f0:f0 + Fl]
        if ht == "uniformadaptive" and nb >= B:
            return H
        dev = H.device
        if ht == "uniformadaptive" and dev.type == "cuda" and C <= 4 and tree_ops.env("H2O3_UA_FOLD") != "torch":
            return self._adapt_hist_dev(H, Fl, n, Bs, C, nb, isnum, depth)
        Hn = H[:, :, :B]
        occ = (Hn != 0).any(-1)                                   # [Fl, n, B]
        idx = torch.arange(B, device=dev)
        first = torch.where(occ, idx, B).amin(-1, keepdim=True)
        last = torch.where(occ, idx, -1).amax(-1, keepdim=True)
        first, last = self._adapt_range(first, last, n, Fl, depth)
        L = (last - first + 1).clamp(min=1)
        inr = (idx >= first) & (idx <= last)
        if ht == "uniformadaptive":
            coarse = torch.div((idx - first).clamp(min=0) * nb, L, rounding_mode="floor")
            nxt = torch.div((idx + 1 - first).clamp(min=0) * nb, L, rounding_mode="floor")
            is_end = inr & ((coarse != nxt) | (idx == last))
            is_end = is_end | (inr & (L <= nb))                   # narrow range: every boundary
        elif ht == "random":
            # per (tree, level, node, feature, bin) uniform draw: keep ~nb - 1 cuts
            key = (torch.arange(Fl, device=dev).view(-1, 1, 1) + f0) * 1000003 + \
                torch.arange(n, device=dev).view(1, -1, 1) * 7919 + idx.view(1, 1, -1) * 104729 + \
                (int(self.p.seed) * 31 + self._tree_no * 131 + depth * 17)
            key = (key * 0x9E3779B1) & 0xFFFFFFFF
            key = ((key ^ (key >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
            u = (key ^ (key >> 12)).to(torch.float64) / 4294967296.0
            pk = ((nb - 1) / (L - 1).clamp(min=1).to(torch.float64))
            is_end = inr & ((u < pk) | (idx == last))
        else:
            qm = self._qmask
            if qm is None:
                qm = torch.zeros((self.Fpad, B), dtype=torch.bool, device=dev)
                for j, qb in enumerate(self.bd.qbounds or []):
                    if qb is not None and len(qb):
                        qm[j, torch.as_tensor(np.minimum(qb, B - 1), device=dev)] = True
                self._qmask = qm
            is_end = inr & (qm[f0:f0 + Fl].view(Fl, 1, B) | (idx == last))
        is_end = is_end | ~isnum.view(Fl, 1, 1)                   # categorical: unchanged
        cs = torch.cumsum(Hn.to(torch.float64), 2)
        E = torch.where(is_end, idx, -1)
        pe_incl = torch.cummax(E, 2).values
        pe = torch.cat([torch.full_like(pe_incl[:, :, :1], -1), pe_incl[:, :, :-1]], 2)
        base = torch.where((pe >= 0).unsqueeze(-1), torch.gather(cs, 2, pe.clamp(min=0).unsqueeze(-1).expand(-1, -1, -1, C)),
                           torch.zeros_like(cs))
        Hf = torch.where(is_end.unsqueeze(-1), cs - base, torch.zeros_like(cs)).to(H.dtype)
        Hf = torch.where(isnum.view(Fl, 1, 1, 1), Hf, Hn)
        return torch.cat([Hf, H[:, :, B:]], 2).contiguous()

    def _adapt_hist_dev(self, H, Fl, n, Bs, C, nb, isnum, depth):
        """UniformAdaptive fold on the device (tree_split.hip ua_range_kernel /
        ua_fold_kernel): the same first / last, parent-range rule and run-end
        folding as the torch chain of _adapt_hist, one wave per (feature,
        node) row, H read twice and written once."""
        lib = _native.get_lib("tree_split")
        if lib is None:
            raise RuntimeError("tree_split native library missing (UniformAdaptive fold)")
        H = H.contiguous()
        rows = Fl * n
        fl = torch.empty(2 * rows, dtype=torch.int32, device=H.device)
        s = stream()
        check(lib.h2o_ua_range(ptr(H), rows, Bs, C, ptr(fl), ptr(fl[rows:]), s), "h2o_ua_range")
        first, last = fl[:rows].view(Fl, n, 1).long(), fl[rows:].view(Fl, n, 1).long()
        first, last = self._adapt_range(first, last, n, Fl, depth)
        fr_ = first.to(torch.int32).contiguous()
        la_ = last.to(torch.int32).contiguous()
        isn = isnum.to(torch.uint8).contiguous()
        out = torch.empty_like(H)
        check(lib.h2o_ua_fold(ptr(H), Fl, n, Bs, C, ptr(fr_), ptr(la_), int(nb), ptr(isn), ptr(out), s), "h2o_ua_fold")
        return out

    def _adapt_range(self, first, last, n, Fl, depth):
        """Code range [first, last] ([Fl, n, 1]) each node's coarse bins span.
        The reference bins a child over its PARENT's observed range of each
        column, and the split column over the parent's range cut at the split
        (DTree.java:337-372, nextLevelHistos); at depth 1 the coarse grid is
        then exactly every (1024 >> 1)-th top-level cell.  The node's own
        occupied range is recorded for its children; without a parent record
        (root, chunk / frontier shapes that do not line up) the node's own
        range is used."""
        off = self._bnd_off
        cur = self._rng_cur
        n_level = off + n if cur is None or off == 0 else max(cur[0].shape[1], off + n)
        if cur is None or off == 0 or cur[0].shape[1] < n_level:
            nf = torch.zeros((Fl, n_level, 1), dtype=first.dtype, device=first.device)
            nl = torch.zeros_like(nf)
            if cur is not None and off > 0:
                k = min(cur[0].shape[1], n_level)
                nf[:, :k], nl[:, :k] = cur[0][:, :k], cur[1][:, :k]
            cur = self._rng_cur = (nf, nl)
        cur[0][:, off:off + n], cur[1][:, off:off + n] = first, last
        par = self._adapt_par
        rp = self._rng_par
        if depth == 0 or par is None or rp is None or rp[0].shape[0] != Fl:
            return first, last
        sids, fs, ts, opts, n_front = par
        if 2 * len(sids) != n_front or off + n > n_front:
            return first, last
        j = np.arange(off, off + n)
        pi = torch.as_tensor(sids[j // 2], device=first.device)
        pf, pl = rp[0][:, pi].clone(), rp[1][:, pi].clone()       # [Fl, n, 1]
        # the split column: left child codes <= t, right child codes > t
        fl = fs[j // 2] - self.f0
        ok = (fl >= 0) & (fl < Fl) & (opts[j // 2] != 2)
        if ok.any():
            jj = np.nonzero(ok)[0]
            side = (j[jj] % 2).astype(bool)
            t = torch.as_tensor(ts[j // 2][jj], device=first.device, dtype=first.dtype)
            fi = torch.as_tensor(fl[jj], device=first.device)
            ji = torch.as_tensor(jj, device=first.device)
            sd = torch.as_tensor(side, device=first.device)
            cf, cl = pf[fi, ji, 0], pl[fi, ji, 0]
            pf[fi, ji, 0] = torch.where(sd, torch.maximum(cf, t + 1), cf)
            pl[fi, ji, 0] = torch.where(sd, cl, torch.minimum(cl, t))
        # empty nodes / columns keep their own (empty) range
        use = (pf <= pl) & (first <= last)
        return torch.where(use, pf, first), torch.where(use, pl, last)

    def _find_splits(self, H, col_mask, node_wyy=None, want_pk=False):
        """Dispatch: fused HIP kernel for numeric features on GPU (categorical
        features, which need a per-node sort of bins, go through the torch path)."""
        H = self._adapt_hist(H)
        if self.dev.type != "cuda" or self.p.criterion.startswith("uplift"):
            Fl_ = H.shape[0]
            cmf = col_mask[:, self.f0:self.f0 + Fl_]
            if not self.p.criterion.startswith("uplift") and cmf.numel() and float(cmf.float().mean()) < 0.5:
                # few eligible features per node (DRF mtries): score only those pairs
                res = self._cat_splits_pairs(H, col_mask, list(range(Fl_)), node_wyy)
                res = self._bound_winners(res)
                res["tot"] = H[0].to(torch.float64).sum(1) if Fl_ > 0 else None
                if self.W > 1:
                    res = self._merge_candidates(res, H.shape[1], H.shape[2], H.shape[3])
                return res
            return self._find_splits_torch(H, col_mask, node_wyy)
        Fl = H.shape[0]
        fsl = slice(self.f0, self.f0 + Fl)
        if self._is_cat_cpu is None:
            self._is_cat_cpu = self.is_cat_t[fsl].cpu()
        is_cat = self._is_cat_cpu
        if bool(is_cat.all()):
            return self._find_splits_torch(H, col_mask, node_wyy)
        if not bool(is_cat.any()):
            # want_pk on a numeric-only frame: every rank takes the packed-record
            # path (split_select2 + one record merge), so the collectives match
            res = self._find_splits_native(H, col_mask, node_wyy,
                                           want_pk=want_pk and not any(self.bd.is_cat))
            if self.W > 1 and "pk" not in res:
                res = self._merge_candidates(res, H.shape[1], H.shape[2], H.shape[3])
            return res
        cm_num = col_mask.clone()
        cm_num[:, fsl] &= ~is_cat.to(cm_num.device).view(1, -1)
        res = self._find_splits_native(H, cm_num, node_wyy)
        if bool(is_cat.any()):
            cat_local = torch.nonzero(is_cat).flatten().tolist()
            rc = self._bound_winners(self._cat_splits_pairs(H, col_mask, cat_local, node_wyy))
            better = rc["gain"] > res["gain"]
            for k in res:
                if res[k] is None or k == "tot":
                    continue
                b = better.view(-1, *([1] * (res[k].dim() - 1))) if res[k].dim() > 1 else better
                res[k] = torch.where(b, rc[k].to(res[k].dtype), res[k])
        if self.W > 1:
            res = self._merge_candidates(res, H.shape[1], H.shape[2], H.shape[3])
        return res

    def _find_splits_native(self, H, col_mask, node_wyy, want_pk=False):
        p = self.p
        Fl, n, Bs, C = H.shape
        lib = _native.get_lib("tree_split")
        fsl = slice(self.f0, self.f0 + Fl)
        cm = col_mask[:, fsl]
        if getattr(col_mask, "_all_true", False) and self.f0 + Fl <= self.bd.F:
            # no column sampling: a cached device mask of ones per frontier size
            ok = self._ok_cache.get(n)
            if ok is None:
                ok = self._ok_cache[n] = torch.ones((n, Fl), dtype=torch.uint8, device=self.dev)
        else:
            ok = cm.to(torch.uint8).contiguous()
            ok = tree_ops._h2d(ok.numpy(), self.dev) if ok.device.type == "cpu" else ok
            if self.f0 + Fl > self.bd.F:
                ok[:, max(0, self.bd.F - self.f0):] = 0
        if self._mono_f32 is None:
            self._mono_f32 = self.mono_t[fsl].to(torch.float32).contiguous()
        mono = self._mono_f32
        H = H.contiguous()
        wyy = node_wyy.to(torch.float64).contiguous() if node_wyy is not None else \
            torch.zeros(n, dtype=torch.float64, device=self.dev)
        out = torch.empty((n * Fl, 4), dtype=torch.float64, device=self.dev)
        crit = 1 if p.criterion == "xgb" else 0
        bnd = self._bnd_dev(n)
        check(lib.h2o_split_find_b(ptr(H), Fl, n, Bs, ptr(wyy), ptr(ok), ptr(mono), float(p.min_rows),
                                   float(p.min_split_improvement), float(p.reg_lambda), float(p.reg_alpha),
                                   float(p.gamma), crit, ptr(out), ptr(bnd), int(bool(p.use_bounds)), stream()),
              "h2o_split_find_b")
        if C == 2 and want_pk and (self.W > 1 or self.f0 < self.bd.F):
            # selection + split decision + partition inputs in one kernel; the
            # packed record (12 doubles per node) is what the host fetches
            # 13 fields: split_select2's 12 + the node's NA weight on the chosen column
            pk = torch.empty((n, 13), dtype=torch.float64, device=self.dev)
            mask = torch.empty((n, Bs), dtype=torch.uint8, device=self.dev)
            feat_i = torch.empty(n, dtype=torch.int32, device=self.dev)
            if self.f0 < self.bd.F:
                min_w2 = -1.0 if p.criterion == "xgb" else 2.0 * float(p.min_rows)
                check(lib.h2o_split_select2(ptr(out), ptr(H), Fl, n, Bs, self.f0, min_w2, 13, ptr(pk), ptr(mask),
                                            ptr(feat_i), stream()), "h2o_split_select2")
            else:
                # a rank holding only padding features: a never-winning record
                pk.zero_()
                pk[:, 0] = NEG_INF
                mask.zero_()
                feat_i.zero_()
            if self.W > 1:
                pk, mask, feat_i = self._merge_records(pk, mask)
            return {"pk": pk, "feat_i32": feat_i, "mask": mask, "gain": pk[:, 0], "feat": pk[:, 1], "t": pk[:, 2],
                    "opt": pk[:, 3], "L": pk[:, 4:6], "R": pk[:, 6:8], "tot": pk[:, 8:10]}
        if C == 2 and self.f0 < self.bd.F:
            # fused per-node selection + mask kernel: few launches, one packed record
            pk = torch.empty((n, 10), dtype=torch.float64, device=self.dev)
            mask = torch.empty((n, Bs), dtype=torch.uint8, device=self.dev)
            check(lib.h2o_split_select(ptr(out), ptr(H), Fl, n, Bs, self.f0, ptr(pk), ptr(mask), stream()),
                  "h2o_split_select")
            opt = pk[:, 3].long()
            return {"gain": pk[:, 0], "feat": pk[:, 1].long(), "t": pk[:, 2].long(), "opt": opt,
                    "na_left": opt == 1, "mask": mask, "L": pk[:, 4:6], "R": pk[:, 6:8], "tot": pk[:, 8:10]}
        gain = out[:, 0].view(n, Fl)
        ints = out.view(torch.int32).view(n * Fl, 8)[:, 6:8]
        best, fl = gain.max(1)
        idx = torch.arange(n, device=self.dev) * Fl + fl
        t = ints[idx, 0].long()
        opt = ints[idx, 1].long()
        Lw = out[idx, 1:3]
        T = H[0].sum(1) if self.f0 < self.bd.F else torch.zeros((n, C), dtype=H.dtype, device=H.device)
        B = Bs - 1
        codes = torch.arange(Bs, device=self.dev).view(1, Bs)
        mask = (codes <= t.view(n, 1)) & (codes < B)
        mask = torch.where((opt == 2).view(n, 1), codes < B, mask)
        mask[:, Bs - 1] = opt == 1
        return {"gain": best, "feat": fl + self.f0, "t": t, "opt": opt, "na_left": opt == 1,
                "mask": mask.to(torch.uint8), "L": Lw, "R": T - Lw, "tot": T}

    def _cat_splits_pairs(self, H, col_mask, sub, node_wyy):
        """Categorical splits scored only on the eligible (node, feature) pairs
        (mtries / column sampling usually leave a few per node): levels sorted
        by mean response per pair (DTree.findBestSplitPoint for categoricals),
        prefix sums, the three NA options, best pair per node by a segment
        arg-max (lowest feature on ties).  On the GPU every pair is one
        workgroup of the HIP kernel `cat_pair_kernel` (tree_split.hip); the
        winners' split masks are then rebuilt from their own bins."""
        p = self.p
        Fl, n, Bs, C = H.shape
        B = Bs - 1
        dev = H.device
        sub_t = torch.as_tensor(sub, dtype=torch.long, device=dev)
        gidx = sub_t + self.f0
        cm = col_mask.to(dev)[:, gidx] & (gidx < self.bd.F).view(1, -1)
        nz = torch.nonzero(cm)
        ninf = torch.full((n,), NEG_INF, dtype=torch.float64, device=dev)
        out = {"gain": ninf, "feat": torch.zeros(n, dtype=torch.long, device=dev),
               "t": torch.zeros(n, dtype=torch.long, device=dev), "opt": torch.zeros(n, dtype=torch.long, device=dev),
               "na_left": torch.zeros(n, dtype=torch.bool, device=dev),
               "mask": torch.zeros((n, Bs), dtype=torch.uint8, device=dev),
               "L": torch.zeros((n, C), dtype=torch.float64, device=dev),
               "R": torch.zeros((n, C), dtype=torch.float64, device=dev), "tot": None}
        if nz.shape[0] == 0:
            return out
        node_i, j = nz[:, 0], nz[:, 1]
        pcat = self.is_cat_t[gidx[j]]                              # numeric pairs keep bin order
        mono_p = self.mono_t[gidx[j]]
        if dev.type == "cuda" and C >= 2 and B <= 4096 and H.dtype == torch.float64:
            best, k = self._pairs_native(H, sub_t[j], node_i, pcat, mono_p, node_wyy)
        else:
            st = self._pair_stats(H[sub_t[j], node_i].to(torch.float64), pcat)
            allg = self._pair_gains(st, mono_p.view(-1, 1), node_wyy, node_i)
            best, k = allg.max(1)
        return self._pair_winners(out, best, k, node_i, gidx[j], pcat, lambda wp: H[sub_t[j[wp]], node_i[wp]])

    def _sample_k(self, depth):
        """(k, n_eligible): columns scored per node at this depth."""
        p = self.p
        base_n = self.bd.F if p.tree_col_mask is None else int(np.count_nonzero(p.tree_col_mask))
        rate = p.col_sample_rate * (p.col_sample_rate_change_per_level ** depth)
        if p.mtries is not None and p.mtries > 0:
            k = p.mtries
        elif rate < 1.0:
            k = max(1, int(math.floor(rate * base_n + 0.5)))
        else:
            k = base_n
        return min(k, base_n), base_n

    def _sampled_cols(self, depth):
        """True when the split search at this depth sees a per-node subset
        of the columns (mtries / col_sample_rate(_change_per_level) /
        col_sample_rate_per_tree)."""
        k, ne = self._sample_k(depth)
        return k < self.bd.F

    def _direct_level(self, mode, depth, chunked):
        """Row-direct pair histograms for this level (tree_ops.pair_hist):
        column-sampled splits where at most a quarter of the features are
        scored per node (DRF's sqrt(F) mtries) or the level histogram would
        need node batching (H2O3_PAIR_DIRECT=auto); at every sampled level
        (=1); never (=0).  Measured on the DRF config (10M x 500, 100
        categoricals of cardinality 1000): 995 ms/tree with level histograms,
        ~500 ms/tree with pair histograms at every sampled level."""
        env = tree_ops.env("H2O3_PAIR_DIRECT", "auto")
        if env == "0" or mode not in (0, 1) or self.p.criterion.startswith("uplift") or \
                not self._sampled_cols(depth):
            return False
        if self.dev.type == "cuda" and self.bd.codes_col is None:
            return False
        k, _ = self._sample_k(depth)
        return env == "1" or chunked or 4 * k <= self.bd.F

    def _flush_masks(self, tb):
        """Collect the categorical mask rows of the previous level from the
        pinned staging buffer into the tree (waits on the copy's event: by the
        time the next level's record arrived it has completed)."""
        if self._mask_pend is None:
            return
        nodes, feats, shape, ev = self._mask_pend
        ev.synchronize()
        n = int(np.prod(shape))
        tb.cat_parts.append((nodes, feats, self._mask_stage[:n].numpy().reshape(shape).copy()))
        self._mask_pend = None

    def _narrow_bins(self):
        """Per-feature code counts [F] int32 on the device when the pair path
        may bound its work by each feature's bins (histograms wider than 256
        bins: H2O3_PAIR_NARROW), else None."""
        if self.dev.type != "cuda" or self.bd.Bs - 1 <= 256 or tree_ops.env("H2O3_PAIR_NARROW", "1") != "1":
            return None
        if self._nbins_t is None:
            nb = np.minimum(np.asarray(self.bd.nbins[:self.bd.F], dtype=np.int64), self.bd.Bs - 1)
            self._nbins_t = torch.as_tensor(nb.astype(np.int32), device=self.dev)
        return self._nbins_t

    def _all_levels_direct(self, mode):
        """True when every level of the tree takes the device pair path (a
        fixed per-node column sample of at most a quarter of the features),
        so no level-histogram kernel ever reads the response by row."""
        p = self.p
        if mode != 0 or self.dev.type != "cuda" or self.bd.codes_col is None or p.criterion.startswith("uplift"):
            return False
        if tree_ops.env("H2O3_PAIR_DIRECT", "auto") == "0":
            return False
        if not (p.mtries is not None and p.mtries > 0) or p.col_sample_rate_change_per_level != 1.0:
            return False
        k, _ = self._sample_k(0)
        return k < self.bd.F and 4 * k <= self.bd.F

    def _pair_direct_splits(self, ridx, va, vb, mode, f_st, f_ct, cm):
        """Best split of every frontier node from row-direct histograms of its
        sampled (node, feature) pairs only: pair histograms built from the rows
        (HIP `pair_hist_kernel`), scored per pair (`cat_pair_kernel`: numeric
        bin order or categorical levels sorted by mean response, three NA
        options), per-node winner + mask (_pair_winners).  Pairs are processed
        in node batches under hist_mem_budget.  Every rank sums the pair
        histograms (all-reduce) and scores all pairs, so no candidate merge."""
        p = self.p
        bd, dev = self.bd, self.dev
        F, Bs, C = bd.F, bd.Bs, 2
        n = len(f_st)
        va, vb, posv = self._hist_response(va, vb, mode)
        st = np.asarray(f_st, dtype=np.int64)
        ct = np.asarray(f_ct, dtype=np.int64)
        nz = torch.nonzero(cm[:, :F]).cpu().numpy()           # node-major pairs
        pn_all, pf_all = nz[:, 0].astype(np.int64), nz[:, 1].astype(np.int64)
        per_pairs = max(1, int(p.hist_mem_budget // (Bs * C * 8)))
        cum = np.cumsum(np.bincount(pn_all, minlength=n))     # pairs of nodes [0, i]
        parts = []
        a = 0
        while a < n:
            base = int(cum[a - 1]) if a > 0 else 0
            b = min(n, max(a + 1, int(np.searchsorted(cum, base + per_pairs, side="right"))))
            lo, hi = base, int(cum[b - 1])
            parts.append(self._pair_direct_part(ridx, va, vb, mode, posv, st[a:b], ct[a:b], pn_all[lo:hi] - a,
                                                pf_all[lo:hi]))
            a = b
        if len(parts) == 1:
            return parts[0]
        return {k: torch.cat([q[k] for q in parts], 0) for k in parts[0]}

    def _pair_direct_dev(self, ridx, va, vb, mode, f_st, f_ct, sel):
        """Device-resident version of _pair_direct_splits: pairs from the
        [n, k] column sample on the device, pair histograms
        (pair_hist_kernel), per-pair scoring (cat_pair_kernel) and the
        per-node winner / record / mask (pair_select_kernel) -- the level's
        split record comes out in the packed form of split_select2, so the
        async partition and the single host transfer of the level apply."""
        p = self.p
        bd, dev = self.bd, self.dev
        Bs = bd.Bs
        if sel is None:
            # no per-node sampling (only the per-tree column mask): every eligible feature
            base = np.ones(bd.F, dtype=bool) if p.tree_col_mask is None else p.tree_col_mask.astype(bool)
            elig = torch.as_tensor(np.nonzero(base)[0], device=dev)
            sel = elig.view(1, -1).expand(len(f_st), -1)
        n, k = sel.shape
        va, vb, posv = self._hist_response(va, vb, mode)
        lib = _native.get_lib("tree_split")
        if self._fcat_u8 is None:
            self._fcat_u8 = self.is_cat_t[:bd.F].to(torch.uint8).contiguous()
        st = np.asarray(f_st, dtype=np.int64)
        ct = np.asarray(f_ct, dtype=np.int64)
        per = max(1, int(p.hist_mem_budget // (k * Bs * 2 * 8)))
        pk = torch.empty((n, 13), dtype=torch.float64, device=dev)
        mask = torch.empty((n, Bs), dtype=torch.uint8, device=dev)
        feat_i = torch.empty(n, dtype=torch.int32, device=dev)
        min_w2 = -1.0 if p.criterion == "xgb" else 2.0 * float(p.min_rows)
        for a in range(0, n, per):
            b = min(n, a + per)
            sl = sel[a:b]
            with phase("tree.hist"), phase("tree.hist.pairs"):
                Hp, wyy_n, pfeat = tree_ops.pair_hist_dev(bd, ridx, va, vb, mode, st[a:b], ct[a:b], sl, self._vmax,
                                                          posv=posv, fbins=self._narrow_bins())
            nb = b - a
            if self.W > 1:
                # node-sharded reduction: every rank receives the summed pair
                # histograms of 1/W of the nodes, packed at each feature's own
                # width (sparse at deep levels: _pair_exchange), scores and
                # selects those nodes, and only the small per-node records are
                # all-gathered
                W = self.W
                npad = -(-nb // W) * W
                wv = wyy_n if wyy_n is not None else torch.zeros(nb, dtype=torch.float64, device=dev)
                nl = npad // W
                lo = self.rank * nl
                pn_all = torch.arange(nb, device=dev).repeat_interleave(k)
                Hmine = self._pair_exchange(Hp.view(nb * k, Bs, 2), pfeat.long(), pn_all, nb, full=False)
                if npad > nb:
                    wv = torch.cat([wv, torch.zeros(npad - nb, dtype=wv.dtype, device=dev)], 0)
                    pfeat = torch.cat([pfeat, torch.zeros((npad - nb) * k, dtype=pfeat.dtype, device=dev)], 0)
                Hl = torch.zeros((nl * k, Bs, 2), dtype=Hp.dtype, device=dev)
                Hl[:Hmine.shape[0]] = Hmine
                wl = coll.reduce_scatter_dim0(wv.contiguous()) if wyy_n is not None else None
                del Hp, Hmine
                pk_l = torch.empty((nl, 13), dtype=torch.float64, device=dev)
                mask_l = torch.empty((nl, Bs), dtype=torch.uint8, device=dev)
                feat_l = torch.empty(nl, dtype=torch.int32, device=dev)
                self._pair_score_select(lib, Hl, nl, k, pfeat[lo * k:(lo + nl) * k].contiguous(), wl, min_w2,
                                        pk_l, mask_l, feat_l)
                pk[a:b] = coll.all_gather_dim0(pk_l)[:nb]
                mask[a:b] = coll.all_gather_dim0(mask_l)[:nb]
                feat_i[a:b] = coll.all_gather_dim0(feat_l)[:nb]
                continue
            self._pair_score_select(lib, Hp, nb, k, pfeat, wyy_n, min_w2, pk[a:b], mask[a:b], feat_i[a:b])
            del Hp
        return {"pk": pk, "feat_i32": feat_i, "mask": mask, "gain": pk[:, 0], "feat": pk[:, 1].long(),
                "t": pk[:, 2].long(), "opt": pk[:, 3].long(), "L": pk[:, 4:6], "R": pk[:, 6:8], "tot": pk[:, 8:10],
                "naw": pk[:, 12]}

    # ------------------------------------------------------------------ multi-GPU pair exchange
    def _pair_exchange(self, Hp, pf, pn, n, full):
        """Sum the (node, feature) pair histograms of every rank without
        shipping empty bins.  Hp: [P, Bs, C] dense rows of node-major pairs
        (pair p belongs to node pn[p], feature pf[p]); node q is owned by rank
        q // ceil(n / W).

        Each pair row is packed at its feature's OWN width (bins + NA: <= 256
        for the numeric columns, the cardinality for a categorical) instead of
        the frame-wide stride Bs, the packed rows of every owner are laid out
        back to back, and the level is summed either by ONE reduce-scatter of
        the packed [W, Lmax] buffer or -- when the bins that are non-zero on
        the busiest rank cost less than half of that (deep levels: nodes of a
        few dozen rows fill a few bins of each 1000-level histogram) -- by ONE
        all_to_all of (position, value) pairs summed by the owner.  Returns the
        owner's dense [P_own, Bs, C] rows (pairs of its nodes, in order), or
        with full=True every pair's summed dense row (packed all-gather).
        Reference: hex/tree/DHistogram.java:366 -- the reference ships
        per-node histograms of nbins = 20 numeric bins."""
        W, r = self.W, self.rank
        dev = Hp.device
        P, Bs, C = Hp.shape
        nl = -(-n // W)
        if self._pw_t is None or self._pw_t.device != dev:
            nb = np.minimum(np.asarray(self.bd.nbins[:self.bd.F], dtype=np.int64), Bs - 1) + 1
            self._pw_t = torch.as_tensor(nb, device=dev)
        w = self._pw_t[pf]
        owner = torch.div(pn, nl, rounding_mode="floor")
        cw = torch.cumsum(w, 0)
        start = cw - w
        E = int(cw[-1]) if P else 0
        own_cnt = torch.bincount(owner, minlength=W)
        own_first = torch.cumsum(own_cnt, 0) - own_cnt                  # first pair of each owner
        ch_start = torch.where(own_cnt > 0, start[own_first.clamp(max=max(P - 1, 0))] if P else own_cnt,
                               torch.zeros_like(own_cnt))
        Lq = torch.zeros(W, dtype=torch.int64, device=dev).index_add_(0, owner, w)
        Lh = Lq.tolist()
        Lmax = max(1, max(Lh))
        # element index arrays in int32 when they fit (a deep DRF level holds
        # 1e8 packed bins: 4 bytes instead of 8 per bin and array)
        it = torch.int32 if P * Bs < 2 ** 31 and E < 2 ** 31 else torch.int64
        pe = torch.repeat_interleave(torch.arange(P, device=dev, dtype=it), w)   # element -> pair
        j = torch.arange(E, device=dev, dtype=it) - start.to(it)[pe]            # element -> packed bin
        dense_idx = pe * Bs + torch.where(j == w.to(it)[pe] - 1, torch.full_like(j, Bs - 1), j)
        oe = owner.to(it)[pe]
        pos = start.to(it)[pe] + j - ch_start.to(it)[oe]                      # position in its owner's chunk
        del pe, j
        vals = Hp.reshape(P * Bs, C)[dense_idx]                          # [E, C]
        nzm = (vals != 0).any(1)
        nnz = int(nzm.sum())
        # lossless integer transport: unweighted / bootstrap-count classification
        # histograms hold whole numbers (w = counts, wy = class counts); when every
        # rank's values are integers below 2^27 the level ships int32 (a sum of
        # 8 ranks stays exact), half the bytes of f64
        big = float(vals.abs().max()) if vals.numel() else 0.0
        not_int = 0.0 if big < 2.0 ** 27 else 1.0
        step_ = 1 << 24
        for a_ in range(0, vals.shape[0] if not_int == 0.0 else 0, step_):
            v_ = vals[a_:a_ + step_]
            if bool((v_ != torch.round(v_)).any()):
                not_int = 1.0
                break
        stat = torch.tensor([float(nnz), not_int], dtype=torch.float64, device=dev)
        coll.allreduce_(stat, "max")
        ints = float(stat[1]) == 0.0
        vb_ = 4 if ints else 8
        dense_b = W * Lmax * C * vb_
        tdt = torch.int32 if ints else Hp.dtype
        if float(stat[0]) * (4 + vb_ * C) < dense_b:
            # sparse: (position, value) of the non-zero bins to their owner, when
            # that ships fewer bytes than the dense reduce-scatter
            from ...core.dist_munge import exchange
            from ...core.vec import T_INT, T_REAL, Vec
            vsend = vals[nzm].to(tdt).contiguous()
            got = exchange([Vec(pos[nzm].to(torch.int32), T_INT), Vec(vsend, T_INT if ints else T_REAL)], oe[nzm])
            chunk = torch.zeros((Lmax, C), dtype=Hp.dtype, device=dev).index_add_(
                0, got[0].data.long(), got[1].data.to(Hp.dtype))
        else:
            buf = torch.zeros((W, Lmax, C), dtype=tdt, device=dev)
            buf[oe, pos] = vals.to(tdt)
            chunk = coll.reduce_scatter_dim0(buf.view(W * Lmax, C)).to(Hp.dtype)
        if full:
            allc = coll.all_gather_dim0(chunk.to(tdt)).view(W, Lmax, C).to(Hp.dtype)
            out = torch.zeros((P * Bs, C), dtype=Hp.dtype, device=dev)
            out[dense_idx] = allc[oe, pos]
            return out.view(P, Bs, C)
        mine = oe == r
        p0 = int(own_first[r]) if P else 0
        Pr = int(own_cnt[r])
        out = torch.zeros((max(Pr, 0) * Bs, C), dtype=Hp.dtype, device=dev)
        out[dense_idx[mine] - p0 * Bs] = chunk[pos[mine]]
        return out.view(Pr, Bs, C)

    def _pair_score_select(self, lib, Hp, n, k, pfeat, wyy_n, min_w2, pk, mask, feat_i):
        """Score the n*k pairs of Hp (cat_pair_kernel) and write the n nodes'
        records / masks / features (pair_select_kernel) into the given
        contiguous output views."""
        p = self.p
        dev = self.dev
        Bs = self.bd.Bs
        P = n * k
        if n <= 0:
            return
        fl = pfeat.long()
        nb_t = self._narrow_bins()
        best_k = self._pairs_native(Hp.view(1, P, Bs, 2), torch.zeros(P, dtype=torch.long, device=dev),
                                    torch.arange(P, device=dev), self.is_cat_t[fl], self.mono_t[fl],
                                    wyy_n.repeat_interleave(k) if wyy_n is not None else None, raw=True,
                                    pbins=nb_t[fl] if nb_t is not None else None)
        xgb = 1 if p.criterion == "xgb" else 0
        check(lib.h2o_pair_select(ptr(Hp), n, Bs, k, ptr(best_k), ptr(pfeat), ptr(self._fcat_u8), xgb, min_w2,
                                  pk.stride(0), ptr(pk), ptr(mask), ptr(feat_i), ptr(nb_t), stream()),
              "h2o_pair_select")

    def _pair_direct_part(self, ridx, va, vb, mode, posv, st, ct, pn, pf):
        p = self.p
        dev = self.dev
        n = st.size
        Bs, C = self.bd.Bs, 2
        out = {"gain": torch.full((n,), NEG_INF, dtype=torch.float64, device=dev),
               "feat": torch.zeros(n, dtype=torch.long, device=dev),
               "t": torch.zeros(n, dtype=torch.long, device=dev), "opt": torch.zeros(n, dtype=torch.long, device=dev),
               "na_left": torch.zeros(n, dtype=torch.bool, device=dev),
               "mask": torch.zeros((n, Bs), dtype=torch.uint8, device=dev),
               "L": torch.zeros((n, C), dtype=torch.float64, device=dev),
               "R": torch.zeros((n, C), dtype=torch.float64, device=dev),
               "tot": torch.zeros((n, C), dtype=torch.float64, device=dev),
               "naw": torch.zeros(n, dtype=torch.float64, device=dev)}
        with phase("tree.hist"), phase("tree.hist.pairs"):
            Hp, wyy_n = tree_ops.pair_hist(self.bd, ridx, va, vb, mode, st, ct, pn, pf, vmax=self._vmax, posv=posv,
                                           want_wyy=mode == 0)
        if self.W > 1:
            if pn.size:
                Hp = self._pair_exchange(Hp, tree_ops._h2d(pf, dev), tree_ops._h2d(pn, dev), n, full=True)
            if wyy_n is not None:
                coll.allreduce_(wyy_n)
        P = pn.size
        if P == 0:
            return out
        pn_t = tree_ops._h2d(pn, dev)
        first = np.ones(P, dtype=bool)
        first[1:] = pn[1:] != pn[:-1]
        fi = np.nonzero(first)[0]
        out["tot"] = out["tot"].index_put((pn_t[tree_ops._h2d(fi, dev)],),
                                          Hp[tree_ops._h2d(fi, dev)].sum(1))
        fglob = tree_ops._h2d(pf, dev)
        pcat = self.is_cat_t[fglob]
        mono_p = self.mono_t[fglob]
        wyy_p = wyy_n[pn_t] if wyy_n is not None else None
        ar = torch.arange(P, device=dev)
        if dev.type == "cuda" and Bs - 1 <= 4096:
            best, k = self._pairs_native(Hp.view(1, P, Bs, C), torch.zeros(P, dtype=torch.long, device=dev), ar,
                                         pcat, mono_p, wyy_p)
        else:
            stt = self._pair_stats(Hp, pcat)
            allg = self._pair_gains(stt, mono_p.view(-1, 1), wyy_p, ar)
            best, k = allg.max(1)
        return self._pair_winners(out, best, k, pn_t, fglob, pcat, lambda wp: Hp[wp])

    def _pair_winners(self, out, best, k, node_i, fglob, pcat, hist_of):
        """Per-node winner among scored (node, feature) pairs (largest gain,
        lowest pair index on ties) and its split record: threshold / NA option
        from k, left statistics and the go-left code mask rebuilt from the
        winner's own bins (hist_of(wp) -> [len(wp), Bs, C])."""
        p = self.p
        n = out["gain"].shape[0]
        dev = best.device
        P = best.numel()
        ninf = torch.full((n,), NEG_INF, dtype=torch.float64, device=dev)
        B = self.bd.Bs - 1
        Bs = self.bd.Bs
        xgb = p.criterion == "xgb"
        node_best = ninf.clone().scatter_reduce(0, node_i, best, reduce="amax", include_self=True)
        cand = torch.where((best == node_best[node_i]) & torch.isfinite(best), torch.arange(P, device=dev),
                           torch.full((P,), P, device=dev))
        win = torch.full((n,), P, dtype=torch.long, device=dev).scatter_reduce(0, node_i, cand, reduce="amin",
                                                                              include_self=True)
        has = win < P
        if not bool(has.any()):
            return out
        nodes = torch.nonzero(has).flatten()
        wp = win[nodes]
        # the winners' sorted order / prefix sums, from their own bins only
        st = self._pair_stats(hist_of(wp).to(torch.float64), pcat[wp])
        h, order, L, totnn, na, T = st["h"], st["order"], st["L"], st["totnn"], st["na"], st["T"]
        nt = B - 1
        kk = k[wp]
        opt = torch.where(kk < nt, torch.zeros_like(kk), torch.where(kk < 2 * nt, torch.ones_like(kk),
                                                                     torch.full_like(kk, 2)))
        t = torch.where(opt == 0, kk, torch.where(opt == 1, kk - nt, torch.zeros_like(kk)))
        na_left = opt == 1
        ar = torch.arange(wp.numel(), device=dev)
        Lw = torch.where((opt == 2).view(-1, 1), totnn,
                         L[ar, t.clamp(max=nt - 1)] + torch.where(na_left.view(-1, 1), na, torch.zeros_like(na)))
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(B, device=dev).view(1, B).expand(order.shape[0], B))
        in_left = rank <= t.view(-1, 1)
        bw = h[:, :B, 1] if xgb else h[:, :B, 0]
        empty = (bw <= 0) & pcat[wp].view(-1, 1)     # empty categorical levels follow the NAs
        in_left = torch.where(empty, na_left.view(-1, 1).expand_as(in_left), in_left)
        in_left = torch.where((opt == 2).view(-1, 1), ~empty | na_left.view(-1, 1), in_left)
        mask = torch.cat([in_left, na_left.view(-1, 1).expand(-1, Bs - B)], 1).to(torch.uint8)
        out["gain"] = out["gain"].index_put((nodes,), best[wp])
        out["feat"] = out["feat"].index_put((nodes,), fglob[wp])
        out["t"] = out["t"].index_put((nodes,), t)
        out["opt"] = out["opt"].index_put((nodes,), opt)
        out["na_left"] = out["na_left"].index_put((nodes,), na_left)
        out["mask"] = out["mask"].index_put((nodes,), mask)
        out["L"] = out["L"].index_put((nodes,), Lw)
        out["R"] = out["R"].index_put((nodes,), T - Lw)
        if "naw" in out:
            out["naw"] = out["naw"].index_put((nodes,), na[:, 0].to(out["naw"].dtype))
        return out

    def _pair_stats(self, h, pcat):
        """Sorted order and prefix sums of pair histograms h [P, Bs, C] f64."""
        B = h.shape[1] - 1
        dev = h.device
        bins, na = h[:, :B], h[:, B]
        if self.p.criterion == "xgb":
            key = torch.where(bins[..., 1] > 0, bins[..., 0] / bins[..., 1].clamp_min(1e-300),
                              torch.full_like(bins[..., 0], float("inf")))
        else:
            key = torch.where(bins[..., 0] > 0, bins[..., 1] / bins[..., 0].clamp_min(1e-300),
                              torch.full_like(bins[..., 0], float("inf")))
        key = torch.where(pcat.view(-1, 1), key, torch.arange(B, device=dev, dtype=key.dtype).view(1, B))
        order = torch.argsort(key, dim=1, stable=True)             # [P, B]
        bs_ = torch.gather(bins, 1, order.unsqueeze(-1).expand(-1, -1, h.shape[2]))
        cum = torch.cumsum(bs_, 1)
        totnn = cum[:, -1]
        L = cum[:, :-1]
        return {"h": h, "na": na, "order": order, "L": L, "totnn": totnn, "R": totnn.unsqueeze(1) - L,
                "T": totnn + na}

    def _pair_gains(self, st, mono, node_wyy, node_i):
        """[P, 2(B-1)+1] gains of every threshold x NA option (torch path)."""
        p = self.p
        xgb = p.criterion == "xgb"
        L, R, totnn, na, T = st["L"], st["R"], st["totnn"], st["na"], st["T"]
        naE = na.unsqueeze(1)
        P = L.shape[0]

        def score(S):
            if xgb:
                g, hh = S[..., 0], S[..., 1]
                if p.reg_alpha > 0:
                    g = torch.sign(g) * torch.clamp(g.abs() - p.reg_alpha, min=0)
                return g * g / (hh + p.reg_lambda)
            w, wy = S[..., 0], S[..., 1]
            return torch.where(w > 0, wy * wy / w.clamp_min(1e-300), torch.zeros_like(w))

        sT = score(T).unsqueeze(1)

        def gain_of(LL, RR):
            g = score(LL) + score(RR) - sT
            if xgb:
                g = 0.5 * g - p.gamma
                ok = (LL[..., 1] >= max(p.min_rows, 1e-12)) & (RR[..., 1] >= max(p.min_rows, 1e-12))
            else:
                wl, wr = LL[..., 0], RR[..., 0]
                ok = (wl >= p.min_rows) & (wr >= p.min_rows) & (wl > 0) & (wr > 0)
                pl = (LL[..., 1] / wl.clamp_min(1e-300))
                pr = (RR[..., 1] / wr.clamp_min(1e-300))
                ok &= pl.to(torch.float32) != pr.to(torch.float32)
            if xgb:
                pl = -LL[..., 0] / (LL[..., 1] + p.reg_lambda)
                pr = -RR[..., 0] / (RR[..., 1] + p.reg_lambda)
            ok &= ~((mono > 0) & (pl > pr)) & ~((mono < 0) & (pl < pr))
            return torch.where(ok, g, torch.full_like(g, NEG_INF))

        gA = gain_of(L, R + naE)
        gB = gain_of(L + naE, R)
        gC = gain_of(totnn.unsqueeze(1), naE)
        has_na = ((na[..., 1] > 0) | (na[..., 0] != 0)) if xgb else (na[..., 0] > 0)
        gB = torch.where(has_na.unsqueeze(1), gB, torch.full_like(gB, NEG_INF))
        gC = torch.where(has_na.unsqueeze(1), gC, torch.full_like(gC, NEG_INF))
        allg = torch.cat([gA, gB, gC], 1)                          # [P, 2(B-1)+1]
        if xgb:
            return torch.where(allg > 0, allg, torch.full_like(allg, NEG_INF))
        wyy = node_wyy.to(torch.float64)[node_i].view(-1, 1) if node_wyy is not None else \
            torch.zeros((P, 1), dtype=torch.float64, device=L.device)
        se_before = (wyy - score(T).unsqueeze(1)).clamp_min(0)
        return torch.where((allg > se_before * p.min_split_improvement) & (se_before > 0), allg,
                           torch.full_like(allg, NEG_INF))

    def _pairs_native(self, H, fslot, node_i, pcat, mono_p, node_wyy, raw=False, pbins=None):
        """(best gain, k) per pair from the HIP pair kernel.  pbins (bins of each
        pair's feature): pairs of narrow (< 256-bin) features are scored by the
        256-wide kernel instance, the rest at the full histogram width."""
        p = self.p
        Fl, n, Bs, C = H.shape
        lib = _native.get_lib("tree_split")
        H = H.contiguous()
        P = fslot.numel()
        pf = fslot.to(torch.int32).contiguous()
        pn = node_i.to(torch.int32).contiguous()
        pc = pcat.to(torch.uint8).contiguous()
        pm = mono_p.to(torch.float32).contiguous()
        wyy = node_wyy.to(torch.float64).contiguous() if node_wyy is not None else None
        res = torch.empty((P, 2), dtype=torch.float64, device=H.device)
        if pbins is not None and Bs - 1 > 256 and tree_ops.env("H2O3_PAIR_NARROW", "1") == "1":
            lists = torch.empty(2 * P + 2, dtype=torch.int32, device=H.device)
            pb = pbins.to(torch.int32).contiguous()
            rc = lib.h2o_cat_pairs2(ptr(H), n, Bs, C, P, ptr(pf), ptr(pn), ptr(pc), ptr(pm), ptr(wyy),
                                    float(p.min_rows), float(p.min_split_improvement), float(p.reg_lambda),
                                    float(p.reg_alpha), float(p.gamma), 1 if p.criterion == "xgb" else 0, ptr(res),
                                    ptr(pb), 255, ptr(lists), stream())
            check(rc, "h2o_cat_pairs2")
            return res if raw else (res[:, 0].contiguous(), res[:, 1].to(torch.long))
        rc = lib.h2o_cat_pairs(ptr(H), n, Bs, C, P, ptr(pf), ptr(pn), ptr(pc), ptr(pm), ptr(wyy),
                               float(p.min_rows), float(p.min_split_improvement), float(p.reg_lambda),
                               float(p.reg_alpha), float(p.gamma), 1 if p.criterion == "xgb" else 0, ptr(res),
                               stream())
        check(rc, "h2o_cat_pairs")
        if raw:
            return res
        return res[:, 0].contiguous(), res[:, 1].to(torch.long)

    def _find_splits_torch(self, H, col_mask, node_wyy=None, merge=True, sub=None):
        """H: [Fl, n, Bs, C] (local feature slice).  Returns dict of per-node
        tensors on device: gain, feat, na_left, mask[n, Bs], stats L/R [n,C],
        tot [n,C].  sub: local feature indices to score (e.g. the categorical
        ones); large frontiers are scored in node chunks to bound memory."""
        Fl0, n0, Bs0, C0 = H.shape
        if sub is not None:
            sub_t = torch.as_tensor(sub, dtype=torch.long, device=H.device)
            gidx = sub_t + self.f0
            H = H.index_select(0, sub_t)
        else:
            gidx = torch.arange(self.f0, self.f0 + Fl0, device=H.device)
        Fs = H.shape[0]
        # chunk the frontier: ~12 live [nc, Fs, Bs, C] float64 temporaries <= ~3 GB
        nc = max(1, int(3e9 // max(1, 12 * Fs * Bs0 * C0 * 8)))
        if n0 > nc:
            parts = [self._find_splits_torch_core(H[:, i:i + nc], col_mask[i:i + nc], gidx,
                                                  None if node_wyy is None else node_wyy[i:i + nc])
                     for i in range(0, n0, nc)]
            res = {k: (torch.cat([q[k] for q in parts], 0) if parts[0][k] is not None else None) for k in parts[0]}
        else:
            res = self._find_splits_torch_core(H, col_mask, gidx, node_wyy)
        if self.W > 1 and merge:
            res = self._merge_candidates(res, n0, Bs0, C0)
        return res

    def _find_splits_torch_core(self, H, col_mask, gidx, node_wyy=None):
        p = self.p
        Fl, n, Bs, C = H.shape
        B = Bs - 1
        h = H.permute(1, 0, 2, 3).to(torch.float64)       # [n, Fl, Bs, C]
        bins = h[:, :, :B]
        na = h[:, :, B]                                    # [n, Fl, C]
        is_cat = self.is_cat_t[gidx]
        order = None
        uplift = p.criterion.startswith("uplift")
        if bool(is_cat.any()):
            if uplift:
                pt = bins[..., 1] / bins[..., 0].clamp_min(1e-300)
                pc = bins[..., 3] / bins[..., 2].clamp_min(1e-300)
                key = torch.where((bins[..., 0] + bins[..., 2]) > 0, pt - pc,
                                  torch.full_like(bins[..., 0], float("inf")))
            elif p.criterion == "xgb":
                key = torch.where(bins[..., 1] > 0, bins[..., 0] / bins[..., 1].clamp_min(1e-300),
                                  torch.full_like(bins[..., 0], float("inf")))
            else:
                key = torch.where(bins[..., 0] > 0, bins[..., 1] / bins[..., 0].clamp_min(1e-300),
                                  torch.full_like(bins[..., 0], float("inf")))
            ar = torch.arange(B, device=h.device).view(1, 1, B).expand(n, Fl, B)
            key = torch.where(is_cat.view(1, Fl, 1), key, ar.to(key.dtype))
            order = torch.argsort(key, dim=2, stable=True)             # [n, Fl, B]
            bins = torch.gather(bins, 2, order.unsqueeze(-1).expand(-1, -1, -1, C))
        cum = torch.cumsum(bins, 2)
        totnn = cum[:, :, -1]                              # [n, Fl, C] non-NA totals
        L = cum[:, :, :-1]                                 # [n, Fl, B-1, C]
        R = totnn.unsqueeze(2) - L
        T = totnn + na                                     # [n, Fl, C] all rows
        naE = na.unsqueeze(2)
        # option 0: NA right, option 1: NA left, option 2: NA vs rest
        LA, RA = L, R + naE
        LB, RB = L + naE, R
        LC, RC = totnn.unsqueeze(2), naE

        def diverg(S):
            # uplift divergence between treatment and control response rates
            wt, wc = S[..., 0], S[..., 2]
            pt = (S[..., 1] / wt.clamp_min(1e-300)).clamp(1e-6, 1 - 1e-6)
            pc = (S[..., 3] / wc.clamp_min(1e-300)).clamp(1e-6, 1 - 1e-6)
            if p.criterion == "uplift_kl":
                d = pt * torch.log(pt / pc) + (1 - pt) * torch.log((1 - pt) / (1 - pc))
            elif p.criterion == "uplift_chisquared":
                d = (pt - pc) ** 2 / pc + ((1 - pt) - (1 - pc)) ** 2 / (1 - pc)
            else:  # euclidean
                d = (pt - pc) ** 2 + ((1 - pt) - (1 - pc)) ** 2
            return torch.where((wt > 0) & (wc > 0), d, torch.zeros_like(d))

        def score(S):
            if uplift:
                return diverg(S)
            if p.criterion == "xgb":
                g, hh = S[..., 0], S[..., 1]
                if p.reg_alpha > 0:
                    g = torch.sign(g) * torch.clamp(g.abs() - p.reg_alpha, min=0)
                return g * g / (hh + p.reg_lambda)
            w, wy = S[..., 0], S[..., 1]
            return torch.where(w > 0, wy * wy / w.clamp_min(1e-300), torch.zeros_like(w))

        sT = score(T).unsqueeze(2)                         # [n, Fl, 1]

        def gain_of(LL, RR):
            if uplift:
                nl = LL[..., 0] + LL[..., 2]
                nr = RR[..., 0] + RR[..., 2]
                nt = (nl + nr).clamp_min(1e-300)
                g = (nl / nt) * diverg(LL) + (nr / nt) * diverg(RR) - sT
                ok = (nl >= p.min_rows) & (nr >= p.min_rows) & (LL[..., 0] > 0) & (LL[..., 2] > 0) & \
                    (RR[..., 0] > 0) & (RR[..., 2] > 0)
                return torch.where(ok, g, torch.full_like(g, NEG_INF))
            g = score(LL) + score(RR) - sT
            if p.criterion == "xgb":
                g = 0.5 * g - p.gamma
                wl, wr = LL[..., 1], RR[..., 1]
                ok = (wl >= max(p.min_rows, 1e-12)) & (wr >= max(p.min_rows, 1e-12))
                predl = -LL[..., 0] / (wl + p.reg_lambda)
                predr = -RR[..., 0] / (wr + p.reg_lambda)
            else:
                wl, wr = LL[..., 0], RR[..., 0]
                ok = (wl >= p.min_rows) & (wr >= p.min_rows) & (wl > 0) & (wr > 0)
                predl = LL[..., 1] / wl.clamp_min(1e-300)
                predr = RR[..., 1] / wr.clamp_min(1e-300)
                ok &= predl.to(torch.float32) != predr.to(torch.float32)
            mono = self.mono_t[gidx].view(1, Fl, 1)
            ok &= ~((mono > 0) & (predl > predr)) & ~((mono < 0) & (predl < predr))
            return torch.where(ok, g, torch.full_like(g, NEG_INF))

        gA = gain_of(LA, RA)
        gB = gain_of(LB, RB)
        has_na = (na[..., 0] > 0) if p.criterion != "xgb" else ((na[..., 1] > 0) | (na[..., 0] != 0))
        if uplift:
            has_na = (na[..., 0] + na[..., 2]) > 0
        gB = torch.where(has_na.unsqueeze(2), gB, torch.full_like(gB, NEG_INF))
        gC = gain_of(LC, RC)
        gC = torch.where(has_na.unsqueeze(2), gC, torch.full_like(gC, NEG_INF))
        # feature eligibility (column sampling, padding, interaction constraints)
        cm = col_mask.to(h.device)[:, gidx] & (gidx < self.bd.F).view(1, -1)
        allg = torch.cat([gA, gB, gC], 2)                  # [n, Fl, 2(B-1)+1]
        allg = torch.where(cm.unsqueeze(2), allg, torch.full_like(allg, NEG_INF))
        # min split improvement (relative to the node's squared error)
        if uplift:
            allg = torch.where(allg > 1e-12, allg, torch.full_like(allg, NEG_INF))
        elif p.criterion != "xgb":
            wyy_tot = node_wyy.view(-1, 1).to(T.dtype) if node_wyy is not None else torch.zeros_like(T[..., 0])
            se_before = (wyy_tot - score(T)).clamp_min(0).unsqueeze(2)
            allg = torch.where(allg > se_before * p.min_split_improvement, allg, torch.full_like(allg, NEG_INF))
            allg = torch.where(se_before > 0, allg, torch.full_like(allg, NEG_INF))
        else:
            allg = torch.where(allg > 0, allg, torch.full_like(allg, NEG_INF))
        K = allg.shape[2]
        bnd = self._bnd_dev(n)
        if bnd is not None and not uplift and Fl > 0:
            # monotone node bounds on each column's best split (DTree.java:1386-1445)
            bk = allg.argmax(2)                                        # [n, Fl]
            gk = allg.gather(2, bk.unsqueeze(2)).squeeze(2)
            LL_all = torch.cat([LA, LB, LC.expand(-1, -1, 1, -1)], 2)
            RR_all = torch.cat([RA, RB, RC.expand(-1, -1, 1, -1)], 2)
            ix = bk.view(n, Fl, 1, 1).expand(-1, -1, 1, C)
            Lb, Rb = LL_all.gather(2, ix).squeeze(2), RR_all.gather(2, ix).squeeze(2)
            pen, viol = self._bound_cost(Lb, Rb, bnd[:, 0].view(n, 1), bnd[:, 1].view(n, 1))
            gk = torch.where(viol & torch.isfinite(gk),
                             gk - pen if p.use_bounds else torch.full_like(gk, NEG_INF), gk)
            allg = torch.full_like(allg, NEG_INF).scatter_(2, bk.unsqueeze(2), gk.unsqueeze(2))
        flat = allg.reshape(n, Fl * K)
        best, arg = flat.max(1)
        fl = arg // K
        k = arg % K
        nt = B - 1
        opt = torch.where(k < nt, torch.zeros_like(k), torch.where(k < 2 * nt, torch.ones_like(k), torch.full_like(k, 2)))
        t = torch.where(opt == 0, k, torch.where(opt == 1, k - nt, torch.zeros_like(k)))
        na_left = opt == 1
        ar_n = torch.arange(n, device=h.device)
        # stats of the winning split
        if nt > 0:
            Lw = torch.where((opt == 2).view(n, 1), totnn[ar_n, fl],
                             L[ar_n, fl, t.clamp(max=nt - 1)] + torch.where(na_left.view(n, 1), na[ar_n, fl], torch.zeros_like(na[ar_n, fl])))
        else:
            Lw = totnn[ar_n, fl]                           # one non-NA bin: NA vs rest is the only candidate
        Tw = T[ar_n, fl]
        Rw = Tw - Lw
        # go-left masks over codes
        codes = torch.arange(Bs, device=h.device).view(1, Bs)
        cat_best = is_cat[fl]
        mask_num = (codes <= t.view(n, 1)) & (codes < B)
        mask_num = torch.where((opt == 2).view(n, 1), codes < B, mask_num)
        if order is not None:
            ordw = order[ar_n, fl]                                     # [n, B]
            rank = torch.empty_like(ordw)
            rank.scatter_(1, ordw, torch.arange(B, device=h.device).view(1, B).expand(n, B))
            in_left = rank <= t.view(n, 1)
            bins_w = h[ar_n, fl, :B, 0] if p.criterion != "xgb" else h[ar_n, fl, :B, 1]
            if uplift:
                bins_w = h[ar_n, fl, :B, 0] + h[ar_n, fl, :B, 2]
            empty = bins_w <= 0
            in_left = torch.where(empty, na_left.view(n, 1).expand(n, B), in_left)
            in_left = torch.where((opt == 2).view(n, 1), ~empty | na_left.view(n, 1), in_left)
            mask_cat = torch.cat([in_left, torch.zeros((n, Bs - B), dtype=torch.bool, device=h.device)], 1)
            mask = torch.where(cat_best.view(n, 1), mask_cat, mask_num)
        else:
            mask = mask_num
        mask = mask.clone()
        mask[:, Bs - 1] = na_left
        res = {"gain": best, "feat": gidx[fl], "t": t, "opt": opt, "na_left": na_left,
               "mask": mask.to(torch.uint8), "L": Lw, "R": Rw, "tot": T[:, 0] if Fl > 0 else None}
        return res

    def _merge_records(self, pk, mask):
        """Multi-GPU merge of the per-rank packed split records (split_select2
        over each rank's feature slice): two all-gathers (records, go-left
        masks as bytes), the highest gain wins per node, ties to the lowest
        rank (= lowest feature).  Node totals are global on every rank (the
        histograms were reduce-scattered), so the winner's record is complete."""
        W = self.W
        n, Bs = mask.shape
        # ONE all-gather: the record's bytes and the mask bytes side by side
        rb = pk.shape[1] * 8
        buf = torch.cat([pk.contiguous().view(torch.uint8).view(n, rb), mask.contiguous()], 1)
        g = coll.all_gather_dim0(buf).view(W, n, rb + Bs)
        gains = g[:, :, :8].contiguous().view(torch.float64).view(W, n)
        best_r = torch.argmax(gains, 0)
        ar = torch.arange(n, device=pk.device)
        win = g[best_r, ar]
        pk_w = win[:, :rb].contiguous().view(torch.float64).view(n, -1)
        mask_w = win[:, rb:].contiguous()
        return pk_w, mask_w, pk_w[:, 1].to(torch.int32)

    def _merge_candidates(self, res, n, Bs, C):
        W = self.W
        packed = torch.cat([res["gain"].view(n, 1), res["feat"].to(torch.float64).view(n, 1),
                            res["t"].to(torch.float64).view(n, 1), res["opt"].to(torch.float64).view(n, 1),
                            res["L"], res["R"], res["tot"], res["mask"].to(torch.float64)], 1)
        g = coll.all_gather_dim0(packed.contiguous()).view(W, n, -1)
        gains = g[:, :, 0]
        # deterministic tie-break: lowest rank (= lowest feature) wins
        best_r = torch.argmax(gains, 0)
        sel = g[best_r, torch.arange(n, device=g.device)]
        off = 4
        out = {"gain": sel[:, 0], "feat": sel[:, 1].long(), "t": sel[:, 2].long(), "opt": sel[:, 3].long()}
        out["na_left"] = out["opt"] == 1
        out["L"] = sel[:, off:off + C]
        out["R"] = sel[:, off + C:off + 2 * C]
        out["tot"] = g[0, :, off + 2 * C:off + 3 * C]   # rank 0 holds feature 0
        out["mask"] = sel[:, off + 3 * C:].to(torch.uint8)
        return out

    # ------------------------------------------------------------------ grow
    def pos_payload_ok(self):
        """True when grow() keeps the 0/1-weighted mode-0 response as a
        position-ordered NaN-masked payload (quad histogram kernels)."""
        return self.dev.type == "cuda" and self.bd.code_bytes == 1 and self.bd.Bs <= 256 \
            and self.bd.Fp % 16 == 0 and tree_ops.env("H2O3_HIST_KERNEL", "quad") == "quad" \
            and tree_ops.env("H2O3_POSV", "1") == "1" and tree_ops.env("H2O3_PART", "ballot") == "ballot"

    def grow(self, va, vb, mode, tree_node_hook=None, want_nid=True, vmax=None, unit_w=None, va_scratch=False):
        """Grow one tree (environment switches read once per tree); see _grow."""
        with tree_ops.env_scope():
            return self._grow(va, vb, mode, tree_node_hook=tree_node_hook, want_nid=want_nid, vmax=vmax,
                              unit_w=unit_w, va_scratch=va_scratch)

    def _grow(self, va, vb, mode, tree_node_hook=None, want_nid=True, vmax=None, unit_w=None, va_scratch=False):
        """Grow one tree.  Returns (Tree, nid[N] leaf index per local row,
        leaf_nodes list (tree node ids, indexed by nid), leaf_tot [n_leaves, C]).
        vmax / unit_w: caller-known bounds (max |channel| for the fixed-point
        histogram scale, 0/1 row weights) that spare the two device syncs at
        the start of the tree."""
        bd, p = self.bd, self.p
        N = bd.nrows_local
        C = tree_ops.channels(mode)
        self._start_tree(va, vb, mode, vmax, unit_w, va_scratch)
        tb = _TreeBuf()
        # interaction constraints (GlobalInteractionConstraints /
        # BranchInteractionConstraints): the features each frontier node may
        # still split on; the root may use every feature named in a set
        ics = self._interaction_map()
        ics_t = torch.as_tensor(ics[0], device=self.dev) if ics is not None else None
        # monotone node prediction bounds (Constraints._min / _max), per frontier node
        mono_b = p.monotone is not None and bool(np.any(np.asarray(p.monotone) != 0))
        fr = _Frontier(id=np.zeros(1, dtype=np.int64), st=np.zeros(1, dtype=np.int64), ct=np.full(1, N, dtype=np.int64),
                       allow=torch.as_tensor(ics[1][None, :].copy(), device=self.dev) if ics is not None else None,
                       lo=np.full(1, -np.inf) if mono_b else None, hi=np.full(1, np.inf) if mono_b else None)
        H_prev = wyy_prev = wyy_level = None
        leaf_parts = []    # per level: (node ids, starts, counts, totals [k, C])
        # the whole frontier is partitioned on the device before the host reads the level record
        part_dev = self.dev.type == "cuda" and not p.max_leaves and \
            tree_ops.env("H2O3_ASYNC_PART", "1") == "1" and tree_ops.env("H2O3_PART", "ballot") == "ballot"
        is_cat_np = np.asarray(bd.is_cat, dtype=bool)
        depth = 0
        coll._TAG.append("tree.L0")
        ntag = len(coll._TAG)
        while fr.id.size:
            coll._TAG[ntag - 1] = f"tree.L{depth}"       # collective bytes per level (coll.bytes_report)
            n_front = int(fr.id.size)
            can_split = depth < p.max_depth
            level_bytes = self.Fpad * n_front * bd.Bs * C * 8
            prev_bytes = 0 if H_prev is None else H_prev.numel() * 8
            chunked = can_split and (level_bytes + prev_bytes) > p.hist_mem_budget and n_front > 1
            self._start_level(fr, depth)
            direct = can_split and fr.allow is None and not self._adaptive and not mono_b and \
                self._direct_level(mode, depth, chunked)
            chunked = chunked or direct
            la, self._la = self._la, None
            if la is not None and (chunked or not can_split or la[0].shape[1] < n_front):
                la = None   # defensive: the look-ahead only matches a full next level
            if chunked:
                # frontier too wide for one level of histograms, or column-sampled
                # levels on the pair path: no parent level kept (no subtraction)
                H, H_prev, wyy_level = None, None, None
            elif not can_split and depth > 0:
                # last level: no histograms needed, leaf totals come from the parent split stats
                H = None
            else:
                H, wyy_level = self._level_hist(fr, va, vb, mode, depth, la, H_prev, wyy_prev, wyy_level)
            if can_split:
                sp = self._level_splits(fr, va, vb, mode, depth, H, wyy_level, direct, chunked, want_pk=part_dev)
                dec = self._level_record(sp, fr, tb, va, vb, mode, depth, H, wyy_level, level_bytes, chunked, part_dev)
                tots = dec.tot
            else:
                dec = None
                tots = self._totals(H).numpy() if H is not None else fr.tot
            tots = np.asarray(tots, dtype=np.float64)
            w_a = _row_weight(tots, mode)
            tb.weight[fr.id] = w_a
            if dec is None:
                ok = np.zeros(n_front, dtype=bool)
            elif dec.ok is not None:
                ok = dec.ok
            else:
                ok = np.isfinite(dec.gain)
                if p.criterion != "xgb":
                    ok &= w_a >= 2 * p.min_rows
            if p.max_leaves:
                self._leaf_budget(ok, dec.gain if dec is not None else None, sum(q[0].size for q in leaf_parts))
            lf = ~ok
            if lf.any():
                leaf_parts.append((fr.id[lf], fr.st[lf], fr.ct[lf], tots[lf]))
            sids = np.nonzero(ok)[0]
            if sids.size == 0:
                if dec is not None and dec.nleft is not None:
                    self._swap_rows()   # the (identity) partition already ran
                break
            nid_s, f_s, Lsel, Rsel = fr.id[sids], dec.feat[sids], dec.L[sids], dec.R[sids]
            cat_s = is_cat_np[f_s]
            wl_a, wr_a = _row_weight(Lsel, mode), _row_weight(Rsel, mode)
            lid = self._write_splits(tb, nid_s, depth, dec, sids, f_s, cat_s, Lsel, Rsel, wl_a, wr_a)
            masks = None
            if cat_s.any() or dec.nleft is None:
                masks = sp["mask"] if sids.size == n_front else sp["mask"][tree_ops._h2d(sids, sp["mask"].device)]
            if cat_s.any():
                self._stage_cat_masks(tb, masks, nid_s, f_s, cat_s)
            if dec.nleft is not None:
                nleft = dec.nleft[sids]
            else:
                nleft = self._partition_sync(f_s, masks, fr.st[sids], fr.ct[sids])
            self._swap_rows()
            fr, H_prev, wyy_prev = self._next_frontier(fr, sids, lid, nleft, f_s, cat_s, Lsel, Rsel, wl_a <= wr_a,
                                                       ics_t, mode, H, wyy_level)
            depth += 1
        del coll._TAG[ntag - 1:]
        self._flush_masks(tb)
        tree = tb.to_tree()
        if leaf_parts:
            leaf_ids, leaf_st, leaf_ct, leaf_tot_np = (np.concatenate(q, 0) for q in zip(*leaf_parts))
        else:
            leaf_ids = leaf_st = leaf_ct = np.zeros(0, dtype=np.int64)
            leaf_tot_np = np.zeros((0, C))
        leaves = leaf_ids.tolist()
        nid = None
        if want_nid:
            with phase("tree.nid"):
                nid = tree_ops.fill_nid(self.ridx, np.arange(len(leaves), dtype=np.int64), leaf_st, leaf_ct, N)
        self.last_segs = (list(range(len(leaves))), leaf_st.tolist(), leaf_ct.tolist())
        leaf_tot_t = torch.from_numpy(np.ascontiguousarray(leaf_tot_np, dtype=np.float64))
        return tree, nid, leaves, leaf_tot_t

    def _start_tree(self, va, vb, mode, vmax, unit_w, va_scratch):
        """Per-tree state: identity row order, histogram scale, the form of the mode-0 response."""
        on_dev = self.dev.type == "cuda"
        self._tree_no = self._trees_grown
        self._trees_grown += 1
        self._adaptive = getattr(self.bd, "hist_type", "auto") in ("uniformadaptive", "random", "roundrobin")
        self._stream_obj = torch.cuda.current_stream() if on_dev else None
        if not (on_dev and tree_ops.iota_i32(self.ridx)):
            torch.arange(self.bd.nrows_local, dtype=torch.int32, device=self.dev, out=self.ridx)
        if not on_dev:
            self._vmax = None
        else:
            self._vmax = list(vmax) if vmax is not None else tree_ops.channel_max(va, vb, mode)
        # 0/1 row weights (unweighted data, row sampling) -> packed histogram atomics
        self._unit_w = mode == 0 and on_dev and (
            vb is None or (bool(unit_w) if unit_w is not None else bool(((vb == 0) | (vb == 1)).all())))
        self._va_eff = None
        quad = self.bd.code_bytes == 1 and self.bd.Bs <= 256 and self.bd.Fp % 16 == 0 and \
            tree_ops.env("H2O3_HIST_KERNEL", "quad") == "quad"
        # every level on the row-direct pair path (DRF's mtries << F): the
        # pair kernels read the position-ordered payload at any histogram width
        all_direct = self._all_levels_direct(mode) and tree_ops.env("H2O3_DRF_POSV", "1") == "1"
        if self._unit_w and (quad or all_direct):
            self._va_eff = torch.where(vb > 0, va, torch.full_like(va, float("nan"))) if vb is not None else va
        self._pos1 = None
        self._mask_pend = None
        self._la = None
        if self._va_eff is not None and tree_ops.env("H2O3_POSV", "1") == "1" and \
                tree_ops.env("H2O3_PART", "ballot") == "ballot":
            # va_scratch: the caller hands over va (a NaN-masked residual it
            # will not read again) as the root payload -- no copy
            p0 = self._va_eff.clone() if (self._va_eff is va and not va_scratch) else self._va_eff
            self._pos1 = [p0, torch.empty_like(p0)]   # root: position order == row order

    def _start_level(self, fr, depth):
        """Per-level state of the split search: parent records (_adapt_range), monotone bounds."""
        self._level = self._depth = depth
        nxt = self._adapt_next
        self._adapt_par = None if (depth == 0 or nxt is None) else nxt + (int(fr.id.size),)
        self._rng_par = None if depth == 0 else self._rng_cur
        self._rng_cur = self._adapt_next = None
        if fr.lo is not None and bool(np.isfinite(fr.lo).any() | np.isfinite(fr.hi).any()):
            self._bnd = torch.as_tensor(np.stack([fr.lo, fr.hi], 1), dtype=torch.float64, device=self.dev)
        else:
            self._bnd = None
        self._bnd_off = 0

    def _swap_rows(self):
        """The partition's output becomes the current row order (and payload)."""
        self.ridx, self.ridx2 = self.ridx2, self.ridx
        if self._pos1 is not None:
            self._pos1.reverse()

    def _part_payload(self):
        return (self._pos1[0], None, self._pos1[1], None) if self._pos1 is not None else None

    def _level_hist(self, fr, va, vb, mode, depth, la, H_prev, wyy_prev, wyy_level):
        """(H, node w*y*y sums) of a level: the look-ahead's result, a build from the rows,
        or each pair's lighter child built and its sibling derived as parent minus built."""
        n_front = int(fr.id.size)
        if la is not None:
            # built on the device before the host read the previous level's decisions (_maybe_lookahead)
            if tree_ops.env("H2O3_LA_CHECK") == "1":
                self._la_check(la, fr.p_build, fr.p_der, fr.p_par)
            return la[0][:, :n_front].contiguous(), (la[1][:n_front] if la[1] is not None else None)
        if depth == 0 or H_prev is None:
            H = self._build_hist(self.ridx, va, vb, mode, fr.st, fr.ct)
            return H, self._last_wyy
        Hb = self._build_hist(self.ridx, va, vb, mode, fr.st[fr.p_build], fr.ct[fr.p_build])
        wyy_b = self._last_wyy if mode == 0 else None
        if self.dev.type == "cuda":
            # copy + parent-minus-built subtraction in one kernel
            H, wyy_n = tree_ops.hist_sibling(Hb, H_prev, fr.p_build, fr.p_der, fr.p_par, n_front, _clamp_mask(mode),
                                             wyy_b=wyy_b, wyy_prev=wyy_prev if wyy_b is not None else None)
            return H, (wyy_n if wyy_n is not None else wyy_level)
        H = torch.empty((Hb.shape[0], n_front) + tuple(Hb.shape[2:]), dtype=Hb.dtype, device=Hb.device)
        bs = torch.as_tensor(fr.p_build, device=Hb.device)
        ds = torch.as_tensor(fr.p_der, device=Hb.device)
        ps = torch.as_tensor(fr.p_par, device=Hb.device)
        H[:, bs] = Hb
        H[:, ds] = (H_prev[:, ps] - Hb).clamp_min_(0) if mode != 1 else (H_prev[:, ps] - Hb)
        if wyy_b is not None:
            wyy_level = torch.empty(n_front, dtype=torch.float64, device=Hb.device)
            wyy_level[bs] = wyy_b
            wyy_level[ds] = wyy_prev[ps] - wyy_b
        if mode == 0:
            # only w / wyy are non-negative; wy may be negative
            H[:, ds, :, 1] = H_prev[:, ps, :, 1] - Hb[:, :, :, 1]
        return H, wyy_level

    def _level_splits(self, fr, va, vb, mode, depth, H, wyy_level, direct, chunked, want_pk):
        """Best split per frontier node (a split search's dict): from the level histogram,
        from row-direct pair histograms, or chunk by chunk under the histogram budget."""
        p, bd = self.p, self.bd
        n_front = int(fr.id.size)
        on_dev = self.dev.type == "cuda"
        sel = self._col_sel(n_front, depth) if direct else None
        cm = None if (direct and on_dev) else self._col_mask(n_front, depth, sel=sel, allow=fr.allow)
        with phase("tree.split"):
            if direct and on_dev:
                return self._pair_direct_dev(self.ridx, va, vb, mode, fr.st, fr.ct, sel)
            if direct:
                return self._pair_direct_splits(self.ridx, va, vb, mode, fr.st, fr.ct, cm)
            if not chunked:
                # node totals of w*y*y (only the total enters the SE split test),
                # fused into the histogram kernel; derived siblings by subtraction
                return self._find_splits(H, cm, wyy_level if mode == 0 else None, want_pk=want_pk)
            per = max(1, int(p.hist_mem_budget // max(1, self.Fpad * bd.Bs * tree_ops.channels(mode) * 8)))
            parts = []
            need = self._hist_need(cm)
            for a in range(0, n_front, per):
                Hc = self._build_hist(self.ridx, va, vb, mode, fr.st[a:a + per], fr.ct[a:a + per],
                                      need_mask=None if need is None else need[a:a + per])
                wyy_c = self._last_wyy if mode == 0 else None
                self._bnd_off = a
                parts.append(self._find_splits(Hc, cm[a:a + per], wyy_c, want_pk=False))
                del Hc
            self._bnd_off = 0
            return {k: (torch.cat([q[k] for q in parts], 0) if parts[0].get(k) is not None else None)
                    for k in parts[0]}

    def _assemble_record(self, sp, H, mode, part):
        """(record, feat, mask) of a split search that returned loose tensors: the level
        record (record.py) put together on the device.  With part, OK holds the split
        decision and (feat, mask) partition the whole frontier (an all-ones mask keeps a
        non-splitting node in place), which writes NL; without, OK / NL are filler."""
        p = self.p
        n = sp["gain"].shape[0]
        f64 = torch.float64
        gain, tot = sp["gain"].view(n, 1).to(f64), sp["tot"].to(f64)
        cols = [gain, sp["feat"].view(n, 1).to(f64), sp["t"].view(n, 1).to(f64), sp["opt"].view(n, 1).to(f64),
                sp["L"].to(f64), sp["R"].to(f64), tot]
        naw = sp["naw"].to(f64) if sp.get("naw") is not None else None
        if naw is None and H is not None and self.W == 1 and mode == 0 and H.shape[1] == n:
            # the winner's NA-bin weight per node (per-node NA direction rule of _write_splits)
            fi = sp["feat"].to(torch.int64).clamp(0, H.shape[0] - 1)
            naw = H[fi, torch.arange(n, device=H.device), H.shape[2] - 1, 0].to(f64)
        feat, mask = sp["feat"], sp["mask"]
        if part:
            ok = torch.isfinite(gain.view(n))
            if p.criterion != "xgb":
                ok &= _row_weight(tot, mode) >= 2 * p.min_rows
            feat = feat.to(torch.int64)
            feat = torch.where(ok, feat, torch.zeros_like(feat))
            mask = torch.where(ok.view(-1, 1), mask.to(torch.uint8), torch.ones_like(mask, dtype=torch.uint8))
            filler = ok.view(n, 1).to(f64)
        else:
            filler = gain
        cols += [filler, filler]
        if naw is not None:
            cols.append(naw.view(n, 1))
        return torch.cat(cols, 1), feat, mask

    def _level_record(self, sp, fr, tb, va, vb, mode, depth, H, wyy_level, level_bytes, chunked, part):
        """The one consumer of the level record, whichever split search made it: partition
        of the whole frontier on the device (no host round trip after the split search),
        the level's single device->host transfer, the look-ahead, then the decoded record."""
        C = tree_ops.channels(mode)
        c = rec_cols(C)
        if "pk" in sp:
            rec, feat, mask = sp["pk"], sp["feat_i32"], sp["mask"]
        else:
            rec, feat, mask = self._assemble_record(sp, H, mode, part)
        if part:
            with phase("tree.partition"):
                # no ridx2 <- ridx copy: every frontier segment is rewritten (non-splitting
                # nodes in place), earlier leaves are identical in both buffers already
                tree_ops.partition_async(self.bd, self.ridx, self.ridx2, feat, mask, fr.st, fr.ct,
                                         payload=self._part_payload(), pk=rec, pk_col=c.NL)
        # the record's copy is queued BEFORE the look-ahead kernels, so the
        # host gets it while the GPU builds the next level
        rec_h = self._d2h_async(rec)
        if part:
            w = weight_col(mode)
            self._maybe_lookahead(rec, (c.OK, c.NL, c.L + w, c.R + w), fr.st, fr.ct, mode, va, vb, self.ridx2, H,
                                  wyy_level, depth, level_bytes, chunked)
        rec_np = self._d2h_wait(rec_h)
        self._flush_masks(tb)
        return decode(rec_np, C, part)

    def _leaf_budget(self, ok, gains, n_leaves):
        """max_leaves: clear ok (in place) where a split would exceed the leaf budget, node by
        node in frontier order (this level's leaves counted as they are decided; n_leaves: those
        of earlier levels); lossguide spends it on the largest loss reductions first (XGBoost's
        best-first expansion order among the nodes of a level)."""
        p = self.p
        n_front = ok.size
        n_split = 0
        order = range(n_front)
        if p.leaf_budget_by_gain and gains is not None:
            order = np.argsort(-np.where(ok, gains, -np.inf), kind="stable")
        for i in order:
            if ok[i] and (n_leaves + n_front + n_split + 1) > p.max_leaves:
                ok[i] = False
            if ok[i]:
                n_split += 1
            else:
                n_leaves += 1

    def _write_splits(self, tb, nid_s, depth, dec, sids, f_s, cat_s, Lsel, Rsel, wl_a, wr_a):
        """Record the level's splits in the tree (vectorized); returns the left child ids."""
        p = self.p
        opt_s, t_s = dec.opt[sids], dec.t[sids]
        first = tb.add_children(depth + 1, Lsel[:, 0], Rsel[:, 0])
        lid = first + 2 * np.arange(sids.size, dtype=np.int64)
        tb.feat[nid_s] = f_s
        tb.gain[nid_s] = dec.gain[sids]
        na_s = opt_s == 1
        hn = getattr(self.bd, "has_na", None)
        if p.criterion != "xgb" and (dec.naw is not None or (hn is not None and len(hn) == self.bd.F)):
            # no NA weight reached THIS node on the split column: NAs of later
            # data go to the heavier child (DTree.java:1475-1478 decides per
            # node, nasplit == None); without the node's NA weight (chunked /
            # pair / multi-rank torch paths) the training-wide flag stands in
            no_na = (dec.naw[sids] == 0) if dec.naw is not None else ~np.asarray(hn, dtype=bool)[f_s]
            free = no_na & (opt_s != 2) & ~cat_s
            na_s = np.where(free, wl_a > wr_a, na_s)
        tb.na_left[nid_s] = na_s
        if self._adaptive:
            self._adapt_next = (sids.copy(), f_s.copy(), t_s.copy(), opt_s.copy())
        tb.left[nid_s] = lid
        tb.right[nid_s] = lid + 1
        num = ~cat_s
        if num.any():
            cutmat = self._cut_matrix()
            tb.thr[nid_s[num]] = np.where(opt_s[num] == 2, np.inf,
                                          cutmat[f_s[num], np.minimum(t_s[num], cutmat.shape[1] - 1)])
            tb.split_code[nid_s[num]] = t_s[num]
        return lid

    def _stage_cat_masks(self, tb, masks, nid_s, f_s, cat_s):
        """The categorical splits' go-left masks: only those rows cross to the host."""
        bd = self.bd
        cj = np.nonzero(cat_s)[0]
        mk = masks[tree_ops._h2d(cj, masks.device)] if cj.size < cat_s.size else masks
        nodes, fcj = nid_s[cj].astype(np.int64), f_s[cj].astype(np.int64)
        tb.is_cat[nodes] = True
        tb.thr[nodes] = np.nan
        for f in np.unique(fcj).tolist():
            if f not in tb.cat_lvm:
                # level -> code of the mask row (grouped high-cardinality levels share a code)
                card = bd.cat_card[f]
                tb.cat_lvm[f] = np.arange(card) if (bd.cat_group[f] == 1 and card <= bd.Bs - 1) else \
                    np.minimum(np.arange(card) // bd.cat_group[f], bd.Bs - 2)
        if not (mk.is_cuda and tree_ops.env("H2O3_ASYNC_MASKS", "1") == "1"):
            tb.cat_parts.append((nodes, fcj, mk.cpu().numpy()))
            return
        # asynchronous copy into a pinned staging buffer: the rows are
        # collected after the next level's record arrives (the GPU has
        # long finished the copy by then) instead of a blocking .cpu()
        self._flush_masks(tb)
        need = mk.numel()
        if self._mask_stage is None or self._mask_stage.numel() < need:
            self._mask_stage = torch.empty(max(need, 1 << 20), dtype=torch.uint8, pin_memory=True)
        self._mask_stage[:need].view(mk.shape).copy_(mk, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._mask_pend = (nodes, fcj, tuple(mk.shape), ev)

    def _partition_sync(self, f_s, masks, st_s, ct_s):
        """Partition the splitting nodes' rows after the host decided; returns the left counts."""
        with phase("tree.partition"):
            self.ridx2.copy_(self.ridx)
            return np.asarray(tree_ops.partition(self.bd, self.ridx, self.ridx2, f_s, masks, st_s, ct_s,
                                                 payload=self._part_payload()), dtype=np.int64)

    def _next_frontier(self, fr, sids, lid, nleft, f_s, cat_s, Lsel, Rsel, build_left, ics_t, mode, H, wyy_level):
        """(frontier, parent histograms, parent w*y*y) of the next level: (left, right) of every
        split node, in order; the lighter child is built from rows, its sibling derived."""
        k = int(sids.size)
        st_s, ct_s = fr.st[sids], fr.ct[sids]
        jj = 2 * np.arange(k, dtype=np.int64)
        nx = _Frontier(id=np.stack([lid, lid + 1], 1).reshape(-1),
                       st=np.stack([st_s, st_s + nleft], 1).reshape(-1),
                       ct=np.stack([nleft, ct_s - nleft], 1).reshape(-1),
                       tot=np.stack([Lsel, Rsel], 1).reshape(2 * k, -1),
                       p_build=jj + (~build_left), p_der=jj + build_left)
        if fr.allow is not None:
            # nextLevelInteractionConstraints: branch set ∩ the split feature's set
            ca = fr.allow[tree_ops._h2d(sids, self.dev)] & ics_t[tree_ops._h2d(f_s, self.dev)]
            nx.allow = torch.repeat_interleave(ca, 2, dim=0)
        if fr.lo is not None:
            nx.lo, nx.hi = self._child_bounds(fr.lo[sids], fr.hi[sids], f_s, cat_s, np.asarray(Lsel, dtype=np.float64),
                                              np.asarray(Rsel, dtype=np.float64), mode)
        # parent hists for the next level (only split nodes)
        if H is None:
            nx.p_par = np.arange(k, dtype=np.int64)
            return nx, None, None   # chunked level: next level builds from rows
        if self.dev.type == "cuda":
            # the sibling kernel indexes the parent level directly: keep the
            # whole level and point the pairs at their parents' slots
            nx.p_par = sids.astype(np.int64)
            return nx, H, (wyy_level if mode == 0 else None)
        sid = torch.as_tensor(sids, device=H.device)
        nx.p_par = np.arange(k, dtype=np.int64)
        return nx, H[:, sid], (wyy_level[sid] if (mode == 0 and wyy_level is not None) else None)

    def _d2h_async(self, t):
        """Queue a device->host copy of t into a reusable pinned slot; returns
        (host view, event).  CPU tensors pass through."""
        if t.device.type != "cuda":
            return (t, None, 0)
        ring, k = self._d2h_ring, self._d2h_k
        self._d2h_k = k ^ 1
        buf = ring[k]
        if buf is None or buf.numel() < t.numel():
            buf = ring[k] = torch.empty(max(t.numel(), 4096), dtype=t.dtype, pin_memory=True)
        h = buf[:t.numel()].view(t.shape)
        h.copy_(t, non_blocking=True)
        # one reusable event per slot, recorded on the stream cached by grow()
        evs = self._d2h_ev
        if evs[k] is None:
            evs[k] = torch.cuda.Event()
        st = self._stream_obj
        evs[k].record(st if st is not None else torch.cuda.current_stream())
        # uploads staged after this record (the look-ahead) are NOT covered
        return (h, evs[k], tree_ops.upload_mark())

    @staticmethod
    def _d2h_wait(hev):
        h, ev = hev[0], hev[1]
        if ev is not None:
            ev.synchronize()
            tree_ops.host_synced(hev[2])   # every upload queued before the record has completed
        return h.numpy().copy()

    def _maybe_lookahead(self, rec, cols, f_st, f_ct, mode, va, vb, ridx_next, H, wyy_level, depth, level_bytes,
                         chunked):
        """Launch the NEXT level's histograms now (device-built work list,
        tree_ops.hist_build_dev + hist_sibling_dev), before the host syncs on
        this level's split record: the host bookkeeping of this level then runs
        while the GPU builds the next level's histograms.  Only for a full next
        level (every node may split) that fits the histogram budget; else the
        next level is built after the sync as before."""
        self._la = None
        p = self.p
        if tree_ops.env("H2O3_LOOKAHEAD", "1") != "1" or self.dev.type != "cuda" or chunked or H is None or \
                depth + 1 >= p.max_depth or mode not in (0, 1) or p.max_leaves:
            return
        if 2 * level_bytes + H.numel() * 8 > p.hist_mem_budget:
            return
        va_n, vb_n, posv = self._hist_response(va, vb, mode, moved=True)   # the payload the partition just moved
        with phase("tree.hist"), phase("tree.hist.lookahead"):
            r = tree_ops.hist_build_dev(self.bd, ridx_next, va_n, vb_n, mode, rec, cols, f_st, f_ct, self._vmax,
                                        posv=posv, unit_w=self._unit_w)
            if r is None:
                return
            Hb, wyy_b, slots, cnts = r
            if self.W > 1:
                Hb, wyy_b = self._rs_hist_wyy(Hb, wyy_b)
            Hn, wyy_n = tree_ops.hist_sibling_dev(Hb, H, slots, cnts, _clamp_mask(mode),
                                                  wyy_b=wyy_b if mode == 0 else None,
                                                  wyy_prev=wyy_level if mode == 0 else None)
        self._la = (Hn, wyy_n, slots, cnts)

    def _la_check(self, la, p_build, p_der, p_par):
        """Debug (H2O3_LA_CHECK=1): the device-built pair slots equal the host's."""
        slots, cnts = la[2].cpu().numpy(), la[3].cpu().numpy()
        nb = len(p_build)
        assert int(cnts[0]) == nb, (int(cnts[0]), nb)
        nl = len(slots) // 3
        assert np.array_equal(slots[:nb], p_build) and np.array_equal(slots[nl:nl + nb], p_der) and \
            np.array_equal(slots[2 * nl:2 * nl + nb], p_par)

    def _cut_matrix(self):
        """[F, max_cuts + 1] numeric split values by (feature, threshold code):
        cuts[f][t], +inf past the last cut (BinnedData.split_value)."""
        cm = self._cutmat
        if cm is None:
            bd = self.bd
            w = 1 + max([len(c) for c in bd.cuts if c is not None] or [0])
            cm = np.full((bd.F, w), np.inf)
            for f, c in enumerate(bd.cuts):
                if c is not None and len(c):
                    cm[f, :len(c)] = c
            self._cutmat = cm
        return cm

    def _totals(self, H):
        """Per-node channel totals [n, C] (global), from feature 0."""
        Fl, n, Bs, C = H.shape
        t = H[0].to(torch.float64).sum(1) if Fl > 0 else torch.zeros((n, C), dtype=torch.float64, device=H.device)
        if self.W > 1:
            t = coll.all_gather_dim0(t.contiguous()).view(self.W, n, C)[0]
        return t.cpu()
