"""Shared tree model machinery: feature prep, binning, forest packing and
GPU scoring, variable importance, leaf-node assignment.

Reference: hex/tree/SharedTree.java (driver skeleton),
hex/tree/SharedTreeModel.java (score0, varimp, predictLeafNodeAssignment),
hex/tree/CompressedForest.java.
"""
from __future__ import annotations

import math

import numpy as np
import pandas as pd
import torch

from ...core.frame import H2OFrame
from ...core.vec import T_ENUM, T_INT, T_REAL, Vec
from ...ops import _native
from ...ops._native import check as _check, ptr as _ptr, stream as _stream
from ...parallel import cloud
from ..base import H2OEstimator
from .binning import bin_frame_tensors
from .engine import Tree

def iter_seed(seed, it, salt=0):
    """Seed of boosting / forest iteration `it`: every tree's randomness
    (row sample, per-tree and per-node column samples) is a function of
    (seed, iteration) only, so a build continued from a checkpoint draws
    exactly what an uninterrupted build draws for the same trees
    (SharedTree.java:144 checkpoint restart)."""
    return (int(seed) * 1000003 + int(it) * 7919 + int(salt) * 104729 + 12345) & 0x7FFFFFFF


def reseed_iteration(drv, seed, it):
    """Re-seed a driver's generators for iteration `it` (row sampling:
    rank-dependent torch generator; host column sampling: rank-independent)."""
    from ...parallel import cloud
    drv.gen.manual_seed(iter_seed(seed, it, 1) + cloud.rank())
    drv.rng = np.random.RandomState(iter_seed(seed, it, 2))
    drv.grower.rng = np.random.RandomState(iter_seed(seed, it, 3))


def checkpoint_model(ck, algo, est):
    """The checkpoint model a build continues (hex/ModelBuilder checkpoint
    checks: same algorithm, same response, the new ntrees must exceed the
    checkpoint's)."""
    from ...core import dkv
    prev = dkv.get(ck) if isinstance(ck, str) else ck
    if prev is None:
        raise ValueError(f"checkpoint: model {ck} not found")
    if getattr(prev, "algo", None) != algo:
        raise ValueError(f"checkpoint: model {getattr(prev, 'model_id', ck)} is a {getattr(prev, 'algo', '?')} "
                         f"model, not {algo}")
    done = len(prev._forest) // max(1, prev._n_tree_classes())
    if int(est._parms["ntrees"]) <= done:
        raise ValueError(f"checkpoint: ntrees ({est._parms['ntrees']}) must be larger than the checkpoint "
                         f"model's number of trees ({done})")
    return prev, done


def forest_varimp(forest, names):
    """Sum of positive split gains per feature over every split node
    (vectorized over each tree's node arrays)."""
    acc = np.zeros(len(names), dtype=np.float64)
    for t in forest.trees:
        l_ = np.asarray(t.left, dtype=np.int64)
        if l_.size == 0:
            continue
        sp = l_ >= 0
        f_ = np.asarray(t.feat, dtype=np.int64)[sp]
        g_ = np.maximum(np.asarray(t.gain, dtype=np.float64)[sp], 0.0)
        np.add.at(acc, f_, g_)
    return {n: float(acc[j]) for j, n in enumerate(names)}


class Forest:
    """Flattened struct-of-arrays forest for the scoring kernel."""

    def __init__(self):
        self.trees: list[Tree] = []
        self.tclass: list[int] = []
        self._packed = None
        self._paths = None

    def add(self, tree: Tree, k: int = 0):
        self.trees.append(tree)
        self.tclass.append(k)
        self._packed = None

    def __len__(self):
        return len(self.trees)

    def pack(self, device, upto=None):
        trees = self.trees if upto is None else self.trees[:upto]
        key = (str(device), len(trees))
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        # vectorized per tree (trees of deep DRF models have ~10^5 nodes; a
        # per-node Python loop here cost seconds per scoring)
        feat, thr, left, right, nal, coff, clen, val, roots, bits = [], [], [], [], [], [], [], [], [], []
        base = 0
        nb = 0
        for t in trees:
            n = t.n_nodes
            roots.append(base)
            f_ = np.asarray(t.feat, dtype=np.int64)
            th = np.asarray(t.thr, dtype=np.float64)
            l_ = np.asarray(t.left, dtype=np.int64)
            r_ = np.asarray(t.right, dtype=np.int64)
            feat.append(np.maximum(f_, 0))
            thr.append(np.where(np.isnan(th), 0.0, th))
            left.append(np.where(l_ >= 0, l_ + base, -1))
            right.append(np.where(r_ >= 0, r_ + base, -1))
            nal.append(np.asarray(t.na_left, dtype=bool).astype(np.uint8))
            co = np.full(n, -1, dtype=np.int64)
            cl = np.zeros(n, dtype=np.int64)
            for i in np.nonzero(np.asarray(t.is_cat, dtype=bool))[0]:
                m = t.cat_left[i]
                if m is None:
                    continue
                mb = np.asarray(m).astype(np.uint8).reshape(-1)
                co[i] = nb
                cl[i] = mb.size
                bits.append(mb)
                nb += mb.size
            coff.append(co)
            clen.append(cl)
            val.append(np.asarray(t.value, dtype=np.float64))
            base += n

        def cat(parts, dt):
            return np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
        d = device
        # packed 16-byte nodes for the HIP kernel: feature | NA-left << 30 |
        # categorical << 31, threshold bits, left, right
        f32 = cat(thr, np.float32)
        cof = cat(coff, np.int32)
        node = np.stack([(cat(feat, np.int64) & 0x3FFFFFFF) | (cat(nal, np.int64) << 30) |
                         ((cof >= 0).astype(np.int64) << 31),
                         f32.view(np.int32).astype(np.int64), cat(left, np.int64), cat(right, np.int64)], 1)
        node = node.astype(np.uint32).view(np.int32) if node.size else np.zeros((0, 4), dtype=np.int32)
        P = {"node": torch.as_tensor(np.ascontiguousarray(node), device=d),
             "feat": torch.as_tensor(cat(feat, np.int32), device=d),
             "thr": torch.as_tensor(cat(thr, np.float32), device=d),
             "left": torch.as_tensor(cat(left, np.int32), device=d),
             "right": torch.as_tensor(cat(right, np.int32), device=d),
             "na_left": torch.as_tensor(cat(nal, np.uint8), device=d),
             "cat_off": torch.as_tensor(cat(coff, np.int32), device=d),
             "cat_len": torch.as_tensor(cat(clen, np.int32), device=d),
             "cat_bits": torch.as_tensor(cat(bits, np.uint8) if bits else np.zeros(1, dtype=np.uint8), device=d),
             "value": torch.as_tensor(cat(val, np.float32), device=d),
             "roots": torch.tensor(roots, dtype=torch.int32, device=d),
             "tclass": torch.tensor(self.tclass[: len(trees)], dtype=torch.int32, device=d),
             "T": len(trees)}
        self._packed = (key, P)
        return P

    def leaf_paths(self, device, upto=None):
        """Leaf-path table for baseline SHAP (ops/shap_ops.py), cached and
        invalidated like pack().  Leaves are numbered tree by tree; per leaf:
        its value (f64), its tree's class, and its path elements (one per
        distinct feature on the root-to-leaf path, ordered by feature id).
        An element's conditions are (packed node index, wants-left) pairs
        into pack()'s node arrays, so thresholds, NA directions and the
        categorical bitsets are read from there.

        Keys: leaf_val [L] f64, leaf_cls [L] i32, el_off [L+1], el_feat [E],
        cond_off [E+1], cond_node [C] i32, cond_left [C] u8, tree_leaf_off
        (host list, T+1), L, max_path (most elements of one leaf),
        max_tree_leaves, max_feat (largest feature id split on, -1 if none),
        el_zero [E] f64 (path-dependent TreeSHAP's zero-fraction of the
        element: the product over its conditions of cover[wanted child] /
        cover[node], covers = max(Tree.weight, 0), a zero node cover counting
        as 1)."""
        trees = self.trees if upto is None else self.trees[:upto]
        # keyed on the pack it indexes into: whatever drops the pack drops this too
        P = self.pack(device, upto)
        cached = self.__dict__.get("_paths")
        if cached is not None and cached[0] is P:
            return cached[1]
        # vectorised per tree: walk every leaf up to the root one level per step
        lval, lcls, nel, efeat, ncond, cnode, cleft, ezero = [], [], [], [], [], [], [], []
        tree_leaf_off = [0]
        base = 0
        for ti, t in enumerate(trees):
            n = t.n_nodes
            l_ = np.asarray(t.left, dtype=np.int64)
            r_ = np.asarray(t.right, dtype=np.int64)
            f_ = np.asarray(t.feat, dtype=np.int64)
            idx = np.arange(n, dtype=np.int64)
            inner = l_ >= 0
            parent = np.full(n, -1, dtype=np.int64)
            isleft = np.zeros(n, dtype=np.uint8)
            parent[l_[inner]] = idx[inner]
            isleft[l_[inner]] = 1
            parent[r_[inner]] = idx[inner]
            leaves = idx[~inner]
            cur = leaves.copy()
            who = np.arange(leaves.size, dtype=np.int64)
            cover = np.maximum(np.asarray(t.weight, dtype=np.float64), 0.0)
            if cover.size != n:                       # a tree without covers: every node counts 1
                cover = np.ones(n, dtype=np.float64)
            denom = np.where(cover > 0, cover, 1.0)
            c_leaf, c_node, c_left, c_frac = [], [], [], []
            top = leaves.copy()                       # highest ancestor reached
            for _ in range(n):
                p = parent[cur]
                live = p >= 0
                if not live.any():
                    break
                who, cur, p = who[live], cur[live], p[live]
                c_leaf.append(who)
                c_node.append(p)
                c_left.append(isleft[cur])
                c_frac.append(cover[cur] / denom[p])
                top[who] = p
                cur = p
            keep = top == 0                           # leaves hanging off the root (drops orphan nodes)
            newid = np.cumsum(keep) - 1
            if c_leaf:
                cl_ = np.concatenate(c_leaf)
                cn_ = np.concatenate(c_node)
                cw_ = np.concatenate(c_left)
                cz_ = np.concatenate(c_frac)
                ok = keep[cl_]
                cl_, cn_, cw_, cz_ = newid[cl_[ok]], cn_[ok], cw_[ok], cz_[ok]
            else:
                cl_ = cn_ = np.zeros(0, dtype=np.int64)
                cw_ = np.zeros(0, dtype=np.uint8)
                cz_ = np.zeros(0, dtype=np.float64)
            cf_ = f_[cn_]
            o = np.lexsort((cn_, cf_, cl_))           # by leaf, then feature, then node (root first)
            cl_, cn_, cw_, cf_, cz_ = cl_[o], cn_[o], cw_[o], cf_[o], cz_[o]
            nl = int(keep.sum())
            first = np.ones(cl_.size, dtype=bool)
            first[1:] = (cl_[1:] != cl_[:-1]) | (cf_[1:] != cf_[:-1])
            starts = np.nonzero(first)[0]
            nel.append(np.bincount(cl_[starts], minlength=nl))
            efeat.append(cf_[starts])
            ezero.append(np.multiply.reduceat(cz_, starts) if starts.size else np.zeros(0, dtype=np.float64))
            ncond.append(np.diff(np.append(starts, cl_.size)))
            cnode.append(cn_ + base)
            cleft.append(cw_)
            kept = leaves[keep]
            lval.append(np.asarray(t.value, dtype=np.float64)[kept])
            lcls.append(np.full(nl, self.tclass[ti], dtype=np.int64))
            tree_leaf_off.append(tree_leaf_off[-1] + nl)
            base += n

        def cat(parts, dt):
            return np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)

        def offs(counts):
            return np.concatenate([[0], np.cumsum(cat(counts, np.int64))]).astype(np.int32)
        ne = cat(nel, np.int64)
        ef = cat(efeat, np.int32)
        d = device
        PT = {"leaf_val": torch.as_tensor(cat(lval, np.float64), device=d),
              "leaf_cls": torch.as_tensor(cat(lcls, np.int32), device=d),
              "el_off": torch.as_tensor(offs(nel), device=d),
              "el_feat": torch.as_tensor(ef, device=d),
              "el_zero": torch.as_tensor(cat(ezero, np.float64), device=d),
              "cond_off": torch.as_tensor(offs(ncond), device=d),
              "cond_node": torch.as_tensor(cat(cnode, np.int32), device=d),
              "cond_left": torch.as_tensor(cat(cleft, np.uint8), device=d),
              "tree_leaf_off": tree_leaf_off,
              "L": tree_leaf_off[-1],
              "max_path": int(ne.max()) if ne.size else 0,
              "max_feat": int(ef.max()) if ef.size else -1,
              "max_tree_leaves": int(np.diff(tree_leaf_off).max()) if trees else 0}
        self._paths = (P, PT)
        return PT

    def predict_range(self, X: torch.Tensor, K: int, start: int, end: int):
        """[N, K] sums of trees [start, end) only (incremental scoring: the
        pack covers just these trees)."""
        sub = Forest()
        sub.trees = self.trees[start:end]
        sub.tclass = self.tclass[start:end]
        return sub.predict(X, K)

    def predict(self, X: torch.Tensor, K: int, upto=None, leaf=False):
        """X: [F, N] float32 column-major.  Returns [N, K] sums (or leaf ids)."""
        N = X.shape[1]
        P = self.pack(X.device, upto)
        T = P["T"]
        out = torch.zeros((N, K), dtype=torch.float32, device=X.device)
        leaf_out = torch.empty((N, T), dtype=torch.int32, device=X.device) if leaf else None
        if T == 0:
            return leaf_out if leaf else out
        if X.device.type == "cuda":
            lib = _native.get_lib("tree_predict")
            X = X.contiguous().to(torch.float32)
            rc = lib.h2o_forest_predict(_ptr(X), N, _ptr(P["node"]), _ptr(P["cat_off"]),
                                        _ptr(P["cat_len"]), _ptr(P["cat_bits"]), _ptr(P["value"]),
                                        _ptr(P["roots"]), _ptr(P["tclass"]), T, K,
                                        _ptr(None if leaf else out), _ptr(leaf_out if leaf else None), _stream())
            _check(rc, "h2o_forest_predict")
            return leaf_out if leaf else out
        return self._predict_torch(X, K, P, leaf)

    def predict_grid(self, X: torch.Tensor, K: int, cols, grid: torch.Tensor, upto=None):
        """X: [F, N] float32 column-major; cols: 1 to 4 feature indices; grid
        [len(cols), G] float32 (NaN = NA).  Returns [G, N, K] sums: out[g] is
        bit for bit predict(X', K) for X' = X with row cols[s] set to
        grid[s, g] for every s (partial dependence; ops/pd_ops.py)."""
        from ...ops import pd_ops
        return pd_ops.forest_grid_sums(self.pack(X.device, upto), X, K, cols, grid).sums

    @staticmethod
    def _predict_torch(X, K, P, leaf=False):
        N = X.shape[1]
        T = P["T"]
        out = torch.zeros((N, K), dtype=torch.float32, device=X.device)
        leaf_out = torch.empty((N, T), dtype=torch.int32, device=X.device) if leaf else None
        ar = torch.arange(N, device=X.device)
        for t in range(T):
            nd = torch.full((N,), int(P["roots"][t]), dtype=torch.int64, device=X.device)
            while True:
                l = P["left"][nd].long()
                active = l >= 0
                if not bool(active.any()):
                    break
                f = P["feat"][nd].long()
                x = X[f, ar]
                isnan = torch.isnan(x)
                co = P["cat_off"][nd].long()
                cl = P["cat_len"][nd].long()
                code = torch.nan_to_num(x, nan=-1).long()
                in_rng = (code >= 0) & (code < cl)
                bit = P["cat_bits"][(co + code.clamp(min=0)).clamp(min=0, max=P["cat_bits"].numel() - 1)] != 0
                nal = P["na_left"][nd] != 0
                go_cat = torch.where(isnan | ~in_rng, nal, bit)
                go_num = torch.where(isnan, nal, x < P["thr"][nd])
                go = torch.where(co >= 0, go_cat, go_num)
                nxt = torch.where(go, l, P["right"][nd].long())
                nd = torch.where(active, nxt, nd)
            if leaf:
                leaf_out[:, t] = (nd - int(P["roots"][t])).to(torch.int32)
            else:
                out[ar, int(P["tclass"][t])] += P["value"][nd]
        return leaf_out if leaf else out


class SharedTreeEstimator(H2OEstimator):
    def _check_response(self, frame, y):
        """SharedTree.init: a constant response is an error unless
        check_constant_response is off; r2_stopping is deprecated there and
        ignored with a warning."""
        p = self._parms
        if y is not None and p.get("check_constant_response", True) and y in frame.names:
            v = frame.vec(y)
            if v.type == "enum":
                codes = v.data
                import torch as _t
                # level counts by bincount: an f64 index_add_ onto 2-3 slots
                # serialises on atomics (2.2 s at 10M rows)
                present = _t.bincount((codes.long() + 1).clamp_min(0),
                                      minlength=len(v.domain or []) + 1).to(_t.float64)
                from ...parallel import collectives as _coll
                _coll.allreduce_(present)
                if int((present[1:] > 0).sum()) < 2:
                    raise ValueError("ERRR on field: _response: Response cannot be constant.")
            elif v.is_const():
                raise ValueError("ERRR on field: _response: Response cannot be constant.")
        r2 = p.get("r2_stopping")
        if r2 is not None and float(r2) < 1.79e308:
            import warnings
            warnings.warn("r2_stopping is no longer supported and will be ignored if set - please use "
                          "stopping_rounds, stopping_metric and stopping_tolerance instead.")

    """Base of GBM / DRF / XGBoost / IsolationForest / UpliftDRF."""

    def _cv_optimal_params(self, cv_models):
        """Main model trains the mean number of trees the early-stopped CV models
        kept (ModelBuilder.cv_computeAndSetOptimalParameters / SharedTree)."""
        import math as _m
        if int(self._parms.get("stopping_rounds") or 0) > 0 and cv_models and \
                all(getattr(m, "_forest", None) is not None for m in cv_models):
            nt = [len(m._forest) // max(1, getattr(m, "_K", 1)) for m in cv_models]
            self._parms["ntrees"] = max(1, int(_m.ceil(sum(nt) / len(nt))))
            self._parms["stopping_rounds"] = 0

    def _feature_inputs(self, frame: H2OFrame, x):
        feats, is_cat, cards = [], [], []
        domains = {}
        for n in x:
            v = frame.vec(n)
            if v.type == T_ENUM:
                feats.append(v.data)
                is_cat.append(True)
                cards.append(len(v.domain))
                domains[n] = list(v.domain)
            else:
                feats.append(v.as_float(torch.float32) if v.data.dtype != torch.float64 else v.data.to(torch.float32))
                is_cat.append(False)
                cards.append(0)
        return feats, is_cat, cards, domains

    def _bin(self, spec, hist_type=None, nbins=None, want_col_major=True):
        p = self._parms
        feats, is_cat, cards, domains = self._feature_inputs(spec.frame, spec.x)
        self._x_domains = domains
        self._x_is_cat = is_cat
        bd = bin_frame_tensors(feats, is_cat, cards, spec.x,
                               hist_type=hist_type or p.get("histogram_type", "AUTO"),
                               nbins=nbins or p.get("nbins", 20), nbins_top_level=p.get("nbins_top_level", 1024),
                               nbins_cats=p.get("nbins_cats", 1024),
                               seed=(p.get("seed") if p.get("seed") not in (None, -1) else 1234),
                               want_col_major=want_col_major)
        return bd

    def _score_matrix(self, frame: H2OFrame) -> torch.Tensor:
        """[F, N] float32 column-major scoring matrix adapted to training."""
        x = self._spec.x
        cols = []
        for n in x:
            if n not in frame.names:
                cols.append(torch.full((frame.nlocal,), float("nan"), device=cloud.device()))
                continue
            v = frame.vec(n)
            if n in self._x_domains:
                codes = self._adapt_enum(v, self._x_domains[n])
                c = codes.to(torch.float32)
                cols.append(torch.where(codes < 0, torch.full_like(c, float("nan")), c))
            else:
                cols.append(v.as_float(torch.float32) if not v.on_host else
                            torch.full((frame.nlocal,), float("nan"), device=cloud.device()))
        if not cols:
            return torch.zeros((0, frame.nlocal), device=cloud.device())
        return torch.stack(cols, 0).contiguous()

    def _varimp_from_forest(self, forest: Forest, names):
        return forest_varimp(forest, names)

    def predict_leaf_node_assignment(self, test_data, type="Path"):
        X = self._score_matrix(test_data)
        K = self._n_tree_classes()
        leaf = self._forest.predict(X, K, leaf=True)
        names = []
        ntrees_iter = len(self._forest) // max(K, 1)
        for t in range(len(self._forest)):
            k = self._forest.tclass[t]
            it = t // max(K, 1)
            cls = "" if K == 1 else f".C{k + 1}"
            names.append(f"T{it + 1}{cls}")
        if type == "Node_ID":
            vecs = [Vec(leaf[:, t].to(torch.float32).contiguous(), T_INT) for t in range(leaf.shape[1])]
            return H2OFrame.from_vecs(vecs, names)
        # Path: string of L/R decisions
        paths = []
        lh = leaf.cpu().numpy()
        for t, tree in enumerate(self._forest.trees):
            pmap = _paths(tree)
            paths.append([pmap.get(int(n), "") for n in lh[:, t]])
        from ...core.vec import make_enum_from_strings
        vecs = [make_enum_from_strings(p) for p in paths]
        return H2OFrame.from_vecs(vecs, names)

    def _n_tree_classes(self):
        return 1

    def staged_predict_proba(self, test_data):
        raise NotImplementedError

    @property
    def ntrees_built(self):
        return len(self._forest) // max(1, self._n_tree_classes())

    def ntrees_actual(self):
        """Trees actually built (early stopping may stop before ntrees)."""
        return self.ntrees_built

    def feature_interaction(self, max_interaction_depth=100, max_tree_depth=100, max_deepening=-1, path=None):
        """Feature interaction tables (hex/FeatureInteractions.java): one
        table per interaction depth, leaf statistics, split value histograms."""
        from .interactions import feature_interactions, interaction_tables
        K = self._n_tree_classes()
        fis = feature_interactions(self._forest, list(self._spec.x), len(self._forest) // max(K, 1), K,
                                   max_interaction_depth, max_tree_depth, max_deepening)
        tables = interaction_tables(fis)
        if path is not None:
            with pd.ExcelWriter(path) as xw:
                for i, t in enumerate(tables):
                    t.to_excel(xw, sheet_name=t.attrs.get("table_header", f"t{i}")[:31], index=False)
        return tables

    def feature_frequencies(self, test_data):
        """Per row: how often each feature is used on its decision paths,
        summed over the trees."""
        from .interactions import feature_frequencies
        X = self._score_matrix(test_data)
        leaf = self._forest.predict(X, self._n_tree_classes(), leaf=True)
        fq = feature_frequencies(self._forest, leaf, len(self._spec.x))
        return H2OFrame.from_vecs([Vec(fq[:, j].contiguous(), T_REAL) for j in range(fq.shape[1])],
                                  list(self._spec.x))

    def update_tree_weights(self, frame, weights_column):
        """Re-populate node covers from `frame` weighted by `weights_column`
        (SharedTreeModel.updateTreeWeights); TreeSHAP then explains that
        sub-population."""
        from .interactions import update_tree_weights
        X = self._score_matrix(frame)
        leaf = self._forest.predict(X, self._n_tree_classes(), leaf=True)
        update_tree_weights(self._forest, leaf, frame.vec(weights_column).as_float(torch.float64))

    def get_tree(self, tree_number=0, tree_class=None):
        K = self._n_tree_classes()
        idx = tree_number * K + (0 if tree_class is None else (tree_class if isinstance(tree_class, int) else
                                                               self._spec.response_domain.index(tree_class)))
        return self._forest.trees[idx]


def _paths(tree: Tree):
    out = {}
    stack = [(0, "")]
    while stack:
        i, p = stack.pop()
        if tree.left[i] < 0:
            out[i] = p
        else:
            stack.append((tree.left[i], p + "L"))
            stack.append((tree.right[i], p + "R"))
    return out
