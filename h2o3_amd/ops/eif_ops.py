"""Path-length sums of a hyperplane forest (Extended Isolation Forest).

`pack_hyperplane_forest` turns the estimator's node lists into the sparse
tables of csrc/tree_eif.hip: a trained node has extension_level + 1 non-zero
normal components, so only those are stored.  `hyperplane_forest_lengths`
dispatches to libtree_eif.so on a GPU tensor and to a row-chunked torch walk
over the same tables on a CPU tensor.

The rule, in f64: xj = the f32 input widened, NaN -> 0, +-inf -> +-DBL_MAX;
proj = sum over the node's entries in ascending column of n_j * (xj - p_j),
each product rounded before it is added; left iff proj <= 0 (a NaN proj goes
right); a leaf adds its value.  Leaf values are added in tree order onto what
`out` holds, so scoring a forest in tree ranges gives the bits of one call.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _native
from ._native import check as _check, ptr as _ptr, stream as _stream

TREES_IN_FLIGHT = (1, 2, 4)   # trees a thread walks together
TILE_MAX_P = 128              # widest X whose rows the kernel stages in LDS (32 KiB per wave)
CPU_CHUNK_BYTES = 64 << 20    # f64 copy of a row chunk on the CPU walk

Plan = namedtuple("Plan", "trees_in_flight tile")


def launch_plan(P, trees_in_flight=None, tile=None) -> Plan:
    """The kernel launch for X of P columns; explicit values override the
    defaults and are checked."""
    tw = 2 if trees_in_flight is None else int(trees_in_flight)
    if tw not in TREES_IN_FLIGHT:
        raise ValueError(f"trees_in_flight must be one of {TREES_IN_FLIGHT}, got {tw}")
    fits = 1 <= int(P) <= TILE_MAX_P
    if tile and not fits:
        raise ValueError(f"the LDS row tile takes at most {TILE_MAX_P} columns, got {P}")
    return Plan(tw, fits if tile is None else bool(tile))


class HyperplanePack:
    """Sparse tables of a hyperplane forest, as host numpy arrays.

    hdr    [N, 4] int32  inner node: left, right (global ids), first entry,
                         entry count; leaf: -1, -1 and its f64 value's 8 bytes
    col    [E] int32     column of each entry, ascending within a node
    np     [E, 2] f64    (normal, point) component of each entry
    roots  [T] int32     first node of each tree
    value  [N] f64       leaf values (0 at inner nodes): hdr's leaf bytes, typed
    P                    columns a scored matrix needs (largest column + 1)
    """

    def __init__(self, hdr, col, np_, roots, value, P):
        self.hdr, self.col, self.np, self.roots, self.value, self.P = hdr, col, np_, roots, value, P
        self._dev = {}
        self._walk = None

    @property
    def ntrees(self):
        return int(self.roots.shape[0])

    def to_device(self, device):
        """The kernel's tables (hdr, col, np, roots) as tensors on `device`,
        moved once per device."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in ("hdr", "col", "np", "roots")}
        return self._dev[key]

    def walk_tables(self):
        """What the torch walk indexes with, made once: hdr and col as int64,
        the (normal, point) pairs and the typed leaf values, on the host."""
        if self._walk is None:
            self._walk = (torch.from_numpy(self.hdr).long(), torch.from_numpy(self.col).long(),
                          torch.from_numpy(self.np), torch.from_numpy(self.value))
        return self._walk


def pack_hyperplane_forest(trees) -> HyperplanePack:
    """trees: list of trees, each a list of (normal | None, point | None, left,
    right, value, rows) with tree-local child ids (-1 at a leaf).  Node ids of
    the pack are the concatenation order, so id - roots[t] indexes tree t."""
    n_nodes = sum(len(tr) for tr in trees)
    hdr = np.full((n_nodes, 4), -1, dtype=np.int32)
    value = np.zeros(n_nodes, dtype=np.float64)
    roots = np.zeros(len(trees), dtype=np.int32)
    cols, pairs = [], []
    base = n_ent = 0
    P = 1
    for t, tr in enumerate(trees):
        if not tr:
            raise ValueError(f"tree {t} has no nodes")
        roots[t] = base
        for i, nd in enumerate(tr):
            nv, pt, l, r, v = nd[:5]
            if l < 0:
                value[base + i] = float(v)
                continue
            if not (0 <= l < len(tr) and 0 <= r < len(tr)):
                raise ValueError(f"tree {t} node {i}: child outside the tree")
            nv = np.asarray(nv, dtype=np.float64)
            pt = np.asarray(pt, dtype=np.float64)
            nz = np.flatnonzero(nv != 0)
            hdr[base + i] = (base + l, base + r, n_ent, nz.size)
            cols.append(nz.astype(np.int32))
            pairs.append(np.stack([nv[nz], pt[nz]], 1))
            n_ent += nz.size
            P = max(P, int(nz[-1]) + 1 if nz.size else 1)
        base += len(tr)
    leaf = hdr[:, 0] < 0
    hdr.view(np.float64)[leaf, 1] = value[leaf]
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int32)
    np_ = np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.float64)
    return HyperplanePack(hdr, col, np.ascontiguousarray(np_), roots, value, P)


def _lengths_torch(pack, X, t0, t1, out, nodes):
    """The rule over the sparse tables, one row chunk and one tree at a time."""
    hdr, col, npair, value = pack.walk_tables()
    n, P = int(X.shape[0]), int(X.shape[1])
    chunk = max(1, CPU_CHUNK_BYTES // (8 * max(P, 1)))
    last = max(int(col.shape[0]) - 1, 0)
    for a in range(0, n, chunk):
        Xc = torch.nan_to_num(X[a:a + chunk].to(torch.float64))
        m = int(Xc.shape[0])
        rows = torch.arange(m, device=X.device)
        acc = out[a:a + m]
        for t in range(t0, t1):
            nd = torch.full((m,), int(pack.roots[t]), dtype=torch.int64, device=X.device)
            while True:
                h = hdr[nd]
                act = h[:, 0] >= 0
                if not bool(act.any()):
                    break
                cnt = torch.where(act, h[:, 3], torch.zeros_like(h[:, 3]))
                proj = torch.zeros(m, dtype=torch.float64, device=X.device)
                for s in range(int(cnt.max())):
                    on = s < cnt
                    e = (h[:, 2] + s).clamp_(0, last)
                    term = npair[e, 0] * (Xc[rows, col[e]] - npair[e, 1])
                    proj = torch.where(on, proj + term, proj)
                nd = torch.where(act, torch.where(proj <= 0, h[:, 0], h[:, 1]), nd)
            acc += value[nd]
            if nodes is not None:
                nodes[a:a + m, t - t0] = (nd - int(pack.roots[t])).to(torch.int32)


def hyperplane_forest_lengths(pack, X, t0=0, t1=None, out=None, node_out=False, plan=None):
    """out[r] += the leaf values of trees t0..t1-1 for row r of X [n, P] f32
    row-major (what DataInfo.expand(pad=False) returns); `out` (f64 [n]) starts
    at zero when not given.  Returns out, or (out, nodes) with node_out, nodes
    being the [n, t1 - t0] int32 tree-local leaf ids.

    On a GPU tensor this is one launch of csrc/tree_eif.hip (`plan`: a
    `launch_plan`, default `launch_plan(P)`) that allocates only the outputs it
    was not given; on a CPU tensor the same rule runs in torch in row chunks."""
    t1 = pack.ntrees if t1 is None else int(t1)
    t0 = int(t0)
    if not 0 <= t0 <= t1 <= pack.ntrees:
        raise ValueError(f"tree range [{t0}, {t1}) outside the forest's {pack.ntrees} trees")
    if X.dim() != 2 or X.dtype != torch.float32 or not X.is_contiguous():
        raise ValueError("hyperplane_forest_lengths: X must be a contiguous [n, P] float32 matrix")
    n, P = int(X.shape[0]), int(X.shape[1])
    if t1 > t0 and n > 0 and P < pack.P:
        raise ValueError(f"the forest reads column {pack.P - 1}, X has {P} columns")
    if out is None:
        out = torch.zeros(n, dtype=torch.float64, device=X.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous() or out.device != X.device:
        raise ValueError("hyperplane_forest_lengths: out must be a contiguous f64 [n] tensor on X's device")
    nodes = torch.empty((n, t1 - t0), dtype=torch.int32, device=X.device) if node_out else None
    if n > 0 and t1 > t0:
        if X.device.type == "cuda":
            plan = launch_plan(P) if plan is None else launch_plan(P, *plan)
            lib = _native.get_lib("tree_eif", required=True)
            tb = pack.to_device(X.device)
            rc = lib.h2o_eif_lengths(_ptr(X), n, P, _ptr(tb["hdr"]), _ptr(tb["col"]), _ptr(tb["np"]),
                                     _ptr(tb["roots"]), t0, t1, _ptr(out), _ptr(nodes), plan.trees_in_flight,
                                     int(plan.tile), _stream())
            _check(rc, "h2o_eif_lengths")
        else:
            _lengths_torch(pack, X, t0, t1, out, nodes)
    return (out, nodes) if node_out else out
