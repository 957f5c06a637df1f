"""Forest sums on a grid of overridden columns: the primitive under partial
dependence, ICE curves and the H statistic of tree models.

`forest_grid_sums` dispatches to libtree_pd.so (csrc/tree_pd.hip) on a GPU
device; `forest_grid_sums_torch` is the definition in torch: per grid point,
override the rows of a copy of X and score it with `Forest._predict_torch`.
It runs on CPU tensors and for forests deeper than the kernel's cap, and is
the kernel tests' oracle.

The definition: for X [F, N], feature indices cols (1 to 4 of them) and grid
[S, G], out[g] == Forest.predict(X', K) where X' is X with row cols[s] set to
grid[s, g] for every s.  The equality is exact: the kernel adds the same f32
leaf values in the same (tree) order as the scoring kernel.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native
from ._native import check as _check, ptr as _ptr, stream as _stream

MAX_COLS = 4                  # columns overridden together
CHUNK = 64                    # grid points per launch: the bits of a uint64 mask
MAX_DEPTH = 64                # deepest forest the kernel takes (splits on one path)


class GridResult:
    """Result of `forest_grid_sums`.

    sums         [G, N, K] f32: sums[g] has Forest.predict's layout
    kernel       True when the HIP kernels produced it
    why          why the torch implementation ran instead (None on the kernel)
    grid_chunks  launches of up to 64 grid points the kernel run took
    """
    __slots__ = ("sums", "kernel", "why", "grid_chunks")

    def __init__(self, sums, kernel, why=None, grid_chunks=0):
        self.sums, self.kernel, self.why, self.grid_chunks = sums, kernel, why, grid_chunks


def max_depth(P) -> int:
    """Most split nodes on one root-to-leaf path of the packed forest P: the
    bound of the walk's stack.  Computed once per pack (every tree one level
    per step, on the host) and kept in P."""
    if "max_depth" not in P:
        left, right = P["left"].cpu().numpy(), P["right"].cpu().numpy()
        level = P["roots"].cpu().numpy().astype(np.int64)
        depth = 0
        while True:
            level = level[left[level] >= 0]
            if level.size == 0:
                break
            level = np.concatenate([left[level], right[level]]).astype(np.int64)
            depth += 1
        P["max_depth"] = depth
    return P["max_depth"]


def forest_grid_sums_torch(P, X, K, cols, grid):
    """The definition above in torch: a loop over the grid points."""
    from ..models.tree.shared import Forest
    X = X.to(torch.float32)
    G = int(grid.shape[1])
    out = torch.zeros((G, int(X.shape[1]), K), dtype=torch.float32, device=X.device)
    Xg = X.clone()
    for g in range(G):
        for s, c in enumerate(cols):
            Xg[c] = grid[s, g]
        out[g] = Forest._predict_torch(Xg, K, P)
    return out


def launch_shape(G, depth):
    """(threads per block, LDS bytes per block) of a kernel launch for a chunk
    of G <= 64 grid points on a forest of that depth."""
    lib = _native.get_lib("tree_pd", required=True)
    sd = max(1, min(int(depth), int(G) - 1))
    th = lib.h2o_pd_block_threads(int(G), sd)
    return th, int(lib.h2o_pd_lds_bytes(th, int(G), sd))


def forest_grid_sums(P, X, K, cols, grid, row0=0, nrows=None) -> GridResult:
    """Per-class leaf sums [G, n, K] of rows [row0, row0 + nrows) of X [F, N]
    (column-major float32, NaN = NA, enum codes as floats) with the rows
    cols[s] of X replaced by grid[s, g], for every grid point g.

    P            Forest.pack() on X's device
    cols         1 to 4 distinct feature indices
    grid         [len(cols), G] float32; NaN is NA, any float is allowed for
                 an enum column (out-of-range codes take the NA direction)
    row0, nrows  a row tile of X: it is read in place through an offset and
                 X's leading dimension, no copy is made

    On a GPU: pd_node_mask_kernel + pd_walk_kernel (csrc/tree_pd.hip) per chunk
    of 64 grid points and per tree class.  `forest_grid_sums_torch` runs for
    CPU tensors and for a forest deeper than MAX_DEPTH = 64 splits on a path
    (the kernel's LDS stack is sized from min(depth, 63), so the cap only keeps
    the walk of a degenerate tree off the GPU); the result then says why."""
    cols = [int(c) for c in cols]
    S = len(cols)
    F, N = int(X.shape[0]), int(X.shape[1])
    if not 1 <= S <= MAX_COLS:
        raise ValueError(f"forest_grid_sums: 1 to {MAX_COLS} columns, got {S}")
    if len(set(cols)) != S or min(cols) < 0 or max(cols) >= F:
        raise ValueError(f"forest_grid_sums: cols must be distinct feature indices below {F}: {cols}")
    if grid.dim() != 2 or int(grid.shape[0]) != S:
        raise ValueError("forest_grid_sums: grid must be [len(cols), G]")
    n = N - row0 if nrows is None else int(nrows)
    if row0 < 0 or n < 0 or row0 + n > N:
        raise ValueError("forest_grid_sums: the row tile is outside X")
    G = int(grid.shape[1])
    grid = grid.to(device=X.device, dtype=torch.float32).contiguous()
    why = None
    if X.device.type != "cuda":
        why = "CPU tensors"
    elif max_depth(P) > MAX_DEPTH:
        why = f"the forest is {max_depth(P)} splits deep, the kernel takes {MAX_DEPTH}"
    if why is not None:
        return GridResult(forest_grid_sums_torch(P, X[:, row0:row0 + n], K, cols, grid), False, why)
    out = torch.zeros((G, n, K), dtype=torch.float32, device=X.device)
    T = P["T"]
    n_nodes = int(P["node"].shape[0])
    if G == 0 or n == 0 or T == 0 or n_nodes == 0:
        return GridResult(out, True, None, 0)
    if int(P["feat"].max()) >= F:
        raise ValueError("forest_grid_sums: the forest splits on a feature the matrix does not have")
    lib = _native.get_lib("tree_pd", required=True)
    X = X.contiguous().to(torch.float32)
    stream = _stream()
    lmask = torch.empty(n_nodes, dtype=torch.int64, device=X.device)
    ccols = (ctypes.c_int * S)(*cols)
    base = ctypes.c_void_p(X.data_ptr() + 4 * row0)
    classes = sorted(set(P["tclass"].tolist())) if K > 1 else [0]
    chunks = 0
    for g0 in range(0, G, CHUNK):
        gc = min(CHUNK, G - g0)
        chunks += 1
        for i, k in enumerate(classes):
            if not 0 <= k < K:
                raise ValueError(f"forest_grid_sums: a tree of class {k} in a forest scored with K = {K}")
            rc = lib.h2o_forest_pd_chunk(base, N, n, _ptr(P["node"]), n_nodes, _ptr(P["cat_off"]),
                                         _ptr(P["cat_len"]), _ptr(P["cat_bits"]), _ptr(P["value"]),
                                         _ptr(P["roots"]), _ptr(P["tclass"]), T, k, ccols, S, _ptr(grid), G, g0, gc,
                                         max_depth(P), _ptr(lmask), 1 if i == 0 else 0,
                                         ctypes.c_void_p(out.data_ptr() + 4 * g0 * n * K), n * K, K, stream)
            _check(rc, "h2o_forest_pd_chunk")
    return GridResult(out, True, None, chunks)
