"""The level record: one row of doubles per frontier node, written by the
split search and read once per level by the host.

Columns, for C histogram channels:

    GAIN FEAT T OPT | L[C] | R[C] | TOT[C] | OK NL | NAW

OK (the node splits) and NL (rows going left) are meaningful only on levels
whose partition ran on the device before the host read the record; NAW (the
node's NA weight on the winning column) is the optional last column.  For
C == 2 this is the 13-double row that `h2o_split_select2` and
`h2o_pair_select` write and the first 13 columns of the device tree's record.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

GAIN, FEAT, T, OPT = range(4)


class RecCols(NamedTuple):
    L: int        # first of C left-child channel sums
    R: int        # first of C right-child channel sums
    TOT: int      # first of C node totals
    OK: int
    NL: int
    NAW: int
    width: int    # columns of a record that carries NAW


def rec_cols(C: int) -> RecCols:
    return RecCols(4, 4 + C, 4 + 2 * C, 4 + 3 * C, 5 + 3 * C, 6 + 3 * C, 7 + 3 * C)


def weight_col(mode: int) -> int:
    """Offset of the row-weight channel inside L / R / TOT (mode 1 keeps
    (g, h): the hessian is the weight)."""
    return 1 if mode == 1 else 0


class LevelSplits(NamedTuple):
    """A level record decoded on the host (numpy arrays, one entry per node)."""
    gain: np.ndarray
    feat: np.ndarray               # int64
    t: np.ndarray                  # int64
    opt: np.ndarray                # int64
    L: np.ndarray                  # [n, C]
    R: np.ndarray                  # [n, C]
    tot: np.ndarray                # [n, C]
    ok: Optional[np.ndarray]       # bool; None unless the partition ran on the device
    nleft: Optional[np.ndarray]    # int64; None unless the partition ran on the device
    naw: Optional[np.ndarray]      # None when the record has no NAW column


def decode(rec: np.ndarray, C: int, part: bool) -> LevelSplits:
    c = rec_cols(C)
    return LevelSplits(rec[:, GAIN], rec[:, FEAT].astype(np.int64), rec[:, T].astype(np.int64),
                       rec[:, OPT].astype(np.int64), rec[:, c.L:c.R], rec[:, c.R:c.TOT], rec[:, c.TOT:c.OK],
                       rec[:, c.OK] > 0 if part else None, rec[:, c.NL].astype(np.int64) if part else None,
                       rec[:, c.NAW] if rec.shape[1] > c.NAW else None)
