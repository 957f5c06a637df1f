"""The level record of the tree grower (models/tree/record.py): the
torch-assembled producer (TreeGrower._assemble_record) and the host decoder
agree on every named column at 1, 2 and 4 channels, and at 2 channels the
names are the columns of h2o_split_select2 at stride 13 and of the device tree.
"""
import numpy as np
import pytest
import torch

from h2o3_amd.models.tree import record as R

MODE_OF_C = {1: 2, 2: 0, 4: 3}
BS = 6


def _grower(min_rows):
    from h2o3_amd.models.tree.binning import BinnedData
    from h2o3_amd.models.tree.engine import GrowParams, TreeGrower
    bd = BinnedData()
    bd.codes = torch.zeros((4, 5), dtype=torch.uint8)
    bd.F = bd.Fp = 5
    bd.Bs = BS
    bd.na_code = BS - 1
    bd.nbins = [BS - 1] * 5
    bd.is_cat = [False] * 5
    bd.names = [f"f{j}" for j in range(5)]
    bd.nrows_local = 4
    return TreeGrower(bd, GrowParams(min_rows=min_rows))


def _level(C):
    """A three-node level: node 0 splits, node 1 has no split (-inf gain),
    node 2 has one but is lighter than 2 * min_rows."""
    rng = np.random.default_rng(C)
    L = rng.integers(1, 50, (3, C)).astype(np.float64) + 0.25
    Rt = rng.integers(1, 50, (3, C)).astype(np.float64) + 0.5
    wcol = [0, 2] if C == 4 else [0]
    L[0, wcol], Rt[0, wcol] = 30.0, 40.25
    L[2, wcol], Rt[2, wcol] = 1.0, 1.5           # node weight 2.5 (5 under uplift) < 2 * min_rows = 20
    sp = {"gain": torch.tensor([3.5, float("-inf"), 0.125], dtype=torch.float64),
          "feat": torch.tensor([4, 0, 2]), "t": torch.tensor([1, 0, 3]), "opt": torch.tensor([1, 0, 2]),
          "L": torch.as_tensor(L), "R": torch.as_tensor(Rt), "tot": torch.as_tensor(L + Rt),
          "mask": torch.as_tensor(rng.integers(0, 2, (3, BS)).astype(np.uint8))}
    return sp


@pytest.mark.parametrize("naw", [False, True])
@pytest.mark.parametrize("part", [False, True])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_assembled_record_round_trips(C, part, naw):
    gr = _grower(min_rows=10)
    sp = _level(C)
    if naw:
        sp["naw"] = torch.tensor([0.0, 2.0, 7.5], dtype=torch.float64)
    rec, feat, mask = gr._assemble_record(sp, None, MODE_OF_C[C], part)
    c = R.rec_cols(C)
    assert rec.dtype == torch.float64 and tuple(rec.shape) == (3, c.width if naw else c.NAW)
    rec = rec.numpy().copy()
    if part:
        # the partition of the whole frontier writes the left counts into NL
        assert np.array_equal(feat.numpy(), [4, 0, 0]) and feat.dtype == torch.int64
        assert np.array_equal(mask.numpy(), np.stack([sp["mask"][0].numpy(), np.ones(BS), np.ones(BS)]))
        assert mask.dtype == torch.uint8
        rec[:, c.NL] = [11.0, 0.0, 5.0]
    d = R.decode(rec, C, part)
    assert np.array_equal(d.gain, sp["gain"].numpy())
    for name in ("feat", "t", "opt"):
        got = getattr(d, name)
        assert got.dtype == np.int64 and np.array_equal(got, sp[name].numpy()), name
    for name in ("L", "R", "tot"):
        assert getattr(d, name).shape == (3, C) and np.array_equal(getattr(d, name), sp[name].numpy()), name
    if part:
        assert d.ok.dtype == bool and d.ok.tolist() == [True, False, False]
        assert d.nleft.dtype == np.int64 and d.nleft.tolist() == [11, 0, 5]
    else:
        assert d.ok is None and d.nleft is None
    if naw:
        assert np.array_equal(d.naw, sp["naw"].numpy())
    else:
        assert d.naw is None


def test_xgb_ok_has_no_weight_test():
    gr = _grower(min_rows=10)
    gr.p.criterion = "xgb"
    rec, _, _ = gr._assemble_record(_level(2), None, 1, True)
    assert R.decode(rec.numpy(), 2, True).ok.tolist() == [True, False, True]


def test_two_channel_names_are_the_kernel_record():
    """h2o_split_select2 / h2o_pair_select at stride 13 (tests/split_common.py,
    test_split_kernels_gpu.py: fields 0..3, L at 4..5, R at 6..7, totals at
    8..9, ok 10, left count 11, NA weight 12) and the device tree's columns."""
    from h2o3_amd.models.tree import devtree as D
    c = R.rec_cols(2)
    assert (R.GAIN, R.FEAT, R.T, R.OPT) == (0, 1, 2, 3)
    assert (c.L, c.R, c.TOT, c.OK, c.NL, c.NAW, c.width) == (4, 6, 8, 10, 11, 12, 13)
    assert (D.GAIN, D.FEAT, D.T, D.OPT, D.L0, D.L1, D.R0, D.R1, D.T0, D.T1, D.OK, D.NL, D.NAW, D.ST, D.CT, D.VAL) \
        == tuple(range(16)) and D.RS == 16
    assert (D.GAIN, D.FEAT, D.T, D.OPT) == (R.GAIN, R.FEAT, R.T, R.OPT)
    assert (D.L0, D.R0, D.T0, D.OK, D.NL, D.NAW) == (c.L, c.R, c.TOT, c.OK, c.NL, c.NAW)
    assert R.weight_col(0) == 0 and R.weight_col(1) == 1
