"""Which histogram kernel `tree_ops.hist_build` launches, and with which launch
plan (work items, group width, fixed-point scales, pack bound, threads).

The native library is replaced by a recorder, so no device and no compiled
library is needed: only the host-side plan and the work table are exercised.
The expected calls are literals recorded from the launch code before the
launch decision moved into `tree_ops.hist_plan`; a plan that differs anywhere
(chunk, scales, group layout) shows up here."""
import types

import pytest
import torch

from h2o3_amd.ops import _native, tree_ops


class Recorder:
    """Stands in for a loaded HIP library: every h2o_* attribute logs its name
    and its scalar (int / float) arguments, then one string with a letter per
    pointer argument ('p' set, '.' null), and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("h2o_"):
            raise AttributeError(name)

        def fn(*args):
            scalars = tuple(a for a in args if isinstance(a, (int, float)))
            ptrs = "".join("." if a is None or a.value is None else "p" for a in args
                           if not isinstance(a, (int, float)))
            self.calls.append((name,) + scalars + ((ptrs,) if ptrs else ()))
            return 0
        return fn


def _bd(F, Fp, Bs, code_bytes, rows):
    dt = torch.uint8 if code_bytes == 1 else torch.int16
    return types.SimpleNamespace(F=F, Fp=Fp, Bs=Bs, code_bytes=code_bytes,
                                 codes=torch.zeros((8, Fp), dtype=dt), codes_col=None, nrows_local=rows)


def _run(monkeypatch, F, Fp, Bs, code_bytes, mode, unit_w, env=None, counts=(300000, 200001), target_blocks=None,
         need_mask=False):
    rec = Recorder()
    monkeypatch.setattr(_native, "get_lib", lambda name, required=None: rec)
    monkeypatch.setattr(tree_ops, "_stream", lambda: None)
    for k in ("H2O3_HIST_BM", "H2O3_HIST_KERNEL", "H2O3_HIST_PACK", "H2O3_HIST_BIG", "H2O3_HIST_TB",
              "H2O3_HIST_CHUNK", "H2O3_HIST_FGL", "H2O3_HIST_FGW", "H2O3_HIST_BM_RAGGED", "H2O3_HIST_BM_RED",
              "H2O3_HIST_BM_LW", "H2O3_HIST_LW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    rows = int(sum(counts))
    bd = _bd(F, Fp, Bs, code_bytes, rows)
    starts = [0]
    for c in counts[:-1]:
        starts.append(starts[-1] + c)
    ridx = torch.zeros(8, dtype=torch.int32)
    va = torch.zeros(8, dtype=torch.float32)
    vb = None if unit_w else torch.zeros(8, dtype=torch.float32)
    nm = None
    if need_mask:
        nm = torch.zeros((len(counts), F), dtype=torch.bool)
        nm[0, 0] = True
        nm[1, F - 1] = True
    tree_ops.hist_build(bd, ridx, va, vb, mode, starts, list(counts), len(counts), use_native=True,
                        target_blocks=target_blocks, vmax=[1.0, 3.5], unit_w=unit_w, need_mask=nm)
    return rec.calls


# Scalar arguments, in call order:
#   h2o_hist_bm:       Fp, n_work, F, f0, Bs, s0, s1, n_slots, mode, posv, pack_bq, G, lw, ragged
#   h2o_hist_quad:     Fp, n_work, F, f0, Bs, s0, s1, n_slots, mode, threads, posv, pack_bq, fgw, lw
#   h2o_hist_build_pk: code_bytes, Fp, n_work, F, FG, Bs, s1, pack_bq, n_slots, threads, posv
#   h2o_hist_build:    code_bytes, Fp, n_work, F, FG, Bs, s0, s1, n_slots, mode, threads, posv
_A = dict(F=100, Fp=128, Bs=256, code_bytes=1, mode=0, unit_w=True)
_BM_2X64_G = ("h2o_hist_bm", 128, 245, 100, 0, 256, 2251799813685248.0, 67108864.0, 2, 0, 0, 234881024, 64)
_BM_2X64 = _BM_2X64_G + (2, 0)
_QUAD_3X36 = ("h2o_hist_quad", 128, 172, 100, 0, 256, 1125899906842624.0, 33554432.0, 2, 0, 512, 0, 117440512, 36)
CASES = {
    "bm_2x64_packed": (_A, [_BM_2X64 + ("ppp.pp...p.",)]),
    "bm_4x32": (dict(F=100, Fp=128, Bs=256, code_bytes=1, mode=1, unit_w=False),
                [("h2o_hist_bm", 128, 129, 100, 0, 256, 1125899906842624.0, 281474976710656.0, 2, 1, 0, -1, 32, 2, 0,
                  "pppppp...p.")]),
    "bm_1x16": (dict(F=13, Fp=16, Bs=256, code_bytes=1, mode=2, unit_w=False),
                [("h2o_hist_bm", 16, 245, 13, 0, 256, 2251799813685248.0, 562949953421312.0, 2, 2, 0, -1, 16, 2, 0,
                  "pppppp...p.")]),
    "wide_packed": (dict(F=100, Fp=200, Bs=1024, code_bytes=2, mode=0, unit_w=True),
                    [("h2o_hist_build_pk", 2, 200, 75, 100, 15, 1024, 16777216.0, 58720256, 2, 256, 0,
                      "ppp.pp...")]),
    "wide_flat": (dict(F=100, Fp=200, Bs=1024, code_bytes=2, mode=1, unit_w=False),
                  [("h2o_hist_build", 2, 200, 27, 100, 5, 1024, 140737488355328.0, 35184372088832.0, 2, 1, 512, 0,
                    "pppppp...")]),
    "quad3_3x36": (dict(_A, env={"H2O3_HIST_BM": "0"}),
                   [_QUAD_3X36 + (1, "ppp.pp....")]),
    # one 2^25-row segment in two target blocks: chunk 2^25 >= 2^23, so the packed
    # path falls back to two channels (4 x 32) and keeps the chunk of the 2-group plan
    "packed_fallback": (dict(_A, counts=(1 << 25,), target_blocks=2),
                        [("h2o_hist_bm", 128, 1, 100, 0, 256, 137438953472.0, 34359738368.0, 1, 0, 0, -1, 32, 2, 0,
                          "ppp.pp...p.")]),
    "need_mask": (dict(_A, need_mask=True), [_BM_2X64 + ("ppp.pp.p.p.",)]),
    "bm_ragged_1": (dict(_A, env={"H2O3_HIST_BM_RAGGED": "1"}), [_BM_2X64_G + (2, 1, "ppp.pp...p.")]),
    # the codes-per-lane switches reach the library as the `lw` argument of the call itself
    "bm_lw_1": (dict(_A, env={"H2O3_HIST_BM_LW": "1"}), [_BM_2X64_G + (1, 0, "ppp.pp...p.")]),
    "quad_lw_2": (dict(_A, env={"H2O3_HIST_BM": "0", "H2O3_HIST_LW": "2"}), [_QUAD_3X36 + (2, "ppp.pp....")]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hist_dispatch(monkeypatch, name):
    kw, expected = CASES[name]
    assert _run(monkeypatch, **kw) == expected
