"""split_kernel, split_select_kernel and split_select2_kernel
(ops/csrc/tree_split.hip) against the exact per-threshold oracle of
split_common.py, through the C entry points; the numeric path of
cat_pair_kernel as a second implementation of the same rule; and the Python
plumbing of TreeGrower._find_splits_native.

Tolerances.  t, opt, feat, mask, ok and feat_out are compared with equality
(the oracle proves, case by case, that every comparison of the rule is
decided by identical operands or a 1e-9 margin above the rounding bound).
Sums of the integer family are compared with tolerance zero.  Gains and the
sums of the float family use the first-order bound derived in
split_common's docstring: each sum over a column of B bins carries at most
e = B 2^-53 sum|terms|, scores are propagated with 2e (a right child is a
difference of two sums), the gain bound is doubled and gets 4 ulps of
|sL| + |sR| + |sT|, and all of it is capped by 1e-9 (1 + |reference|).

A record whose gain is -inf carries no other defined field (the kernel leaves
whatever candidate the threshold or the bound veto rejected), so only its
gain, the node totals and split_select2's ok / feat_out / all-ones mask are
compared there.

What these tests found.  Before the in-lane tie fix the case
tie_opt0_later_chunk came back as opt 1, t 3 (tie_three_chunks: opt 1, t 5)
where the rule gives opt 0, t 67 (opt 0, t 197).  The float family found a
second one: a threshold on an empty bin repeats the partition of the
threshold below it, and both kernels (split_kernel, cat_pair_kernel's numeric
path) let the rounding of their parallel prefix sums pick between the two, so
12 float cases came back with t one to three empty bins too high; the
searches now skip the repeated threshold."""
import numpy as np
import pytest
import torch

import split_common as sc

pytestmark = pytest.mark.gpu

ALL = sorted(sc.CASES)
REC = np.dtype([("gain", "<f8"), ("lw", "<f8"), ("ly", "<f8"), ("t", "<i4"), ("opt", "<i4")])
NINF = -np.inf


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from h2o3_amd.ops import _native
    lib = _native.get_lib("tree_split")
    assert lib is not None, "libtree_split.so not loaded"
    return lib, _native.ptr, _native.stream


def _dev(a):
    return torch.as_tensor(np.array(a, copy=True)).cuda()


def _find(case, how):
    """Per-(node, feature) records [n][Fl]; how: 'b' (h2o_split_find_b with the
    case's bounds or a null pointer), 'plain' (h2o_split_find), 'inf' (infinite bounds)."""
    lib, ptr, stream = _lib()
    Fl, n, Bs, _ = case.H.shape
    H, wyy, ok = _dev(case.H), _dev(case.wyy), _dev(case.ok)
    mono = None if case.mono is None else _dev(case.mono)
    out = torch.full((n * Fl, 4), sc.SENTINEL, dtype=torch.float64, device="cuda")
    args = (ptr(H), Fl, n, Bs, ptr(wyy), ptr(ok), ptr(mono), case.min_rows, case.msi, case.lam, case.alpha,
            case.gamma, case.crit, ptr(out))
    if how == "plain":
        rc = lib.h2o_split_find(*args, stream())
    else:
        bnd = None
        if how == "inf":
            bnd = _dev(np.tile([-np.inf, np.inf], (n, 1)))
        elif case.bnd is not None:
            bnd = _dev(case.bnd)
        rc = lib.h2o_split_find_b(*args, ptr(bnd), case.use_bounds, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, out.cpu().numpy().view(REC).reshape(n, Fl), H


def _check_sum(case, col, got, ref, what):
    tol = sc.sum_tol(case, col, ref)
    print(f"{what}: got {got!r} ref {float(ref)!r} tol {tol:.3e}")
    assert abs(got - float(ref)) <= tol, what


@pytest.mark.parametrize("name", ALL)
def test_split_find_records(name):
    """Every eligible (node, feature) record, not only the node winners."""
    case, res = sc.CASES[name], sc.oracle(name)
    _, rec, _ = _find(case, "b")
    Fl, n = case.H.shape[:2]
    bad = []
    for i in range(n):
        for f in range(Fl):
            col, r = res.cols[i][f], rec[i, f]
            if col.gain is None:
                if r["gain"] != NINF:
                    bad.append((i, f, "gain", float(r["gain"]), None))
                continue
            if (int(r["t"]), int(r["opt"])) != (col.t, col.opt):
                bad.append((i, f, "t/opt", (int(r["t"]), int(r["opt"])), (col.t, col.opt)))
            if not abs(r["gain"] - float(col.gain)) <= col.gtol:
                bad.append((i, f, "gain", float(r["gain"]), float(col.gain), col.gtol))
            for key, ref in (("lw", col.L[0]), ("ly", col.L[1])):
                if not abs(r[key] - float(ref)) <= sc.sum_tol(case, col, ref):
                    bad.append((i, f, key, float(r[key]), float(ref)))
    print(name, "mismatches (node, feature, field, got, expected):", bad)
    assert not bad
    if case.bnd is None:
        # the older entry point and infinite bounds are the same search
        assert np.array_equal(_find(case, "plain")[1].view(np.uint8), rec.view(np.uint8))
        assert np.array_equal(_find(case, "inf")[1].view(np.uint8), rec.view(np.uint8))


def _check_record(case, nd, row, what):
    """Fields 0..9 of a node that splits."""
    assert abs(row[0] - float(nd.gain)) <= nd.gtol, (what, row[0], float(nd.gain), nd.gtol)
    assert (row[1], row[2], row[3]) == (nd.feat, nd.t, nd.opt), (what, row[1:4], (nd.feat, nd.t, nd.opt))
    for j, ref in ((4, nd.L[0]), (5, nd.L[1]), (6, nd.R[0]), (7, nd.R[1]), (8, nd.T[0]), (9, nd.T[1])):
        _check_sum(case, nd, row[j], ref, f"{what} field {j}")


@pytest.mark.parametrize("name", ALL)
def test_split_select(name):
    """split_select_kernel: fields 0..9 and the go-left mask."""
    lib, ptr, stream = _lib()
    case, res = sc.CASES[name], sc.oracle(name)
    Fl, n, Bs, _ = case.H.shape
    out, rec, H = _find(case, "b")
    pk = torch.full((n * 10 + 4,), sc.SENTINEL, dtype=torch.float64, device="cuda")
    mask = torch.full((n * Bs + 8,), 7, dtype=torch.uint8, device="cuda")
    assert lib.h2o_split_select(ptr(out), ptr(H), Fl, n, Bs, case.f0, ptr(pk), ptr(mask), stream()) == 0
    torch.cuda.synchronize()
    pk, mask = pk.cpu().numpy(), mask.cpu().numpy()
    assert np.all(pk[n * 10:] == sc.SENTINEL) and np.all(mask[n * Bs:] == 7)
    pk, mask = pk[:n * 10].reshape(n, 10), mask[:n * Bs].reshape(n, Bs)
    for i, nd in enumerate(res.nodes):
        what = f"{name} node {i}"
        if nd.gain is not None:
            _check_record(case, nd, pk[i], what)
            assert np.array_equal(mask[i], nd.mask), what
            continue
        # no finite gain: -inf, the first feature, the node totals; the rest is feature 0's own record
        assert pk[i, 0] == NINF and pk[i, 1] == case.f0, what
        for j in (8, 9):
            _check_sum(case, nd, pk[i, j], nd.T[j - 8], f"{what} field {j}")
        r = rec[i, 0]
        assert (pk[i, 2], pk[i, 3], pk[i, 4], pk[i, 5]) == (r["t"], r["opt"], r["lw"], r["ly"]), what
        assert pk[i, 6] == pk[i, 8] - pk[i, 4] and pk[i, 7] == pk[i, 9] - pk[i, 5], what
        assert np.array_equal(mask[i], sc._mask(Bs, int(r["opt"]), int(r["t"]))), what


@pytest.mark.parametrize("name", ALL)
def test_split_select2(name):
    """split_select2_kernel: the record, ok, min_w2, the all-ones mask and
    feat_out = 0 of a node that does not split, field 12, and every field it
    must leave alone, at each row stride."""
    lib, ptr, stream = _lib()
    case, res = sc.CASES[name], sc.oracle(name)
    Fl, n, Bs, _ = case.H.shape
    out, rec, H = _find(case, "b")
    for min_w2, stride in case.sel2:
        pk = torch.full((n * stride + 4,), sc.SENTINEL, dtype=torch.float64, device="cuda")
        mask = torch.full((n * Bs + 8,), 7, dtype=torch.uint8, device="cuda")
        feat = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
        assert lib.h2o_split_select2(ptr(out), ptr(H), Fl, n, Bs, case.f0, float(min_w2), stride, ptr(pk), ptr(mask),
                                     ptr(feat), stream()) == 0
        torch.cuda.synchronize()
        pk, mask, feat = pk.cpu().numpy(), mask.cpu().numpy(), feat.cpu().numpy()
        assert np.all(pk[n * stride:] == sc.SENTINEL) and np.all(mask[n * Bs:] == 7) and np.all(feat[n:] == -7)
        pk, mask = pk[:n * stride].reshape(n, stride), mask[:n * Bs].reshape(n, Bs)
        for i, nd in enumerate(res.nodes):
            what = f"{name} node {i} min_w2 {min_w2} stride {stride}"
            ok = sc.select2_ok(case, nd, min_w2)
            assert pk[i, 10] == (1.0 if ok else 0.0), what
            assert pk[i, 11] == sc.SENTINEL and np.all(pk[i, 13:] == sc.SENTINEL), what
            if stride > 12:
                assert pk[i, 12] == nd.naw, (what, pk[i, 12], nd.naw)
            assert feat[i] == (nd.feat if ok else 0), what
            assert np.array_equal(mask[i], nd.mask if ok else np.ones(Bs, dtype=np.uint8)), what
            if nd.gain is not None:
                _check_record(case, nd, pk[i], what)
            else:
                assert pk[i, 0] == NINF and pk[i, 1] == case.f0, what
                for j in (8, 9):
                    _check_sum(case, nd, pk[i, j], nd.T[j - 8], f"{what} field {j}")


@pytest.mark.parametrize("name", sc.PAIR_CASES)
def test_cat_pairs_numeric_path_agrees(name):
    """cat_pair_kernel with pcat = 0 is a second implementation of the numeric
    search (block scan in LDS, one thread per threshold): same k, same gain."""
    lib, ptr, stream = _lib()
    case, res = sc.CASES[name], sc.oracle(name)
    _, n, Bs, _ = case.H.shape
    nodes = [i for i in range(n) if case.ok[i, 0]]
    P = len(nodes)
    H, wyy = _dev(case.H), _dev(case.wyy)
    pf = torch.zeros(P, dtype=torch.int32, device="cuda")
    pn = _dev(np.asarray(nodes, dtype=np.int32))
    pcat = torch.zeros(P, dtype=torch.uint8, device="cuda")
    pmono = _dev(np.full(P, 0.0 if case.mono is None else case.mono[0], dtype=np.float32))
    out = torch.full((P, 2), sc.SENTINEL, dtype=torch.float64, device="cuda")
    assert lib.h2o_cat_pairs(ptr(H), n, Bs, 2, P, ptr(pf), ptr(pn), ptr(pcat), ptr(pmono), ptr(wyy), case.min_rows,
                             case.msi, case.lam, case.alpha, case.gamma, case.crit, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for p, i in enumerate(nodes):
        col = res.cols[i][0]
        print(name, "node", i, "got", out[p], "expected", None if col.gain is None else (float(col.gain), col.k))
        if col.gain is None:
            assert out[p, 0] == NINF, (name, i)
            continue
        assert abs(out[p, 0] - float(col.gain)) <= col.gtol and out[p, 1] == col.k, (name, i)


@pytest.mark.parametrize("want_pk", [False, True])
@pytest.mark.parametrize("name", ["float_B65_n5_F3_se", "bounds_float_xgb", "f0_5_float"])
def test_find_splits_native_plumbing(name, want_pk):
    """The Python around the kernels: column mask, bounds, monotone vector,
    packed (split_select2, stride 13) and unpacked (split_select) records."""
    _lib()
    case, res = sc.CASES[name], sc.oracle(name)
    gr, cm = sc.make_grower(case, "cuda")
    Bs = case.H.shape[2]
    out = gr._find_splits_native(_dev(case.H), cm, _dev(case.wyy), want_pk=want_pk)
    torch.cuda.synchronize()
    assert ("pk" in out) == want_pk
    min_w2 = -1.0 if case.crit == 1 else 2.0 * case.min_rows
    o = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    for i, nd in enumerate(res.nodes):
        what = f"{name} node {i}"
        if nd.gain is None:
            assert o["gain"][i] == NINF, what
            if want_pk:
                assert o["pk"][i, 10] == 0.0 and o["feat_i32"][i] == 0 and np.all(o["mask"][i] == 1), what
            continue
        row = np.concatenate([[o["gain"][i], o["feat"][i], o["t"][i], o["opt"][i]], o["L"][i], o["R"][i], o["tot"][i]])
        _check_record(case, nd, row, what)
        ok = sc.select2_ok(case, nd, min_w2) if want_pk else True
        assert np.array_equal(o["mask"][i], nd.mask if ok else np.ones(Bs, dtype=np.uint8)), what
        if want_pk:
            assert o["pk"].shape[1] == 13 and o["pk"][i, 10] == float(ok) and o["pk"][i, 12] == nd.naw, what
            assert o["feat_i32"][i] == (nd.feat if ok else 0), what
        else:
            assert bool(o["na_left"][i]) == (nd.opt == 1), what
