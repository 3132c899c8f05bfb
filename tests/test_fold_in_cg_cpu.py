"""CPU-only checks of the Newton-CG form of the two exact block steps (include/mfcd.h: mfcd_fold_in_users_cg,
mfcd_item_step_cg; mfcd/foldin.py: the `method` of fold_in_users, fold_in_items_cg): the entries are declared and bound,
every limit is refused before the device is touched, there is no CPU form, and the numpy model of
tests/foldin_cg_model.py certifies every row of exactly the inputs of the GPU tests (tests/test_fold_in_cg.py,
tests/test_item_step_cg.py) and lies within the parity bound of the Cholesky models, which are the reference there."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import foldin_cg_model as CG
import foldin_model as FM
import itemstep_model as IM
from conftest import ROOT

U_TOL = 2.0 ** -22


def lib():
    from mfcd import _lib
    return _lib.load()


def test_cg_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_fold_in_cg_max_d", 0), ("mfcd_fold_in_cg_chunk", 1), ("mfcd_fold_in_cg_resident", 1),
                        ("mfcd_fold_in_cg_workspace_bytes", 3), ("mfcd_fold_in_users_cg", 17),
                        ("mfcd_item_step_cg_workspace_bytes", 3), ("mfcd_item_step_cg", 20)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t)\s+%s\(([^)]*)\);" % name, header, re.M | re.S).group(1)
        assert (0 if decl.strip() == "void" else len(decl.split(","))) == nargs, name
    assert "Out of scope: d > 64" not in header
    L = lib()
    assert L.mfcd_fold_in_cg_max_d() == 256
    for d in (1, 64, 65, 128, 256):
        C, R = L.mfcd_fold_in_cg_chunk(d), L.mfcd_fold_in_cg_resident(d)
        assert 2 <= C <= R, (d, C, R)                                    # a streamed row's chunk fits the resident stage
    for d in (-1, 0, 257, 1 << 20):
        assert L.mfcd_fold_in_cg_chunk(d) == 0 and L.mfcd_fold_in_cg_resident(d) == 0, d
    for size in (L.mfcd_fold_in_cg_workspace_bytes, L.mfcd_item_step_cg_workspace_bytes):
        for rows, d, records in ((4, 0, 1), (4, 257, 1), (-1, 8, 1), (4, 8, -1)):
            assert size(rows, d, records) == 0, (rows, d, records)
        for rows, d, records in ((0, 1, 0), (9, 65, 1), (9, 256, 33), (1 << 30, 128, 1 << 40)):
            assert size(rows, d, records) > 0 and size(rows, d, records) % 256 == 0, (rows, d, records)
        assert size(4, 128, 1000) >= 256 + 24 * 1000 and size(4, 128, 2000) > size(4, 128, 1000)


def test_user_entry_limits_are_refused_before_the_device():
    L = lib()
    P = 1 << 20                                  # non-null addresses that are never dereferenced: every call is refused
    base = dict(V=P, m=97, d=128, records=2 * P, row_off=3 * P, rows=4, l2=1.0, U_init=4 * P, max_iter=50, gtol=2.0 ** -26,
                U_out=5 * P, objective=6 * P, info=7 * P, cg=10 * P, ws=8 * P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        return L.mfcd_fold_in_users_cg(a["V"], a["m"], a["d"], a["records"], a["row_off"], a["rows"], a["l2"], a["U_init"],
                                       a["max_iter"], a["gtol"], a["U_out"], a["objective"], a["info"], a["cg"], a["ws"],
                                       a["ws_bytes"], None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(d=0), dict(d=257), dict(m=0), dict(rows=-1), dict(V=None), dict(row_off=None), dict(U_out=None),
                dict(info=None), dict(l2=0.0), dict(l2=-1.0), dict(l2=inf), dict(l2=nan), dict(max_iter=0),
                dict(max_iter=1001), dict(gtol=-1e-30), dict(gtol=inf), dict(gtol=nan),
                dict(U_out=P), dict(U_out=4 * P), dict(U_out=P + 16), dict(U_out=4 * P + 64), dict(ws=None)):
        assert call(**bad) == -1, bad
    assert call(rows=0, l2=0.0) == -1 and call(rows=0, d=257) == -1 and call(rows=0, U_out=P) == -1    # refused all the same
    assert call(ws_bytes=16) == -2
    assert call(ws_bytes=L.mfcd_fold_in_cg_workspace_bytes(4, 128, 0) - 1) == -2
    assert call(rows=0) == 0 and call(rows=0, ws=None, ws_bytes=0) == 0
    assert call(rows=0, U_init=None, objective=None, records=None, cg=None) == 0
    assert call(rows=0, max_iter=1, gtol=0.0, l2=1e-300, d=256, m=1) == 0 and call(rows=0, max_iter=1000, d=1) == 0


def test_item_entry_limits_are_refused_before_the_device():
    L = lib()
    P = 1 << 20
    base = dict(U=P, n=53, V=2 * P, m=97, d=128, records=3 * P, row_off=4 * P, row_item=5 * P, rows=4, l2=1.0, theta=0.5,
                max_iter=50, gtol=2.0 ** -26, V_out=6 * P, objective=7 * P, info=8 * P, cg=10 * P, ws=9 * P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        return L.mfcd_item_step_cg(a["U"], a["n"], a["V"], a["m"], a["d"], a["records"], a["row_off"], a["row_item"],
                                   a["rows"], a["l2"], a["theta"], a["max_iter"], a["gtol"], a["V_out"], a["objective"],
                                   a["info"], a["cg"], a["ws"], a["ws_bytes"], None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(d=0), dict(d=257), dict(n=0), dict(m=0), dict(rows=-1), dict(U=None), dict(V=None), dict(row_off=None),
                dict(V_out=None), dict(info=None), dict(l2=0.0), dict(l2=-1.0), dict(l2=inf), dict(l2=nan),
                dict(theta=0.0), dict(theta=-0.5), dict(theta=1.0 + 2.0 ** -52), dict(theta=inf), dict(theta=nan),
                dict(max_iter=0), dict(max_iter=1001), dict(gtol=-1e-30), dict(gtol=inf), dict(gtol=nan),
                dict(V_out=P), dict(V_out=2 * P), dict(V_out=P + 16), dict(V_out=2 * P + 64), dict(V_out=P - 64), dict(ws=None),
                dict(row_item=None, rows=98), dict(row_item=None, rows=4, m=3)):
        assert call(**bad) == -1, bad
    assert call(rows=0, l2=0.0) == -1 and call(rows=0, d=257) == -1 and call(rows=0, V_out=P) == -1
    assert call(ws_bytes=16) == -2
    assert call(ws_bytes=L.mfcd_item_step_cg_workspace_bytes(4, 128, 0) - 1) == -2
    assert call(rows=0) == 0 and call(rows=0, ws=None, ws_bytes=0) == 0
    assert call(rows=0, row_item=None, objective=None, records=None, cg=None) == 0
    assert call(rows=0, max_iter=1, gtol=0.0, l2=1e-300, d=256, m=1, n=1, theta=1.0) == 0


def test_there_is_no_cpu_form_and_the_method_is_checked():
    from mfcd import _lib, foldin
    V, rec, off, _ = FM.make_case(2, "hard", [3, 0, 5], seed=1)
    Vt, rt, ot = torch.from_numpy(V), torch.from_numpy(rec), torch.from_numpy(off)
    with pytest.raises(_lib.MfcdError):
        foldin.fold_in_users(Vt, rt, ot, 1.0, method="cg")
    U, Vi, irec, ioff, items = IM.make_case(2, "hard", [3, 0, 5, 1, 1, 1, 1, 1, 1], seed=1)
    with pytest.raises(_lib.MfcdError):
        foldin.fold_in_items_cg(*(torch.from_numpy(a) for a in (U, Vi, irec, ioff)), 1.0, torch.from_numpy(items))
    L = lib()
    with pytest.raises(ValueError):
        foldin.fold_in_users(Vt, rt, ot, 1.0, method="nonsense")
    with pytest.raises(ValueError):
        foldin._use_cg(L, 8, "nonsense", "the fold-in kernel")
    assert [foldin._use_cg(L, d, "auto", "x") for d in (1, 64, 65, 256)] == [False, False, True, True]
    assert foldin._use_cg(L, 16, "cg", "x") and not foldin._use_cg(L, 16, "cholesky", "x")
    for d, method in ((0, "auto"), (257, "auto"), (257, "cg"), (65, "cholesky")):
        with pytest.raises(_lib.MfcdError, match=r"range \[1, (64|256)\]"):
            foldin._use_cg(L, d, method, "the fold-in kernel")
    assert foldin.FoldInResult(1, 2, 3, 4).cg_iters is None and foldin.ItemStepResult(1, 2, 3, 4, 5).cg_iters is None


@functools.lru_cache(maxsize=None)
def capacity(d):
    L = lib()
    return L.mfcd_fold_in_cg_chunk(d), L.mfcd_fold_in_cg_resident(d)


@pytest.mark.parametrize("start", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("labels", FM.LABELS)
@pytest.mark.parametrize("d", CG.DS)
def test_model_certifies_the_gpu_tests_inputs_within_the_parity_bound(d, labels, start):
    """Both sides and both l2 on the inputs of one (d, labels, start): the Cholesky models with max_iter = 1000 report
    status 0 on every row (they are the GPU tests' reference), the CG model reports status 0 with the device's
    max_iter, and the two minimisers differ by at most 2^-22 of the scale the GPU tests use."""
    C, R = capacity(d)
    V, rec, off, U0 = CG.user_case(d, labels, start, C, R)
    U, Vi, irec, ioff, items = CG.item_case(d, labels, start, C, R)
    assert (np.diff(off) == CG.row_lengths(C, R)).all() and (np.diff(ioff) == CG.row_lengths(C, R)).all()
    worst = 0.0
    for l2 in CG.L2S:
        ref = FM.solve(V, rec, off, l2, U0, max_iter=CG.MODEL_MAX_ITER)
        got = CG.solve_users(V, rec, off, l2, U0, max_iter=CG.DEVICE_MAX_ITER)
        for r, (a, b) in enumerate(zip(ref, got)):
            assert a.status == FM.CONVERGED and b.status == FM.CONVERGED, ("user", l2, r, a.status, b.status)
            scale = np.abs(a.u).max()
            assert np.abs(a.u - b.u).max() <= U_TOL * scale, ("user", l2, r)
            assert abs(a.objective - b.objective) <= 1e-9 * max(1.0, a.objective)
            if scale > 0:
                worst = max(worst, np.abs(a.u - b.u).max() / (U_TOL * scale))
        ref = IM.solve(U, Vi, irec, ioff, l2, items, max_iter=CG.MODEL_MAX_ITER)
        got = CG.solve_items(U, Vi, irec, ioff, l2, items, max_iter=CG.DEVICE_MAX_ITER)
        for r, (a, b) in enumerate(zip(ref, got)):
            assert a.status == FM.CONVERGED and b.status == FM.CONVERGED, ("item", l2, r, a.status, b.status)
            scale = max(np.abs(a.v_star).max(), np.abs(Vi[items[r]]).max())
            assert np.abs(a.v_star - b.u).max() <= U_TOL * scale, ("item", l2, r)
            assert abs(a.f_start - b.f_start) <= 1e-9 * max(1.0, a.f_start)
            assert abs(a.objective - b.objective) <= 1e-9 * max(1.0, a.objective)
            if scale > 0:
                worst = max(worst, np.abs(a.v_star - b.u).max() / (U_TOL * scale))
    print(f"worst share of the parity bound: {worst:.4f}")


def test_model_status_paths():
    d, l2 = 65, 1e-3
    V, rec, off, U0 = FM.make_case(d, "hard", [40, 0, 25], seed=9, start=True)
    z = rec[:, 3].copy().view(np.float32)
    full = CG.solve_users(V, rec, off, l2, U0)
    assert [r.status for r in full] == [0, 0, 0] and full[0].iters > 1 and full[0].cg_iters >= full[0].iters
    assert full[1].iters == 0 and full[1].cg_iters == 0 and not full[1].u.any()
    # status 1: the cap on CG solves; the iterate is the last accepted one and lowers f
    one = CG.solve_user_row(V, rec[:40, 1], rec[:40, 2], z[:40], l2, U0[0], max_iter=1)
    assert one.status == FM.STOPPED and one.iters == 1 and one.objective < one.f_start
    # a certified start takes no solve: the f64 solution itself, and the start 0 of a row whose minimiser is 0
    again = CG.solve_problem(FM.deltas(V, rec[:40, 1], rec[:40, 2]), np.zeros(40), z[:40].astype(np.float64), l2, full[0].u)
    assert again.status == FM.CONVERGED and again.iters == 0 and again.cg_iters == 0
    half = np.array([0.5], dtype=np.float32)
    at0 = CG.solve_user_row(V, rec[:1, 1], rec[:1, 2], half, l2)
    assert at0.status == FM.CONVERGED and at0.iters == 0 and not at0.u.any() and at0.objective == np.log(2.0)
    away = CG.solve_user_row(V, rec[:1, 1], rec[:1, 2], half, l2, U0[0])       # |u|_inf shrinks with |g|_2: never certified
    assert away.status == FM.STOPPED and away.iters == 50
    # status 2
    bad = rec[:40].copy()
    bad[3, 1] = FM.M_ITEMS
    row = CG.solve_user_row(V, bad[:, 1], bad[:, 2], z[:40], l2, U0[0])
    assert row.status == FM.INVALID and row.iters == 0 and np.isnan(row.u).all() and np.isnan(row.objective)
    # the fp32 rounding of a solution, fed back, is certified within 2 solves
    u32 = full[0].u.astype(np.float32)
    back = CG.solve_user_row(V, rec[:40, 1], rec[:40, 2], z[:40], l2, u32)
    assert back.status == FM.CONVERGED and back.iters <= 2
