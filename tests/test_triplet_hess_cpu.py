"""CPU-only checks of the sampled objective's second-order route (include/mfcd.h: mfcd_triplet_rows; mfcd/newton.py;
structure.refit_newton): the numpy model of tests/newton_model.py, which the GPU tests take as their reference, is
consistent with itself (product against differences of the gradient, symmetry, the Gauss-Newton form, the diagonal), its
fit certifies the four fit cases within the GPU test's max_iter, the row model agrees with the plain one, and the
entries are declared, bound and refuse every limit before the device is touched."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import newton_model as NM
from conftest import ROOT


def lib():
    from mfcd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def small(n=9, m=7, d=3, N=120, seed=5):
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    u, i, j = rng.integers(0, n, N), rng.integers(0, m, N), rng.integers(0, m, N)
    j[:3] = i[:3]                                                 # comparisons of an item with itself
    z = rng.integers(0, 5, N) / 4.0
    return U, V, u, i, j, z


def flat(a, b):
    return np.concatenate((a.ravel(), b.ravel()))


def test_model_product_is_the_derivative_of_the_model_gradient():
    U, V, u, i, j, z = small()
    rng = np.random.default_rng(6)
    P, Q = rng.standard_normal(U.shape), rng.standard_normal(V.shape)
    l2, h = 0.7, 1e-5
    up = NM.gradient(U + h * P, V + h * Q, u, i, j, z, l2)
    dn = NM.gradient(U - h * P, V - h * Q, u, i, j, z, l2)
    fd = flat((up[1] - dn[1]) / (2 * h), (up[2] - dn[2]) / (2 * h))
    hp = flat(*NM.hvp(U, V, u, i, j, z, P, Q, l2))
    assert np.abs(fd - hp).max() <= 1e-6 * np.abs(hp).max()
    # and the gradient is the derivative of F
    at = NM.gradient(U, V, u, i, j, z, l2)
    dF = (up[0] - dn[0]) / (2 * h)
    assert abs(dF - flat(at[1], at[2]) @ flat(P, Q)) <= 1e-6 * abs(dF)


def test_model_product_is_symmetric_and_gauss_newton_is_positive():
    U, V, u, i, j, z = small()
    rng = np.random.default_rng(7)
    a, b = (rng.standard_normal(U.shape), rng.standard_normal(V.shape)), (rng.standard_normal(U.shape), rng.standard_normal(V.shape))
    for gn in (False, True):
        Ha, Hb = flat(*NM.hvp(U, V, u, i, j, z, *a, 0.3, gn)), flat(*NM.hvp(U, V, u, i, j, z, *b, 0.3, gn))
        lhs, rhs = flat(*a) @ Hb, flat(*b) @ Ha
        assert abs(lhs - rhs) <= 1e-12 * np.abs(flat(*a)) @ np.abs(Hb), gn
    for seed in range(20):
        rng = np.random.default_rng(seed)
        q = (rng.standard_normal(U.shape), rng.standard_normal(V.shape))
        assert flat(*q) @ flat(*NM.hvp(U, V, u, i, j, z, *q, 1e-9, True)) >= 0.0


def test_model_diagonal_is_the_diagonal_of_the_gauss_newton_blocks():
    """D_U and D_V against e . H e over unit vectors: the own block holds no r_t term, so exact and Gauss-Newton agree."""
    U, V, u, i, j, z = small(4, 3, 2, 30, 8)
    _, _, _, DU, DV = NM.gradient(U, V, u, i, j, z, 0.25)
    for gn in (False, True):
        for r in range(U.shape[0]):
            for c in range(U.shape[1]):
                P, Q = np.zeros_like(U), np.zeros_like(V)
                P[r, c] = 1.0
                assert abs(NM.hvp(U, V, u, i, j, z, P, Q, 0.25, gn)[0][r, c] - DU[r, c]) <= 1e-13 * DU[r, c]
        for k in range(V.shape[0]):
            for c in range(V.shape[1]):
                P, Q = np.zeros_like(U), np.zeros_like(V)
                Q[k, c] = 1.0
                assert abs(NM.hvp(U, V, u, i, j, z, P, Q, 0.25, gn)[1][k, c] - DV[k, c]) <= 1e-13 * DV[k, c]


def test_row_model_agrees_with_the_plain_model():
    U, V, u, i, j, z = small()
    n, m = U.shape[0], V.shape[0]
    rng = np.random.default_rng(9)
    P, Q = rng.standard_normal(U.shape), rng.standard_normal(V.shape)
    l2 = 0.4
    by_user, by_item = NM.group_by_user(u, i, j, z, n), NM.group_by_item(u, i, j, z, m)
    assert len(by_item[0]) == 2 * len(u) and by_item[1][-1] == 2 * len(u)
    F, gU, gV, DU, DV = NM.gradient(U, V, u, i, j, z, l2)
    ru, ri = NM.rows_pass(0, 0, 0, U, V, None, None, *by_user, None, l2), NM.rows_pass(1, 0, 0, U, V, None, None, *by_item, None, l2)
    for got, want in ((ru.out, gU), (ri.out, gV), (ru.diag, DU), (ri.diag, DV)):
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert abs(ru.loss.sum() + 0.5 * l2 * ((U * U).sum() + (V * V).sum()) - F) <= 1e-13 * F
    for gn in (0, 1):
        HU, HV = NM.hvp(U, V, u, i, j, z, P, Q, l2, gn)
        hu = NM.rows_pass(0, 1, gn, U, V, P, Q, *by_user, None, l2)
        hi = NM.rows_pass(1, 1, gn, U, V, P, Q, *by_item, None, l2)
        assert np.abs(hu.out - HU).max() <= 1e-13 * np.abs(HU).max() and np.abs(hi.out - HV).max() <= 1e-13 * np.abs(HV).max()
        assert (hu.abs_out >= np.abs(hu.out) * (1 - 1e-15)).all() and (hi.abs_out >= np.abs(hi.out) * (1 - 1e-15)).all()


@pytest.mark.parametrize("case", NM.FIT_CASES, ids=lambda c: "n%d-m%d-d%d-N%d-l2_%g" % c)
def test_model_fit_certifies_the_fit_cases(case):
    n, m, d, N, l2 = case
    U0, V0, u, i, j, z = NM.make_fit_case(n, m, d, N)
    res = NM.fit(U0, V0, u, i, j, z, l2, max_iter=100)
    print(f"outer iterations {len(res.history)}, Hessian products {res.products}, F {res.history[-1]!r}")
    assert res.status == 0 and len(res.history) <= 100
    assert (np.diff(res.history) <= 0).all()
    assert res.grad_inf[-1] <= NM.GTOL * l2 * max(np.abs(res.U).max(), np.abs(res.V).max())
    assert res.products == res.cg_iters.sum() + len(res.cg_iters)


def test_segment_rows():
    from mfcd import newton
    S = lib().mfcd_triplet_rows_segment()
    assert S == 256
    lengths = np.array([0, 1, S - 1, S, S + 1, 2 * S + 3, 0])
    off = np.concatenate(([0], np.cumsum(lengths)))
    seg_off, n_seg = newton.segment_rows(torch.from_numpy(off))
    assert seg_off.dtype == torch.int64 and seg_off.tolist() == [0, 0, 1, 2, 3, 5, 8, 8] and n_seg == 8
    ref = NM.segment_rows(off, S)
    assert ref[0].tolist() == seg_off.tolist() and ref[1] == n_seg
    seg_off, n_seg = newton.segment_rows(torch.zeros(1, dtype=torch.int64))
    assert seg_off.tolist() == [0] and n_seg == 0


def test_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_triplet_rows_segment", 0), ("mfcd_triplet_rows_workspace_bytes", 3), ("mfcd_triplet_rows", 24)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t)\s+%s\(([^)]*)\);" % name, header, re.M | re.S).group(1)
        assert (0 if decl.strip() == "void" else len(decl.split(","))) == nargs, name
    L = lib()
    assert L.mfcd_abi_version() == 4
    size = L.mfcd_triplet_rows_workspace_bytes
    for rows, d, n_seg in ((4, 0, 1), (4, 257, 1), (-1, 8, 1), (4, 8, -1), (4, 8, (1 << 31) + 1)):
        assert size(rows, d, n_seg) == 0, (rows, d, n_seg)
    for rows, d, n_seg in ((0, 1, 0), (9, 65, 1), (9, 256, 33), (1 << 30, 128, 1 << 31)):
        assert size(rows, d, n_seg) > 0 and size(rows, d, n_seg) % 256 == 0, (rows, d, n_seg)
    assert size(4, 100, 1000) >= 256 + (2 * 100 + 1) * 8 * 1000 + 4 * 1000 and size(4, 100, 2000) > size(4, 100, 1000)


def test_entry_limits_are_refused_before_the_device():
    L = lib()
    A = 1 << 24                                  # non-null addresses that are never dereferenced: every call is refused
    base = dict(side=0, pas=1, gn=0, U=A, n=53, V=2 * A, m=97, d=100, P=3 * A, Q=4 * A, records=5 * A, row_off=6 * A,
                row_id=7 * A, rows=4, seg_off=8 * A, n_seg=6, l2=1.0, out=9 * A, diag=10 * A, loss=11 * A, status=12 * A,
                ws=13 * A, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        return L.mfcd_triplet_rows(a["side"], a["pas"], a["gn"], a["U"], a["n"], a["V"], a["m"], a["d"], a["P"], a["Q"],
                                   a["records"], a["row_off"], a["row_id"], a["rows"], a["seg_off"], a["n_seg"], a["l2"],
                                   a["out"], a["diag"], a["loss"], a["status"], a["ws"], a["ws_bytes"], None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(d=0), dict(d=257), dict(n=0), dict(m=0), dict(rows=-1), dict(n_seg=-1), dict(side=2), dict(side=-1),
                dict(pas=2), dict(pas=-1), dict(gn=2), dict(gn=-1), dict(U=None), dict(V=None), dict(row_off=None),
                dict(seg_off=None), dict(out=None), dict(status=None), dict(records=None), dict(P=None), dict(Q=None),
                dict(l2=0.0), dict(l2=-1.0), dict(l2=inf), dict(l2=nan),
                dict(out=A), dict(out=2 * A), dict(out=3 * A), dict(out=4 * A), dict(out=A + 16), dict(out=2 * A + 64),
                dict(out=3 * A + 8), dict(out=4 * A - 8), dict(pas=0, diag=A), dict(pas=0, diag=2 * A + 8),
                dict(pas=0, loss=A + 8), dict(pas=0, side=1, row_id=None, rows=98), dict(row_id=None, rows=54), dict(ws=None)):
        assert call(**bad) == -1, bad
    assert call(rows=0, l2=0.0) == -1 and call(rows=0, d=257) == -1 and call(rows=0, out=A) == -1    # refused all the same
    assert call(ws_bytes=16) == -2
    assert call(ws_bytes=L.mfcd_triplet_rows_workspace_bytes(4, 100, 6) - 1) == -2
    assert call(pas=0, side=1, ws_bytes=L.mfcd_triplet_rows_workspace_bytes(4, 100, 6) - 1) == -2
    assert call(rows=0) == 0 and call(rows=0, ws=None, ws_bytes=0) == 0
    assert call(rows=0, pas=0, P=None, Q=None, diag=None, loss=None, row_id=None) == 0
    assert call(rows=0, n_seg=0, records=None) == 0 and call(rows=0, d=256, n=1, m=1, l2=1e-300, gn=1, side=1) == 0
    assert call(rows=0, pas=1, diag=A, loss=A) == 0                  # diag and loss are ignored in pass 1


def test_there_is_no_cpu_form_and_the_public_signatures():
    import structure as S
    from mfcd import _lib, newton
    U, V, u, i, j, z = small()
    Ut, Vt = torch.from_numpy(U), torch.from_numpy(V)
    data = tuple(torch.from_numpy(a) for a in (u, i, j, z))
    with pytest.raises(_lib.MfcdError):
        newton.fit_newton(Ut.float(), Vt.float(), *data, 1.0)
    rows = newton.Rows(torch.zeros((0, 4), dtype=torch.int32), torch.zeros(10, dtype=torch.int64), torch.zeros(10, dtype=torch.int64), 0)
    with pytest.raises(_lib.MfcdError):
        newton.triplet_rows(0, 0, Ut, Vt, rows, 1.0)
    with pytest.raises(_lib.MfcdError):
        newton.triplet_pass(Ut, Vt, rows, rows, 1.0)
    with pytest.raises(_lib.MfcdError):
        newton.triplet_hvp(Ut, Vt, rows, rows, Ut, Vt, 1.0)
    model = S.MatrixFactorization(U.shape[0], V.shape[0], U.shape[1])
    with pytest.raises(RuntimeError):
        S.refit_newton(model, data, 1e-5)
    assert list(inspect.signature(S.refit_newton).parameters) == ["model", "train_loader", "weight_decay", "max_iter"]
    assert inspect.signature(S.refit_newton).parameters["max_iter"].default == 100
    assert S.refit_newton.__doc__.startswith("Extension (not in the reference)") and "Not part of the result dict" in S.refit_newton.__doc__
    sig = inspect.signature(newton.fit_newton).parameters
    assert list(sig) == ["U", "V", "u", "i", "j", "z", "l2", "max_iter", "gtol", "cg_cap"]
    assert sig["max_iter"].default == 100 and sig["gtol"].default == 2.0 ** -26 and sig["cg_cap"].default is None
    assert list(inspect.signature(newton.segment_rows).parameters) == ["row_off"]
    assert list(inspect.signature(newton.triplet_pass).parameters) == ["U", "V", "by_user", "by_item", "l2"]
    sig = inspect.signature(newton.triplet_hvp).parameters
    assert list(sig) == ["U", "V", "by_user", "by_item", "P", "Q", "l2", "gauss_newton"] and sig["gauss_newton"].default is False
    assert newton.NewtonResult._fields == ("U", "V", "history", "grad_inf", "cg_iters", "products", "status")
