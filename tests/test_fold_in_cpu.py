"""CPU-only checks of the fold-in entries (include/mfcd.h: mfcd_fold_in_users; mfcd/foldin.py; structure.fit_users,
structure.refit_users): the entries are declared and bound under the unchanged ABI version, every limit is refused
before the device is touched, there is no CPU form of the solve, group_by_user is a stable grouping, and the host model
of tests/foldin_model.py — the reference of the GPU tests — is a minimiser and follows the status rules."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import foldin_model as FM
from conftest import ROOT


def test_fold_in_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_fold_in_max_d", 0), ("mfcd_fold_in_chunk", 0), ("mfcd_fold_in_workspace_bytes", 2),
                        ("mfcd_fold_in_users", 16)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t)\s+%s\(([^)]*)\);" % name, header, re.M | re.S).group(1)
        assert (0 if decl.strip() == "void" else len(decl.split(","))) == nargs, name
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header)) - {"mfcd_sample"}
    assert declared == set(_lib.SIGNATURES)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4
    assert L.mfcd_fold_in_max_d() == 64
    T = L.mfcd_fold_in_chunk()
    assert T >= 2 and len(set(FM.row_lengths(T))) == 9       # the GPU test's row lengths are nine different ones
    size = L.mfcd_fold_in_workspace_bytes
    assert size(0, 1) > 0 and size(4096, 64) > 0 and size(1 << 30, 64) % 256 == 0
    for rows, d in ((4, 0), (4, 65), (-1, 8)):
        assert size(rows, d) == 0, (rows, d)


def test_fold_in_limits_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    P = 1 << 20                                  # non-null addresses that are never dereferenced: every call is refused
    base = dict(V=P, m=97, d=8, records=2 * P, row_off=3 * P, rows=4, l2=1.0, U_init=4 * P, max_iter=50, xtol=2.0 ** -30,
                U_out=5 * P, objective=6 * P, info=7 * P, ws=8 * P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        return L.mfcd_fold_in_users(a["V"], a["m"], a["d"], a["records"], a["row_off"], a["rows"], a["l2"], a["U_init"],
                                    a["max_iter"], a["xtol"], a["U_out"], a["objective"], a["info"], a["ws"],
                                    a["ws_bytes"], None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(d=0), dict(d=65), dict(m=0), dict(rows=-1), dict(V=None), dict(row_off=None), dict(U_out=None),
                dict(info=None), dict(l2=0.0), dict(l2=-1.0), dict(l2=inf), dict(l2=nan), dict(max_iter=0),
                dict(max_iter=1001), dict(xtol=-1e-30), dict(xtol=inf), dict(xtol=nan),
                dict(U_out=P), dict(U_out=4 * P), dict(U_out=P + 16), dict(U_out=4 * P + 64), dict(ws=None)):
        assert call(**bad) == -1, bad
    assert call(rows=0, l2=0.0) == -1 and call(rows=0, d=65) == -1 and call(rows=0, U_out=P) == -1     # refused all the same
    assert call(ws_bytes=16) == -2
    assert call(ws_bytes=L.mfcd_fold_in_workspace_bytes(4, 8) - 1) == -2
    # rows = 0: success with nothing launched, whatever the workspace; the nullable arguments may be absent
    assert call(rows=0) == 0 and call(rows=0, ws=None, ws_bytes=0) == 0
    assert call(rows=0, U_init=None, objective=None, records=None) == 0
    assert call(rows=0, max_iter=1, xtol=0.0, l2=1e-300, d=64, m=1) == 0 and call(rows=0, max_iter=1000, d=1) == 0


def test_there_is_no_cpu_form_of_the_solve():
    import structure as S
    from mfcd import _lib, foldin
    V, rec, off, U0 = FM.make_case(2, "hard", [3, 0, 5], seed=1, start=True)
    Vt, rt, ot = torch.from_numpy(V), torch.from_numpy(rec), torch.from_numpy(off)
    with pytest.raises(_lib.MfcdError):
        foldin.fold_in_users(Vt, rt, ot, 1.0)
    model = S.MatrixFactorization(3, FM.M_ITEMS, 2)
    data = (rt[:, 0], rt[:, 1], rt[:, 2], rt[:, 3].contiguous().view(torch.float32))
    with pytest.raises(RuntimeError):
        S.fit_users(Vt, data, 1.0)
    with pytest.raises(RuntimeError):
        S.fit_users(model, data, 1.0)
    with pytest.raises(RuntimeError):
        S.refit_users(model, data, 1e-5)
    for fn, first in ((S.fit_users, ["V_or_model", "data", "l2", "U_init"]),
                      (S.refit_users, ["model", "train_loader", "weight_decay"])):
        assert list(inspect.signature(fn).parameters) == first
        assert fn.__doc__.startswith("Extension (not in the reference)")
    sig = inspect.signature(foldin.fold_in_users).parameters
    assert sig["max_iter"].default == 50 and sig["xtol"].default == 2.0 ** -30 and sig["U_init"].default is None
    assert foldin.FoldInResult._fields == ("U", "objective", "iters", "status")


def test_group_by_user_is_stable_and_its_offsets_are_right():
    from mfcd import foldin
    rng = np.random.default_rng(5)
    n, N = 9, 200
    u = rng.integers(0, n, N)
    u[(u == 4) | (u == 8)] = 3                                   # users 4 and 8 (the last) have no records
    i, j = rng.integers(0, 50, N), rng.integers(0, 50, N)
    z = rng.random(N).astype(np.float32)
    rec, off = foldin.group_by_user(torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(j), torch.from_numpy(z), n)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (N, 4) and off.dtype == torch.int64
    rec, off = rec.numpy(), off.numpy()
    assert off.tolist() == np.concatenate(([0], np.cumsum(np.bincount(u, minlength=n)))).tolist()
    assert off[4] == off[5] and off[8] == off[9] == N
    for r in range(n):
        mine = np.flatnonzero(u == r)                            # in their original order
        blk = rec[off[r]:off[r + 1]]
        assert (blk[:, 0] == r).all()
        assert blk[:, 1].tolist() == i[mine].tolist() and blk[:, 2].tolist() == j[mine].tolist()
        assert blk[:, 3].copy().view(np.float32).tolist() == z[mine].tolist()
    empty = torch.zeros(0, dtype=torch.int64)
    rec, off = foldin.group_by_user(empty, empty, empty, torch.zeros(0), 3)
    assert tuple(rec.shape) == (0, 4) and off.tolist() == [0, 0, 0, 0]
    with pytest.raises(IndexError):
        foldin.group_by_user(torch.tensor([0, 3]), torch.tensor([1, 1]), torch.tensor([2, 2]), torch.tensor([0.0, 1.0]), 3)
    with pytest.raises(ValueError):
        foldin.group_by_user(torch.tensor([0, 1]), torch.tensor([1]), torch.tensor([2, 2]), torch.tensor([0.0, 1.0]), 3)


@pytest.mark.parametrize("hessian", [np.float64, np.float32])
@pytest.mark.parametrize("d,l2,labels,start", [(1, 1.0, "hard", False), (2, 1e-3, "separable", True),
                                               (7, 1e-3, "soft", True), (16, 1.0, "separable", False),
                                               (64, 1e-3, "hard", True)])
def test_host_model_is_a_minimiser(d, l2, labels, start, hessian):
    """The torch-autograd f64 gradient of f at the model's solution: |.|_inf <= 1e-9 (1 + sum_t |delta_t|_inf).  Each
    term's gradient is (p_t - z_t) delta_t with |p_t - z_t| <= 1, so the sum bounds the size of what cancels."""
    lengths = [0, 1, 3, 50, 300, 63, 64, 65, 131]
    V, rec, off, U0 = FM.make_case(d, labels, lengths, seed=100 + d, start=start)
    rows = FM.solve(V, rec, off, l2, U0, hessian_dtype=hessian)
    z = torch.from_numpy(rec[:, 3].copy().view(np.float32)).double()
    for r, row in enumerate(rows):
        b, e = off[r], off[r + 1]
        assert row.status == FM.CONVERGED and row.iters <= 50 and row.halvings < 30
        if e == b:
            assert row.iters == 0 and row.objective == 0.0 and not row.u.any()
            continue
        assert row.iters >= 1
        D = torch.from_numpy(FM.deltas(V, rec[b:e, 1], rec[b:e, 2]))
        u = torch.from_numpy(row.u).clone().requires_grad_(True)
        x = D @ u
        f = (torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs())) - z[b:e] * x).sum() + 0.5 * l2 * (u * u).sum()
        f.backward()
        bound = 1e-9 * (1.0 + float(D.abs().max(1)[0].sum()))
        assert float(u.grad.abs().max()) <= bound, (r, float(u.grad.abs().max()), bound)
        assert abs(float(f.detach()) - row.objective) <= 1e-12 * max(1.0, abs(row.objective))


def test_host_model_status_paths():
    V, rec, off, U0 = FM.make_case(7, "hard", [40, 0, 25, 12, 9], seed=9, start=True)
    z = rec[:, 3].copy().view(np.float32)
    full = FM.solve(V, rec, off, 1e-3, U0)
    assert [r.status for r in full] == [0] * 5 and full[0].iters > 1
    # status 1: the iteration cap; the iterate is the last accepted one, and f did not go up
    one = FM.solve_row(V, rec[:40, 1], rec[:40, 2], z[:40], 1e-3, U0[0], max_iter=1)
    start_f = FM.objective(U0[0].astype(np.float64), FM.deltas(V, rec[:40, 1], rec[:40, 2]), z[:40].astype(np.float64), 1e-3)
    assert one.status == FM.STOPPED and one.iters == 1 and np.isfinite(one.u).all() and one.objective <= start_f
    capped = FM.solve_row(V, rec[:40, 1], rec[:40, 2], z[:40], 1e-3, U0[0], max_iter=full[0].iters - 1)
    assert capped.status == FM.STOPPED and capped.iters == full[0].iters - 1
    # status 2: each rule on its own; an empty row is valid whatever its U_init
    def bad(**kw):
        a = dict(V=V, i=rec[:40, 1].copy(), j=rec[:40, 2].copy(), z=z[:40].copy(), u_init=U0[0].copy())
        for k, (pos, val) in kw.items():
            a[k] = a[k].copy()
            a[k][pos] = val
        return FM.solve_row(a["V"], a["i"], a["j"], a["z"], 1e-3, a["u_init"])
    for kw in (dict(i=(3, FM.M_ITEMS)), dict(j=(0, -1)), dict(z=(5, 1.5)), dict(z=(5, -0.25)), dict(z=(5, np.nan)),
               dict(u_init=(2, np.inf)), dict(V=((int(rec[7, 1]), 0), np.inf)), dict(V=((int(rec[7, 2]), 3), np.nan))):
        row = bad(**kw)
        assert row.status == FM.INVALID and row.iters == 0 and np.isnan(row.u).all() and np.isnan(row.objective), kw
    unused = sorted(set(range(FM.M_ITEMS)) - set(rec[:40, 1].tolist()) - set(rec[:40, 2].tolist()))[0]
    assert bad(V=((unused, 0), np.inf)).status == FM.CONVERGED           # a V row the user does not use
    # a minimiser of exactly 0 (one comparison labelled 1/2): from 0 the step is exactly 0, status 0 after one iteration;
    # from anywhere else the iterates shrink for ever without meeting a relative step test, status 1 at the cap
    half = np.array([0.5], dtype=np.float32)
    at0 = FM.solve_row(V, rec[:1, 1], rec[:1, 2], half, 1e-3)
    assert at0.status == FM.CONVERGED and at0.iters == 1 and not at0.u.any() and at0.objective == np.log(2.0)
    away = FM.solve_row(V, rec[:1, 1], rec[:1, 2], half, 1e-3, U0[0])
    assert away.status == FM.STOPPED and away.iters == 50 and np.abs(away.u).max() < 1e-12
    empty = FM.solve_row(V, [], [], [], 1e-3, np.full(7, np.nan, dtype=np.float32))
    assert empty.status == FM.CONVERGED and empty.iters == 0 and empty.objective == 0.0 and not empty.u.any()


def test_host_model_converges_at_once_from_its_own_fp32_solution():
    """A warm start from the fp32 rounding of the solution: one step that removes the rounding, one below xtol.  The
    decrease of the first is below the last bit of f for rows with small logits (l2 = 1: |u*| is small), so this holds
    only because the Armijo test is taken on the term-wise decrease (foldin_model.decrease)."""
    V, rec, off, _ = FM.make_case(2, "hard", [40, 55, 60, 70, 80, 90, 100, 120], seed=31)
    first = FM.solve(V, rec, off, 1.0)
    U32 = np.stack([r.u for r in first]).astype(np.float32)
    again = FM.solve(V, rec, off, 1.0, U32)
    assert [r.status for r in again] == [0] * 8 and max(r.iters for r in again) <= 2, [r.iters for r in again]
    for a, b in zip(first, again):
        assert np.abs(a.u - b.u).max() <= 1e-12 * np.abs(a.u).max()
