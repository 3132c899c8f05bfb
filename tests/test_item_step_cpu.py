"""CPU-only checks of the item step and the alternating fit (include/mfcd.h: mfcd_item_step; mfcd/foldin.py:
group_by_item, fold_in_items, total_objective; mfcd/alternating.py; structure.fit_items, refit_items, refit_alternating):
the entries are declared and bound under the unchanged ABI version, every limit is refused before the device is touched,
there is no CPU form of the solve, group_by_item is a stable grouping with both copies of every comparison, and the host
model of tests/itemstep_model.py — the reference of the GPU tests — is a minimiser, follows the status rules and
satisfies the Jensen bound that makes simultaneous half steps safe."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import itemstep_model as IM
from conftest import ROOT


def test_item_step_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_item_step_workspace_bytes", 3), ("mfcd_item_step", 19)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t)\s+%s\(([^)]*)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == nargs, name
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header)) - {"mfcd_sample"}
    assert declared == set(_lib.SIGNATURES)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4
    size = L.mfcd_item_step_workspace_bytes
    assert size(0, 1, 0) == 256 and size(9, 64, 1) == 512 and size(9, 64, 32) == 512 and size(9, 64, 33) == 768
    assert size(1 << 30, 64, 1 << 40) == 256 + 8 * (1 << 40)
    for rows, d, records in ((4, 0, 1), (4, 65, 1), (-1, 8, 1), (4, 8, -1)):
        assert size(rows, d, records) == 0, (rows, d, records)
    for text in (header, open(os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc", "foldin.hip")).read()):
        assert "does not separate" not in text and "not separable" not in text


def test_item_step_limits_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    P = 1 << 20                                  # non-null addresses that are never dereferenced: every call is refused
    base = dict(U=P, n=53, V=2 * P, m=97, d=8, records=3 * P, row_off=4 * P, row_item=5 * P, rows=4, l2=1.0, theta=0.5,
                max_iter=50, xtol=2.0 ** -30, V_out=6 * P, objective=7 * P, info=8 * P, ws=9 * P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        return L.mfcd_item_step(a["U"], a["n"], a["V"], a["m"], a["d"], a["records"], a["row_off"], a["row_item"],
                                a["rows"], a["l2"], a["theta"], a["max_iter"], a["xtol"], a["V_out"], a["objective"],
                                a["info"], a["ws"], a["ws_bytes"], None)

    inf, nan = float("inf"), float("nan")
    for bad in (dict(d=0), dict(d=65), dict(n=0), dict(m=0), dict(rows=-1), dict(U=None), dict(V=None), dict(row_off=None),
                dict(V_out=None), dict(info=None), dict(l2=0.0), dict(l2=-1.0), dict(l2=inf), dict(l2=nan),
                dict(theta=0.0), dict(theta=-0.5), dict(theta=1.0 + 2.0 ** -52), dict(theta=inf), dict(theta=nan),
                dict(max_iter=0), dict(max_iter=1001), dict(xtol=-1e-30), dict(xtol=inf), dict(xtol=nan),
                dict(V_out=P), dict(V_out=2 * P), dict(V_out=P + 16), dict(V_out=2 * P + 64), dict(V_out=P - 64),
                dict(V_out=2 * P + 97 * 8 * 4 - 4), dict(ws=None),
                dict(row_item=None, rows=98), dict(row_item=None, rows=4, m=3)):
        assert call(**bad) == -1, bad
    assert call(rows=0, l2=0.0) == -1 and call(rows=0, d=65) == -1 and call(rows=0, V_out=P) == -1    # refused all the same
    assert call(rows=0, theta=0.0) == -1 and call(rows=0, row_item=None, m=1) == 0
    assert call(ws_bytes=16) == -2
    assert call(ws_bytes=L.mfcd_item_step_workspace_bytes(4, 8, 0) - 1) == -2
    # rows = 0: success with nothing launched, whatever the workspace; the nullable arguments may be absent
    assert call(rows=0) == 0 and call(rows=0, ws=None, ws_bytes=0) == 0
    assert call(rows=0, row_item=None, objective=None, records=None) == 0
    assert call(rows=0, max_iter=1, xtol=0.0, l2=1e-300, d=64, m=1, n=1, theta=1.0) == 0
    assert call(rows=0, max_iter=1000, d=1, theta=2.0 ** -60) == 0
    assert call(rows=0, V_out=2 * P + 97 * 8 * 4) == 0          # V_out may start where V ends


def test_there_is_no_cpu_form_of_the_item_step():
    import structure as S
    from mfcd import _lib, alternating, foldin
    U, V, rec, off, items = IM.make_case(2, "hard", [3, 0, 5, 1, 1, 1, 1, 1, 1], seed=1)
    Ut, Vt, rt, ot = (torch.from_numpy(a) for a in (U, V, rec, off))
    with pytest.raises(_lib.MfcdError):
        foldin.fold_in_items(Ut, Vt, rt, ot, 1.0, torch.from_numpy(items))
    data = (rt[:, 0], rt[:, 1], rt[:, 2], rt[:, 3].contiguous().view(torch.float32))
    with pytest.raises(_lib.MfcdError):
        alternating.fit_alternating(Ut, Vt, *data, 1.0)
    model = S.MatrixFactorization(IM.N_USERS, IM.M_ITEMS, 2)
    with pytest.raises(RuntimeError):
        S.fit_items((Ut, Vt), data, 1.0)
    with pytest.raises(RuntimeError):
        S.fit_items(model, data, 1.0, [5, 12])
    with pytest.raises(RuntimeError):
        S.refit_items(model, data, 1e-5)
    with pytest.raises(RuntimeError):
        S.refit_alternating(model, data, 1e-5)
    with pytest.raises(TypeError):
        S.fit_items(Vt, data, 1.0)
    for fn, first in ((S.fit_items, ["model_or_UV", "data", "l2", "items"]),
                      (S.refit_items, ["model", "train_loader", "weight_decay"]),
                      (S.refit_alternating, ["model", "train_loader", "weight_decay", "sweeps", "item_steps"])):
        assert list(inspect.signature(fn).parameters) == first
        assert fn.__doc__.startswith("Extension (not in the reference)")
    sig = inspect.signature(S.refit_alternating).parameters
    assert sig["sweeps"].default == 10 and sig["item_steps"].default == 2 and inspect.signature(S.fit_items).parameters["items"].default is None
    sig = inspect.signature(foldin.fold_in_items).parameters
    assert list(sig) == ["U", "V", "records", "row_off", "l2", "row_item", "theta", "max_iter", "xtol"]
    assert sig["row_item"].default is None and sig["theta"].default == 1.0 and sig["max_iter"].default == 50 \
        and sig["xtol"].default == 2.0 ** -30
    sig = inspect.signature(alternating.fit_alternating).parameters
    assert list(sig) == ["U", "V", "u", "i", "j", "z", "l2", "sweeps", "item_steps", "max_iter", "xtol"]
    assert sig["sweeps"].default == 10 and sig["item_steps"].default == 2 and sig["max_iter"].default == 50 \
        and sig["xtol"].default == 2.0 ** -30
    assert list(inspect.signature(foldin.group_by_item).parameters) == ["u", "i", "j", "z", "m"]
    assert list(inspect.signature(foldin.total_objective).parameters) == ["U", "V", "u", "i", "j", "z", "l2"]
    assert foldin.ItemStepResult._fields == ("V", "objective_start", "objective", "iters", "status")
    assert alternating.AlternatingResult._fields == ("U", "V", "history", "user_status", "item_status")


def test_group_by_item_keeps_both_copies_in_a_stable_order():
    from mfcd import foldin
    rng = np.random.default_rng(5)
    m, N = 11, 300
    u = rng.integers(0, 50, N)
    i, j = rng.integers(0, m, N), rng.integers(0, m, N)
    for a in (i, j):
        a[(a == 4) | (a == 10)] = 3                               # items 4 and 10 (the last) appear nowhere
    assert (i == j).any()
    z = rng.random(N).astype(np.float32)
    rec, off = foldin.group_by_item(*(torch.from_numpy(a) for a in (u, i, j, z)), m)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (2 * N, 4) and off.dtype == torch.int64
    rec, off = rec.numpy(), off.numpy()
    assert tuple(off.shape) == (m + 1,) and off[0] == 0 and off[-1] == 2 * N and (np.diff(off) >= 0).all()
    assert off[4] == off[5] and off[10] == off[11]
    assert np.diff(off).sum() == 2 * N
    for k in range(m):
        # comparison t gives its i-copy and then its j-copy, comparisons in their original order
        copies = [t for t in range(N) for slot in (i[t], j[t]) if slot == k]
        blk = rec[off[k]:off[k + 1]]
        assert len(copies) == len(blk)
        assert ((blk[:, 1] == k) | (blk[:, 2] == k)).all()
        assert blk[:, 0].tolist() == u[copies].tolist() and blk[:, 1].tolist() == i[copies].tolist()
        assert blk[:, 2].tolist() == j[copies].tolist()
        assert blk[:, 3].copy().view(np.float32).tolist() == z[copies].tolist()
    t = int(np.flatnonzero(i == j)[0])                             # a comparison of an item with itself: twice in one row
    k = int(i[t])
    blk = rec[off[k]:off[k + 1]]
    twice = np.flatnonzero((blk[:, 0] == u[t]) & (blk[:, 1] == k) & (blk[:, 2] == k) & (blk[:, 3] == z[t:t + 1].view(np.int32)[0]))
    assert len(twice) >= 2 and (np.diff(twice) == 1).any()
    mrec, moff = IM.group_by_item(u, i, j, z, m)                   # the model's numpy twin agrees
    assert np.array_equal(mrec, rec) and np.array_equal(moff, off)
    empty = torch.zeros(0, dtype=torch.int64)
    rec, off = foldin.group_by_item(empty, empty, empty, torch.zeros(0), 3)
    assert tuple(rec.shape) == (0, 4) and off.tolist() == [0, 0, 0, 0]
    one = torch.tensor([0, 1])
    for bad_i, bad_j in (([1, 3], [2, 2]), ([1, 1], [2, 3]), ([-1, 1], [2, 2])):
        with pytest.raises(IndexError):
            foldin.group_by_item(one, torch.tensor(bad_i), torch.tensor(bad_j), torch.tensor([0.0, 1.0]), 3)
    with pytest.raises(ValueError):
        foldin.group_by_item(one, torch.tensor([1]), torch.tensor([2, 2]), torch.tensor([0.0, 1.0]), 3)


def test_total_objective_matches_the_model():
    from mfcd import foldin
    U0, V0, u, i, j, z = IM.descent_case()
    F = foldin.total_objective(*(torch.from_numpy(a) for a in (U0, V0, u, i, j, z)), 0.5)
    ref = IM.total_objective(U0, V0, u, i, j, z, 0.5)
    assert F.dtype == torch.float64 and F.dim() == 0 and abs(float(F) - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("d,l2,labels,start", [(1, 1.0, "hard", False), (2, 1e-3, "separable", True),
                                               (7, 1e-3, "soft", True), (16, 1.0, "separable", False),
                                               (64, 1e-3, "hard", True), (3, 1e-3, "hard", False)])
def test_host_model_is_a_minimiser(d, l2, labels, start):
    """|grad f_k(v*)|_inf <= 1e-9 max(1, |grad f_k(start)|_inf), the gradient formed in f64 from the staged problem."""
    lengths = [0, 1, 3, 50, 300, 63, 64, 65, 131]
    U, V, rec, off, items = IM.make_case(d, labels, lengths, seed=200 + d, start=start)
    rows = IM.solve(U, V, rec, off, l2, items)
    for r, row in enumerate(rows):
        assert row.status == IM.CONVERGED and row.iters <= 50 and row.halvings < 30
        v_old = V[items[r]].astype(np.float64)
        if lengths[r] == 0:
            assert row.iters == 0 and row.objective == 0.0 and not row.v_star.any() and not row.v_out.any()
            assert row.f_start == 0.5 * l2 * float(v_old @ v_old)
            continue
        assert row.iters >= 1
        D, c, z = row.problem
        g_end, g_start = IM.gradient(row.v_star, D, c, z, l2), IM.gradient(v_old, D, c, z, l2)
        assert np.abs(g_end).max() <= 1e-9 * max(1.0, np.abs(g_start).max()), (r, np.abs(g_end).max())
        assert row.objective <= row.f_start
        assert abs(IM.objective(row.v_star, D, c, z, l2) - row.objective) <= 1e-12 * max(1.0, abs(row.objective))
        # f_k is F restricted to the row, up to what does not depend on V[k]
        W = V.copy().astype(np.float64)
        b, e = off[r], off[r + 1]
        zz = rec[b:e, 3].copy().view(np.float32)
        part = []
        for v in (v_old, row.v_star):
            W[items[r]] = v
            x = np.einsum("tk,tk->t", U.astype(np.float64)[rec[b:e, 0]], W[rec[b:e, 1]] - W[rec[b:e, 2]])
            part.append(float(np.sum(IM.softplus(x) - zz * x) + 0.5 * l2 * (v @ v)))
        assert abs((part[0] - part[1]) - (row.f_start - row.objective)) <= 1e-9 * max(1.0, row.f_start)
        half = IM.solve_item(U, V, int(items[r]), rec[b:e, 0], rec[b:e, 1], rec[b:e, 2], zz, l2, theta=0.5)
        assert np.array_equal(half.v_star, row.v_star) and np.array_equal(half.v_out, v_old + 0.5 * (row.v_star - v_old))


@pytest.mark.parametrize("l2", [0.01, 0.5])
def test_jensen_bound_holds_for_the_models_sweeps(l2):
    """n = 40, m = 30, d = 3, N = 600, 20 sweeps of one user step and two simultaneous item steps at theta = 1/2:
    F(V_new) <= F(V) - (1/2) sum_k (f_k(v_k) - f_k(v*_k)) + slack at every item step, and no user step raises F beyond its
    slack.  The tables are rounded to fp32 after every sub-step as the device's are; the slack is the first-order effect
    of that one rounding, 2 x 2^-24 sum |dF/dW| |W| at the new table, plus 1e-12 |F| (itemstep_model.rounding_slack)."""
    U, V, u, i, j, z = IM.descent_case()
    data = (u, i, j, z)
    F = IM.total_objective(U, V, *data, l2)
    F0, worst = F, 0.0
    for sweep in range(20):
        U = IM.model_user_step(U, V, *data, l2)
        Fn = IM.total_objective(U, V, *data, l2)
        assert Fn <= F + IM.rounding_slack(IM.total_gradients(U, V, *data, l2)[0], U, Fn), (sweep, F, Fn)
        F = Fn
        for step in range(2):
            V, gain = IM.model_item_step(U, V, *data, l2, 0.5)
            assert gain >= 0.0
            Fn = IM.total_objective(U, V, *data, l2)
            slack = IM.rounding_slack(IM.total_gradients(U, V, *data, l2)[1], V, Fn)
            assert Fn <= F - 0.5 * gain + slack, (sweep, step, F, Fn, gain, slack)
            if gain > 0:
                worst = max(worst, (Fn - (F - 0.5 * gain)) / slack)
            F = Fn
    print(f"l2 {l2}: F {F0:.6f} -> {F:.6f}; largest (F_new - bound) / slack {worst:.3f}")
    assert F < F0


def test_host_model_status_paths():
    lengths = [40, 0, 25, 12, 9, 3, 3, 3, 3]
    U, V, rec, off, items = IM.make_case(7, "hard", lengths, seed=9, start=True)
    z = rec[:, 3].copy().view(np.float32)
    full = IM.solve(U, V, rec, off, 1e-3, items)
    assert [r.status for r in full] == [0] * 9 and full[0].iters > 1
    k = int(items[0])
    blk = dict(u=rec[:40, 0], i=rec[:40, 1], j=rec[:40, 2], z=z[:40])

    def bad(k=k, l2=1e-3, **kw):
        a = dict(U=U, V=V, **blk)
        for name, (pos, val) in kw.items():
            a[name] = a[name].copy()
            a[name][pos] = val
        return IM.solve_item(a["U"], a["V"], k, a["u"], a["i"], a["j"], a["z"], l2)

    one = IM.solve_item(U, V, k, l2=1e-3, max_iter=1, **blk)
    assert one.status == IM.STOPPED and one.iters == 1 and np.isfinite(one.v_out).all() and one.objective <= one.f_start
    slot = "i" if rec[3, 1] == k else "j"                          # where the solved item sits in record 3
    other = "j" if slot == "i" else "i"
    partner = int(rec[7, 2] if rec[7, 1] == k else rec[7, 1])
    foreign = [x for x in range(IM.M_ITEMS) if x != k][0]
    for kw in (dict(u=(3, IM.N_USERS)), dict(u=(3, -1)), dict(**{other: (3, IM.M_ITEMS)}), dict(**{other: (3, -1)}),
               dict(**{slot: (3, foreign)}),                                                    # a record that does not hold k
               dict(z=(5, 1.5)), dict(z=(5, -0.25)), dict(z=(5, np.nan)),
               dict(V=((k, 2), np.inf)), dict(V=((partner, 0), np.nan)), dict(U=((int(rec[11, 0]), 6), np.inf))):
        row = bad(**kw)
        assert row.status == IM.INVALID and row.iters == 0 and np.isnan(row.v_out).all() and np.isnan(row.objective) \
            and np.isnan(row.f_start), kw
    for kk in (-1, IM.M_ITEMS):
        assert bad(k=kk).status == IM.INVALID
    used = set(rec[:40, 1].tolist()) | set(rec[:40, 2].tolist())
    unused_item = sorted(set(range(IM.M_ITEMS)) - used)[0]
    unused_user = sorted(set(range(IM.N_USERS)) - set(rec[:40, 0].tolist()))
    assert bad(V=((unused_item, 0), np.inf)).status == IM.CONVERGED              # rows the item does not use
    if unused_user:
        assert bad(U=((unused_user[0], 0), np.nan)).status == IM.CONVERGED
    # a comparison of the item with itself: sigma = 0, the term is the constant log 2
    self_row = bad(**{other: (3, k)})
    rest = {name: np.delete(a, 3) for name, a in blk.items()}
    without = IM.solve_item(U, V, k, l2=1e-3, **rest)
    assert self_row.status == IM.CONVERGED and np.abs(self_row.v_star - without.v_star).max() <= 1e-12 * np.abs(without.v_star).max()
    assert abs(self_row.objective - without.objective - np.log(2.0)) <= 1e-12 * max(1.0, without.objective)
    # the empty row: v* = 0, v_out = (1 - theta) v_old, objectives {(l2 / 2) |v_old|^2, 0}; invalid only by its own item
    v_old = V[k].astype(np.float64)
    for theta in (1.0, 0.5):
        empty = IM.solve_item(U, V, k, [], [], [], [], 0.25, theta=theta)
        assert empty.status == IM.CONVERGED and empty.iters == 0 and empty.objective == 0.0
        assert np.array_equal(empty.v_out, (1.0 - theta) * v_old) and empty.f_start == 0.125 * float(v_old @ v_old)
    Vbad = V.copy()
    Vbad[k, 0] = np.nan
    assert IM.solve_item(U, Vbad, k, [], [], [], [], 0.25).status == IM.INVALID
