"""f64 numpy restatement of the Newton-CG form of the two exact block steps (include/mfcd.h: mfcd_fold_in_users_cg,
mfcd_item_step_cg), one row at a time, the algorithm exactly as the header fixes it: damped Newton whose step comes from
Jacobi-preconditioned conjugate gradients on Hessian-vector products (the Hessian is never formed), the line search of
the Cholesky form, and the stop rule |g|_2 <= l2 gtol |u|_inf on the gradient of each pass.  Both sides are one
function: a row is (D, c, z) with x = D u + c, c = 0 on the user side.  softplus, sigmoid and the constants come from
tests/foldin_model.py, the item side's staging and term-wise decrease from tests/itemstep_model.py; no code is shared
with the kernel, and the order of the sums is numpy's, so the device agrees to rounding, not bit for bit."""
import numpy as np

import foldin_model as FM
import itemstep_model as IM
from foldin_model import ARMIJO, CONVERGED, HALVINGS, INVALID, STOPPED, sigmoid

ETA = 1e-3                                                       # CG stops at |r|_2 <= ETA |g|_2 ...


def cg_cap(d):
    return 4 * d + 50                                            # ... or after this many iterations


class CgRow:
    """One row's result: u (the f64 iterate), objective, f_start, iters (CG solves), cg_iters (their iterations in
    all), status."""

    def __init__(self, u, f, f_start, iters, cg_iters, status):
        self.u, self.objective, self.f_start, self.iters, self.cg_iters, self.status = u, f, f_start, iters, cg_iters, status


def solve_problem(D, c, z, l2, u, max_iter=50, gtol=2.0 ** -26):
    """min over u of sum softplus(x) - z x + (l2 / 2) |u|^2, x = D u + c, from the start u."""
    d = D.shape[1]
    u = u.copy()
    it = cg_total = 0
    f_start = None
    while True:
        x = D @ u + c
        p = sigmoid(x)
        f = IM.objective(u, D, c, z, l2)
        if f_start is None:
            f_start = f
        g = D.T @ (p - z) + l2 * u
        w = p * (1.0 - p)
        gnorm = float(np.sqrt(g @ g))
        if gnorm <= l2 * gtol * np.abs(u).max():
            return CgRow(u, f, f_start, it, cg_total, CONVERGED)
        if it >= max_iter:
            return CgRow(u, f, f_start, it, cg_total, STOPPED)
        it += 1
        minv = 1.0 / ((D * D).T @ w + l2)
        s, r = np.zeros(d), -g
        zr = minv * r
        pv, rz = zr.copy(), float(r @ zr)
        for _ in range(cg_cap(d)):
            q = D.T @ (w * (D @ pv)) + l2 * pv
            pq = float(pv @ q)
            if not (pq > 0.0 and np.isfinite(pq)):
                return CgRow(u, f, f_start, it, cg_total, STOPPED)
            alpha = rz / pq
            s, r = s + alpha * pv, r - alpha * q
            cg_total += 1
            if float(np.sqrt(r @ r)) <= ETA * gnorm:
                break
            zr = minv * r
            rz_new = float(r @ zr)
            pv, rz = zr + (rz_new / rz) * pv, rz_new
        gs = float(g @ s)
        t, accepted = 1.0, False
        for _ in range(HALVINGS + 1):
            trial = u + t * s
            if IM.decrease(u, s, t, D, c, z, l2) <= ARMIJO * t * gs or IM.objective(trial, D, c, z, l2) <= f + ARMIJO * t * gs:
                accepted = True
                break
            t *= 0.5
        if not accepted:
            return CgRow(u, f, f_start, it, cg_total, STOPPED)
        u = trial


def _nan_row(d):
    return CgRow(np.full(d, np.nan), float("nan"), float("nan"), 0, 0, INVALID)


def solve_user_row(V, i, j, z, l2, u_init=None, max_iter=50, gtol=2.0 ** -26):
    V = np.asarray(V, dtype=np.float32)
    m, d = V.shape
    i, j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
    z = np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    if i.size == 0:
        return CgRow(np.zeros(d), 0.0, 0.0, 0, 0, CONVERGED)
    if ((i < 0) | (i >= m) | (j < 0) | (j >= m)).any() or not ((z >= 0.0) & (z <= 1.0)).all():
        return _nan_row(d)
    if u_init is not None and not np.isfinite(np.asarray(u_init, dtype=np.float32)).all():
        return _nan_row(d)
    if not np.isfinite(V[i]).all() or not np.isfinite(V[j]).all():
        return _nan_row(d)
    u = np.zeros(d) if u_init is None else np.asarray(u_init, dtype=np.float32).astype(np.float64)
    return solve_problem(FM.deltas(V, i, j), np.zeros(i.size), z, l2, u, max_iter, gtol)


def solve_users(V, records, row_off, l2, U_init=None, max_iter=50, gtol=2.0 ** -26):
    """All rows of a user call → list of CgRow."""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int32)).reshape(-1, 4)
    z = records[:, 3].copy().view(np.float32)
    out = []
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        out.append(solve_user_row(V, records[b:e, 1], records[b:e, 2], z[b:e], l2, None if U_init is None else U_init[r],
                                  max_iter, gtol))
    return out


def solve_item_row(U, V, k, u, i, j, z, l2, max_iter=50, gtol=2.0 ** -26):
    """Item k's v* (CgRow.u; the theta step is the caller's), started at V[k]."""
    U, V = np.asarray(U, dtype=np.float32), np.asarray(V, dtype=np.float32)
    (n, d), m = U.shape, V.shape[0]
    u, i, j = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (u, i, j))
    z = np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    if not 0 <= k < m:
        return _nan_row(d)
    if ((u < 0) | (u >= n) | (i < 0) | (i >= m) | (j < 0) | (j >= m)).any() or ((i != k) & (j != k)).any() \
            or not ((z >= 0.0) & (z <= 1.0)).all():
        return _nan_row(d)
    if not np.isfinite(V[k]).all() or not np.isfinite(U[u]).all() or not np.isfinite(V[np.where(i == k, j, i)]).all():
        return _nan_row(d)
    v_old = V[k].astype(np.float64)
    if u.size == 0:
        return CgRow(np.zeros(d), 0.0, 0.5 * l2 * float(v_old @ v_old), 0, 0, CONVERGED)
    D, c = IM.staged(U, V, k, u, i, j)
    return solve_problem(D, c, z, l2, v_old, max_iter, gtol)


def solve_items(U, V, records, row_off, l2, row_item=None, max_iter=50, gtol=2.0 ** -26):
    """All rows of an item call → list of CgRow (u = v*)."""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int32)).reshape(-1, 4)
    z = records[:, 3].copy().view(np.float32)
    out = []
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        k = r if row_item is None else int(row_item[r])
        out.append(solve_item_row(U, V, k, records[b:e, 0], records[b:e, 1], records[b:e, 2], z[b:e], l2, max_iter, gtol))
    return out


# ---- the inputs the CG tests share (tests/test_fold_in_cg.py, tests/test_item_step_cg.py, tests/test_fold_in_cg_cpu.py) ----
DS = (65, 128, 256)
L2S = (1e-3, 1.0)
MODEL_MAX_ITER = 1000         # the Cholesky models: itemstep_model.solve needs up to 99 iterations at l2 = 1e-3
DEVICE_MAX_ITER = 200


def row_lengths(C, R):
    """The empty row, less than a chunk, the chunk edges, the last resident row and the first streamed one."""
    return sorted({0, 1, 3, 50, 1000} | {C - 1, C, C + 1, 2 * C + 3} | {R - 1, R, R + 1})


def seed(d, labels, start):
    return 1000 * d + 10 * FM.LABELS.index(labels) + int(start)


def user_case(d, labels, start, C, R):
    return FM.make_case(d, labels, row_lengths(C, R), seed(d, labels, start), start)


def item_case(d, labels, start, C, R):
    """itemstep_model.make_case solves nine items; the CG lengths may be more or fewer, so the recipe runs with as many
    solved items as there are lengths (the first ones of a longer SOLVED list)."""
    lengths = row_lengths(C, R)
    solved = [5 + 7 * r for r in range(len(lengths))]
    assert solved[-1] < IM.M_ITEMS
    keep = IM.SOLVED
    IM.SOLVED = solved
    try:
        return IM.make_case(d, labels, lengths, 5000 + seed(d, labels, start), start)
    finally:
        IM.SOLVED = keep
