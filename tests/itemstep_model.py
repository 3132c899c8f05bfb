"""f64 numpy restatement of the item step (include/mfcd.h: mfcd_item_step) and of an alternating sweep, one item's row at
a time: with U and the other items fixed, item k minimises
    f_k(v) = sum_t softplus(x_t) - z_t x_t + (l2 / 2) |v|^2,   x_t = v . delta_t + c_t,
    delta_t = sigma_t U[u_t],   sigma_t = [i_t = k] - [j_t = k],   c_t = -sigma_t U[u_t] . V[o_t],
by the iteration the header fixes for the user step (damped Newton, Cholesky, at most 30 halvings on the Armijo rule
with 1e-4 taken on the term-wise decrease, stop on |t s|_inf <= xtol |v|_inf).  It shares no code with the kernel or with
mfcd/foldin.py; only softplus, sigmoid and the constants come from tests/foldin_model.py.  The order of its sums is
numpy's, so the device agrees with it to rounding, not bit for bit.  Also here: the inputs the item-step tests share."""
import numpy as np

import foldin_model as FM
from foldin_model import ARMIJO, CONVERGED, HALVINGS, INVALID, STOPPED, sigmoid, softplus

N_USERS, M_ITEMS = 53, 97
SOLVED = [5 + 7 * r for r in range(9)]                      # the nine items a call of the recipe solves
LABELS = FM.LABELS


def objective(v, D, c, z, l2):
    x = D @ v + c
    return float(np.sum(softplus(x) - z * x) + 0.5 * l2 * (v @ v))


def decrease(v, s, t, D, c, z, l2):
    """f(v + t s) - f(v) summed term by term, as foldin_model.decrease, with the offset in x."""
    x, h = D @ v + c, t * (D @ s)
    small = np.abs(h) < 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        near = np.log1p(sigmoid(x) * np.expm1(np.where(small, h, 0.0)))
    terms = np.where(small, near, softplus(x + h) - softplus(x)) - z * h
    return float(np.sum(terms) + l2 * (t * (v @ s) + 0.5 * t * t * (s @ s)))


def gradient(v, D, c, z, l2):
    return D.T @ (sigmoid(D @ v + c) - z) + l2 * v


class ItemRow:
    """One row's result in f64: v_out = v_old + theta (v* - v_old) (not yet rounded to fp32), v_star, f_start = f_k(v_old),
    objective = f_k(v*), iters, status, the most halvings of one iteration, and (D, c, z) for checks."""

    def __init__(self, v_out, v_star, f_start, f, iters, status, halvings=0, problem=None):
        self.v_out, self.v_star, self.f_start, self.objective = v_out, v_star, f_start, f
        self.iters, self.status, self.halvings, self.problem = iters, status, halvings, problem


def staged(U, V, k, u, i, j):
    """(delta [T, d], c [T]) of item k's comparisons in f64 from the fp32 tables."""
    U64, V64 = np.asarray(U, dtype=np.float32).astype(np.float64), np.asarray(V, dtype=np.float32).astype(np.float64)
    sigma = (i == k).astype(np.float64) - (j == k).astype(np.float64)
    other = np.where(i == k, j, i)
    D = sigma[:, None] * U64[u]
    c = -sigma * np.einsum("tk,tk->t", U64[u], V64[other])
    return D, c


def solve_item(U, V, k, u, i, j, z, l2, theta=1.0, max_iter=50, xtol=2.0 ** -30):
    """Item k's row over the comparisons (u[t], i[t], j[t], z[t]), started at V[k]."""
    U, V = np.asarray(U, dtype=np.float32), np.asarray(V, dtype=np.float32)
    (n, d), m = U.shape, V.shape[0]
    u, i, j = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (u, i, j))
    z = np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    nan = float("nan")
    nan_row = ItemRow(np.full(d, nan), np.full(d, nan), nan, nan, 0, INVALID)
    if not 0 <= k < m:
        return nan_row
    if ((u < 0) | (u >= n) | (i < 0) | (i >= m) | (j < 0) | (j >= m)).any() or ((i != k) & (j != k)).any() \
            or not ((z >= 0.0) & (z <= 1.0)).all():                                      # a NaN label fails both
        return nan_row
    if not np.isfinite(V[k]).all() or not np.isfinite(U[u]).all() or not np.isfinite(V[np.where(i == k, j, i)]).all():
        return nan_row
    v_old = V[k].astype(np.float64)
    if u.size == 0:
        return ItemRow(v_old + theta * (0.0 - v_old), np.zeros(d), 0.5 * l2 * float(v_old @ v_old), 0.0, 0, CONVERGED)
    D, c = staged(U, V, k, u, i, j)
    v = v_old.copy()
    f = f_start = objective(v, D, c, z, l2)

    def done(status, it, worst):
        return ItemRow(v_old + theta * (v - v_old), v, f_start, f, it, status, worst, (D, c, z))

    it, worst = 0, 0
    while True:
        it += 1
        p = sigmoid(D @ v + c)
        g = D.T @ (p - z) + l2 * v
        H = (D * (p * (1.0 - p))[:, None]).T @ D + l2 * np.eye(d)
        try:
            Lc = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return done(STOPPED, it, worst)
        s = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        if not s.any():
            return done(CONVERGED, it, worst)
        gs = float(g @ s)
        t, accepted = 1.0, False
        for h in range(HALVINGS + 1):
            trial = v + t * s
            f_trial = objective(trial, D, c, z, l2)
            if decrease(v, s, t, D, c, z, l2) <= ARMIJO * t * gs or f_trial <= f + ARMIJO * t * gs:
                accepted = True
                worst = max(worst, h)
                break
            t *= 0.5
        if not accepted:
            return done(STOPPED, it, HALVINGS)
        v, f = trial, f_trial
        if t * np.abs(s).max() <= xtol * np.abs(v).max():
            return done(CONVERGED, it, worst)
        if it >= max_iter:
            return done(STOPPED, it, worst)


def solve(U, V, records, row_off, l2, row_item=None, theta=1.0, max_iter=50, xtol=2.0 ** -30):
    """All rows of a call: records int32 [N, 4] (u, i, j, z as fp32 bits), row_off [rows + 1] → list of ItemRow."""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int32)).reshape(-1, 4)
    z = records[:, 3].copy().view(np.float32)
    out = []
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        k = r if row_item is None else int(row_item[r])
        out.append(solve_item(U, V, k, records[b:e, 0], records[b:e, 1], records[b:e, 2], z[b:e], l2, theta, max_iter, xtol))
    return out


def group_by_item(u, i, j, z, m):
    """numpy twin of mfcd.foldin.group_by_item: every comparison once in the row of i and once in the row of j, stable,
    the i-copy first → (records int32 [2 N, 4], row_off int64 [m + 1])."""
    u, i, j = (np.asarray(a, dtype=np.int64) for a in (u, i, j))
    z = np.asarray(z, dtype=np.float32)
    key = np.stack((i, j), 1).reshape(-1)
    order = np.argsort(key, kind="stable")
    rec = np.stack((u, i, j, z.view(np.int32).astype(np.int64)), 1).astype(np.int32)[order // 2]
    off = np.concatenate(([0], np.cumsum(np.bincount(key, minlength=m)))).astype(np.int64)
    return np.ascontiguousarray(rec), off


# ---- the total objective and what the descent tests need ----
def total_objective(U, V, u, i, j, z, l2):
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    x = np.einsum("tk,tk->t", U[u], V[i] - V[j])
    return float(np.sum(softplus(x) - np.asarray(z, dtype=np.float64) * x) + 0.5 * l2 * (np.sum(U * U) + np.sum(V * V)))


def total_gradients(U, V, u, i, j, z, l2):
    """(dF/dU, dF/dV) in f64."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    dv = V[i] - V[j]
    r = sigmoid(np.einsum("tk,tk->t", U[u], dv)) - np.asarray(z, dtype=np.float64)
    GU, GV = l2 * U, l2 * V
    np.add.at(GU, u, r[:, None] * dv)
    np.add.at(GV, i, r[:, None] * U[u])
    np.add.at(GV, j, -r[:, None] * U[u])
    return GU, GV


def rounding_slack(G, W, F):
    """What one fp32 rounding of every entry of the table W (relative error <= 2^-24 each) can add to F to first order,
    sum |dF/dW| |W| 2^-24, with a factor 2, plus 1e-12 |F| for the f64 evaluation of F itself."""
    return 2.0 * 2.0 ** -24 * float(np.sum(np.abs(G) * np.abs(W))) + 1e-12 * abs(F)


def model_user_step(U, V, u, i, j, z, l2):
    """The exact user step by foldin_model.solve_row, warm-started from U → U_new fp32 (each row rounded once)."""
    out = np.zeros_like(np.asarray(U, dtype=np.float32))
    for r in range(U.shape[0]):
        at = np.flatnonzero(u == r)
        row = FM.solve_row(V, i[at], j[at], z[at], l2, U[r])
        assert row.status == CONVERGED or at.size == 0, r
        out[r] = row.u.astype(np.float32)
    return out


def model_item_step(U, V, u, i, j, z, l2, theta=0.5):
    """All items at once, each against the given rows of the others → (V_new fp32, sum_k f_k(v_k) - f_k(v*_k))."""
    rec, off = group_by_item(u, i, j, z, V.shape[0])
    rows = solve(U, V, rec, off, l2, None, theta)
    assert all(r.status == CONVERGED for r in rows)
    return np.stack([r.v_out for r in rows]).astype(np.float32), float(sum(r.f_start - r.objective for r in rows))


def descent_case(seed=7, n=40, m=30, d=3, N=600):
    """The small problem of the descent tests: start 0.1 N(0, I) in fp32, hard labels from hidden tables N(0, I)."""
    rng = np.random.default_rng(seed)
    U0, V0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32), (0.1 * rng.standard_normal((m, d))).astype(np.float32)
    u, i, j = rng.integers(0, n, N), rng.integers(0, m, N), rng.integers(0, m, N)
    Uh, Vh = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    z = (rng.random(N) < sigmoid(np.einsum("tk,tk->t", Uh[u], Vh[i] - Vh[j]))).astype(np.float32)
    return U0, V0, u, i, j, z


# ---- the inputs the item-step tests share (tests/test_item_step.py, tests/test_item_step_cpu.py) ----
def make_case(d, labels, lengths, seed, start=False):
    """One ragged call of nine rows (row r solves item SOLVED[r] over lengths[r] comparisons): U ~ N(0, 2 / d) in fp32,
    a hidden item table ~ N(0, 9 I) in fp32, users uniform, the partner item uniform over the 88 items no row solves,
    sigma = +-1 by a fair coin (whether the solved item sits in the i or the j slot), labels from sigmoid(x) at the
    hidden table — "hard", "soft", "separable" as in foldin_model.make_case.  The table handed to the kernel is the
    hidden one with the solved rows replaced by the start: 0, or N(0, 100 I) in fp32 with start=True.
    → (U, V, records int32 [N, 4], row_off int64 [10], row_item int32 [9])."""
    assert len(lengths) == len(SOLVED)
    rng = np.random.default_rng(seed)
    n, m = N_USERS, M_ITEMS
    U = (rng.standard_normal((n, d)) * np.sqrt(2.0 / d)).astype(np.float32)
    hidden = (3.0 * rng.standard_normal((m, d))).astype(np.float32)
    row_off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    N = int(row_off[-1])
    own = np.repeat(np.asarray(SOLVED), lengths)
    partners = np.asarray(sorted(set(range(m)) - set(SOLVED)))
    users = rng.integers(0, n, N)
    partner = partners[rng.integers(0, partners.size, N)]
    first = rng.random(N) < 0.5                                  # the solved item is i (sigma = +1)
    i, j = np.where(first, own, partner), np.where(first, partner, own)
    H64 = hidden.astype(np.float64)
    x = np.einsum("tk,tk->t", U.astype(np.float64)[users], H64[i] - H64[j])
    p = sigmoid(x)
    if labels == "hard":
        z = (rng.random(N) < p).astype(np.float32)
    elif labels == "soft":
        z = (rng.random((4, N)) < p).mean(0).astype(np.float32)
        for r in range(len(lengths)):    # all labels 1/2: see foldin_model.make_case
            b, e = row_off[r], row_off[r + 1]
            if e > b and (z[b:e] == 0.5).all():
                z[b] = 0.75
    elif labels == "separable":
        z = (x > 0).astype(np.float32)
    else:
        raise ValueError(labels)
    rec = np.empty((N, 4), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = users, i, j, z.view(np.int32)
    V = hidden.copy()
    V[SOLVED] = (10.0 * rng.standard_normal((len(SOLVED), d))).astype(np.float32) if start else 0.0
    return U, V, rec, row_off, np.asarray(SOLVED, dtype=np.int32)
