"""f64 numpy restatement of the fold-in solve (include/mfcd.h: mfcd_fold_in_users): one user's row at a time, the
algorithm exactly as the header fixes it — damped Newton with a Cholesky solve, backtracking from t = 1 with at most 30
halvings on the Armijo rule with 1e-4 (taken on the decrease of f summed term by term, as the header says), stop on
|t s|_inf <= xtol |u|_inf.  It shares no code with the kernel or with
mfcd/foldin.py; the order of its sums is numpy's, so the device agrees with it to rounding, not bit for bit."""
import numpy as np

HALVINGS = 30
ARMIJO = 1e-4
CONVERGED, STOPPED, INVALID = 0, 1, 2


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def deltas(V, i, j):
    """delta_t = V[i_t] - V[j_t] in f64 from the fp32 table: exact."""
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    return V[np.asarray(i, dtype=np.int64)] - V[np.asarray(j, dtype=np.int64)]


def objective(u, D, z, l2):
    x = D @ u
    return float(np.sum(softplus(x) - z * x) + 0.5 * l2 * (u @ u))


def decrease(u, s, t, D, z, l2):
    """f(u + t s) - f(u), summed term by term: softplus(x + h) - softplus(x) = log1p(sigmoid(x) expm1(h)) for |h| < 1 (exact
    to the rounding of the difference itself), the difference of the two values for a longer step.  Close to the
    minimiser the decrease of a full Newton step is below the last bit of f; the Armijo test is taken on this sum."""
    x, h = D @ u, t * (D @ s)
    small = np.abs(h) < 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        near = np.log1p(sigmoid(x) * np.expm1(np.where(small, h, 0.0)))
    terms = np.where(small, near, softplus(x + h) - softplus(x)) - z * h
    return float(np.sum(terms) + l2 * (t * (u @ s) + 0.5 * t * t * (s @ s)))


class Row:
    """One row's result: u (f64), objective, iters, status, and what the line searches did (most halvings of one
    iteration)."""

    def __init__(self, u, f, iters, status, halvings=0):
        self.u, self.objective, self.iters, self.status, self.halvings = u, f, iters, status, halvings


def solve_row(V, i, j, z, l2, u_init=None, max_iter=50, xtol=2.0 ** -30, hessian_dtype=np.float64):
    """The row whose comparisons are (i[t], j[t], z[t]).  hessian_dtype=np.float32 forms the Hessian's data sum in fp32
    (the contract allows it): the fixed point is the same."""
    V = np.asarray(V, dtype=np.float32)
    m, d = V.shape
    i, j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
    z = np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    nan_row = Row(np.full(d, np.nan), float("nan"), 0, INVALID)
    if i.size == 0:
        return Row(np.zeros(d), 0.0, 0, CONVERGED)
    if ((i < 0) | (i >= m) | (j < 0) | (j >= m)).any() or not ((z >= 0.0) & (z <= 1.0)).all():     # NaN fails both
        return nan_row
    if u_init is not None and not np.isfinite(np.asarray(u_init, dtype=np.float32)).all():
        return nan_row
    if not np.isfinite(V[i]).all() or not np.isfinite(V[j]).all():
        return nan_row
    D = deltas(V, i, j)
    u = np.zeros(d) if u_init is None else np.asarray(u_init, dtype=np.float32).astype(np.float64)
    f = objective(u, D, z, l2)
    it, worst = 0, 0
    while True:
        it += 1
        p = sigmoid(D @ u)
        g = D.T @ (p - z) + l2 * u
        w = p * (1.0 - p)
        if hessian_dtype == np.float64:
            H = (D * w[:, None]).T @ D
        else:
            A = (np.sqrt(w)[:, None] * D).astype(np.float32)
            H = (A.T @ A).astype(np.float64)
        H = H + l2 * np.eye(d)
        try:
            Lc = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return Row(u, f, it, STOPPED, worst)
        s = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        if not s.any():
            return Row(u, f, it, CONVERGED, worst)
        gs = float(g @ s)
        t, accepted = 1.0, False
        for h in range(HALVINGS + 1):
            trial = u + t * s
            f_trial = objective(trial, D, z, l2)
            if decrease(u, s, t, D, z, l2) <= ARMIJO * t * gs or f_trial <= f + ARMIJO * t * gs:
                accepted = True
                worst = max(worst, h)
                break
            t *= 0.5
        if not accepted:
            return Row(u, f, it, STOPPED, HALVINGS)
        u, f = trial, f_trial
        if t * np.abs(s).max() <= xtol * np.abs(u).max():
            return Row(u, f, it, CONVERGED, worst)
        if it >= max_iter:
            return Row(u, f, it, STOPPED, worst)


def solve(V, records, row_off, l2, U_init=None, max_iter=50, xtol=2.0 ** -30, hessian_dtype=np.float64):
    """All rows of a call: records int32 [N, 4] (u, i, j, z as fp32 bits), row_off [rows + 1] → list of Row."""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int32)).reshape(-1, 4)
    z = records[:, 3].copy().view(np.float32)
    out = []
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        out.append(solve_row(V, records[b:e, 1], records[b:e, 2], z[b:e], l2, None if U_init is None else U_init[r],
                             max_iter, xtol, hessian_dtype))
    return out


# ---- the inputs the fold-in tests share (tests/test_fold_in.py, tests/test_fold_in_cpu.py) ----
M_ITEMS = 97
LABELS = ("hard", "soft", "separable")


def row_lengths(T):
    return [0, 1, 3, 50, 1000, T - 1, T, T + 1, 2 * T + 3]


def make_case(d, labels, lengths, seed, start=False, m=M_ITEMS):
    """One ragged call: V ~ N(0, 1 / d) in fp32, per row a hidden u0 ~ N(0, 9 I), items i != j uniform, labels from
    sigmoid(u0 . delta): "hard" one Bernoulli draw, "soft" the mean of K = 4 draws (a row whose labels all come out 1/2
    gets 3/4 for its first: see below), "separable" the sign of u0 . delta.
    start: U_init ~ N(0, 100 I) in fp32 instead of None → (V, records int32 [N, 4], row_off int64, U_init or None)."""
    rng = np.random.default_rng(seed)
    V = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    rows = len(lengths)
    row_off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    N = int(row_off[-1])
    owner = np.repeat(np.arange(rows), lengths)
    i = rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, m - 1, N)) % m
    U0 = 3.0 * rng.standard_normal((rows, d))
    x = np.einsum("tk,tk->t", U0[owner], deltas(V, i, j))
    p = sigmoid(x)
    if labels == "hard":
        z = (rng.random(N) < p).astype(np.float32)
    elif labels == "soft":
        z = (rng.random((4, N)) < p).mean(0).astype(np.float32)
        for r in range(rows):       # all labels 1/2: the minimiser is exactly 0, which no relative step test certifies
            b, e = row_off[r], row_off[r + 1]
            if e > b and (z[b:e] == 0.5).all():
                z[b] = 0.75
    elif labels == "separable":
        z = (x > 0).astype(np.float32)
    else:
        raise ValueError(labels)
    rec = np.empty((N, 4), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = owner, i, j, z.view(np.int32)
    U_init = (10.0 * rng.standard_normal((rows, d))).astype(np.float32) if start else None
    return V, rec, row_off, U_init
