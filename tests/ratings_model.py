"""CPU model of the ragged entries (include/mfcd.h: mfcd_pair_ragged_stats, mfcd_pair_ragged_grad, mfcd_ragged_dot,
mfcd_ragged_gather_sum) and of the ratings risk built on them, for the tests: numpy float64, a loop over the rows that
applies the row functions of pairs_model / pair_grad_model to each CSR slice.

Skip-ties: a pair tied in x lies inside exactly one group of equal x values, and inside such a group every pair is tied.
So "the row without its tied pairs" is the row's value minus the values of its groups taken as rows of their own: the same
row functions again, nothing restated."""
import numpy as np

import pair_grad_model as GM
import pairs_model as M


def rows_of(row_off):
    return [slice(int(b), int(e)) for b, e in zip(row_off[:-1], row_off[1:])]


def tie_groups(x):
    """Index arrays of the groups of equal values with more than one member (-0.0 equals +0.0)."""
    x = np.asarray(x, dtype=np.float64)
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    return [np.flatnonzero(inv == k) for k in np.flatnonzero(cnt > 1)]


def row_sums(a, x, scale, skip_ties=False):
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = M.pair_sums(a, x, scale)
    if skip_ties and np.isfinite(out).all():
        for g in tie_groups(x):
            out = out - M.pair_sums(a[g], x[g], scale)
    return out


def row_grad(a, x, scale, skip_ties=False):
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = GM.pair_grad(a, x, scale)
    if skip_ties and np.isfinite(out).all():
        for g in tie_groups(x):
            out[g] -= GM.pair_grad(a[g], x[g], scale)
    return out


def row_support(x, skip_ties=False):
    L = len(x)
    n0 = L * (L - 1) // 2
    return n0 - sum(len(g) * (len(g) - 1) // 2 for g in tie_groups(x)) if skip_ties else n0


def stats(a, x, row_off, scale, skip_ties=False):
    """(counts int64 [rows, 4], sums f64 [rows, 4], support int64 [rows])."""
    sl = rows_of(row_off)
    counts = np.array([M.pair_counts(a[s], x[s]) for s in sl], dtype=np.int64).reshape(-1, 4)
    sums = np.array([row_sums(a[s], x[s], scale, skip_ties) for s in sl], dtype=np.float64).reshape(-1, 4)
    return counts, sums, np.array([row_support(x[s], skip_ties) for s in sl], dtype=np.int64)


def grad(a, x, row_off, scale, skip_ties=False):
    out = np.zeros(len(a), dtype=np.float64)
    for s in rows_of(row_off):
        out[s] = row_grad(a[s], x[s], scale, skip_ties)
    return out


def dot(R, C, row_off, idx):
    """(a, sum of |terms|) per entry: a_e = R[r] . C[idx_e]."""
    R, C = np.asarray(R, dtype=np.float64), np.asarray(C, dtype=np.float64)
    a, mag = np.zeros(len(idx)), np.zeros(len(idx))
    for r, s in enumerate(rows_of(row_off)):
        terms = R[r][None, :] * C[idx[s]]
        a[s], mag[s] = terms.sum(1), np.abs(terms).sum(1)
    return a, mag


def gather_sum(T, row_off, idx, coef, perm=None):
    """(out [rows, d], sum of |terms| [rows, d]): out[r] = sum over the row's entries of coef[perm[e] or e] T[idx_e]."""
    T, coef = np.asarray(T, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    rows = len(row_off) - 1
    out, mag = np.zeros((rows, T.shape[1])), np.zeros((rows, T.shape[1]))
    for r, s in enumerate(rows_of(row_off)):
        c = coef[s] if perm is None else coef[perm[s]]
        terms = c[:, None] * T[idx[s]]
        out[r], mag[r] = terms.sum(0), np.abs(terms).sum(0)
    return out, mag


def ratings_risk(U, V, row_off, item, value, s, skip_ties=False):
    """sum over the rows of the risk sums / sum over the rows of the supports."""
    a, _ = dot(U, V, row_off, item)
    _, sums, support = stats(a, np.asarray(value, dtype=np.float64), row_off, s, skip_ties)
    return sums[:, 0].sum() / support.sum()


def ratings_grad(U, V, row_off, item, value, s, skip_ties=False):
    """(dRisk/dU, dRisk/dV, g): the gradient of ratings_risk and the per-entry score gradients it is made of."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    x = np.asarray(value, dtype=np.float64)
    a, _ = dot(U, V, row_off, item)
    g = grad(a, x, row_off, s, skip_ties)
    c = 1.0 / sum(row_support(x[sl], skip_ties) for sl in rows_of(row_off))
    dU, dV = np.zeros_like(U), np.zeros_like(V)
    for r, sl in enumerate(rows_of(row_off)):
        dU[r] = c * (g[sl] @ V[item[sl]])
        np.add.at(dV, item[sl], c * g[sl][:, None] * U[r][None, :])
    return dU, dV, g


def fit(U, V, row_off, item, value, s, steps, lr, weight_decay=0.0, log_every=0, skip_ties=False):
    """pair_grad_model.fit on ratings_risk → (U, V, steps at each log point, risks there)."""
    opt = GM.Adam([U, V], lr, weight_decay=weight_decay)
    at, risks = [], []
    for t in range(steps):
        if log_every and t % log_every == 0:
            at.append(t)
            risks.append(ratings_risk(opt.p[0], opt.p[1], row_off, item, value, s, skip_ties))
        dU, dV, _ = ratings_grad(opt.p[0], opt.p[1], row_off, item, value, s, skip_ties)
        opt.step([dU, dV])
    if log_every:
        at.append(steps)
        risks.append(ratings_risk(opt.p[0], opt.p[1], row_off, item, value, s, skip_ties))
    return opt.p[0], opt.p[1], at, risks
