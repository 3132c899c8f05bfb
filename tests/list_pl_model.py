"""The numpy f64 model of the Plackett–Luce list loss (include/mfcd.h: mfcd_list_pl) the tests hold the kernel to.  A row
is a list of scores in rank order, best first; `depth` of its positions are ranked, stages = min(depth, L - 1).  Both sums
are np.logaddexp.accumulate: lse backwards over the scores, N forwards over -lse of the stages."""
import numpy as np


def stages_of(L, depth=None):
    depth = L if depth is None else int(depth)
    return max(min(depth, L - 1), 0)


def row(a, depth=None):
    """→ (loss, stages, hits, g) of one list; a non-finite score gives (NaN, -1, -1, all NaN)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    L = a.size
    stages = stages_of(L, depth)
    if not np.isfinite(a).all():
        return np.nan, -1, -1, np.full(L, np.nan)
    if stages == 0:
        return 0.0, 0, 0, np.zeros(L)
    lse = np.logaddexp.accumulate(a[::-1])[::-1]
    loss = float((lse[:stages] - a[:stages]).sum())
    neg = np.full(L, -np.inf)
    neg[:stages] = -lse[:stages]
    N = np.logaddexp.accumulate(neg)
    g = np.exp(a + N)
    g[:stages] -= 1.0
    suffix_max = np.maximum.accumulate(a[::-1])[::-1]
    hits = int((a[:stages] >= suffix_max[:stages]).sum())
    return loss, stages, hits, g


def rows(a, row_off, depth=None):
    """Every row of a CSR layout → (loss f64 [rows], counts int64 [rows, 2], g f64 [entries])."""
    a = np.asarray(a, dtype=np.float64)
    n = len(row_off) - 1
    loss, counts, g = np.zeros(n), np.zeros((n, 2), dtype=np.int64), np.zeros(a.size)
    for r in range(n):
        b, e = int(row_off[r]), int(row_off[r + 1])
        loss[r], counts[r, 0], counts[r, 1], g[b:e] = row(a[b:e], None if depth is None else depth[r])
    return loss, counts, g


def uniform_loss(L, depth=None):
    """The loss of the all-equal model: sum over the stages of log(L - k)."""
    return float(np.log(L - np.arange(stages_of(L, depth), dtype=np.float64)).sum())


def risk(U, V, user, item, row_off, depth=None):
    """The mean negative log-likelihood per choice of the f64 tables on the lists and its gradients → (risk, dU, dV),
    g carried to the tables by numpy gathers."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    a = (U[user] * V[item]).sum(1)
    loss, counts, g = rows(a, row_off, depth)
    total = counts[:, 0].sum()
    dU, dV = np.zeros_like(U), np.zeros_like(V)
    np.add.at(dU, user, g[:, None] * V[item])
    np.add.at(dV, item, g[:, None] * U[user])
    return loss.sum() / total, dU / total, dV / total
