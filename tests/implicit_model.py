"""A plain numpy float64 model of mfcd_implicit_rows (include/mfcd.h) and of mfcd/implicit.py's risk, written from the
definitions: the counts by brute force on the ordered keys, the sums and g from the formulas, the table gradients by f64
GEMM.  Invalid rows are not modelled: the tests state their fills themselves."""
import numpy as np

from rank_entries_model import best_keys


def classes(m, pos, excl):
    """→ (P, N): the row's admissible positives (ascending) and its negatives, as int64 column arrays."""
    barred = np.zeros(m, dtype=bool)
    barred[np.asarray(excl, dtype=np.int64)] = True
    observed = np.zeros(m, dtype=bool)
    observed[np.asarray(pos, dtype=np.int64)] = True
    return np.flatnonzero(observed & ~barred), np.flatnonzero(~observed & ~barred)


def softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def sigmoid(v):
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def row(scores, pos, excl=(), coef=1.0):
    """One row: fp32 scores [m], its observed and barred columns → (counts int64 [4], sum f64, g f64 [m])."""
    a32 = np.asarray(scores, dtype=np.float32)
    m = a32.size
    P, N = classes(m, pos, excl)
    keys = best_keys(a32).astype(np.int64)
    kp, kn = keys[P][:, None], keys[N][None, :]
    inverted = int(((kn < kp) | ((kn == kp) & (N[None, :] < P[:, None]))).sum())
    tied = int((kn == kp).sum())
    counts = np.array([P.size, N.size, inverted, tied], dtype=np.int64)
    g = np.zeros(m, dtype=np.float64)
    adm = np.concatenate((P, N))
    if not np.isfinite(a32[adm]).all():
        g[:] = np.nan
        return counts, np.nan, g
    a = a32.astype(np.float64)
    v = a[N][None, :] - a[P][:, None]                    # [pos, neg]
    s = sigmoid(v)
    g[N] = coef * s.sum(0)
    g[P] = -coef * s.sum(1)
    return counts, float(softplus(v).sum()), g


def rows(S, p_off, p_items, e_off=None, e_items=None, row_ids=None, coef=None):
    """S [n, m] → (counts [rows, 4], sums [rows], g [rows, m]) for valid lists indexed by requested row."""
    S = np.asarray(S, dtype=np.float32)
    nrows = len(p_off) - 1
    counts = np.zeros((nrows, 4), dtype=np.int64)
    sums = np.zeros(nrows)
    g = np.zeros((nrows, S.shape[1]))
    for r in range(nrows):
        excl = () if e_off is None else e_items[e_off[r]:e_off[r + 1]]
        counts[r], sums[r], g[r] = row(S[r if row_ids is None else row_ids[r]], p_items[p_off[r]:p_off[r + 1]], excl,
                                       1.0 if coef is None else float(coef[r]))
    return counts, sums, g


def coefficients(counts, normalize):
    """The per-user factor of the risk: 1 / total pairs, or 1 / (users with a pair x the user's pairs)."""
    pn = (counts[:, 0] * counts[:, 1]).astype(np.float64)
    has = pn > 0
    if normalize == "pairs":
        return np.where(has, 1.0 / pn.sum(), 0.0)
    return np.where(has, 1.0 / (has.sum() * np.maximum(pn, 1.0)), 0.0)


def risk(U, V, p_off, p_items, e_off=None, e_items=None, normalize="pairs"):
    """f64 tables → (risk, dU, dV): the scores are rounded to fp32 as the device's are, everything else is f64."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    S = (U @ V.T).astype(np.float32)
    counts, sums, _ = rows(S, p_off, p_items, e_off, e_items)
    coef = coefficients(counts, normalize)
    _, _, g = rows(S, p_off, p_items, e_off, e_items, coef=coef)
    return float((sums * coef).sum()), g @ V, g.T @ U


def risk_f64(U, V, p_off, p_items, e_off=None, e_items=None, normalize="pairs"):
    """The same risk with f64 scores (no rounding to fp32) → (risk, g [n, m] with the normaliser applied)."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    A = U @ V.T
    n, m = A.shape
    R, pn, G = np.zeros(n), np.zeros(n), np.zeros((n, m))
    for u in range(n):
        excl = () if e_off is None else e_items[e_off[u]:e_off[u + 1]]
        P, N = classes(m, p_items[p_off[u]:p_off[u + 1]], excl)
        v = A[u][N][None, :] - A[u][P][:, None]
        s = sigmoid(v)
        R[u], pn[u] = softplus(v).sum(), P.size * N.size
        G[u, N], G[u, P] = s.sum(0), -s.sum(1)
    coef = coefficients(np.stack((pn, np.ones(n)), 1), normalize)
    return float((R * coef).sum()), G * coef[:, None]


def adam_fit(U, V, p_off, p_items, steps, lr, e_off=None, e_items=None, normalize="pairs", b1=0.9, b2=0.999, eps=1e-8):
    """`steps` steps of torch.optim.Adam (no weight decay) on `risk` in f64 → (U, V, the risk before every step and
    after the last)."""
    U, V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
    mom = [np.zeros_like(U), np.zeros_like(V)]
    var = [np.zeros_like(U), np.zeros_like(V)]
    seen = []
    for t in range(1, steps + 1):
        r, dU, dV = risk(U, V, p_off, p_items, e_off, e_items, normalize)
        seen.append(r)
        for k, (W, gW) in enumerate(((U, dU), (V, dV))):
            mom[k] = b1 * mom[k] + (1 - b1) * gW
            var[k] = b2 * var[k] + (1 - b2) * gW * gW
            W -= lr * (mom[k] / (1 - b1 ** t)) / (np.sqrt(var[k] / (1 - b2 ** t)) + eps)
    seen.append(risk(U, V, p_off, p_items, e_off, e_items, normalize)[0])
    return U, V, seen
