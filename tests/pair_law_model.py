"""CPU model of the pair-law kernels (include/mfcd.h: mfcd_pair_law_stats_rows, mfcd_pair_law_grad_rows), of the globally
normalised population risk under a law and of the fit on it, for the tests: numpy float64, the definitions written out.
The per-pair terms are pairs_model's, the Adam step pair_grad_model's.

A law is a plain dict here (`spec`): alpha, beta [k]; labels [k] or [n, k]; margin; columns [k] or [n, k]; users — each
may be None / absent.  `attempt_law` enumerates, per strategy, the ordered law P(i, j | u) of one attempt of the
reference's sampler, line by line, independently of mfcd.pairs.strategy_law."""
import functools

import numpy as np

import pair_grad_model as GM
import pairs_model as M


def floor32(margin):
    """The largest fp32 <= margin."""
    f = np.float32(margin)
    return np.nextafter(f, np.float32(-np.inf)) if float(f) > margin else f


def weights(x, alpha=None, beta=None, margin=None, labels=None):
    """[m, m] float64, symmetric, zero diagonal: w_ij of the header.  The alpha / beta product in f64 from the fp32
    inputs; the margin decision on the fp32 difference of x against the rounded-down fp32 margin."""
    x = np.asarray(x, dtype=np.float32)
    m = x.size
    if alpha is None:
        w = np.ones((m, m))
    else:
        a, b = np.asarray(alpha, dtype=np.float32).astype(np.float64), np.asarray(beta, dtype=np.float32).astype(np.float64)
        w = a[:, None] * b[None, :] + a[None, :] * b[:, None]
    if margin is not None:
        with np.errstate(invalid="ignore"):
            d = np.abs(x[:, None] - x[None, :])                   # fp32
            w = w * (d <= floor32(margin))
    if labels is not None:
        lab = np.asarray(labels)
        w = w * (lab[:, None] != lab[None, :])
    np.fill_diagonal(w, 0.0)
    return w


@functools.lru_cache(maxsize=8)
def _pairs_of(m):
    return np.triu_indices(m, k=1)


def law_row(a, x, scale, w):
    """(support, [W, risk, bayes_risk, exp_acc, bayes_acc] over the pairs i < j, g [m]) of one row, with
    g_i = sum over j != i of w_ij (sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j))) by the m x m broadcast.  Five NaN and
    an all-NaN g for a non-finite row; its support is still counted."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    i, j = _pairs_of(a.size)
    wp = w[i, j]
    support = int((wp > 0).sum())
    if not (np.isfinite(a).all() and np.isfinite(x).all()):
        return support, np.full(5, np.nan), np.full(a.size, np.nan)
    da = a[i] - a[j]
    t = scale * (x[i] - x[j])
    q = M.sigmoid(t)
    terms = (M.softplus(da) - q * da, M.softplus(t) - q * t, np.where(da > 0, q, np.where(da < 0, 1.0 - q, 0.5)),
             np.maximum(q, 1.0 - q))
    sums = np.array([wp.sum()] + [(wp * term).sum() for term in terms])
    with np.errstate(over="ignore"):                      # exp(+large) = inf gives sigmoid = 0, which is right
        g = (w * (M.sigmoid(a[:, None] - a[None, :]) - M.sigmoid(scale * (x[:, None] - x[None, :])))).sum(axis=1)
    return support, sums, g


def law_sums(a, x, scale, w):
    return law_row(a, x, scale, w)[:2]


def law_grad(a, x, scale, w):
    return law_row(a, x, scale, w)[2]


# ---- a law over a whole model ----
def _row_of(v, u):
    return None if v is None else (v[u] if np.ndim(v) == 2 else v)


def user_parts(spec, X32, u):
    """(columns of user u, the [k, k] weights of its restricted truth row)."""
    m = X32.shape[1]
    cols = _row_of(spec.get("columns"), u)
    cols = np.arange(m) if cols is None else np.asarray(cols, dtype=np.int64)
    return cols, weights(X32[u][cols], spec.get("alpha"), spec.get("beta"), spec.get("margin"),
                         _row_of(spec.get("labels"), u))


def user_matrix(spec, X32, u):
    """The law of user u as a full [m, m] weight matrix over the items (a column named twice adds)."""
    cols, w = user_parts(spec, X32, u)
    full = np.zeros((X32.shape[1],) * 2)
    np.add.at(full, (cols[:, None], cols[None, :]), w)
    return full


def _ids(spec, n, users):
    if users is not None:
        return np.asarray(users, dtype=np.int64)
    return np.arange(n) if spec.get("users") is None else np.asarray(spec["users"], dtype=np.int64)


def population(U, V, X32, s, spec, users=None):
    """→ (risk, dRisk/dU, dRisk/dV, G [k, m]: the score gradients before the 1 / W coefficient, Wi [k, m]: each item's
    weight total, W) of the globally normalised risk sum_u sum_{i<j} w l / sum_u sum_{i<j} w."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    X32 = np.asarray(X32, dtype=np.float32)
    ids = _ids(spec, U.shape[0], users)
    S = U @ V.T
    G, Wi = np.zeros((len(ids), V.shape[0])), np.zeros((len(ids), V.shape[0]))
    risk = W = 0.0
    for r, u in enumerate(ids):
        cols, w = user_parts(spec, X32, u)
        a, x = S[u][cols], X32[u][cols].astype(np.float64)
        _, sums, g = law_row(a, x, s, w)
        W += sums[0]
        risk += sums[1]
        np.add.at(G[r], cols, g)
        np.add.at(Wi[r], cols, w.sum(axis=1))
    dU = np.zeros_like(U)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.add.at(dU, ids, (G @ V) / W)
        return risk / W, dU, (G.T @ U[ids]) / W, G, Wi, W


def bayes_risk(X32, s, spec):
    X32 = np.asarray(X32, dtype=np.float32)
    tot = np.zeros(5)
    for u in _ids(spec, X32.shape[0], None):
        cols, w = user_parts(spec, X32, u)
        x = X32[u][cols].astype(np.float64)
        tot += law_sums(x, x, s, w)[1]
    return tot[2] / tot[0]


def fit(U, V, X32, s, spec, steps, lr, weight_decay=0.0, log_every=0):
    """pair_grad_model.fit on the law's risk → (U, V, steps at the log points, risks there)."""
    opt = GM.Adam([U, V], lr, weight_decay=weight_decay)
    at, risks = [], []
    for t in range(steps):
        risk, dU, dV = population(opt.p[0], opt.p[1], X32, s, spec)[:3]
        if log_every and t % log_every == 0:
            at.append(t)
            risks.append(risk)
        opt.step([dU, dV])
    if log_every:
        at.append(steps)
        risks.append(population(opt.p[0], opt.p[1], X32, s, spec)[0])
    return opt.p[0], opt.p[1], at, risks


# ---- the reference's attempt laws, enumerated ----
def attempt_law(strategy, X32, u, num_triplets=None, probs=None, k=None, clusters=None, top_items=None):
    """P(i, j | u) of ONE attempt of the reference's sampler for user u, as an [m, m] matrix over ordered pairs, up to the
    factor that does not depend on (i, j); rejected attempts (i == j, outside the margin) have probability 0.
    generation_data.py of the reference, by line:
      random      22-24   i, j uniform in [0, m), i != j
      proximity   36-41   i uniform among the k largest of x, j uniform among the k smallest, i != j
      margin      67-73   i, j uniform, i != j, |x_i - x_j| <= margin (fp32 difference, f64 threshold of 56-57)
      variance    95      multinomial(probs, 2, replacement=False): p_i then p_j / (1 - p_i)
      popularity  124     choice(size=2, replace=False, p): the same sequential law
      svd         169     an ordered pair of distinct items, uniform among top_items
      top_k       208-213 i uniform among the k largest, j redrawn until != i: uniform among the others
      cluster     241-245 an ordered pair of distinct clusters uniform, i uniform in the first, j in the second"""
    x = np.asarray(X32, dtype=np.float32)[u]
    m = x.size
    off = 1.0 - np.eye(m)
    if strategy == "random":
        return off / m ** 2
    if strategy == "proximity":
        top, bottom = np.argsort(-x, kind="stable")[:k], np.argsort(x, kind="stable")[:k]
        P = np.zeros((m, m))
        P[np.ix_(top, bottom)] = 1.0 / k ** 2
        return P * off
    if strategy == "margin":
        n = np.shape(X32)[0]
        head = np.asarray(X32, dtype=np.float32)[:min(10, n)]
        margin = np.mean(head.max(axis=1) - head.min(axis=1)) * num_triplets / (n * m)
        return off / m ** 2 * (np.abs(x[:, None] - x[None, :]).astype(np.float64) <= margin)
    if strategy in ("variance", "popularity"):
        p = np.asarray(probs, dtype=np.float64)
        return off * p[:, None] * p[None, :] / (1.0 - p[:, None])
    if strategy == "svd":
        P = np.zeros((m, m))
        P[np.ix_(top_items, top_items)] = 1.0 / (len(top_items) * (len(top_items) - 1))
        return P * off
    if strategy == "top_k":
        top = np.argsort(-x, kind="stable")[:k]
        P = np.zeros((m, m))
        P[np.ix_(top, top)] = 1.0 / (k * (k - 1))
        return P * off
    if strategy == "cluster":
        lab = np.asarray(clusters)
        K = int(lab.max()) + 1
        size = np.bincount(lab, minlength=K).astype(np.float64)
        P = (lab[:, None] != lab[None, :]) / (K * (K - 1)) / size[lab][:, None] / size[lab][None, :]
        return P * off
    raise ValueError(strategy)
