"""CPU model of the per-user D-optimal comparison design (mfcd/design.py: user_design), for the tests: numpy float64, one
user at a time, the algorithm of the module's docstring written out with every quantity formed by the k x k broadcast.

    maximise  Phi(xi) = log det(M0 + M(xi)),   M(xi) = sum_p xi_p s_p delta_p delta_p^T,
    s_p = sigmoid'(a_i - a_j),  delta_p = b_i - b_j,  over probability measures xi on the admissible pairs p = {i, j}.

Pairwise Frank-Wolfe: the start measure is the law's own normalised information, kept as one dense atom of mass `rest`;
per iteration the pair with the largest gradient g_p = s_p delta_p^T P delta_p, P = (M0 + M)^-1, receives mass from the
held atom with the smallest gradient tr(P A_q); the step gamma in [0, w_q] by bisection on the sign of
phi'(gamma) = tr((C + gamma D)^-1 D), a trial point that does not factor counting as phi' < 0.  gap = max_p g_p - tr(P M)
bounds Phi* - Phi(xi) from above."""
import numpy as np

import pair_hvp_model as HM

BISECTIONS = 50


def _chol(C):
    try:
        return np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        return None


def _logdet(C):
    L = _chol(C)
    return np.nan if L is None else 2.0 * np.log(np.diag(L)).sum()


def pair_terms(a, B, w=None):
    """(S [k, k] curvature with a zero diagonal, D [k, k, d] differences, adm [k, k], start [d, d]: the law's normalised
    information sum_{i<j} w s delta delta^T / sum_{i<j} w)."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    k = a.size
    off = 1.0 - np.eye(k)
    W = off if w is None else np.asarray(w, dtype=np.float64) * off
    S = HM.curvature(a)
    D = B[:, None, :] - B[None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        start = 0.5 * np.einsum("ij,ijp,ijq->pq", S * W, D, D) / (0.5 * W.sum())
    return S, D, W > 0, start


def gradients(S, D, adm, P):
    """g_p for every ordered pair, -inf where not admissible."""
    return np.where(adm, S * np.einsum("ijp,pq,ijq->ij", D, P, D), -np.inf)


def step_length(C, Dm, top):
    """argmax over gamma in [0, top] of log det(C + gamma Dm) by bisection on the sign of the derivative."""
    def slope(gm):
        L = _chol(C + gm * Dm)
        if L is None:
            return -1.0
        Y = np.linalg.solve(L, Dm)
        return np.trace(np.linalg.solve(L.T, Y))

    if slope(top) >= 0:
        return top
    lo, hi = 0.0, top
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        if slope(mid) > 0:
            lo = mid
        else:
            hi = mid
    return lo


def design_row(a, B, w=None, prior=None, gtol=1e-3, max_iter=300):
    """One user's design → dict(pairs [(i, j)], weights, rest, info, logdet, logdet_start, gap, iters, status, start).
    prior: None, a scalar tau (M0 = tau I) or [d, d]."""
    B = np.asarray(B, dtype=np.float64)
    d = B.shape[1]
    M0 = np.zeros((d, d)) if prior is None else prior * np.eye(d) if np.ndim(prior) == 0 else np.asarray(prior, dtype=np.float64)
    S, D, adm, start = pair_terms(a, B, w)
    nan = dict(pairs=[], weights=[], rest=np.nan, info=np.full((d, d), np.nan), logdet=np.nan, logdet_start=np.nan,
               gap=np.nan, iters=0, status=2, start=start)
    if not np.isfinite(start).all() or _chol(M0 + start) is None:
        return nan
    atom = lambda p: S[p] * np.outer(D[p], D[p])
    held, rest, iters = {}, 1.0, 0                       # held: pair (i < j) -> mass, in the order they were first taken
    while True:
        M = rest * start + sum(wq * atom(p) for p, wq in held.items())
        C = M0 + M
        P = np.linalg.inv(C)
        g = gradients(S, D, adm, P)
        i, j = np.unravel_index(np.argmax(g), g.shape)
        new = (min(i, j), max(i, j))
        gap = g[new] - np.trace(P @ M)
        if gap <= gtol * d:
            status = 0
            break
        if iters == max_iter:
            status = 1
            break
        grads = {p: np.trace(P @ atom(p)) for p, wq in held.items() if wq > 0}
        if rest > 0:
            grads["rest"] = np.trace(P @ start)
        q = min(grads, key=grads.get)
        top = rest if q == "rest" else held[q]
        gm = step_length(C, atom(new) - (start if q == "rest" else atom(q)), top)
        if q == "rest":
            rest = rest - gm
        else:
            held[q] = held[q] - gm
        held[new] = held.get(new, 0.0) + gm
        iters += 1
    pairs = [p for p, wq in held.items() if wq > 0]
    return dict(pairs=pairs, weights=[held[p] for p in pairs], rest=rest, info=M, logdet=_logdet(C),
                logdet_start=_logdet(M0 + start), gap=gap, iters=iters, status=status, start=start)


def kkt(a, B, info, w=None, prior=None):
    """(max_p g_p, tr(P M)) at a returned information matrix, by brute force over the admissible pairs."""
    B = np.asarray(B, dtype=np.float64)
    d = B.shape[1]
    M0 = np.zeros((d, d)) if prior is None else prior * np.eye(d) if np.ndim(prior) == 0 else np.asarray(prior, dtype=np.float64)
    S, D, adm, _ = pair_terms(a, B, w)
    P = np.linalg.inv(M0 + info)
    return gradients(S, D, adm, P).max(), np.trace(P @ info)


def uniform_efficiency(a, B, res):
    """exp((Phi(start) - Phi(design)) / d): the D-efficiency of the start measure against the design found."""
    return float(np.exp((res["logdet_start"] - res["logdet"]) / np.asarray(B).shape[1]))
