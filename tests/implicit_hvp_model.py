"""A plain numpy float64 model of mfcd_implicit_hvp_rows (include/mfcd.h), of mfcd/implicit.py's implicit_hvp and of the
block problems of mfcd/implicit_exact.py, written from the definitions: the weights w_ij = sigmoid'(a_j - a_i) over a
row's (admissible positive, negative) pairs as a dense [pos, neg] array, the Laplacian as a dense m x m matrix, the block
minimisers by Newton with dense Hessians.  Invalid rows are not modelled: the tests state their fills themselves."""
import functools

import numpy as np

import implicit_model as IM
from rank_entries_model import csr


def weights(a, P, N):
    """w [pos, neg] = sigmoid(v) sigmoid(-v), v = a_j - a_i, from exp(-|v|) only."""
    e = np.exp(-np.abs(a[N][None, :] - a[P][:, None]))
    return e / (1.0 + e) ** 2


def hvp_row(scores, y, pos, excl=(), coef=1.0):
    """One row: scores and direction [m] (used as f64), its observed and barred columns → (q, deg, mag) f64 [m]: the
    Laplacian applied to y, its diagonal, and the sums of magnitudes coef sum w |y_i - y_j| the tolerance is stated on."""
    a, y = np.asarray(scores, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = a.size
    P, N = IM.classes(m, pos, excl)
    q, deg, mag = np.zeros(m), np.zeros(m), np.zeros(m)
    if P.size * N.size == 0:
        return q, deg, mag
    w = weights(a, P, N)
    dy = y[P][:, None] - y[N][None, :]
    q[P], q[N] = coef * (w * dy).sum(1), -coef * (w * dy).sum(0)
    deg[P], deg[N] = coef * w.sum(1), coef * w.sum(0)
    mag[P], mag[N] = coef * (w * np.abs(dy)).sum(1), coef * (w * np.abs(dy)).sum(0)
    return q, deg, mag


def hvp_rows(S, Y, p_off, p_items, e_off=None, e_items=None, row_ids=None, coef=None):
    """S, Y [n, m] → (q, deg, mag) [rows, m] for valid lists indexed by requested row."""
    out = []
    for r in range(len(p_off) - 1):
        u = r if row_ids is None else row_ids[r]
        excl = () if e_off is None else e_items[e_off[r]:e_off[r + 1]]
        out.append(hvp_row(S[u], Y[u], p_items[p_off[r]:p_off[r + 1]], excl, 1.0 if coef is None else float(coef[r])))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def partners(m, pos, excl=()):
    """The number of pairs every column of a row takes part in: neg for a positive, pos for a negative, 0 for a barred
    column (and 1 where that is 0, as a divisor)."""
    P, N = IM.classes(m, pos, excl)
    k = np.zeros(m)
    k[P], k[N] = N.size, P.size
    return np.maximum(k, 1.0)


def laplacian(a, pos, excl=()):
    """The dense m x m Hessian of the row's risk sum in score space."""
    a = np.asarray(a, dtype=np.float64)
    m = a.size
    P, N = IM.classes(m, pos, excl)
    W = np.zeros((m, m))
    if P.size * N.size:
        W[np.ix_(P, N)] = weights(a, P, N)
        W = W + W.T
    return np.diag(W.sum(1)) - W


class Problem:
    """A table of observed items (lists of columns per user, optional barred lists) with its normaliser, in f64: the
    objective F of mfcd/implicit_exact.py, its gradients, its Hessian-vector product and the block minimisers."""

    def __init__(self, m, pos, excl=None, normalize="pairs", coef=None):
        self.m, self.pos, self.n = m, [np.asarray(p, dtype=np.int64) for p in pos], len(pos)
        self.excl = [np.zeros(0, dtype=np.int64)] * self.n if excl is None else [np.asarray(e, dtype=np.int64) for e in excl]
        self.classes = [IM.classes(m, p, e) for p, e in zip(self.pos, self.excl)]
        pn = np.array([P.size * N.size for P, N in self.classes], dtype=np.float64)
        self.paired = pn > 0
        c = IM.coefficients(np.stack((pn, np.ones(self.n)), 1), normalize)
        self.c = c if coef is None else np.where(self.paired, np.broadcast_to(np.asarray(coef, dtype=np.float64), (self.n,)), 0.0)

    def row_risk(self, a, u):
        P, N = self.classes[u]
        return float(IM.softplus(a[N][None, :] - a[P][:, None]).sum())

    def row_grad(self, a, u):
        P, N = self.classes[u]
        g = np.zeros(self.m)
        s = IM.sigmoid(a[N][None, :] - a[P][:, None])
        g[N], g[P] = s.sum(0), -s.sum(1)
        return g

    def objective(self, U, V, l2):
        A = U @ V.T
        return float(sum(self.c[u] * self.row_risk(A[u], u) for u in range(self.n))) + \
            0.5 * l2 * float((U * U).sum() + (V * V).sum())

    def score_grads(self, U, V):
        """[n, m], the normaliser applied."""
        A = U @ V.T
        return np.stack([self.c[u] * self.row_grad(A[u], u) for u in range(self.n)])

    def grads(self, U, V):
        G = self.score_grads(U, V)
        return G @ V, G.T @ U

    def hvp(self, U, V, dU, dV, gauss_newton=False):
        """→ (HU, HV, (mag [n, m], ymax [n], G [n, m])): the product with the Hessian of the risk, and what the tests'
        bound is made of."""
        A, Y = U @ V.T, dU @ V.T + U @ dV.T
        rows = [hvp_row(A[u], Y[u], self.pos[u], self.excl[u], self.c[u]) for u in range(self.n)]
        Q, mag = np.stack([r[0] for r in rows]), np.stack([r[2] for r in rows])
        G = self.score_grads(U, V)
        HU, HV = Q @ V, Q.T @ U
        if not gauss_newton:
            HU, HV = HU + G @ dV, HV + G.T @ dU
        return HU, HV, (mag, np.abs(Y).max(1), G)

    # ---- the block problems and their plain Newton solves with the dense Hessian ----
    def user_objective(self, u, V, r, l2):
        return self.c[r] * self.row_risk(V @ u, r) + 0.5 * l2 * float(u @ u)

    def user_grad(self, u, V, r, l2):
        return self.c[r] * (V.T @ self.row_grad(V @ u, r)) + l2 * u

    def solve_user(self, u0, V, r, l2, tol=1e-13, max_iter=60):
        V = np.asarray(V, dtype=np.float64)
        u = np.array(u0, dtype=np.float64)
        for it in range(max_iter):
            g = self.user_grad(u, V, r, l2)
            if np.linalg.norm(g) <= tol:
                return u, it
            H = self.c[r] * (V.T @ laplacian(V @ u, self.pos[r], self.excl[r]) @ V) + l2 * np.eye(u.size)
            p, t, f = np.linalg.solve(H, -g), 1.0, self.user_objective(u, V, r, l2)
            while self.user_objective(u + t * p, V, r, l2) > f + 1e-14 * abs(f) and t > 1e-10:   # f's own rounding
                t *= 0.5
            u = u + t * p
        raise AssertionError("the model's user solve did not converge")

    def item_objective(self, U, V, l2):
        return self.objective(U, V, l2) - 0.5 * l2 * float((U * U).sum())

    def item_grad(self, U, V, l2):
        return self.grads(U, V)[1] + l2 * V

    def solve_items(self, U, V0, l2, tol=1e-13, max_iter=60):
        """The minimiser over all of V by Newton with the dense (m d) x (m d) Hessian sum_u c_u kron(L_u, U_u U_u^T) +
        l2 I → (V, iterations)."""
        U = np.asarray(U, dtype=np.float64)
        V = np.array(V0, dtype=np.float64)
        m, d = V.shape
        for it in range(max_iter):
            g = self.item_grad(U, V, l2)
            if np.linalg.norm(g) <= tol:
                return V, it
            S = U @ V.T
            Ls = np.stack([self.c[u] * laplacian(S[u], self.pos[u], self.excl[u]).reshape(-1) for u in range(self.n)])
            outer = np.stack([np.outer(U[u], U[u]).reshape(-1) for u in range(self.n)])
            H = (Ls.T @ outer).reshape(m, m, d, d).transpose(0, 2, 1, 3).reshape(m * d, m * d)
            H[np.diag_indices(m * d)] += l2
            p, t, f = np.linalg.solve(H, -g.reshape(-1)).reshape(m, d), 1.0, self.item_objective(U, V, l2)
            while self.item_objective(U, V + t * p, l2) > f + 1e-14 * abs(f) and t > 1e-10:
                t *= 0.5
            V = V + t * p
        raise AssertionError("the model's item solve did not converge")

    def score_noise(self, U, V):
        """[n, m]: the worst-case error of the device's score gradient (normaliser applied) at the tables given.  The
        kernel's fp32 tolerance on the mean term, 2e-5 |g_c| + 2e-6 x the column's partners, and the rounding of the
        device's fp32 scores — at most (d + 1) 2^-24 sum_k |u_k v_ck| each, which moves g_c by at most twice that times
        the column's degree in the Laplacian."""
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        G = self.score_grads(U, V)
        A = U @ V.T
        delta = (U.shape[1] + 1) * 2.0 ** -24 * (np.abs(U) @ np.abs(V).T).max(1)
        out = np.zeros_like(G)
        for u in range(self.n):
            deg = np.diag(laplacian(A[u], self.pos[u], self.excl[u]))
            k = partners(self.m, self.pos[u], self.excl[u]) * (np.abs(G[u]) > 0)
            out[u] = 2e-5 * np.abs(G[u]) + self.c[u] * (2e-6 * k + 2.0 * delta[u] * deg)
        return out

    def user_noise(self, U, V):
        """Per user, the worst-case error of the device's block gradient: sum_c noise_c |V_c|_2."""
        return self.score_noise(U, V) @ np.linalg.norm(np.asarray(V, dtype=np.float64), axis=1)

    def item_noise(self, U, V):
        """The same for the item block, in the Frobenius norm: sum_u sum_c noise_uc |U_u|_2."""
        return float((self.score_noise(U, V).sum(1) * np.linalg.norm(np.asarray(U, dtype=np.float64), axis=1)).sum())


def step_inputs(m, k=8, d=3):
    """The step tests' inputs: default_rng(1), V and U* standard normal rounded to fp32; user u observes the items of the
    top 30 % of U*[u] V^T, each kept with probability 0.7, and a tenth of the others; user 1 has observed nothing and
    user 2 everything (no pair either way) → (Ustar, V, lists of observed items)."""
    rng = np.random.default_rng(1)
    V = rng.standard_normal((m, d)).astype(np.float32)
    Ustar = rng.standard_normal((k, d)).astype(np.float32)
    X = Ustar.astype(np.float64) @ V.astype(np.float64).T
    top = X >= np.quantile(X, 0.7, axis=1, keepdims=True)
    keep = (top & (rng.random((k, m)) < 0.7)) | (~top & (rng.random((k, m)) < 0.1))
    pos = [np.flatnonzero(keep[u]) for u in range(k)]
    pos[1], pos[2] = np.zeros(0, dtype=np.int64), np.arange(m)
    return Ustar, V, pos


def lists(pos):
    return csr([np.asarray(p) for p in pos])


GTOL, L2 = 1e-3, 3e-2       # the step tests' certificate and ridge


@functools.lru_cache(maxsize=None)
def user_minimisers(m):
    """(the problem, the model's minimiser of every user's row from zero, the worst-case gradient noise there)."""
    Ustar, V, pos = step_inputs(m)
    prob = Problem(m, pos)
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(3), V64, r, L2)[0] for r in range(len(pos))])
    return prob, Uopt, prob.user_noise(Uopt, V64)


@functools.lru_cache(maxsize=None)
def item_minimiser(m):
    """(the problem, the model's minimiser over V from zero with U = U*, the worst-case gradient noise there)."""
    Ustar, V, pos = step_inputs(m)
    prob = Problem(m, pos)
    U64 = Ustar.astype(np.float64)
    Vopt = prob.solve_items(U64, np.zeros((m, 3)), L2)[0]
    return prob, Vopt, prob.item_noise(U64, Vopt)
