"""CPU model of the ragged Hessian-vector entry (include/mfcd.h: mfcd_pair_ragged_hvp), of the table-level product
mfcd.ratings.ratings_hvp, of the ridge-regularised ratings objective
    F(U, V) = c * sum over the users of risk_u + (l2 / 2)(|U|^2 + |V|^2)
and of its two exact block steps (mfcd/ratings_exact.py), for the tests: numpy float64, the definitions written out.  The
row functions are pair_hvp_model's and ratings_model's applied to each CSR slice; skip-ties is the weight [x_e != x_l]."""
import numpy as np

import pair_hvp_model as HM
import ratings_model as RM


def tie_weights(x, skip):
    """[L, L] weights of a row's pairs: None (every pair weighs 1), or under skip-ties [x_e != x_l] (-0.0 equals +0.0)."""
    if not skip:
        return None
    x = np.asarray(x, dtype=np.float64)
    return (x[:, None] != x[None, :]).astype(np.float64)


def row_hvp(a, y, x, skip=False):
    """(q, deg, mag) of one row, float64 [L]: q_e = sum_l w s (y_e - y_l), deg_e = sum_l w s, mag_e = sum_l w s |y_e - y_l|
    over the other entries of the row, s = sigmoid'(a_e - a_l).  x is read under skip-ties only: without it a
    non-finite x changes nothing; a non-finite a or y (or x under skip) makes all three NaN."""
    return HM.pair_hvp(a, y, tie_weights(x, skip), x if skip else None)


def hvp(a, y, x, row_off, skip=False):
    """(q, deg, mag) over all entries."""
    out = [np.zeros(len(a)) for _ in range(3)]
    for sl in RM.rows_of(row_off):
        if sl.stop > sl.start:
            for o, v in zip(out, row_hvp(a[sl], y[sl], x[sl], skip)):
                o[sl] = v
    return tuple(out)


class Problem:
    """A ratings table (CSR arrays row_off, item, value), scale s and skip-ties; c = 1 / (sum of the users' supports) or
    `coef`.  U [n, d], V [m, d] are passed to every method."""

    def __init__(self, row_off, item, value, s, skip=False, coef=None):
        self.row_off, self.item = np.asarray(row_off, dtype=np.int64), np.asarray(item, dtype=np.int64)
        self.x = np.asarray(value, dtype=np.float64)
        self.s, self.skip = float(s), bool(skip)
        self.rows = RM.rows_of(self.row_off)
        self.lengths = np.diff(self.row_off)
        self.support = np.array([RM.row_support(self.x[sl], skip) for sl in self.rows], dtype=np.int64)
        self.c = 1.0 / self.support.sum() if coef is None else float(coef)

    # ---- entries ----
    def scores(self, U, V):
        return RM.dot(U, V, self.row_off, self.item)[0]

    def row_risk(self, a, r):
        sl = self.rows[r]
        return float(RM.row_sums(a, self.x[sl], self.s, self.skip)[0]) if sl.stop > sl.start else 0.0

    def score_grads(self, U, V):
        return RM.grad(self.scores(U, V), self.x, self.row_off, self.s, self.skip)

    def laplacian(self, a, r):
        return HM.laplacian(a, tie_weights(self.x[self.rows[r]], self.skip))

    # ---- the objective and the product ----
    def risk(self, U, V):
        a = self.scores(U, V)
        return self.c * sum(self.row_risk(a[sl], r) for r, sl in enumerate(self.rows))

    def objective(self, U, V, l2):
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        return self.risk(U, V) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum())

    def tables(self, coef, U, V):
        """(sum over a user's entries of coef_e V[item_e], sum over an item's entries of coef_e U[user_e])."""
        hu, hv = np.zeros_like(U), np.zeros_like(V)
        for r, sl in enumerate(self.rows):
            hu[r] = coef[sl] @ V[self.item[sl]]
            np.add.at(hv, self.item[sl], coef[sl][:, None] * U[r][None, :])
        return hu, hv

    def hvp(self, U, V, dU, dV, gauss_newton=False):
        """The Hessian of the risk at (U, V) applied to (dU, dV) → (HU, HV, parts): with y = dU[user] . V[item] +
        U[user] . dV[item], q = L y and g the score gradient, HU = c (q -> V by user + g -> dV by user), HV the mirror
        image; gauss_newton drops the g terms.  parts = (mag, y, g) per entry, for the tests' bounds."""
        U, V, dU, dV = (np.asarray(t, dtype=np.float64) for t in (U, V, dU, dV))
        a = self.scores(U, V)
        y = self.scores(dU, V) + self.scores(U, dV)
        q, _, mag = hvp(a, y, self.x, self.row_off, self.skip)
        g = RM.grad(a, self.x, self.row_off, self.s, self.skip)
        HU, HV = self.tables(q, U, V)
        if not gauss_newton:
            gU, gV = self.tables(g, dU, dV)
            HU, HV = HU + gU, HV + gV
        return self.c * HU, self.c * HV, (mag, y, g)

    # ---- the block problems and their plain Newton solves with the dense Hessian ----
    def user_objective(self, u, V, r, l2):
        sl = self.rows[r]
        return self.c * self.row_risk(V[self.item[sl]] @ u, r) + 0.5 * l2 * float(u @ u)

    def user_grad(self, u, V, r, l2):
        sl = self.rows[r]
        if sl.stop == sl.start:
            return l2 * u
        Vi = V[self.item[sl]]
        return self.c * (Vi.T @ RM.row_grad(Vi @ u, self.x[sl], self.s, self.skip)) + l2 * u

    def solve_user(self, u0, V, r, l2, tol=1e-11, max_iter=50):
        """The minimiser of user r's problem by Newton with the dense d x d Hessian c V_r^T L V_r + l2 I, halving the step
        until the objective does not rise → (u, iterations until |grad| <= tol).  tol: c makes the objective small
        (about 1e-2), so near the minimiser a step changes it by less than its own rounding; 1e-11 / l2 is still seven
        orders below the distances the tests resolve."""
        V = np.asarray(V, dtype=np.float64)
        u = np.array(u0, dtype=np.float64)
        Vi = V[self.item[self.rows[r]]]
        for it in range(max_iter):
            g = self.user_grad(u, V, r, l2)
            if np.linalg.norm(g) <= tol:
                return u, it
            H = l2 * np.eye(u.size)
            if len(Vi):
                H = H + self.c * (Vi.T @ self.laplacian(Vi @ u, r) @ Vi)
            p, t, f = np.linalg.solve(H, -g), 1.0, self.user_objective(u, V, r, l2)
            while self.user_objective(u + t * p, V, r, l2) > f * (1.0 + 1e-15) and t > 1e-10:
                t *= 0.5
            u = u + t * p
        raise AssertionError("the model's user solve did not converge")

    def item_objective(self, U, V, l2):
        return self.risk(U, V) + 0.5 * l2 * float((V * V).sum())

    def item_grad(self, U, V, l2):
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        return self.c * self.tables(self.score_grads(U, V), U, V)[1] + l2 * V

    def grads(self, U, V, l2=0.0):
        """(dF/dU, dF/dV): the block gradients of F (of the risk alone at l2 = 0)."""
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        gU, gV = self.tables(self.score_grads(U, V), U, V)
        return self.c * gU + l2 * U, self.c * gV + l2 * V

    def solve_items(self, U, V0, l2, tol=1e-11, max_iter=50):
        """The minimiser over all of V by Newton with the dense (m d) x (m d) Hessian: user r adds
        c L_r[e, l] U_r U_r^T to the block of (item_e, item_l) → (V, iterations)."""
        U = np.asarray(U, dtype=np.float64)
        V = np.array(V0, dtype=np.float64)
        m, d = V.shape
        for it in range(max_iter):
            g = self.item_grad(U, V, l2)
            if np.linalg.norm(g) <= tol:
                return V, it
            a = self.scores(U, V)
            H = np.zeros((m, d, m, d))
            for r, sl in enumerate(self.rows):
                if sl.stop - sl.start > 1:
                    it_r = self.item[sl]
                    H[np.ix_(it_r, np.arange(d), it_r, np.arange(d))] += \
                        self.c * self.laplacian(a[sl], r)[:, None, :, None] * np.outer(U[r], U[r])[None, :, None, :]
            H = H.reshape(m * d, m * d)
            H[np.diag_indices(m * d)] += l2
            p, t, f = np.linalg.solve(H, -g.reshape(-1)).reshape(m, d), 1.0, self.item_objective(U, V, l2)
            while self.item_objective(U, V + t * p, l2) > f * (1.0 + 1e-15) and t > 1e-10:
                t *= 0.5
            V = V + t * p
        raise AssertionError("the model's item solve did not converge")

    def user_noise(self, U, V):
        """Per user, the worst-case error of the device's block gradient from the pair kernel's fp32 tolerance:
        c sum over the user's entries of (2e-5 |g_e| + 2e-6 (L - 1)) |V[item_e]|_2."""
        V = np.asarray(V, dtype=np.float64)
        g = self.score_grads(U, V)
        vn = np.linalg.norm(V, axis=1)
        return np.array([self.c * float(((2e-5 * np.abs(g[sl]) + 2e-6 * max(sl.stop - sl.start - 1, 0)) * vn[self.item[sl]]).sum())
                         for sl in self.rows])


# ---- the exact-step inputs the GPU tests and the CPU test of their noise bound share ----
STEP_N, STEP_M, STEP_D, STEP_L2, STEP_GTOL = 12, 40, 3, 3e-2, 1e-3
EMPTY_USER, SINGLE_USER, LEVEL_USER = 2, 5, 7


def step_inputs(skip=False, p=0.5):
    """(U0, V fp32, users, items, values): X = U* V^T from default_rng(1), `structure.observe_ratings(X, p, levels=5)` on
    the CPU, then user 2 emptied, user 5 cut to its first rating and, for the skip-ties runs, user 7 cut to the ratings
    of its most frequent level (at least two entries: pairs, but none with different values; without skip-ties such a
    user has pairs and the minimiser 0, which no certificate relative to |u|_inf can reach, so it keeps its ratings
    there).  U0 is a second draw, the steps' start."""
    import structure as S
    import torch
    rng = np.random.default_rng(1)
    V = rng.standard_normal((STEP_M, STEP_D)).astype(np.float32)
    Ustar = rng.standard_normal((STEP_N, STEP_D)).astype(np.float32)
    U0 = (0.3 * rng.standard_normal((STEP_N, STEP_D))).astype(np.float32)
    X = (Ustar.astype(np.float64) @ V.astype(np.float64).T).astype(np.float32)
    data = S.observe_ratings(torch.from_numpy(X), p, levels=5)
    users, items, values = data.user.numpy().astype(np.int64), data.item.numpy().astype(np.int64), data.value.numpy()
    keep = users != EMPTY_USER
    keep &= (users != SINGLE_USER) | (np.arange(users.size) == np.flatnonzero(users == SINGLE_USER)[0])
    mine = values[users == LEVEL_USER]
    level = np.bincount(mine.astype(np.int64)).argmax()
    assert (mine == level).sum() >= 2
    if skip:
        keep &= (users != LEVEL_USER) | (values == level)
    return U0, V, users[keep], items[keep], values[keep]
