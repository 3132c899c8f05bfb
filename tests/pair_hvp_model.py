"""CPU model of the pair Hessian-vector kernels (include/mfcd.h: mfcd_pair_hvp_rows, mfcd_pair_law_hvp_rows), of the
table-level product mfcd.pairs.population_hvp, of the ridge-regularised population objective
    F(U, V) = R(U, V) + (l2 / 2)(|U|^2 + |V|^2)
and of its two exact block steps (mfcd/population.py), for the tests: numpy float64, the definitions written out.  The
risk and its gradient are pair_grad_model's and pair_law_model's; a law is pair_law_model's `spec` dict (None: the
plain risk), turned into each user's full [m, m] weight matrix."""
import numpy as np

import pair_grad_model as GM
import pair_law_model as LM
import pairs_model as M


def dsigmoid(v):
    """sigmoid'(v) = e / (1 + e)^2 with e = exp(-|v|): symmetric, no overflow."""
    e = np.exp(-np.abs(v))
    return e / (1.0 + e) ** 2


def curvature(a, w=None):
    """[m, m] float64: w_ij sigmoid'(a_i - a_j) with a zeroed diagonal (w None: every pair weighs 1)."""
    a = np.asarray(a, dtype=np.float64)
    S = dsigmoid(a[:, None] - a[None, :])
    if w is not None:
        S = S * w
    np.fill_diagonal(S, 0.0)
    return S


def pair_hvp(a, y, w=None, x=None):
    """(q, deg, mag) of one row, each float64 [m]: q_i = sum_j S_ij (y_i - y_j), deg_i = sum_j S_ij and the sum of the
    magnitudes mag_i = sum_j S_ij |y_i - y_j| (what a tolerance on q is relative to: q itself can cancel), by the m x m
    broadcast.  All NaN if a, y or x holds a non-finite entry."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64)
    rows = (a, y) if x is None else (a, y, np.asarray(x, dtype=np.float64))
    if not all(np.isfinite(r).all() for r in rows):
        return (np.full(a.size, np.nan),) * 3
    S = curvature(a, w)
    dy = y[:, None] - y[None, :]
    return (S * dy).sum(axis=1), S.sum(axis=1), (S * np.abs(dy)).sum(axis=1)


def laplacian(a, w=None):
    """The Hessian of the row's risk sum as a dense [m, m] matrix: diag(deg) - S."""
    S = curvature(a, w)
    return np.diag(S.sum(axis=1)) - S


# ---- the population objective over a whole model ----
class Problem:
    """U [n, d], V [m, d], X [n, m] (fp32 values), scale s, an optional law `spec` and user list: every user's weight
    matrix, and the normaliser c = 1 / (users x pairs) or 1 / (sum of the weights of the pairs i < j of all users)."""

    def __init__(self, X, s, spec=None, users=None):
        self.X32 = np.asarray(X, dtype=np.float32)
        self.X = self.X32.astype(np.float64)
        self.s, self.spec = float(s), spec
        n, m = self.X.shape
        self.m = m
        if spec is None:
            self.ids = np.arange(n) if users is None else np.asarray(users, dtype=np.int64)
            off = 1.0 - np.eye(m)
            self.w = [off] * len(self.ids)
            self.c = 1.0 / (len(self.ids) * (m * (m - 1) // 2))
        else:
            self.ids = LM._ids(spec, n, users)
            self.w = [LM.user_matrix(spec, self.X32, u) for u in self.ids]
            self.c = 1.0 / sum(w.sum() / 2.0 for w in self.w)

    def row_risk(self, a, r):
        """sum over i < j of w (softplus(da) - q da) of row r of the user list."""
        i, j = np.triu_indices(self.m, k=1)
        x = self.X[self.ids[r]]
        da, t = a[i] - a[j], self.s * (x[i] - x[j])
        return float((self.w[r][i, j] * (M.softplus(da) - M.sigmoid(t) * da)).sum())

    def row_grad(self, a, r):
        x = self.X[self.ids[r]]
        with np.errstate(over="ignore"):
            t = M.sigmoid(a[:, None] - a[None, :]) - M.sigmoid(self.s * (x[:, None] - x[None, :]))
        return (self.w[r] * t).sum(axis=1)

    def risk(self, U, V):
        S = np.asarray(U, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T
        return self.c * sum(self.row_risk(S[u], r) for r, u in enumerate(self.ids))

    def score_grads(self, U, V):
        S = np.asarray(U, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T
        return np.stack([self.row_grad(S[u], r) for r, u in enumerate(self.ids)])

    def objective(self, U, V, l2):
        return self.risk(U, V) + 0.5 * l2 * ((np.asarray(U, dtype=np.float64) ** 2).sum()
                                            + (np.asarray(V, dtype=np.float64) ** 2).sum())

    def grads(self, U, V, l2=0.0):
        """(dF/dU, dF/dV, G): the block gradients of F (of the risk alone at l2 = 0) and the score gradients."""
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        G = self.score_grads(U, V)
        dU = np.zeros_like(U)
        np.add.at(dU, self.ids, self.c * (G @ V))
        return dU + l2 * U, self.c * (G.T @ U[self.ids]) + l2 * V, G

    def hvp(self, U, V, dU, dV, gauss_newton=False):
        """The Hessian of the risk at (U, V) applied to (dU, dV) → (HU, HV, parts): with Y = dU V^T + U dV^T,
        HU = c (L Y V + G dV), HV = c ((L Y)^T U + G^T dU); gauss_newton drops the G terms.  parts = (mag, ymax, G): the
        per-entry sums of magnitudes of L Y, the largest |y| per row and the score gradients, for the tests' bounds."""
        U, V, dU, dV = (np.asarray(t, dtype=np.float64) for t in (U, V, dU, dV))
        S = U @ V.T
        Y = dU @ V.T + U @ dV.T
        rows = [pair_hvp(S[u], Y[u], self.w[r]) for r, u in enumerate(self.ids)]
        Q, mag = np.stack([r[0] for r in rows]), np.stack([r[2] for r in rows])
        G = self.score_grads(U, V)
        HU_rows, HV = Q @ V, Q.T @ U[self.ids]
        if not gauss_newton:
            HU_rows, HV = HU_rows + G @ dV, HV + G.T @ dU[self.ids]
        HU = np.zeros_like(U)
        np.add.at(HU, self.ids, self.c * HU_rows)
        return HU, self.c * HV, (mag, np.abs(Y[self.ids]).max(axis=1), G)

    # ---- the block problems and their plain Newton solves with the dense Hessian ----
    def user_objective(self, u, V, r, l2):
        return self.c * self.row_risk(V @ u, r) + 0.5 * l2 * float(u @ u)

    def user_grad(self, u, V, r, l2):
        return self.c * (V.T @ self.row_grad(V @ u, r)) + l2 * u

    def solve_user(self, u0, V, r, l2, tol=1e-13, max_iter=50):
        """The minimiser of row r's problem by Newton with the dense d x d Hessian c V^T L V + l2 I, halving the step
        until the objective does not rise → (u, iterations until |grad| <= tol)."""
        V = np.asarray(V, dtype=np.float64)
        u = np.array(u0, dtype=np.float64)
        for it in range(max_iter):
            g = self.user_grad(u, V, r, l2)
            if np.linalg.norm(g) <= tol:
                return u, it
            H = self.c * (V.T @ laplacian(V @ u, self.w[r]) @ V) + l2 * np.eye(u.size)
            p, t, f = np.linalg.solve(H, -g), 1.0, self.user_objective(u, V, r, l2)
            while self.user_objective(u + t * p, V, r, l2) > f and t > 1e-10:
                t *= 0.5
            u = u + t * p
        raise AssertionError("the model's user solve did not converge")

    def item_objective(self, U, V, l2):
        return self.risk(U, V) + 0.5 * l2 * float((V * V).sum())

    def item_grad(self, U, V, l2):
        return self.grads(U, V)[1] + l2 * V

    def solve_items(self, U, V0, l2, tol=1e-13, max_iter=50):
        """The minimiser over all of V by Newton with the dense (m d) x (m d) Hessian
        c sum_u kron(L_u, U_u U_u^T) + l2 I → (V, iterations)."""
        U = np.asarray(U, dtype=np.float64)
        V = np.array(V0, dtype=np.float64)
        m, d = V.shape
        for it in range(max_iter):
            g = self.item_grad(U, V, l2)
            if np.linalg.norm(g) <= tol:
                return V, it
            S = U @ V.T
            Ls = np.stack([laplacian(S[u], self.w[r]).reshape(-1) for r, u in enumerate(self.ids)])      # [k, m m]
            outer = np.stack([np.outer(U[u], U[u]).reshape(-1) for u in self.ids])                       # [k, d d]
            H = self.c * (Ls.T @ outer).reshape(m, m, d, d).transpose(0, 2, 1, 3).reshape(m * d, m * d)
            H[np.diag_indices(m * d)] += l2
            p, t, f = np.linalg.solve(H, -g.reshape(-1)).reshape(m, d), 1.0, self.item_objective(U, V, l2)
            while self.item_objective(U, V + t * p, l2) > f and t > 1e-10:
                t *= 0.5
            V = V + t * p
        raise AssertionError("the model's item solve did not converge")

    def user_noise(self, U, V):
        """Per user of the list, the worst-case error of the device's block gradient from the pair kernel's fp32
        tolerance: c sum_i (2e-5 |g_i| + 2e-6 (m - 1)) |V_i|_2."""
        V = np.asarray(V, dtype=np.float64)
        G = self.score_grads(U, V)
        return self.c * ((2e-5 * np.abs(G) + 2e-6 * (self.m - 1)) @ np.linalg.norm(V, axis=1))

    def item_noise(self, U, V):
        """The same for the item block, in the Frobenius norm: c sum_u sum_i (2e-5 |g_ui| + 2e-6 (m - 1)) |U_u|_2."""
        U = np.asarray(U, dtype=np.float64)
        G = self.score_grads(U, V)
        return self.c * float(((2e-5 * np.abs(G) + 2e-6 * (self.m - 1)).sum(axis=1) * np.linalg.norm(U[self.ids], axis=1)).sum())


def solver_inputs(m, k=8, d=3):
    """The step tests' inputs: default_rng(1), V and U* standard normal, X = U* V^T as fp32 → (Ustar, V, X), the tables
    rounded to fp32 so that the device and the model hold the same numbers."""
    rng = np.random.default_rng(1)
    V = rng.standard_normal((m, d)).astype(np.float32)
    Ustar = rng.standard_normal((k, d)).astype(np.float32)
    X = (Ustar.astype(np.float64) @ V.astype(np.float64).T).astype(np.float32)
    return Ustar, V, X
