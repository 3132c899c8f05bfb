"""CPU model of the list Hessian-vector entry (include/mfcd.h: mfcd_list_pl_hvp), of the table-level product
mfcd.lists.pl_hvp, of the ridge-regularised Plackett–Luce objective
    F(U, V) = c * sum over the users of loss_u + (l2 / 2)(|U|^2 + |V|^2)
and of its exact user step (mfcd/lists_exact.py), for the tests: numpy, float64 in and out.  The row function shares nothing with the
kernel's (max, sum, payload) triples: y is split into its positive and negative parts and every sum is a
np.logaddexp.accumulate of logarithms, backwards over the entries and forwards over the stages, as list_pl_model.row
forms the gradient.  `dense` builds the Hessian from the definition, softmax by softmax."""
import numpy as np

import list_pl_model as LM


# The sums are held as logarithms, numbers of the size of the scores: in f64 a score of 3000 costs every one of them
# ulp(3000) = 4.5e-13, four thousand of the 2^-53 the tests' bounds count in, and the row function would be a worse
# witness than the kernel it judges.  They are formed in numpy's widest float instead (x86-64: 64 bits of mantissa, so
# ulp(3000) = 2.2e-16; a platform without one falls back to f64) and returned as f64.
WIDE = np.longdouble


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(x)


def row(a, y, depth=None):
    """→ (q, deg, scale, psum) of one list, float64 [L]:
        q_l = sum_k p_{k,l} (y_l - ybar_k),   deg_l = sum_k p_{k,l} (1 - p_{k,l})        over the stages k <= l
        scale_l = sum_k p_{k,l} (|y_l| + sum_j p_{k,j} |y_j|),   psum_l = sum_k p_{k,l}
    the last two the sizes the tests' bounds are stated in.  A non-finite score or y makes all four NaN."""
    a, y = np.asarray(a, dtype=WIDE).reshape(-1), np.asarray(y, dtype=WIDE).reshape(-1)
    L = a.size
    stages = LM.stages_of(L, depth)
    if not (np.isfinite(a).all() and np.isfinite(y).all()):
        return tuple(np.full(L, np.nan) for _ in range(4))
    if stages == 0:
        return tuple(np.zeros(L) for _ in range(4))
    return tuple(np.asarray(v, dtype=np.float64) for v in _row(a, y, L, stages))


def _row(a, y, L, stages):
    back = lambda v: np.logaddexp.accumulate(v[::-1])[::-1]                   # noqa: E731

    def fwd(v):                                                               # over the stages only
        w = np.full(L, -np.inf, dtype=WIDE)
        w[:stages] = v[:stages]
        return np.logaddexp.accumulate(w)

    lse = back(a)
    N = fwd(-lse)
    psum = np.exp(a + N)
    # log of sum_{j >= k} exp(a_j) y+_j, of y-_j and of |y_j|; minus 2 lse_k, summed forwards: sum_k p_{k,l} ybar+-_k / exp(a_l)
    parts = [np.exp(a + fwd(back(a + _log(v)) - 2.0 * lse)) for v in (np.maximum(y, 0.0), np.maximum(-y, 0.0), np.abs(y))]
    q = y * psum - (parts[0] - parts[1])
    deg = np.maximum(psum - np.exp(2.0 * a + fwd(-2.0 * lse)), 0.0)
    scale = np.abs(y) * psum + parts[2]
    return q, deg, scale, psum


def rows(a, y, row_off, depth=None):
    """Every row of a CSR layout → (q, deg, scale, psum), float64 [entries]."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = [np.zeros(a.size) for _ in range(4)]
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        for o, v in zip(out, row(a[b:e], y[b:e], None if depth is None else depth[r])):
            o[b:e] = v
    return tuple(out)


def dense(a, depth=None):
    """The Hessian of a short row's loss in its scores from the definition: sum over the stages of diag(p_k) - p_k p_k^T,
    p_k the softmax of a[k:] (shifted by its maximum), zero before k."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    L = a.size
    H = np.zeros((L, L))
    for k in range(LM.stages_of(L, depth)):
        p = np.zeros(L)
        e = np.exp(a[k:] - a[k:].max())
        p[k:] = e / e.sum()
        H += np.diag(p) - np.outer(p, p)
    return H


class Problem:
    """Ranked lists as CSR arrays (row_off, item in rank order, depth per user); c = 1 / (sum of the users' stages) or
    `coef`.  U [n, d], V [m, d] are passed to every method."""

    def __init__(self, row_off, item, depth, coef=None):
        self.row_off, self.item = np.asarray(row_off, dtype=np.int64), np.asarray(item, dtype=np.int64)
        self.depth = np.asarray(depth, dtype=np.int64)
        self.n = self.row_off.size - 1
        self.rows = [slice(int(self.row_off[r]), int(self.row_off[r + 1])) for r in range(self.n)]
        self.user = np.repeat(np.arange(self.n), np.diff(self.row_off))
        self.stages = np.array([LM.stages_of(sl.stop - sl.start, self.depth[r]) for r, sl in enumerate(self.rows)])
        self.c = 1.0 / self.stages.sum() if coef is None else float(coef)

    def scores(self, U, V):
        return (np.asarray(U, dtype=np.float64)[self.user] * np.asarray(V, dtype=np.float64)[self.item]).sum(1)

    def score_grads(self, a):
        return LM.rows(a, self.row_off, self.depth)[2]

    def risk(self, U, V):
        return self.c * LM.rows(self.scores(U, V), self.row_off, self.depth)[0].sum()

    def objective(self, U, V, l2):
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        return self.risk(U, V) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum())

    def tables(self, coef, U, V):
        """(sum over a user's entries of coef_e V[item_e], sum over an item's entries of coef_e U[user_e])."""
        hu, hv = np.zeros_like(U), np.zeros_like(V)
        np.add.at(hu, self.user, coef[:, None] * V[self.item])
        np.add.at(hv, self.item, coef[:, None] * U[self.user])
        return hu, hv

    def grads(self, U, V, l2=0.0):
        """(dF/dU, dF/dV): the block gradients of F (of the risk alone at l2 = 0)."""
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        gU, gV = self.tables(self.score_grads(self.scores(U, V)), U, V)
        return self.c * gU + l2 * U, self.c * gV + l2 * V

    def hvp(self, U, V, dU, dV, gauss_newton=False, a=None, y=None):
        """The Hessian of the risk at (U, V) applied to (dU, dV) → (HU, HV, parts): with y = dU[user] . V[item] +
        U[user] . dV[item], q = H y and g the score gradient, HU = c (q -> V by user + g -> dV by user), HV the mirror
        image; gauss_newton drops the g terms.  a, y: the entries' scores and the direction's, where the caller holds the
        device's own (fp32) values.  parts = (q, scale, g) per entry, for the tests' bounds."""
        U, V, dU, dV = (np.asarray(t, dtype=np.float64) for t in (U, V, dU, dV))
        a = self.scores(U, V) if a is None else np.asarray(a, dtype=np.float64)
        y = self.scores(dU, V) + self.scores(U, dV) if y is None else np.asarray(y, dtype=np.float64)
        q, _, scale, _ = rows(a, y, self.row_off, self.depth)
        g = self.score_grads(a)
        HU, HV = self.tables(q, U, V)
        if not gauss_newton:
            gU, gV = self.tables(g, dU, dV)
            HU, HV = HU + gU, HV + gV
        return self.c * HU, self.c * HV, (q, scale, g)

    # ---- the user block and its plain Newton solve with the dense Hessian ----
    def user_objective(self, u, V, r, l2):
        sl = self.rows[r]
        return self.c * LM.row(V[self.item[sl]] @ u, self.depth[r])[0] + 0.5 * l2 * float(u @ u)

    def user_grad(self, u, V, r, l2):
        Vi = V[self.item[self.rows[r]]]
        return self.c * (Vi.T @ LM.row(Vi @ u, self.depth[r])[3]) + l2 * u

    def solve_user(self, u0, V, r, l2, tol=1e-12, max_iter=50):
        """The minimiser of user r's problem by Newton with the dense d x d Hessian c V_r^T H V_r + l2 I, halving the step
        until the objective does not rise → (u, iterations until |grad| <= tol)."""
        V = np.asarray(V, dtype=np.float64)
        u = np.array(u0, dtype=np.float64)
        Vi = V[self.item[self.rows[r]]]
        for it in range(max_iter):
            g = self.user_grad(u, V, r, l2)
            if np.linalg.norm(g) <= tol:
                return u, it
            H = l2 * np.eye(u.size) + self.c * (Vi.T @ dense(Vi @ u, self.depth[r]) @ Vi)
            p, t, f = np.linalg.solve(H, -g), 1.0, self.user_objective(u, V, r, l2)
            while self.user_objective(u + t * p, V, r, l2) > f * (1.0 + 1e-15) and t > 1e-10:
                t *= 0.5
            u = u + t * p
        raise AssertionError("the model's user solve did not converge")

    def item_objective(self, U, V, l2):
        return self.risk(U, V) + 0.5 * l2 * float((np.asarray(V, dtype=np.float64) ** 2).sum())

    def user_noise(self, U, V):
        """Per user, the worst-case error of the device's block gradient from the list kernel's fp32 tolerance
        (test_lists.py: RTOL |g_e| + ATOL per entry): c sum over the user's entries of (2e-5 |g_e| + 2e-6) |V[item_e]|_2."""
        V = np.asarray(V, dtype=np.float64)
        g = self.score_grads(self.scores(U, V))
        vn = np.linalg.norm(V, axis=1)
        return np.array([self.c * float(((2e-5 * np.abs(g[sl]) + 2e-6) * vn[self.item[sl]]).sum()) for sl in self.rows])


# ---- the exact-step inputs the GPU tests and the CPU test of their noise bound share ----
STEP_N, STEP_M, STEP_D, STEP_L2, STEP_GTOL = 24, 30, 3, 5e-2, 1e-3
SPARE_ITEM = STEP_M - 1                # in no list: the tests give it to one user to poison that user alone


def step_inputs():
    """(U0, V fp32, users, items, positions, depth [n]): 24 users with lists of 0, 1, 2..14 items (every length from 2 up
    to 10 twice) out of the first 29 of 30 items, ordered by an exact Plackett–Luce draw from U* V^T, default_rng(1); the
    depths are the full list, half of it, 1, and for two users 0.  U0 is a second draw, the steps' start."""
    rng = np.random.default_rng(1)
    V = rng.standard_normal((STEP_M, STEP_D)).astype(np.float32)
    Ustar = rng.standard_normal((STEP_N, STEP_D)).astype(np.float32)
    U0 = (0.3 * rng.standard_normal((STEP_N, STEP_D))).astype(np.float32)
    lengths = [0, 1] + list(range(2, 15)) + list(range(2, 11))
    assert len(lengths) == STEP_N
    users, items, positions, depth = [], [], [], []
    for u, L in enumerate(lengths):
        shown = rng.choice(STEP_M - 1, L, replace=False)
        key = V[shown].astype(np.float64) @ Ustar[u].astype(np.float64) + rng.gumbel(size=L)
        users += [u] * L
        items += shown[np.argsort(-key)].tolist()
        positions += list(range(L))
        depth.append((L, (L + 1) // 2, min(L, 1), L)[u % 4])
    depth[6], depth[17] = 0, 0                                                # lists of 6 and of 4 items, none ranked
    return U0, V, np.array(users), np.array(items), np.array(positions), np.array(depth)
