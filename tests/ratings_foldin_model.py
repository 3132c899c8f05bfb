"""CPU model of the one-launch ratings fold-in (include/mfcd.h: mfcd_ratings_fold_in_users; mfcd/ratings_foldin.py), for
the tests: numpy float64.  The objective, its gradient, the Laplacian, the plain Newton minimisers and the gradient's
noise bound are ratings_hvp_model.Problem's; this file restates the kernel's fixed algorithm on them (population._newton
with solver "direct", per row: the centring, the trial rule, the iteration count, the statuses, the closed form) and
builds the input family the CPU condition test and the GPU tests share."""
import functools

import numpy as np

import ratings_hvp_model as RH

ARMIJO, MIN_STEP = 1e-4, 2.0 ** -12          # population.ARMIJO, population.MIN_STEP
L2, GTOL, SCALE = 3e-2, 1e-3, 1.0
M_ITEMS = 600
LS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 515]   # closed forms, the 64-term run, the 256-entry tile, two tiles and more
DS = [1, 2, 3, 16, 17, 33, 64]                      # the kernel's four widths (4, 16, 32, 64 columns) on either side


def centred(V, items):
    """The row's gathered item vectors minus their column mean, as the kernel forms them (in f64 here)."""
    B = np.asarray(V, dtype=np.float64)[items]
    return B - B.mean(axis=0, keepdims=True) if len(items) else B


def info(prob, V, r, u):
    """sum over the pairs e < l of row r of w_el sigmoid'(a_e - a_l)(v_e - v_l)(v_e - v_l)^T at a = u . v, [d, d]: the
    Laplacian between the centred rows (its rows sum to 0, so the centre drops out)."""
    B = centred(V, prob.item[prob.rows[r]])
    if len(B) < 2:
        return np.zeros((B.shape[1], B.shape[1]))
    return B.T @ prob.laplacian(B @ np.asarray(u, dtype=np.float64), r) @ B


def fold_in(prob, V, r, u0, l2, gtol=GTOL, max_newton=20):
    """The fixed algorithm on row r from u0 → (u, iterations, status, f at the start, f at u, grad_ratio)."""
    V = np.asarray(V, dtype=np.float64)
    u = np.array(u0, dtype=np.float64)
    if prob.support[r] == 0:                                   # the closed form: no supporting pair
        return np.zeros_like(u), 0, 0, 0.5 * l2 * float(u @ u), 0.0, 0.0
    f = prob.user_objective(u, V, r, l2)
    f0, t, it, p, moved = f, 1.0, 0, None, True
    while True:
        g = prob.user_grad(u, V, r, l2)
        gnorm, umax = np.linalg.norm(g), np.abs(u).max()
        if gnorm <= gtol * l2 * umax:
            status = 0
            break
        if it == max_newton:
            status = 1
            break
        if moved or p is None:
            H = prob.c * info(prob, V, r, u) + l2 * np.eye(u.size)
            try:
                C = np.linalg.cholesky(H)
                p = -np.linalg.solve(C.T, np.linalg.solve(C, g))
            except np.linalg.LinAlgError:
                p = -g / np.diag(H).mean()
        ut = u + t * p
        ft = prob.user_objective(ut, V, r, l2)
        it += 1
        if ft <= f + ARMIJO * t * float(g @ p):                # a NaN trial is a rejected one
            u, f, t, moved = ut, ft, min(2.0 * t, 1.0), True
        else:
            t, moved = 0.5 * t, False
            if t < MIN_STEP:
                status = 1
                break
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = gnorm / (l2 * umax)
    return u, it, status, f0, f, ratio


def quantise(score):
    """Five levels 1..5 over the row's own range."""
    if score.size == 0:
        return score.astype(np.float32)
    lo, hi = score.min(), score.max()
    if hi == lo:
        return np.full(score.size, 3.0, np.float32)
    return (1.0 + np.minimum(np.floor(5.0 * (score - lo) / (hi - lo)), 4.0)).astype(np.float32)


class Family:
    """The GPU inputs for width d: V fp32 [600, d] with a decaying column spectrum, one row per length of LS (and under
    skip-ties a row of five equal ratings: pairs, but no support) in a shuffled order, ratings from a planted user vector
    plus noise in five levels; the model problem, its minimisers and the gradient noise there."""

    def __init__(self, d, skip):
        rng = np.random.default_rng(7 + d)
        col = 0.8 ** np.arange(d)
        self.d, self.skip = d, skip
        self.V = (rng.standard_normal((M_ITEMS, d)) * (col / np.linalg.norm(col))).astype(np.float32)
        Ustar = 2.0 * rng.standard_normal((len(LS), d))
        rows = []
        for r, L in enumerate(LS):
            items = np.sort(rng.choice(M_ITEMS, L, replace=False))
            score = self.V[items].astype(np.float64) @ Ustar[r] + 0.5 * rng.standard_normal(L)
            rows.append((items, quantise(score)))
        if skip:
            rows.append((np.sort(rng.choice(M_ITEMS, 5, replace=False)), np.full(5, 3.0, np.float32)))
        order = rng.permutation(len(rows))
        self.lengths = np.array([len(rows[i][0]) for i in order])
        self.n = len(rows)
        self.users = np.concatenate([np.full(len(rows[i][0]), k, np.int64) for k, i in enumerate(order)])
        self.items = np.concatenate([rows[i][0] for i in order]).astype(np.int64)
        self.values = np.concatenate([rows[i][1] for i in order]).astype(np.float32)
        self.row_off = np.concatenate(([0], np.cumsum(self.lengths)))
        self.prob = RH.Problem(self.row_off, self.items, self.values, SCALE, skip)
        self.V64 = self.V.astype(np.float64)
        self.start = (3.0 * np.random.default_rng(100 + d).standard_normal((self.n, d))).astype(np.float32)
        self.Uopt = np.stack([self.prob.solve_user(np.zeros(d), self.V64, r, L2)[0] for r in range(self.n)])
        self.noise = self.prob.user_noise(self.Uopt, self.V64)
        self.paired = self.prob.support > 0


@functools.lru_cache(maxsize=None)
def family(d, skip):
    return Family(d, skip)
