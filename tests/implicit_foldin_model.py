"""CPU model of the one-launch implicit fold-in (include/mfcd.h: mfcd_implicit_fold_in_users; mfcd/implicit_foldin.py), for
the tests: numpy float64.  The objective, its gradient, the Laplacian and the plain Newton minimisers are
implicit_hvp_model.Problem's; this file restates the kernel's fixed algorithm on them (population._newton with solver
"direct", per row: the centring, the trial rule, the iteration count, the statuses, the closed form), the bipartite forms
of the gradient and the Hessian the kernel uses (from the |P| x |N| weight block: the m x m Laplacian takes seconds per
row at m = 4000), and builds the input family the CPU condition test and the GPU tests share."""
import functools

import numpy as np

import implicit_hvp_model as HM
import implicit_model as IM

ARMIJO, MIN_STEP = 1e-4, 2.0 ** -12          # population.ARMIJO, population.MIN_STEP
L2, GTOL = 3e-2, 1e-3
CHUNK = 2048                                 # mfcd_implicit_fold_in_chunk(): columns per stage of the kernel's column loop
M_THIRD = 2 * CHUNK + 37                     # several stages and a ragged last one
DS = [1, 2, 3, 16, 17, 33, 64]               # the kernel's four widths (4, 16, 32, 64 columns) on either side
LENGTHS = {97: [0, 1, 2, 63, 64, 65, 96, 97],
           600: [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 515, 599, 600],   # 599 is an odd row: its one other column is barred
           M_THIRD: [0, 1, 65, 257, CHUNK - 1, CHUNK + 1, M_THIRD - 1]}
CASES = [(m, d) for m in (97, 600) for d in DS] + [(M_THIRD, 3), (M_THIRD, 64)]
RTOL, ATOL = 2e-5, 2e-6                      # the project's fp32 pair tolerance (pair_info_model.py)


def centred(V, P):
    """V minus the mean of the rows the admissible positives name, as the kernel forms it (in f64 here)."""
    V = np.asarray(V, dtype=np.float64)
    return V - V[P].mean(axis=0, keepdims=True)


def grad(prob, V, r, u, l2):
    """coef (sum_j g_j v~_j - sum_i G_i v~_i) + l2 u: the gradient by its bipartite structure."""
    P, N = prob.classes[r]
    u = np.asarray(u, dtype=np.float64)
    if P.size * N.size == 0:
        return l2 * u
    B = centred(V, P)
    a = B @ u
    s = IM.sigmoid(a[N][None, :] - a[P][:, None])                # [pos, neg]
    return prob.c[r] * (s.sum(0) @ B[N] - s.sum(1) @ B[P]) + l2 * u


def info(prob, V, r, u):
    """sum over i in P, j in N of sigmoid'(a_i - a_j)(v_i - v_j)(v_i - v_j)^T at a = V u, [d, d], from the |P| x |N|
    weight block: (T + T^T) / 2 with T = sum_i v~_i (D_i v~_i)^T + sum_j v~_j (D_j v~_j - 2 y_j)^T, y_j = sum_i w_ij v~_i."""
    P, N = prob.classes[r]
    d = np.asarray(V).shape[1]
    if P.size * N.size == 0:
        return np.zeros((d, d))
    B = centred(V, P)
    w = HM.weights(B @ np.asarray(u, dtype=np.float64), P, N)
    Bp, Bn = B[P], B[N]
    T = Bp.T @ (w.sum(1)[:, None] * Bp) + Bn.T @ (w.sum(0)[:, None] * Bn - 2.0 * (w.T @ Bp))
    return 0.5 * (T + T.T)


def minimiser(prob, V, r, l2, tol=1e-13, max_iter=60):
    """Problem.solve_user from zero with the Hessian from the weight block."""
    V = np.asarray(V, dtype=np.float64)
    u = np.zeros(V.shape[1])
    for _ in range(max_iter):
        g = prob.user_grad(u, V, r, l2)
        if np.linalg.norm(g) <= tol:
            return u
        H = prob.c[r] * info(prob, V, r, u) + l2 * np.eye(u.size)
        p, t, f = np.linalg.solve(H, -g), 1.0, prob.user_objective(u, V, r, l2)
        while prob.user_objective(u + t * p, V, r, l2) > f + 1e-14 * abs(f) and t > 1e-10:   # f's own rounding
            t *= 0.5
        u = u + t * p
    raise AssertionError("the model's user solve did not converge")


def fold_in(prob, V, r, u0, l2, gtol=GTOL, max_newton=20, trace=None):
    """The fixed algorithm on row r from u0 → (u, iterations, status, f at the start, f at u, grad_ratio).  trace: a list
    that receives (t, accepted) per trial."""
    V = np.asarray(V, dtype=np.float64)
    u = np.array(u0, dtype=np.float64)
    if not prob.paired[r]:                                     # the closed form: no pair
        return np.zeros_like(u), 0, 0, 0.5 * l2 * float(u @ u), 0.0, 0.0
    f = prob.user_objective(u, V, r, l2)
    f0, t, it, p, moved = f, 1.0, 0, None, True
    while True:
        g = grad(prob, V, r, u, l2)
        gnorm, umax = np.linalg.norm(g), np.abs(u).max()
        if gnorm <= gtol * l2 * umax:
            status = 0
            break
        if it == max_newton:
            status = 1
            break
        if moved or p is None:
            H = prob.c[r] * info(prob, V, r, u) + l2 * np.eye(u.size)
            try:
                C = np.linalg.cholesky(H)
                p = -np.linalg.solve(C.T, np.linalg.solve(C, g))
            except np.linalg.LinAlgError:
                p = -g / np.diag(H).mean()
        ut = u + t * p
        ft = prob.user_objective(ut, V, r, l2)
        it += 1
        if trace is not None:
            trace.append((t, bool(ft <= f + ARMIJO * t * float(g @ p))))
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


def user_noise(prob, V, r, u):
    """Problem.user_noise of one row, with the columns' degrees from the weight block instead of the m x m Laplacian."""
    V, u = np.asarray(V, dtype=np.float64), np.asarray(u, dtype=np.float64)
    P, N = prob.classes[r]
    if P.size * N.size == 0:
        return 0.0
    a = V @ u
    G = prob.c[r] * prob.row_grad(a, r)
    delta = (u.size + 1) * 2.0 ** -24 * (np.abs(V) @ np.abs(u)).max()
    w = HM.weights(a, P, N)
    deg, k = np.zeros(prob.m), np.zeros(prob.m)
    deg[P], deg[N] = w.sum(1), w.sum(0)
    k[P], k[N] = N.size, P.size
    noise = 2e-5 * np.abs(G) + prob.c[r] * (2e-6 * k * (np.abs(G) > 0) + 2.0 * delta * deg)
    return float(noise @ np.linalg.norm(V, axis=1))


def info_bound(a, V, P, N):
    """pair_info_model.bounds(a, V, W)[1] for the bipartite 0/1 weights W (1 between P and N, 0 elsewhere, barred columns
    included), without the m x m x d arrays: with C = 2e-5 S + 2e-6 W and x_c = |v_c - mean of all rows of V|,
        sum over c < e of C_ce (x_c + x_e)(x_c + x_e)^T = X^T diag(C 1) X + X^T C X."""
    V = np.asarray(V, dtype=np.float64)
    X = np.abs(V - V.mean(axis=0, keepdims=True))
    C = RTOL * HM.weights(np.asarray(a, dtype=np.float64), P, N) + ATOL
    Xp, Xn = X[P], X[N]
    cross = Xp.T @ C @ Xn
    return Xp.T @ (C.sum(1)[:, None] * Xp) + Xn.T @ (C.sum(0)[:, None] * Xn) + cross + cross.T


def bipartite_weights(m, P, N):
    W = np.zeros((m, m))
    W[np.ix_(P, N)] = 1.0
    return W + W.T


class Family:
    """The inputs for m items and width d: V fp32 [m, d] with a decaying column spectrum, one row per length of
    LENGTHS[m] in a shuffled order, the observed items drawn towards the top of a planted user's scores, odd rows with
    barred columns; the model problem under normalize="pairs", its minimisers and the gradient noise there."""

    def __init__(self, m, d):
        rng = np.random.default_rng(7 + d)
        col = 0.8 ** np.arange(d)
        lengths = LENGTHS[m]
        self.m, self.d = m, d
        self.V = (rng.standard_normal((m, d)) * (col / np.linalg.norm(col))).astype(np.float32)
        self.V64 = self.V.astype(np.float64)
        Ustar = 2.0 * rng.standard_normal((len(lengths), d))
        rows = []
        for r, L in enumerate(lengths):
            s = self.V64 @ Ustar[r] + 0.5 * rng.standard_normal(m)
            pos = np.sort(np.argsort(-(s + rng.gumbel(size=m)), kind="stable")[:L])
            rest = np.setdiff1d(np.arange(m), pos)
            excl = np.sort(rng.choice(rest, min(5, rest.size), replace=False)) if r % 2 == 1 else np.zeros(0, np.int64)
            rows.append((pos, excl))
        order = rng.permutation(len(rows))
        self.n = len(rows)
        self.pos = [rows[i][0] for i in order]
        self.excl = [rows[i][1] for i in order]
        self.lengths = np.array([len(p) for p in self.pos])
        self.prob = HM.Problem(m, self.pos, self.excl, "pairs")
        self.paired = self.prob.paired
        self.pairs = np.array([P.size * N.size for P, N in self.prob.classes])
        self.start = (3.0 * np.random.default_rng(100 + d).standard_normal((self.n, d))).astype(np.float32)
        self.Uopt = np.stack([minimiser(self.prob, self.V64, r, L2) if self.paired[r] else np.zeros(d) for r in range(self.n)])
        self.noise = np.array([user_noise(self.prob, self.V64, r, self.Uopt[r]) for r in range(self.n)])


@functools.lru_cache(maxsize=None)
def family(m, d):
    return Family(m, d)


DECREASE_COEF, DECREASE_L2 = 1e-7, 1e-5      # a whole table's 1 / pairs, and a ridge that is light against the risk


class DecreaseFamily:
    """Inputs on which the Armijo test needs the decrease summed pair by pair: the family's V at m = 600, four rows each
    of 3, 16, 64 and 200 observed items drawn uniformly (no planted user: the risk stays of order |P| |N| at the
    minimiser), coef = 1e-7, l2 = 1e-5.  The risk part of f is then 50 to 10 000 times the ridge part, f's fp32 rounding
    (1e-7 of the risk part) exceeds the last steps' decrease (gtol^2 = 1e-6 of the ridge part), and the gradient is
    still resolved well enough for the certificate."""

    def __init__(self, d):
        fam = family(600, d)
        rng = np.random.default_rng(900 + d)
        self.d, self.V, self.V64 = d, fam.V, fam.V64
        self.pos = [np.sort(rng.choice(600, L, replace=False)) for L in (3, 16, 64, 200) for _ in range(4)]
        self.n = len(self.pos)
        self.start = (3.0 * rng.standard_normal((self.n, d))).astype(np.float32)
        self.prob = HM.Problem(600, self.pos, None, coef=DECREASE_COEF)
        self.Uopt = np.stack([minimiser(self.prob, self.V64, r, DECREASE_L2) for r in range(self.n)])
        self.noise = np.array([user_noise(self.prob, self.V64, r, self.Uopt[r]) for r in range(self.n)])


@functools.lru_cache(maxsize=None)
def decrease_family(d):
    return DecreaseFamily(d)
