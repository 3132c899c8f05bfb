"""Numpy f64 model of the sampled BTL objective's second-order route (include/mfcd.h: mfcd_triplet_rows; mfcd/newton.py):
    F(U, V) = sum_t softplus(x_t) - z_t x_t + (l2 / 2)(|U|^2 + |V|^2),   x_t = U[u_t] . (V[i_t] - V[j_t]).
`rows_pass` restates the kernel's per-row outputs on grouped records (np.add.at), with the sum of absolute values of every
output's terms beside it; `gradient` / `hvp` are the two passes on plain comparisons (incidence-matrix products);
`fit` is the trust-region Newton-CG iteration of mfcd.newton.fit_newton, step for step.  Everything the GPU tests compare against comes from here."""
import collections

import numpy as np

# (n, m, d, N, l2) of the fit tests
FIT_CASES = ((60, 40, 3, 3000, 3.0), (60, 40, 3, 3000, 0.03), (30, 20, 64, 4000, 0.4), (40, 25, 100, 3000, 0.3))
GTOL = 2.0 ** -26
PRED_FLOOR = 2.0 ** -44


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def make_fit_case(n, m, d, N, seed=1):
    """The inputs of the fit tests → (U0 fp32 [n, d], V0 fp32 [m, d], u, i, j int64 [N], z float64 [N] of 0 / 1)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, d))
    B = rng.standard_normal((m, d)) / np.sqrt(d)
    u, i, j = rng.integers(0, n, N), rng.integers(0, m, N), rng.integers(0, m, N)
    z = (rng.random(N) < sigmoid(3.0 * np.sum(A[u] * (B[i] - B[j]), 1))).astype(np.float64)
    U0 = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V0 = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    return U0, V0, u, i, j, z


# ---- grouped records, as mfcd.foldin.group_by_user / group_by_item make them ----
def records(u, i, j, z):
    rec = np.empty((len(u), 4), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = u, i, j
    rec[:, 3] = np.asarray(z, dtype=np.float32).view(np.int32)
    return rec


def group_by_user(u, i, j, z, n):
    order = np.argsort(u, kind="stable")
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(u, minlength=n))
    return records(u, i, j, z)[order], off


def group_by_item(u, i, j, z, m):
    key = np.stack((i, j), 1).reshape(-1)
    order = np.argsort(key, kind="stable")
    off = np.zeros(m + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(key, minlength=m))
    return records(u, i, j, z)[order >> 1], off


def segment_rows(row_off, S):
    seg = np.zeros(len(row_off), dtype=np.int64)
    seg[1:] = np.cumsum((np.diff(row_off) + S - 1) // S)
    return seg, int(seg[-1])


RowsPass = collections.namedtuple("RowsPass", ("out", "diag", "loss", "abs_out", "abs_diag", "abs_loss"))


def rows_pass(side, pas, gauss_newton, U, V, P, Q, rec, row_off, row_id, l2):
    """What mfcd_triplet_rows returns for valid rows, [rows, d] / [rows], and for each output the sum of the absolute
    values of its terms, the l2 term included (abs_* of the shape of the output)."""
    rows, d = len(row_off) - 1, U.shape[1]
    own_of = np.arange(rows) if row_id is None else np.asarray(row_id, dtype=np.int64)
    owner = np.repeat(np.arange(rows), np.diff(row_off))
    u, i, j = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    z = np.ascontiguousarray(rec[:, 3]).view(np.float32).astype(np.float64)
    own = own_of[owner]
    delta = V[i] - V[j]
    if side == 0:
        a, sigma = U[own], np.ones(len(own))
    else:
        a, sigma = U[u], (i == own).astype(np.float64) - (j == own)
    x = np.sum(a * delta, 1)
    p = sigmoid(x)
    r, w = p - z, p * (1.0 - p)
    if pas == 0:
        terms = r[:, None] * delta if side == 0 else (sigma * r)[:, None] * a
        dterms = w[:, None] * delta * delta if side == 0 else (sigma * sigma * w)[:, None] * a * a
        reg = l2 * (U if side == 0 else V)[own_of]
    else:
        dq = Q[i] - Q[j]
        ad = P[own] if side == 0 else P[u]
        y = np.sum(ad * delta, 1) + np.sum(a * dq, 1)
        rr = np.zeros_like(r) if gauss_newton else r
        if side == 0:
            terms = (w * y)[:, None] * delta + rr[:, None] * dq
        else:
            terms = sigma[:, None] * ((w * y)[:, None] * a + rr[:, None] * ad)
        dterms = np.zeros_like(terms)
        reg = l2 * (P if side == 0 else Q)[own_of]
    lterms = (softplus(x) - z * x) * (sigma != 0)
    out, diag, abs_out, abs_diag = (np.zeros((rows, d)) for _ in range(4))
    loss, abs_loss = np.zeros(rows), np.zeros(rows)
    np.add.at(out, owner, terms)
    np.add.at(abs_out, owner, np.abs(terms))
    np.add.at(diag, owner, dterms)
    np.add.at(loss, owner, lterms)
    np.add.at(abs_loss, owner, np.abs(softplus(x)) + np.abs(z * x))
    return RowsPass(out + reg, diag + l2, loss, abs_out + np.abs(reg), diag + l2, abs_loss)


# ---- the two passes on plain comparisons ----
def _incidence(u, i, j, n, m):
    """S [n, N] with S[u_t, t] = 1 and T [m, N] with T[k, t] = sigma_t = [i_t = k] - [j_t = k]: S @ terms and T @ terms are
    the sums over a user's and over an item's comparisons."""
    t = np.arange(len(u))
    S, T = np.zeros((n, len(u))), np.zeros((m, len(u)))
    S[u, t] = 1.0
    np.add.at(T, (i, t), 1.0)
    np.add.at(T, (j, t), -1.0)
    return S, T


def gradient(U, V, u, i, j, z, l2):
    """→ (F, gU, gV, DU, DV): the objective, its gradient and the Jacobi diagonal of the Hessian."""
    S, T = _incidence(u, i, j, U.shape[0], V.shape[0])
    delta = V[i] - V[j]
    x = np.sum(U[u] * delta, 1)
    p = sigmoid(x)
    r, w = p - z, p * (1.0 - p)
    F = np.sum(softplus(x) - z * x) + 0.5 * l2 * (np.sum(U * U) + np.sum(V * V))
    return (F, S @ (r[:, None] * delta) + l2 * U, T @ (r[:, None] * U[u]) + l2 * V,
            S @ (w[:, None] * delta * delta) + l2, (T * T) @ (w[:, None] * U[u] * U[u]) + l2)


def hvp(U, V, u, i, j, z, P, Q, l2, gauss_newton=False):
    """→ (HU, HV): the Hessian of F (or its Gauss-Newton part plus l2) applied to the direction (P, Q)."""
    S, T = _incidence(u, i, j, U.shape[0], V.shape[0])
    delta, dq = V[i] - V[j], Q[i] - Q[j]
    x = np.sum(U[u] * delta, 1)
    p = sigmoid(x)
    r, w = (0.0 if gauss_newton else 1.0) * (p - z), p * (1.0 - p)
    wy = w * (np.sum(P[u] * delta, 1) + np.sum(U[u] * dq, 1))
    return S @ (wy[:, None] * delta + r[:, None] * dq) + l2 * P, T @ (wy[:, None] * U[u] + r[:, None] * P[u]) + l2 * Q


def hessian_inf_norm_bound(U, V, u, i, j, z, l2):
    """An upper bound of |H|_inf (the largest absolute row sum of the Hessian of F): every sum of `hvp` with the absolute
    value of each factor and |P|, |Q| <= 1."""
    delta = V[i] - V[j]
    x = np.sum(U[u] * delta, 1)
    p = sigmoid(x)
    r, w = np.abs(p - z), p * (1.0 - p)
    ymax = w * (np.sum(np.abs(delta), 1) + 2.0 * np.sum(np.abs(U[u]), 1))
    HU, HV = np.zeros_like(U), np.zeros_like(V)
    np.add.at(HU, u, ymax[:, None] * np.abs(delta) + 2.0 * r[:, None])
    tv = ymax[:, None] * np.abs(U[u]) + r[:, None]
    np.add.at(HV, i, tv)
    np.add.at(HV, j, tv)
    return max(HU.max(), HV.max()) + l2


# ---- the fit ----
NewtonModelResult = collections.namedtuple("NewtonModelResult", ("U", "V", "history", "grad_inf", "cg_iters", "products",
                                                                 "status"))


def _to_boundary(s, p, D, radius):
    """tau >= 0 with |s + tau p|_M = radius."""
    a, b, c = np.sum(D * p * p), np.sum(D * s * p), np.sum(D * s * s) - radius * radius
    return (-b + np.sqrt(np.maximum(b * b - a * c, 0.0))) / a


def fit(U0, V0, u, i, j, z, l2, max_iter=100, gtol=GTOL, cg_cap=None):
    """The iteration of mfcd.newton.fit_newton on f64 copies of the tables → NewtonModelResult with f64 U, V (the
    iterate before its one rounding to fp32)."""
    (n, d), m = U0.shape, V0.shape[0]
    cut = n * d
    cap = 2 * (n + m) * d if cg_cap is None else int(cg_cap)

    def split(v):
        return v[:cut].reshape(n, d), v[cut:].reshape(m, d)

    def grad_at(v):
        F, gU, gV, DU, DV = gradient(*split(v), u, i, j, z, l2)
        return F, np.concatenate((gU.ravel(), gV.ravel())), np.concatenate((DU.ravel(), DV.ravel()))

    def product(v, q):
        return np.concatenate([h.ravel() for h in hvp(*split(v), u, i, j, z, *split(q), l2)])

    x = np.concatenate((U0.astype(np.float64).ravel(), V0.astype(np.float64).ravel()))
    F, g, D = grad_at(x)
    radius, history, grad_inf, cg_iters, products, status = None, [], [], [], 0, 1
    for _ in range(int(max_iter)):
        history.append(F)
        grad_inf.append(np.abs(g).max())
        if not np.isfinite(F) or not np.isfinite(grad_inf[-1]):
            break
        if grad_inf[-1] <= gtol * l2 * np.abs(x).max():
            status = 0
            break
        gnorm = np.sqrt(np.sum(g * g / D))
        if radius is None:
            radius = gnorm                                  # |M^-1 g|_M
        tol = min(0.1, np.sqrt(gnorm)) * gnorm
        s, r = np.zeros_like(x), g.copy()
        p = -r / D
        rz = np.sum(r * r / D)
        hit, k = False, 0
        while k < cap:
            Hp = product(x, p)
            k += 1
            pHp = np.sum(p * Hp)
            if not np.isfinite(pHp):
                break
            alpha = rz / pHp if pHp > 0 else 0.0
            s_new = s + alpha * p
            if pHp <= 0 or np.sum(D * s_new * s_new) >= radius * radius:
                s = s + _to_boundary(s, p, D, radius) * p
                hit = True
                break
            s = s_new
            r = r + alpha * Hp
            zr = r / D
            rz_new = np.sum(r * zr)
            if np.sqrt(rz_new) <= tol:
                break
            p = -zr + (rz_new / rz) * p
            rz = rz_new
        cg_iters.append(k)
        products += k + 1
        pred = -(np.sum(g * s) + 0.5 * np.sum(s * product(x, s)))
        Ft, gt, Dt = grad_at(x + s)
        snorm = np.sqrt(np.sum(D * s * s))
        if pred <= PRED_FLOOR * abs(F):                    # the ratio is at its rounding level, and so is F - Ft:
            accept = np.sqrt(np.sum(gt * gt / D)) < gnorm  # the step is judged by the gradient, and F keeps the lower
            Ft = min(F, Ft)                                # of two values that differ by their rounding alone
            if not accept:
                radius = 0.25 * snorm
        else:
            rho = (F - Ft) / pred
            if rho < 0.25:
                radius = 0.25 * snorm
            elif rho > 0.75 and hit:
                radius = 2.0 * radius
            accept = rho > 1e-4
        if accept:
            x, F, g, D = x + s, Ft, gt, Dt
    U, V = split(x)
    return NewtonModelResult(U.copy(), V.copy(), np.array(history), np.array(grad_inf), np.array(cg_iters, dtype=np.int64),
                             products, status)
