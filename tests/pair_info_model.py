"""CPU model of the multi-column pair Laplacian kernel and of the per-user information matrices built on it
(include/mfcd.h: mfcd_pair_hvp_multi_rows; mfcd/pairs.py: pair_hvp_multi_rows, pair_info_rows, user_information), for the
tests: numpy float64, the definitions written out by the m x m broadcast.  The curvature s_ij = sigmoid'(a_i - a_j) and the
weights are pair_hvp_model's and pair_law_model's; a row's item table is given already gathered, B [k, d]."""
import numpy as np

import pair_hvp_model as HM
import pair_law_model as LM

RTOL, ATOL = 2e-5, 2e-6          # the project's fp32 pair tolerance (test_pair_hvp.py)


def _pair_sum(coef, D):
    """sum over i < j of coef_ij D_ij D_ij^T for a symmetric coef with a zero diagonal and D [k, k, d] → [d, d]."""
    k, _, d = D.shape
    M = D.reshape(k * k, d)
    return 0.5 * ((M * coef.reshape(-1, 1)).T @ M)


def info_row(a, B, w=None, x=None):
    """(z [k, d], deg [k], H [d, d]) of one row: with S = curvature(a, w),
        z_i = sum_j S_ij (b_i - b_j),   deg_i = sum_j S_ij,   H = sum over i < j of S_ij (b_i - b_j)(b_i - b_j)^T.
    All NaN if a, x or B holds a non-finite entry."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    k, d = B.shape
    parts = (a, B) if x is None else (a, B, np.asarray(x, dtype=np.float64))
    if not all(np.isfinite(p).all() for p in parts):
        return np.full((k, d), np.nan), np.full(k, np.nan), np.full((d, d), np.nan)
    S = HM.curvature(a, w)
    D = B[:, None, :] - B[None, :, :]
    return (S[:, :, None] * D).sum(axis=1), S.sum(axis=1), _pair_sum(S, D)


def bounds(a, B, w=None):
    """(z_bound [k, d], H_bound [d, d]) of one row.  With b~ = B minus its f64 column mean, beta_ij,p = |b~_ip| + |b~_jp|,
    c_ij = w_ij s_ij:
        z_bound_ip = 2e-5 sum_j c_ij beta_ij,p + 2e-6 sum_j w_ij beta_ij,p
        H_bound_pq = sum over i < j of w_ij (2e-5 s_ij + 2e-6) beta_ij,p beta_ij,q
    — the pair tolerance applied to a sum of magnitudes that dominates, term by term, both the difference form
    sum c (b_i - b_j) and the centred Laplacian form deg b~_i - sum c b~_j."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    k = a.size
    S = HM.curvature(a, w)
    W = (np.ones((k, k)) - np.eye(k)) if w is None else np.asarray(w, dtype=np.float64)
    Bt = np.abs(B - B.mean(axis=0, keepdims=True))
    beta = Bt[:, None, :] + Bt[None, :, :]
    zb = RTOL * (S[:, :, None] * beta).sum(axis=1) + ATOL * (W[:, :, None] * beta).sum(axis=1)
    return zb, _pair_sum(RTOL * S + ATOL * W, beta)


def user_rows(U, V, X32, s, spec=None, users=None, at="model"):
    """[(a, gathered V, weights or None, x, W)] per user of the list: what `user_information` evaluates, in f64 from the
    fp32 tables.  at="truth": a = s x, formed in fp32 as the device forms it."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    X32 = np.asarray(X32, dtype=np.float32)
    n, m = X32.shape
    ids = (np.arange(n) if users is None else np.asarray(users, dtype=np.int64)) if spec is None else LM._ids(spec, n, users)
    out = []
    for u in ids:
        if spec is None:
            cols, w, W = np.arange(m), None, m * (m - 1) / 2.0
        else:
            cols, w = LM.user_parts(spec, X32, u)
            W = w.sum() / 2.0
        x = X32[u][cols]
        a = (V[cols] @ U[u]) if at == "model" else (x * np.float32(s)).astype(np.float64)
        out.append((a, V[cols], w, x.astype(np.float64), W))
    return out
