"""CPU model of the pair arg-max kernel (include/mfcd.h: mfcd_pair_best_rows; mfcd/pairs.py: pair_best_rows), for the
tests: numpy float64, the definition written out by the k x k broadcast.  The curvature s_ij = sigmoid'(a_i - a_j) is
pair_hvp_model's, the weights pair_law_model's; a row's table is G [k, d]."""
import numpy as np

import pair_hvp_model as HM
from pair_info_model import ATOL, RTOL          # the project's fp32 pair tolerance


def scores(a, G, w=None, x=None):
    """(S64 [k, k], E [k, k], adm [k, k] bool) of one row:
        S64_ij = s_ij |g_i - g_j|^2, the difference formed first, in f64;
        E_ij   = (2e-5 s_ij + 2e-6) sum_p (|g_ip| + |g_jp|)^2: the pair tolerance applied to a sum of magnitudes that
                 dominates, term by term, both the difference form and the Gram form n_i + n_j - 2 g_i . g_j;
        adm_ij = i != j and w_ij > 0 (w None: every pair).
    S64 is all NaN if a, x or G holds a non-finite entry."""
    a, G = np.asarray(a, dtype=np.float64), np.asarray(G, dtype=np.float64)
    k = a.size
    adm = ~np.eye(k, dtype=bool) if w is None else (np.asarray(w) > 0) & ~np.eye(k, dtype=bool)
    parts = (a, G) if x is None else (a, G, np.asarray(x, dtype=np.float64))
    if not all(np.isfinite(p).all() for p in parts):
        return np.full((k, k), np.nan), np.full((k, k), np.nan), adm
    s = HM.dsigmoid(a[:, None] - a[None, :])
    D = G[:, None, :] - G[None, :, :]
    mag = np.abs(G)[:, None, :] + np.abs(G)[None, :, :]
    return s * (D * D).sum(axis=2), (RTOL * s + ATOL) * (mag * mag).sum(axis=2), adm


def best(S64, adm):
    """(val [k], j [k]) of the model: the largest admissible score of every column and the smallest j that attains it;
    (+0, -1) without an admissible partner, (NaN, -1) for a NaN row."""
    k = S64.shape[0]
    if np.isnan(S64).any():
        return np.full(k, np.nan), np.full(k, -1, dtype=np.int64)
    masked = np.where(adm, S64, -1.0)                       # every score is >= 0
    j = masked.argmax(axis=1)                               # the first of equal maxima: the smallest j
    has = adm.any(axis=1)
    return np.where(has, masked[np.arange(k), j], 0.0), np.where(has, j, -1)
