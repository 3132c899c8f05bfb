"""CPU model of mfcd_pair_stats_rows (include/mfcd.h) for the tests: numpy float64, O(m^2) over np.triu_indices, the
definitions of the header written out verbatim.  One row at a time."""
import numpy as np


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def pair_counts(a, x):
    """[C, D, Ta, Tx] over the pairs i < j as Python ints; [-1] * 4 if either row holds a NaN."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if np.isnan(a).any() or np.isnan(x).any():
        return [-1, -1, -1, -1]
    i, j = np.triu_indices(a.size, k=1)
    ai, aj, xi, xj = a[i], a[j], x[i], x[j]
    C = ((ai < aj) & (xi < xj)) | ((ai > aj) & (xi > xj))
    D = ((ai < aj) & (xi > xj)) | ((ai > aj) & (xi < xj))
    return [int(C.sum()), int(D.sum()), int((ai == aj).sum()), int((xi == xj).sum())]


def pair_sums(a, x, scale):
    """[risk, bayes_risk, exp_acc, bayes_acc] summed over the pairs i < j (float64); NaN x 4 if either row holds a
    non-finite entry."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not (np.isfinite(a).all() and np.isfinite(x).all()):
        return np.full(4, np.nan)
    i, j = np.triu_indices(a.size, k=1)
    da = a[i] - a[j]
    t = scale * (x[i] - x[j])
    q = sigmoid(t)
    risk = softplus(da) - q * da
    bayes_risk = softplus(t) - q * t
    exp_acc = np.where(a[i] > a[j], q, np.where(a[i] < a[j], 1.0 - q, 0.5))
    bayes_acc = np.maximum(q, 1.0 - q)
    return np.array([risk.sum(), bayes_risk.sum(), exp_acc.sum(), bayes_acc.sum()])


def direct_risk(a, x, scale):
    """Sum over the pairs of -(q log p + (1 - q) log(1 - p)) with p = sigmoid(a_i - a_j): the BCE the risk is defined as."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(a.size, k=1)
    p = sigmoid(a[i] - a[j])
    q = sigmoid(scale * (x[i] - x[j]))
    return float(-(q * np.log(p) + (1.0 - q) * np.log(1.0 - p)).sum())


def tau_b(counts, m):
    """Kendall's tau-b from [C, D, Ta, Tx]; NaN when a factor of the denominator is 0, the row held a NaN, or m < 2."""
    C, D, Ta, Tx = counts
    n0 = m * (m - 1) // 2
    if C < 0 or n0 - Ta <= 0 or n0 - Tx <= 0:
        return float("nan")
    return (C - D) / (np.sqrt(float(n0 - Ta)) * np.sqrt(float(n0 - Tx)))


def pairwise_accuracy(counts, m):
    C, _, _, Tx = counts
    n0 = m * (m - 1) // 2
    return float("nan") if C < 0 or n0 - Tx <= 0 else C / float(n0 - Tx)
