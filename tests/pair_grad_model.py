"""CPU model of mfcd_pair_grad_rows (include/mfcd.h), of the population risk built on it and of the dense Adam step
(mfcd_adam_dense) for the tests: numpy float64, the definitions written out.  The risk itself is pairs_model's."""
import numpy as np

import pairs_model as M


def pair_grad(a, x, scale):
    """g_i = sum over j != i of sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j)), by the m x m broadcast with a zeroed
    diagonal (float64 [m]); NaN x m if either row holds a non-finite entry."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not (np.isfinite(a).all() and np.isfinite(x).all()):
        return np.full(a.size, np.nan)
    with np.errstate(over="ignore"):                      # exp(+large) = inf gives sigmoid = 0, which is right
        t = M.sigmoid(a[:, None] - a[None, :]) - M.sigmoid(scale * (x[:, None] - x[None, :]))
    np.fill_diagonal(t, 0.0)
    return t.sum(axis=1)


def row_risk(a, x, scale):
    """The row's risk sum over the pairs i < j: sums[0] of pairs_model.pair_sums."""
    return M.pair_sums(a, x, scale)[0]


def population_risk(U, V, X, s, users=None):
    """Mean over the users (None: all; repeats count) and the m (m - 1) / 2 pairs of the risk, float64."""
    U, V, X = (np.asarray(t, dtype=np.float64) for t in (U, V, X))
    ids = np.arange(U.shape[0]) if users is None else np.asarray(users, dtype=np.int64)
    m = V.shape[0]
    S = U @ V.T
    return sum(row_risk(S[u], X[u], s) for u in ids) / (len(ids) * (m * (m - 1) // 2))


def population_grad(U, V, X, s, users=None):
    """(dRisk/dU, dRisk/dV, G64): the gradient of population_risk and the [k, m] score gradients it is made of."""
    U, V, X = (np.asarray(t, dtype=np.float64) for t in (U, V, X))
    ids = np.arange(U.shape[0]) if users is None else np.asarray(users, dtype=np.int64)
    m = V.shape[0]
    S = U @ V.T
    G = np.stack([pair_grad(S[u], X[u], s) for u in ids])
    c = 1.0 / (len(ids) * (m * (m - 1) // 2))
    dU = np.zeros_like(U)
    np.add.at(dU, ids, c * (G @ V))
    return dU, c * (G.T @ U[ids]), G


def bayes_risk(X, s):
    X = np.asarray(X, dtype=np.float64)
    m = X.shape[1]
    return sum(M.pair_sums(x, x, s)[1] for x in X) / (X.shape[0] * (m * (m - 1) // 2))


def reconstruction_error(U, V, X, s):
    """||(U V^T - column mean) - s X||_F / ||s X||_F."""
    P = np.asarray(U, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T
    P = P - P.mean(axis=1, keepdims=True)
    sX = s * np.asarray(X, dtype=np.float64)
    return float(np.linalg.norm(P - sX) / np.linalg.norm(sX))


class Adam:
    """torch.optim.Adam's step as mfcd_adam_dense applies it: coupled L2 weight decay added to the gradient, bias
    correction, eps outside the square root."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, (self.b1, self.b2), self.eps, self.wd, self.t = lr, betas, eps, weight_decay, 0

    def step(self, grads):
        self.t += 1
        c1, c2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            g = g + self.wd * p
            m *= self.b1
            m += (1.0 - self.b1) * g
            v *= self.b2
            v += (1.0 - self.b2) * g * g
            p -= (self.lr / c1) * m / (np.sqrt(v) / np.sqrt(c2) + self.eps)


def fit(U, V, X, s, steps, lr, weight_decay=0.0, log_every=0):
    """`steps` Adam steps on population_risk from (U, V) → (U, V, steps taken at each log point, risks there): the risk
    after 0, log_every, 2 log_every, ... steps and after the last one."""
    opt = Adam([U, V], lr, weight_decay=weight_decay)
    at, risks = [], []
    for t in range(steps):
        if log_every and t % log_every == 0:
            at.append(t)
            risks.append(population_risk(opt.p[0], opt.p[1], X, s))
        dU, dV, _ = population_grad(opt.p[0], opt.p[1], X, s)
        opt.step([dU, dV])
    if log_every:
        at.append(steps)
        risks.append(population_risk(opt.p[0], opt.p[1], X, s))
    return opt.p[0], opt.p[1], at, risks
