"""Alternating exact fit of the regularised BTL objective
    F(U, V) = sum_t softplus(x_t) - z_t x_t + (l2 / 2)(|U|^2 + |V|^2),   x_t = U[u_t] . (V[i_t] - V[j_t]),
from the two exact block steps of mfcd.foldin.  A sweep is one exact user step (every user's row to its minimiser with V
fixed) and then `item_steps` simultaneous item steps at theta = 1/2: every item moves half of the way to its own exact
minimiser against the current rows of the others.  Every loss term holds two item rows and the penalty one, so by
convexity, term by term, F(V_new) <= F(V) - (1/2) sum_k (f_k(v_k) - f_k(v*_k)): F falls at every sub-step, without
colouring the items and without any dependence on order.  F is invariant under a joint rescaling of U and V up to the
penalty, so convergence is linear and slow at small l2, as for any alternating scheme; mfcd.newton.fit_newton moves both
tables at once and certifies a stationary point."""
import collections

import torch

from . import foldin

class AlternatingResult(collections.namedtuple("AlternatingResult", ("U", "V", "history", "user_status", "item_status"))):
    """What `fit_alternating` returns, on the tables' device: U fp32 [n, d], V fp32 [m, d]; history f64 [sweeps,
    1 + item_steps], F after the user step and after every item step of each sweep; user_status int32 [n] and
    item_status int32 [m] of the last sweep's user step and last item step (0 converged, 1 stopped, 2 invalid data).
    The attribute `objective_start` (a 0-dim f64 tensor, not a field of the tuple) is F0, F at the tables given."""
    objective_start = None


def fit_alternating(U, V, u, i, j, z, l2, sweeps=10, item_steps=2, max_iter=50, xtol=2.0 ** -30):
    """U fp32 [n, d], V fp32 [m, d] on a GPU, comparisons (u, i, j, z), l2 > 0 → AlternatingResult: `sweeps` sweeps of
    one exact user step warm-started from U and `item_steps` (>= 1) simultaneous item steps at theta = 1/2.  The
    comparisons are grouped once per side; inside the loop nothing waits for the device; the inputs are not modified.
    Deterministic: two runs are bit-equal, and k sweeps equal k chained calls of one sweep."""
    sweeps, item_steps = int(sweeps), int(item_steps)
    if sweeps < 0 or item_steps < 1:
        raise ValueError("sweeps must be >= 0 and item_steps >= 1")
    if not torch.is_tensor(U) or not torch.is_tensor(V) or not U.is_cuda or not V.is_cuda:
        raise foldin._lib.MfcdError("fit_alternating needs U and V on a GPU device (there is no CPU fallback)")
    dev = V.device
    n, m = U.shape[0], V.shape[0]
    u, i, j, z = (torch.as_tensor(t).reshape(-1).to(dev) for t in (u, i, j, z))
    by_user = foldin.group_by_user(u, i, j, z, n)
    by_item = foldin.group_by_item(u, i, j, z, m)
    U, V = U.detach().float().contiguous(), V.detach().float().contiguous()
    history = [foldin.total_objective(U, V, u, i, j, z, l2)]
    user_status = torch.zeros(n, dtype=torch.int32, device=dev)
    item_status = torch.zeros(m, dtype=torch.int32, device=dev)
    for _ in range(sweeps):
        step = foldin.fold_in_users(V, by_user[0], by_user[1], l2, U, max_iter, xtol)
        U, user_status = step.U, step.status
        history.append(foldin.total_objective(U, V, u, i, j, z, l2))
        for _ in range(item_steps):
            step = foldin.fold_in_items(U, V, by_item[0], by_item[1], l2, None, 0.5, max_iter, xtol)
            V, item_status = step.V, step.status
            history.append(foldin.total_objective(U, V, u, i, j, z, l2))
    out = AlternatingResult(U, V, torch.stack(history)[1:].reshape(sweeps, 1 + item_steps), user_status, item_status)
    out.objective_start = history[0]
    return out
