"""The exact user step on implicit feedback in one launch (include/mfcd.h: mfcd_implicit_fold_in_users; csrc/
implicit_foldin.hip): `implicit_exact.implicit_user_step`'s problem, objective, rule, certificate and
statuses, solved by one workgroup per user that runs the whole damped Newton iteration with the user's d x d Hessian and
a Cholesky factor in LDS, instead of all users in lockstep through a chain of small launches per iteration.  d <= 64.
The serving-time step: a user who was not in training, a handful of observed items, V held fixed → the user's vector,
ready for `recommend_items`.

As a by-product the kernel returns the Hessian of a user's risk sum in the user's row,
    H_u = sum over i in P_u, j in N_u of sigmoid'(a_i - a_j) (v_i - v_j)(v_i - v_j)^T,
the implicit line's `pairs.user_information`.  There is no CPU form of any of it."""
import torch

from . import _lib
from .implicit_exact import _setup
from .pairs import UserInformation
from .population import PopulationStepResult


def max_d():
    return _lib.load().mfcd_implicit_fold_in_max_d()


def max_pos():
    """The most admissible observed items one workgroup takes: a user with more gets status 3."""
    return _lib.load().mfcd_implicit_fold_in_max_pos()


def max_pairs():
    """The most (observed, unobserved) pairs one workgroup takes: a user with more gets status 3 (`implicit_user_step`
    takes users of any size)."""
    return _lib.load().mfcd_implicit_fold_in_max_pairs()


def _call(U, V, plan, l2, gtol, max_newton, want_info):
    """One call of the entry → (rows, iters_status [n, 2], objective [n, 2], grad_ratio [n], info or None)."""
    n, (m, d), dev = plan.n, V.shape, V.device
    if d > max_d():
        raise ValueError(f"the one-launch implicit fold-in forms a Cholesky factor for d <= {max_d()}, got d = {d}: "
                         "implicit_user_step takes wider tables")
    L = _lib.load()
    p_off, p_items, entries, e_off, e_items, excl_entries = plan.lists
    # a user without a pair has coefficient 0 in the plan; the kernel answers it in closed form under any valid one
    coef = torch.where(plan.coef64 > 0, plan.coef64, torch.ones_like(plan.coef64)).contiguous()
    rows = torch.empty((n, d), dtype=torch.float32, device=dev)
    objective = torch.empty((n, 2), dtype=torch.float64, device=dev)
    ratio = torch.empty(n, dtype=torch.float64, device=dev)
    iters_status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    info = torch.empty((n, d, d), dtype=torch.float64, device=dev) if want_info else None
    work = _lib.workspace(L.mfcd_implicit_fold_in_workspace_bytes(n, m, d), dev)
    _lib.check(L.mfcd_implicit_fold_in_users(
        _lib.ptr(V), m, d, _lib.ptr(p_off), _lib.ptr(p_items) if entries else None, entries, _lib.ptr(e_off),
        _lib.ptr(e_items), excl_entries, n, _lib.ptr(coef), float(l2), _lib.ptr(U), int(max_newton), float(gtol),
        _lib.ptr(rows), _lib.ptr(objective), _lib.ptr(ratio), _lib.ptr(iters_status), _lib.ptr(info), _lib.ptr(work),
        work.numel(), _lib.stream_ptr(dev)))
    return rows, iters_status, objective, ratio, info


def implicit_fold_in_users(U, V, data, l2, exclude=None, normalize="pairs", coef=None, gtol=1e-3, max_newton=20, info=False):
    """`implicit_exact.implicit_user_step` in one launch: fp32 tables U [n, d] (None: zeros, the fold-in of users who were
    not in training) and V [m, d] on a GPU, d <= 64, the observed items of n users (a `ratings.RatingsData` on the device
    or a CSR pair), l2 > 0 → `population.PopulationStepResult` with the same meaning of every field: for every user the
    minimiser over the row u of
        f(u) = c_u R_u(u V^T) + (l2 / 2) |u|^2,
    R_u the risk sum of `implicit.implicit_rows` under `exclude`, c_u the normaliser of `implicit.implicit_risk` under
    `normalize` or `coef` (a scalar, or one value per user: the training table's normaliser for a fold-in), by damped
    Newton with the user's d x d Hessian (`cg_iters` is all zeros).  A user without an (observed, unobserved) pair gets
    the zero row, status 0, 0 iterations and objective_after 0; a user with an invalid list, or a non-finite start row or
    item vector, gets status 2 and a NaN row; a user with more than `max_pos()` admissible observed items or more than
    `max_pairs()` pairs gets status 3 and a NaN row.  A user's results do not depend on the other users.
    info=True: → (result, H), H f64 [n, d, d] the Hessian of every user's risk sum (without c_u and the ridge) at the
    returned row.  d > 64: ValueError (use `implicit_user_step`).  The inputs are not modified."""
    U, V, plan = _setup(U, V, data, l2, exclude, normalize, coef, None, "the one-launch implicit fold-in")
    max_newton = int(max_newton)
    if max_newton < 0:
        raise ValueError("max_newton must be >= 0")
    rows, its, obj, ratio, H = _call(U, V, plan, l2, gtol, max_newton, bool(info))
    result = PopulationStepResult(rows, its[:, 1].contiguous(), its[:, 0].contiguous(), torch.zeros_like(its[:, 0]),
                                  obj[:, 0].contiguous(), obj[:, 1].contiguous(), ratio)
    return (result, H) if info else result


def implicit_user_information(U, V, data, exclude=None):
    """For every user of `data` the d x d matrix
        H_u = sum over i in P_u, j in N_u of sigmoid'(a_i - a_j) (v_i - v_j)(v_i - v_j)^T,
    a = U[u] V^T, P_u the user's admissible observed items and N_u the unobserved ones: the Hessian of the user's risk
    sum in the row u → `pairs.UserInformation` (info f64 [n, d, d]; weight f64 [n], the user's pairs |P_u| |N_u|, 0 for
    an invalid list;
    status int32 [n]: 0, 2 for invalid data and 3 for a user beyond `max_pos()` or `max_pairs()`, the matrix is NaN
    then).  A user without a pair has the zero matrix.  One call of the fold-in kernel with no Newton iteration."""
    if U is None:
        raise _lib.MfcdError("the implicit user information needs U and V on a GPU device (there is no CPU fallback)")
    U, V, plan = _setup(U, V, data, 1.0, exclude, "pairs", 1.0, None, "the implicit user information")
    _, its, _, _, H = _call(U, V, plan, 1.0, 1e-3, 0, True)
    status = its[:, 1].contiguous()
    status = torch.where(status == 1, torch.zeros_like(status), status)     # "stopped" says nothing without iterations
    pos, neg = plan.counts[:, 0], plan.counts[:, 1]
    weight = torch.where((pos >= 0) & (neg >= 0), pos * neg, torch.zeros_like(pos)).double()    # an invalid list: -1, -1
    return UserInformation(H, weight, status)
