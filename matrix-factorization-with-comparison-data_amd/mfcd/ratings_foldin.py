"""The exact user step on a ratings table in one launch (include/mfcd.h: mfcd_ratings_fold_in_users; csrc/
ratings_foldin.hip): `ratings_exact.ratings_user_step`'s problem, objective, rule, certificate and
statuses, solved by one workgroup per user that runs the whole damped Newton iteration with the user's d x d Hessian and
a Cholesky factor in LDS, instead of all users in lockstep through a chain of small launches per iteration.  d <= 64.

As a by-product the kernel returns the Hessian of a user's risk sum in the user's row,
    H_u = sum over the pairs e < l of the user's items of w_el sigmoid'(a_e - a_l) (v_e - v_l)(v_e - v_l)^T,
the ratings line's `pairs.user_information`.  There is no CPU form of any of it."""
import torch

from . import _lib
from .pairs import UserInformation
from .population import PopulationStepResult
from .ratings_exact import _setup


def max_d():
    return _lib.load().mfcd_ratings_fold_in_max_d()


def max_len():
    """The longest row one workgroup takes: a longer one gets status 3 (`ratings_user_step` takes rows of any length)."""
    return _lib.load().mfcd_ratings_fold_in_max_len()


def _call(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, want_info):
    """One call of the entry → (rows, iters_status [n, 2], objective [n, 2], grad_ratio [n], info or None)."""
    n, d, dev = data.n, V.shape[1], V.device
    if d > max_d():
        raise ValueError(f"the one-launch ratings fold-in forms a Cholesky factor for d <= {max_d()}, got d = {d}: "
                         "ratings_user_step takes wider tables")
    L = _lib.load()
    rows = torch.empty((n, d), dtype=torch.float32, device=dev)
    objective = torch.empty((n, 2), dtype=torch.float64, device=dev)
    ratio = torch.empty(n, dtype=torch.float64, device=dev)
    iters_status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    info = torch.empty((n, d, d), dtype=torch.float64, device=dev) if want_info else None
    nbytes = L.mfcd_ratings_fold_in_workspace_bytes(n, d, data.entries)
    work = _lib.workspace(nbytes, dev)
    _lib.check(L.mfcd_ratings_fold_in_users(
        _lib.ptr(V), data.m, d, _lib.ptr(data.item), _lib.ptr(data.value), data.entries, _lib.ptr(data.row_off), n,
        float(s), 1 if skip_ties else 0, coef, float(l2), _lib.ptr(U), int(max_newton), float(gtol), _lib.ptr(rows),
        _lib.ptr(objective), _lib.ptr(ratio), _lib.ptr(iters_status), _lib.ptr(info), _lib.ptr(work), work.numel(),
        _lib.stream_ptr(dev)))
    return rows, iters_status, objective, ratio, info


def ratings_fold_in_users(U, V, data, s, l2, skip_ties=False, coef=None, gtol=1e-3, max_newton=20, info=False):
    """`ratings_exact.ratings_user_step` in one launch: fp32 tables U [data.n, d] (None: zeros, the fold-in of users who
    were not in training) and V [data.m, d] on a GPU, d <= 64, a `ratings.RatingsData` there, l2 > 0 →
    `population.PopulationStepResult` with the same meaning of every field: for every user the minimiser over the row u of
        f(u) = c * (risk sum of u V[items_u]^T against the user's ratings) + (l2 / 2) |u|^2,
    c = 1 / data.support(skip_ties) or `coef`, by damped Newton with the user's d x d Hessian (`cg_iters` is all zeros).
    A user without a supporting pair gets the zero row, status 0, 0 iterations and objective_after 0; a user with a
    non-finite rating, start row or item vector, or an item outside V, gets status 2 and a NaN row; a user with more
    than `max_len()` ratings gets status 3 and a NaN row.  A user's results do not depend on the other users.
    info=True: → (result, H), H f64 [n, d, d] the Hessian of every user's risk sum (without c and the ridge) at the
    returned row.  d > 64: ValueError (use `ratings_user_step`).  The inputs are not modified."""
    U, V, coef = _setup(U, V, data, l2, skip_ties, coef, "the one-launch ratings fold-in")
    max_newton = int(max_newton)
    if max_newton < 0:
        raise ValueError("max_newton must be >= 0")
    rows, its, obj, ratio, H = _call(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, bool(info))
    result = PopulationStepResult(rows, its[:, 1].contiguous(), its[:, 0].contiguous(), torch.zeros_like(its[:, 0]),
                                  obj[:, 0].contiguous(), obj[:, 1].contiguous(), ratio)
    return (result, H) if info else result


def ratings_user_information(U, V, data, s=1.0, skip_ties=False):
    """For every user of `data` the d x d matrix
        H_u = sum over the pairs e < l of the user's items of w_el sigmoid'(a_e - a_l) (v_e - v_l)(v_e - v_l)^T,
    a = U[u] V[items_u]^T, w_el = 1 or [x_e != x_l] under skip_ties: the Hessian of the user's risk sum in the row u →
    `pairs.UserInformation` (info f64 [n, d, d]; weight f64 [n], the user's support; status int32 [n]: 0, 2 for invalid
    data and 3 for a row longer than `max_len()`, the matrix is NaN then).  A user without a supporting pair has the
    zero matrix.  One call of the fold-in kernel with no Newton iteration.  The scores are those of the model: the
    kernel forms u . v itself, so there is no `at="ratings"` form (scores s x) here."""
    if U is None:
        raise _lib.MfcdError("the ratings user information needs U and V on a GPU device (there is no CPU fallback)")
    U, V, _ = _setup(U, V, data, 1.0, skip_ties, 1.0, "the ratings user information")
    _, its, _, _, H = _call(U, V, data, s, 1.0, skip_ties, 1.0, 1e-3, 0, True)
    status = its[:, 1].contiguous()
    status = torch.where(status == 1, torch.zeros_like(status), status)     # "stopped" says nothing without iterations
    weight = torch.from_numpy(data.user_support(skip_ties)).to(V.device).double()
    return UserInformation(H, weight, status)
