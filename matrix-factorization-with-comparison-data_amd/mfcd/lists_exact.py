"""Exact block steps of the ridge-regularised Plackett–Luce objective on ranked lists
    F(U, V) = c * sum over the users of loss_u(U[u] V[items_u]^T) + (l2 / 2)(|U|^2 + |V|^2),
loss_u the list loss of `lists.pl_rows` over the user's stages and c = 1 / lists.stages, `lists.pl_risk`'s global
normaliser: mfcd/ratings_exact.py on ranked lists.  With V fixed F is strongly convex (modulus l2) and separable in the
users' rows; with U fixed it is one strongly convex problem of m d unknowns.

`lists_user_step` and `lists_item_step` minimise the two blocks with `population._newton` and `population._cg`, the same
damped Newton-CG iteration, rule, certificate and statuses; the problem classes are `ratings_exact`'s with the three
kernel calls replaced: the list loss and its score gradient (mfcd_list_pl) and the row Hessian applied to a score-space
vector with its diagonal (mfcd_list_pl_hvp), carried between entries and tables by mfcd_ragged_dot and
mfcd_ragged_gather_sum on the lists' layout.

A user without a stage (fewer than two entries, or depth 0) has a loss that is identically 0 and the zero row as
minimiser; such users are answered in closed form and never enter the solver, as `ratings_exact` answers users without a
pair.  `coef` overrides c: a caller who folds new users into a trained model passes the training lists' normaliser, so
that the ridge keeps the weight it had in training.  There is no CPU form of any of it."""
import torch

from . import _lib
from . import lists as L
from . import ratings_exact as RE
from .population import INVALID, PopulationFitResult, PopulationStepResult, _newton


class _ListKernels:
    """The three kernel calls of `ratings_exact._Problem`, on ranked lists."""

    def risk(self, a):
        return L.pl_rows(a, self.data, "loss")[0]

    def score_grad(self, a):
        return L.pl_rows(a, self.data, "grad")[2]

    def score_hvp(self, a, y, deg):
        out = L.pl_hvp_rows(a, y, self.data, deg)
        return (out[0], out[1]) if deg else (out[0], None)


class _UserProblem(_ListKernels, RE._UserProblem):
    """The users of `lists` as independent problems in u [n, d]: f = c * loss_u(u V[items_u]^T) + (l2 / 2) |u|^2."""

    def __init__(self, lists, V, coef, l2):
        RE._UserProblem.__init__(self, lists, V, 1.0, False, coef, l2)


class _ItemProblem(_ListKernels, RE._ItemProblem):
    """All of V as one problem, v = V flattened [1, m d]: f = c * sum over the users of loss_u + (l2 / 2) |v|^2."""

    def __init__(self, lists, U, m, coef, l2):
        RE._ItemProblem.__init__(self, lists, U, m, 1.0, False, coef, l2)


def _setup(U, V, lists, l2, coef, who):
    """The checks the steps share → (U or None, V, the normaliser c), the tables detached and contiguous."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (V,) + (() if U is None else (U,))):
        raise _lib.MfcdError(f"{who} needs U and V on a GPU device (there is no CPU fallback)")
    if V.dtype != torch.float32 or (U is not None and U.dtype != torch.float32):
        raise _lib.MfcdError(f"{who} takes float32 factor tables")
    L._need_lists(lists, who)
    if not float(l2) > 0.0:
        raise ValueError("l2 must be > 0: the block problems are strongly convex only with the ridge")
    if V.dim() != 2 or V.shape[0] != lists.m or (U is not None and tuple(U.shape) != (lists.n, V.shape[1])):
        raise ValueError(f"tables of shapes {None if U is None else tuple(U.shape)}, {tuple(V.shape)} for lists of "
                         f"{lists.n} users, {lists.m} items")
    stages = L._stages(lists)                                              # lists without a stage: ValueError
    if coef is None:
        coef = 1.0 / stages
    elif not 0.0 < float(coef) < float("inf"):
        raise ValueError("coef must be positive and finite")
    return (None if U is None else U.detach().contiguous()), V.detach().contiguous(), float(coef)


def _user_step(U, V, lists, l2, coef, gtol, max_newton, max_cg):
    d, dev = V.shape[1], V.device
    max_cg = min(d, 64) if max_cg is None else int(max_cg)
    staged = torch.from_numpy(lists.user_stages > 0).to(dev)              # a function of the lists alone
    start = torch.zeros((lists.n, d), dtype=torch.float64, device=dev) if U is None else U.double()
    # a user without a stage starts at its minimiser, the zero row: certified before the first iteration
    x0 = torch.where(staged[:, None], start, torch.zeros_like(start))
    prob = _UserProblem(lists, V, coef, float(l2))
    x, status, newton, cgs, f0, f, ratio = _newton(prob, x0, float(l2), float(gtol), max_newton, max_cg)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    x = torch.where((status == INVALID)[:, None], nan, x)
    rows = torch.where(staged[:, None], x, zero).float()                  # the closed form: exactly +0
    none = torch.zeros_like(status)
    return PopulationStepResult(rows, torch.where(staged, status, none), torch.where(staged, newton, none),
                                torch.where(staged, cgs, none),
                                torch.where(staged, f0, 0.5 * float(l2) * (start * start).sum(1)),
                                torch.where(staged, f, zero), torch.where(staged, ratio, zero))


def lists_user_step(U, V, lists, l2, coef=None, gtol=1e-3, max_newton=20, max_cg=None):
    """fp32 tables U [lists.n, d] (None: zeros) and V [lists.m, d] on a GPU, a `lists.RankedLists` there, l2 > 0 →
    `population.PopulationStepResult`: with V fixed, for every user of `lists` the minimiser over the user's row u of
        f(u) = c * (the Plackett–Luce loss of u V[items_u]^T on the user's list) + (l2 / 2) |u|^2,
    c = 1 / lists.stages or `coef`, started at the row of U.  U=None is the fold-in of users who were not in training:
    their vectors from one ranked list each (pass the training lists' normaliser as `coef`).  All users advance in
    lockstep through the same kernel calls (`population._newton`); max_cg: CG iterations per Newton step (None:
    min(d, 64)).  A user without a stage gets the zero row, status 0, 0 iterations and objective_after 0 in closed form.
    A user with a non-finite score, or whose list names an item outside V, gets status 2 and a NaN row; the other users'
    problems are those of a call without that user.  Lists without any stage: ValueError.  The inputs are not modified."""
    U, V, coef = _setup(U, V, lists, l2, coef, "the list user step")
    return _user_step(U, V, lists, l2, coef, gtol, max_newton, max_cg)


def _item_step(U, V, lists, l2, coef, gtol, max_newton, max_cg):
    prob = _ItemProblem(lists, U, V.shape[0], coef, float(l2))
    x, status, newton, cgs, f0, f, ratio = _newton(prob, V.double().reshape(1, -1), float(l2), float(gtol), max_newton,
                                                   int(max_cg))
    rows = torch.where(status == INVALID, V.reshape(1, -1), x.float()).reshape(V.shape)
    return PopulationStepResult(rows, status[0], newton[0], cgs[0], f0[0], f[0], ratio[0])


def lists_item_step(U, V, lists, l2, coef=None, gtol=1e-3, max_newton=20, max_cg=25):
    """`lists_user_step`'s twin: with U fixed, the minimiser over all of V of
        f(V) = c * (sum over the users of the Plackett–Luce loss of U[u] V[items_u]^T) + (l2 / 2) |V|^2
    — one problem of m d unknowns, because a user's list couples its items — started at V → PopulationStepResult with
    rows = V [m, d] and 0-dim fields: certified when |grad f|_F <= gtol l2 max |V|.  A non-finite score anywhere gives
    status 2 and V unchanged.  The inputs are not modified."""
    if U is None:
        raise _lib.MfcdError("the list item step needs U and V on a GPU device (there is no CPU fallback)")
    U, V, coef = _setup(U, V, lists, l2, coef, "the list item step")
    return _item_step(U, V, lists, l2, coef, gtol, max_newton, max_cg)


def fit_lists_exact(U, V, lists, l2, sweeps, gtol=1e-3, max_newton=20):
    """`sweeps` sweeps of one exact user step and one exact item step of F, in place on the contiguous fp32 tables U and
    V → `population.PopulationFitResult`; F is recorded after every sub-step (`objective_start`: at the tables given)
    and does not increase.  A step with status 2 changes nothing of the rows it names."""
    sweeps = int(sweeps)
    if sweeps < 0:
        raise ValueError("sweeps must be >= 0")
    if U is None:
        raise _lib.MfcdError("the exact list fit needs U and V on a GPU device (there is no CPU fallback)")
    Ud, Vd, coef = _setup(U, V, lists, l2, None, "the exact list fit")
    if not (U.is_contiguous() and V.is_contiguous()):
        raise _lib.MfcdError("the exact list fit updates contiguous tables in place")
    l2, dev = float(l2), V.device
    history = torch.zeros((sweeps, 2), dtype=torch.float64, device=dev)
    user_status = torch.zeros(lists.n, dtype=torch.int32, device=dev)
    item_status = torch.zeros((), dtype=torch.int32, device=dev)
    start = None

    def penalty(t):
        return 0.5 * l2 * (t.double() ** 2).sum()

    with torch.no_grad():
        for k in range(sweeps):
            step = _user_step(Ud, Vd, lists, l2, coef, gtol, max_newton, None)   # Ud, Vd alias U, V
            if start is None:
                start = step.objective_before.sum() + penalty(V)
            U.copy_(torch.where((step.status != INVALID)[:, None], step.rows, U))
            user_status = step.status
            step = _item_step(Ud, Vd, lists, l2, coef, gtol, max_newton, 25)
            history[k, 0] = step.objective_before + penalty(U)
            V.copy_(step.rows)
            item_status = step.status
            history[k, 1] = step.objective_after + penalty(U)
    out = PopulationFitResult(U, V, history, user_status, item_status)
    out.objective_start = start
    return out
