"""Exact block steps of the ridge-regularised ratings objective
    F(U, V) = c * sum over the users of risk_u(U[u] V[items_u]^T) + (l2 / 2)(|U|^2 + |V|^2),
risk_u the `risk` sum of `ratings.pair_ragged_stats` over the pairs among the items user u rated and c = 1 /
data.support(skip_ties), `ratings.ratings_risk`'s global normaliser: mfcd/population.py on a ratings table.  With V fixed F
is strongly convex (modulus l2) and separable in the users' rows; with U fixed it is one strongly convex problem of m d
unknowns.

`ratings_user_step` and `ratings_item_step` minimise the two blocks with `population._newton` and `population._cg`, the
same damped Newton-CG iteration, rule, certificate and statuses; only the problem classes are new.  They are made of four
kernels: the entries' scores (mfcd_ragged_dot), the risk sums (mfcd_pair_ragged_stats), the score gradient
(mfcd_pair_ragged_grad) and the row Laplacian applied to a score-space vector with its diagonal (mfcd_pair_ragged_hvp),
carried between entries and tables by mfcd_ragged_gather_sum on the user side or on the item side.  The d-sized vectors
are f64 torch tensors, kernel inputs fp32; a solve adds no host wait to `_newton`'s one read per iteration.

A user without a supporting pair (fewer than two ratings; under skip_ties also ratings of one value only) has a risk
that is identically 0 and the zero row as minimiser.  Such users are answered in closed form and never enter the solver:
the certificate |grad f|_2 <= gtol l2 |u|_inf cannot be met by a non-zero iterate of a pure-ridge problem, and in f64 a
Newton step lands near 0 but not on it.

`coef` overrides c: a caller who folds new users into a trained model passes the training table's normaliser, so that
the ridge keeps the weight it had in training.  There is no CPU form of any of it."""
import torch

from . import _lib
from . import ratings as R
from .population import INVALID, PopulationFitResult, PopulationStepResult, _newton


def _gs(coef, data, table, side):
    return R.ragged_gather_sum(coef, data, table, side)[0].double()


class _Problem:
    """What the two blocks share: the four kernels on the entries' scores of one ratings table."""

    def __init__(self, data, s, skip_ties, coef, l2):
        self.data, self.s, self.skip, self.coef, self.l2 = data, s, skip_ties, coef, l2

    def risk(self, a):
        return R.pair_ragged_stats(a, self.data, self.s, "sums", self.skip)[1][:, 0]

    def score_grad(self, a):
        return R.pair_ragged_grad(a, self.data, self.s, self.skip)[0]

    def score_hvp(self, a, y, deg):
        out = R.pair_ragged_hvp(a, y, self.data, self.skip, deg)
        return (out[0], out[1]) if deg else (out[0], None)


class _UserProblem(_Problem):
    """The users of `data` as independent problems in u [n, d]: f = c * risk_u(u V[items_u]^T) + (l2 / 2) |u|^2."""

    def __init__(self, data, V, s, skip_ties, coef, l2):
        super().__init__(data, s, skip_ties, coef, l2)
        self.V, self.VV, self.user = V, V * V, data.user.long()

    def prepare(self, u):
        return R.ragged_scores(u.float(), self.V, self.data)[0]

    def select(self, ok, new, old):
        return torch.where(ok[self.user], new, old)

    def objective(self, a, u):
        return self.coef * self.risk(a) + 0.5 * self.l2 * (u * u).sum(1)

    def grad(self, a, u):
        return self.coef * _gs(self.score_grad(a), self.data, self.V, "user") + self.l2 * u

    def hess(self, a, u, p, deg):
        q, dg = self.score_hvp(a, self.prepare(p), deg)
        out = self.coef * _gs(q, self.data, self.V, "user") + self.l2 * p
        return out, (self.coef * _gs(dg, self.data, self.VV, "user") + self.l2 if deg else None)


class _ItemProblem(_Problem):
    """All of V as one problem, v = V flattened [1, m d]: f = c * sum over the users of risk_u + (l2 / 2) |v|^2."""

    def __init__(self, data, U, m, s, skip_ties, coef, l2):
        super().__init__(data, s, skip_ties, coef, l2)
        self.U, self.UU, self.shape = U, U * U, (m, U.shape[1])

    def prepare(self, v):
        return R.ragged_scores(self.U, v.reshape(self.shape).float(), self.data)[0]

    def select(self, ok, new, old):
        return torch.where(ok, new, old)

    def objective(self, a, v):
        return (self.coef * self.risk(a).sum() + 0.5 * self.l2 * (v * v).sum()).reshape(1)

    def grad(self, a, v):
        return self.coef * _gs(self.score_grad(a), self.data, self.U, "item").reshape(1, -1) + self.l2 * v

    def hess(self, a, v, p, deg):
        q, dg = self.score_hvp(a, self.prepare(p), deg)
        out = self.coef * _gs(q, self.data, self.U, "item").reshape(1, -1) + self.l2 * p
        return out, (self.coef * _gs(dg, self.data, self.UU, "item").reshape(1, -1) + self.l2 if deg else None)


def _setup(U, V, data, l2, skip_ties, coef, who):
    """The checks the steps share → (U or None, V, the normaliser c), the tables detached and contiguous."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (V,) + (() if U is None else (U,))):
        raise _lib.MfcdError(f"{who} needs U and V on a GPU device (there is no CPU fallback)")
    if V.dtype != torch.float32 or (U is not None and U.dtype != torch.float32):
        raise _lib.MfcdError(f"{who} takes float32 factor tables")
    R._need_data(data, who)
    if not float(l2) > 0.0:
        raise ValueError("l2 must be > 0: the block problems are strongly convex only with the ridge")
    if V.dim() != 2 or V.shape[0] != data.m or (U is not None and tuple(U.shape) != (data.n, V.shape[1])):
        raise ValueError(f"tables of shapes {None if U is None else tuple(U.shape)}, {tuple(V.shape)} for ratings of "
                         f"{data.n} users, {data.m} items")
    if coef is None:
        coef = 1.0 / R._support(data, skip_ties)
    elif not 0.0 < float(coef) < float("inf"):
        raise ValueError("coef must be positive and finite")
    return (None if U is None else U.detach().contiguous()), V.detach().contiguous(), float(coef)


def _user_step(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, max_cg):
    d, dev = V.shape[1], V.device
    max_cg = min(d, 64) if max_cg is None else int(max_cg)
    paired = torch.from_numpy(data.user_support(skip_ties) > 0).to(dev)     # a function of the table alone
    start = torch.zeros((data.n, d), dtype=torch.float64, device=dev) if U is None else U.double()
    # a user without a supporting pair starts at its minimiser, the zero row: certified before the first iteration
    x0 = torch.where(paired[:, None], start, torch.zeros_like(start))
    prob = _UserProblem(data, V, float(s), bool(skip_ties), coef, float(l2))
    x, status, newton, cgs, f0, f, ratio = _newton(prob, x0, float(l2), float(gtol), max_newton, max_cg)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    x = torch.where((status == INVALID)[:, None], nan, x)
    rows = torch.where(paired[:, None], x, zero).float()                    # the closed form: exactly +0
    none = torch.zeros_like(status)
    return PopulationStepResult(rows, torch.where(paired, status, none), torch.where(paired, newton, none),
                                torch.where(paired, cgs, none),
                                torch.where(paired, f0, 0.5 * float(l2) * (start * start).sum(1)),
                                torch.where(paired, f, zero), torch.where(paired, ratio, zero))


def ratings_user_step(U, V, data, s, l2, skip_ties=False, coef=None, gtol=1e-3, max_newton=20, max_cg=None):
    """fp32 tables U [data.n, d] (None: zeros) and V [data.m, d] on a GPU, a `ratings.RatingsData` there, l2 > 0 →
    `population.PopulationStepResult`: with V fixed, for every user of `data` the minimiser over the user's row u of
        f(u) = c * (risk sum of u V[items_u]^T against the user's ratings) + (l2 / 2) |u|^2,
    c = 1 / data.support(skip_ties) or `coef`, started at the row of U.  U=None is the fold-in of users who were not in
    training: their vectors from their ratings alone (pass the training table's normaliser as `coef`).  All users advance
    in lockstep through the same kernel calls (`population._newton`); max_cg: CG iterations per Newton step (None:
    min(d, 64)).  A user without a supporting pair gets the zero row, status 0, 0 iterations and objective_after 0 in
    closed form.  A user with a non-finite rating or score, or whose ratings name an item outside V, gets status 2 and a
    NaN row; the other users' problems are those of a call without that user.  The inputs are not modified."""
    U, V, coef = _setup(U, V, data, l2, skip_ties, coef, "the ratings user step")
    return _user_step(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, max_cg)


def _item_step(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, max_cg):
    prob = _ItemProblem(data, U, V.shape[0], float(s), bool(skip_ties), coef, float(l2))
    x, status, newton, cgs, f0, f, ratio = _newton(prob, V.double().reshape(1, -1), float(l2), float(gtol), max_newton,
                                                   int(max_cg))
    rows = torch.where(status == INVALID, V.reshape(1, -1), x.float()).reshape(V.shape)
    return PopulationStepResult(rows, status[0], newton[0], cgs[0], f0[0], f[0], ratio[0])


def ratings_item_step(U, V, data, s, l2, skip_ties=False, coef=None, gtol=1e-3, max_newton=20, max_cg=25):
    """`ratings_user_step`'s twin: with U fixed, the minimiser over all of V of
        f(V) = c * (sum over the users of the risk sum of U[u] V[items_u]^T) + (l2 / 2) |V|^2
    — one problem of m d unknowns, because a user's pairs couple the items — started at V → PopulationStepResult with
    rows = V [m, d] and 0-dim fields: certified when |grad f|_F <= gtol l2 max |V|.  A non-finite rating or score
    anywhere gives status 2 and V unchanged.  The inputs are not modified."""
    if U is None:
        raise _lib.MfcdError("the ratings item step needs U and V on a GPU device (there is no CPU fallback)")
    U, V, coef = _setup(U, V, data, l2, skip_ties, coef, "the ratings item step")
    return _item_step(U, V, data, s, l2, skip_ties, coef, gtol, max_newton, max_cg)


def fit_ratings_exact(U, V, data, s, l2, sweeps, skip_ties=False, gtol=1e-3, max_newton=20):
    """`sweeps` sweeps of one exact user step and one exact item step of F, in place on the contiguous fp32 tables U and
    V → `population.PopulationFitResult`; F is recorded after every sub-step (`objective_start`: at the tables given)
    and does not increase.  A step with status 2 changes nothing of the rows it names."""
    sweeps = int(sweeps)
    if sweeps < 0:
        raise ValueError("sweeps must be >= 0")
    if U is None:
        raise _lib.MfcdError("the exact ratings fit needs U and V on a GPU device (there is no CPU fallback)")
    Ud, Vd, coef = _setup(U, V, data, l2, skip_ties, None, "the exact ratings fit")
    if not (U.is_contiguous() and V.is_contiguous()):
        raise _lib.MfcdError("the exact ratings fit updates contiguous tables in place")
    l2, dev = float(l2), V.device
    history = torch.zeros((sweeps, 2), dtype=torch.float64, device=dev)
    user_status = torch.zeros(data.n, dtype=torch.int32, device=dev)
    item_status = torch.zeros((), dtype=torch.int32, device=dev)
    start = None

    def penalty(t):
        return 0.5 * l2 * (t.double() ** 2).sum()

    with torch.no_grad():
        for k in range(sweeps):
            step = _user_step(Ud, Vd, data, s, l2, skip_ties, coef, gtol, max_newton, None)   # Ud, Vd alias U, V
            if start is None:
                start = step.objective_before.sum() + penalty(V)
            U.copy_(torch.where((step.status != INVALID)[:, None], step.rows, U))
            user_status = step.status
            step = _item_step(Ud, Vd, data, s, l2, skip_ties, coef, gtol, max_newton, 25)
            history[k, 0] = step.objective_before + penalty(U)
            V.copy_(step.rows)
            item_status = step.status
            history[k, 1] = step.objective_after + penalty(U)
    out = PopulationFitResult(U, V, history, user_status, item_status)
    out.objective_start = start
    return out
