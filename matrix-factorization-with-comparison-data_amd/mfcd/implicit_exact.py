"""Exact block steps of the ridge-regularised implicit-feedback objective
    F(U, V) = sum over the users of c_u R_u(U[u] V^T) + (l2 / 2)(|U|^2 + |V|^2),
R_u the observed-versus-unobserved risk sum of `implicit.implicit_rows` and c_u the normaliser of
`implicit.implicit_risk` (normalize="pairs": 1 / total pairs; "user": 1 / (users with a pair x the user's pairs)):
mfcd/population.py on a table of observed items.  With V fixed F is strongly convex (modulus l2) and separable in the
users' rows; with U fixed it is one strongly convex problem of m d unknowns.

`implicit_user_step` and `implicit_item_step` minimise the two blocks with `population._newton` and `population._cg`, the
same damped Newton-CG iteration, rule, certificate and statuses; only the problem classes are new.  The state carried
through the iteration is the fp32 table being solved for: every evaluation forms the scores anew through the kernels'
bounded slab, in blocks of `row_block` users, so nothing n x m is kept.  Three kernels: the risk sums and the score
gradient (mfcd_implicit_rows) and the score-space Laplacian applied to a direction with its diagonal
(mfcd_implicit_hvp_rows: the user step passes B = By = V, the item step A = Ay = U), carried between score rows and
tables by library GEMMs in f64.  A solve adds no host wait to `_newton`'s one read per iteration.

A user without an (observed, unobserved) pair has a risk that is identically 0 and the zero row as minimiser.  Such
users are answered in closed form and never move in the solver, for the reason mfcd/ratings_exact.py gives: the
certificate |grad f|_2 <= gtol l2 |u|_inf cannot be met by a non-zero iterate of a pure-ridge problem.

`coef` overrides c_u (a scalar, or one value per user): a caller who folds new users into a trained model passes the
training table's normaliser, so that the ridge keeps the weight it had in training.  A user's row depends on nothing but
its own lists, its coefficient and V; the user-side GEMMs run on blocks padded to whole multiples of 128 rows, so the
row does not depend on how many users the call names either, as long as both calls pad to the same height.  There is
no CPU form of any of it."""
import torch

from . import _lib
from . import implicit as I
from .population import INVALID, PopulationFitResult, PopulationStepResult, _newton

_PAD = 128      # user-side GEMMs see whole multiples of this many rows


class _Problem:
    """What the two blocks share: the plan of a table (lists, coefficients, row blocks) and the two kernels on it, with
    the scores A B^T and the direction Ay By^T formed per call."""

    def __init__(self, plan, l2):
        self.plan, self.l2 = plan, l2
        height = (min(plan.row_block, plan.n) + _PAD - 1) // _PAD * _PAD
        self.buf = torch.zeros((2, height, plan.m), dtype=torch.float32, device=plan.dev)

    def _blocks(self):
        p, rb = self.plan, self.plan.row_block
        p_off, p_items, entries, e_off, e_items, excl_entries = p.lists
        for u0 in range(0, p.n, rb):
            u1 = min(p.n, u0 + rb)
            yield u0, u1, (p_off[u0:u1 + 1], p_items, entries, e_off[u0:u1 + 1] if e_off is not None else None, e_items,
                           excl_entries)

    def risk(self, A, B):
        """c_u R_u of every user → f64 [n]; NaN for a user with an invalid list or a non-finite score."""
        p, d = self.plan, A.shape[1]
        for u0, u1, lists in self._blocks():
            I._launch(None, A, B, p.n, p.m, d, p.dev, p.ids[u0:u1], u1 - u0, *lists, None, p.counts[u0:u1], p.sums[u0:u1],
                      None, p.status[u0:u1])
        return p.coef64 * p.sums

    def score_grad(self, A, B):
        """Per block (u0, u1, g): g fp32 [u1 - u0, m], the gradient of c_u R_u with respect to the score rows."""
        p, d = self.plan, A.shape[1]
        for u0, u1, lists in self._blocks():
            g = self.buf[0, :u1 - u0]
            I._launch(None, A, B, p.n, p.m, d, p.dev, p.ids[u0:u1], u1 - u0, *lists, p.coef[u0:u1], p.counts[u0:u1],
                      p.sums[u0:u1], g, p.status[u0:u1])
            yield u0, u1, g

    def score_hvp(self, A, B, Ay, By, deg):
        """Per block (u0, u1, q, deg or None): the Laplacian of c_u R_u applied to the rows of Ay By^T, its diagonal."""
        p, d = self.plan, A.shape[1]
        for u0, u1, lists in self._blocks():
            q, dg = self.buf[0, :u1 - u0], self.buf[1, :u1 - u0] if deg else None
            I._launch_hvp(None, None, A, B, Ay, By, p.n, p.m, d, p.dev, p.ids[u0:u1], u1 - u0, *lists, p.coef[u0:u1], q, dg,
                          p.status[u0:u1])
            yield u0, u1, q, dg

    def padded(self, k, rows):
        """Block `k` of the scratch with its first `rows` rows filled, as f64 of whole multiples of _PAD rows.  The
        padding rows are zeroed: an earlier, taller block may have left anything there, NaN rows included."""
        height = (rows + _PAD - 1) // _PAD * _PAD
        self.buf[k, rows:height].zero_()
        return self.buf[k, :height].double()


class _UserProblem(_Problem):
    """The users of the plan as independent problems in u [n, d]: f = c_u R_u(u V^T) + (l2 / 2) |u|^2."""

    def __init__(self, plan, V, l2):
        super().__init__(plan, l2)
        self.V, self.V64 = V, V.double()
        self.VV = self.V64 * self.V64

    def prepare(self, u):
        return u.float().contiguous()

    def select(self, ok, new, old):
        return torch.where(ok[:, None], new, old)

    def objective(self, u32, u):
        return self.risk(u32, self.V) + 0.5 * self.l2 * (u * u).sum(1)

    def grad(self, u32, u):
        out = torch.empty_like(u)
        for u0, u1, _ in self.score_grad(u32, self.V):
            out[u0:u1] = (self.padded(0, u1 - u0) @ self.V64)[:u1 - u0]
        return out + self.l2 * u

    def hess(self, u32, u, p, deg):
        out = torch.empty_like(u)
        diag = torch.empty_like(u) if deg else None
        for u0, u1, _, dg in self.score_hvp(u32, self.V, p.float().contiguous(), self.V, deg):
            out[u0:u1] = (self.padded(0, u1 - u0) @ self.V64)[:u1 - u0]
            if deg:
                diag[u0:u1] = (self.padded(1, u1 - u0) @ self.VV)[:u1 - u0]
        return out + self.l2 * p, (diag + self.l2 if deg else None)


class _ItemProblem(_Problem):
    """All of V as one problem, v = V flattened [1, m d]: f = sum over the users of c_u R_u(U[u] v^T) + (l2 / 2) |v|^2."""

    def __init__(self, plan, U, l2):
        super().__init__(plan, l2)
        self.U, self.U64, self.shape = U, U.double(), (plan.m, U.shape[1])
        self.UU = self.U64 * self.U64

    def prepare(self, v):
        return v.reshape(self.shape).float().contiguous()

    def select(self, ok, new, old):
        return torch.where(ok, new, old)

    def objective(self, V32, v):
        return (self.risk(self.U, V32).sum() + 0.5 * self.l2 * (v * v).sum()).reshape(1)

    def grad(self, V32, v):
        out = torch.zeros(self.shape, dtype=torch.float64, device=v.device)
        for u0, u1, g in self.score_grad(self.U, V32):
            out.addmm_(g.double().t(), self.U64[u0:u1])
        return out.reshape(1, -1) + self.l2 * v

    def hess(self, V32, v, p, deg):
        out = torch.zeros(self.shape, dtype=torch.float64, device=v.device)
        diag = torch.zeros_like(out) if deg else None
        for u0, u1, q, dg in self.score_hvp(self.U, V32, self.U, p.reshape(self.shape).float().contiguous(), deg):
            out.addmm_(q.double().t(), self.U64[u0:u1])
            if deg:
                diag.addmm_(dg.double().t(), self.UU[u0:u1])
        return out.reshape(1, -1) + self.l2 * p, (diag.reshape(1, -1) + self.l2 if deg else None)


def _users_of(data):
    if isinstance(data, (tuple, list)) and len(data) == 2 and torch.is_tensor(data[0]):
        return data[0].numel() - 1
    if hasattr(data, "n"):
        return data.n
    raise TypeError("data must be a RatingsData or a CSR pair (offsets, items)")


def _setup(U, V, data, l2, exclude, normalize, coef, row_block, who):
    """The checks the steps share → (U or None, V, the table's plan with the coefficients c_u), the tables detached and
    contiguous.  plan.closed: the users answered in closed form."""
    if not float(l2) > 0.0:
        raise ValueError("l2 must be > 0: the block problems are strongly convex only with the ridge")
    if not all(torch.is_tensor(t) for t in (V,) + (() if U is None else (U,))):
        raise _lib.MfcdError(f"{who} needs U and V on a GPU device (there is no CPU fallback)")
    n = _users_of(data)
    if V.dim() != 2 or (U is not None and (U.dim() != 2 or tuple(U.shape) != (n, V.shape[1]))):
        raise ValueError(f"tables of shapes {None if U is None else tuple(U.shape)}, {tuple(V.shape)} for a table of "
                         f"{n} users")
    if not all(t.is_cuda for t in (V,) + (() if U is None else (U,))):
        raise _lib.MfcdError(f"{who} needs U and V on a GPU device (there is no CPU fallback)")
    if V.dtype != torch.float32 or (U is not None and U.dtype != torch.float32):
        raise _lib.MfcdError(f"{who} takes float32 factor tables")
    dev = V.device
    plan = I._Plan(n, V.shape[0], dev, data, exclude, normalize, row_block)
    paired = plan.coef64 > 0
    plan.closed = ~paired & (plan.status == 0)
    if coef is not None:
        c = torch.as_tensor(coef, dtype=torch.float64, device=dev).reshape(-1)
        if c.numel() not in (1, n):
            raise ValueError(f"{c.numel()} coefficients for {n} users")
        if not bool(((c > 0) & torch.isfinite(c)).all()):
            raise ValueError("coef must be positive and finite")
        plan.coef64 = torch.where(paired, c.expand(n), torch.zeros_like(plan.coef64))
        plan.coef = plan.coef64.float()
    return (None if U is None else U.detach().contiguous()), V.detach().contiguous(), plan


def _user_step(plan, U, V, l2, gtol, max_newton, max_cg):
    d, dev = V.shape[1], V.device
    max_cg = min(d, 64) if max_cg is None else int(max_cg)
    closed = plan.closed
    start = torch.zeros((plan.n, d), dtype=torch.float64, device=dev) if U is None else U.double()
    # a user without a pair starts at its minimiser, the zero row: certified before the first iteration
    x0 = torch.where(closed[:, None], torch.zeros_like(start), start)
    x, status, newton, cgs, f0, f, ratio = _newton(_UserProblem(plan, V, float(l2)), x0, float(l2), float(gtol), max_newton,
                                                   max_cg)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    x = torch.where((status == INVALID)[:, None], nan, x)
    rows = torch.where(closed[:, None], zero, x).float()                    # the closed form: exactly +0
    none = torch.zeros_like(status)
    return PopulationStepResult(rows, torch.where(closed, none, status), torch.where(closed, none, newton),
                                torch.where(closed, none, cgs),
                                torch.where(closed, 0.5 * float(l2) * (start * start).sum(1), f0),
                                torch.where(closed, zero, f), torch.where(closed, zero, ratio))


def implicit_user_step(U, V, data, l2, exclude=None, normalize="pairs", coef=None, gtol=1e-3, max_newton=20, max_cg=None,
                       row_block=None):
    """fp32 tables U [n, d] (None: zeros) and V [m, d] on a GPU, the observed items of n users (a `ratings.RatingsData` on
    the device or a CSR pair), l2 > 0 → `population.PopulationStepResult`: with V fixed, for every user the minimiser
    over the user's row u of
        f(u) = c_u R_u(u V^T) + (l2 / 2) |u|^2,
    R_u the risk sum of `implicit.implicit_rows` under `exclude`, c_u the normaliser of `implicit.implicit_risk` under
    `normalize` or `coef` (a scalar, or one value per user), started at the row of U.  U=None is the fold-in of users who
    were not in training: their vectors from their observed items alone; `data` then lists just those users and `coef`
    carries the training table's normaliser.  All users advance in lockstep through the same kernel calls
    (`population._newton`), `row_block` users per call (None: `implicit.default_row_block`); max_cg: CG iterations per
    Newton step (None: min(d, 64)).  A user without an (observed, unobserved) pair gets the zero row, status 0, 0
    iterations and objective_after 0 in closed form.  A user with a non-finite score or an invalid list gets status 2 and
    a NaN row; the other users' problems are those of a call without that user.  The inputs are not modified."""
    U, V, plan = _setup(U, V, data, l2, exclude, normalize, coef, row_block, "the implicit user step")
    return _user_step(plan, U, V, l2, gtol, max_newton, max_cg)


def _item_step(plan, U, V, l2, gtol, max_newton, max_cg):
    x, status, newton, cgs, f0, f, ratio = _newton(_ItemProblem(plan, U, float(l2)), V.double().reshape(1, -1), float(l2),
                                                   float(gtol), max_newton, int(max_cg))
    rows = torch.where(status == INVALID, V.reshape(1, -1), x.float()).reshape(V.shape)
    return PopulationStepResult(rows, status[0], newton[0], cgs[0], f0[0], f[0], ratio[0])


def implicit_item_step(U, V, data, l2, exclude=None, normalize="pairs", coef=None, gtol=1e-3, max_newton=20, max_cg=25,
                       row_block=None):
    """`implicit_user_step`'s twin: with U fixed, the minimiser over all of V of
        f(V) = sum over the users of c_u R_u(U[u] V^T) + (l2 / 2) |V|^2
    — one problem of m d unknowns, because a user's pairs couple the items — started at V → PopulationStepResult with
    rows = V [m, d] and 0-dim fields: certified when |grad f|_F <= gtol l2 max |V|.  A non-finite score or an invalid
    list anywhere gives status 2 and V unchanged.  The inputs are not modified."""
    if U is None:
        raise _lib.MfcdError("the implicit item step needs U and V on a GPU device (there is no CPU fallback)")
    U, V, plan = _setup(U, V, data, l2, exclude, normalize, coef, row_block, "the implicit item step")
    return _item_step(plan, U, V, l2, gtol, max_newton, max_cg)


def fit_implicit_exact(U, V, data, l2, sweeps, exclude=None, normalize="pairs", gtol=1e-3, max_newton=20, row_block=None):
    """`sweeps` sweeps of one exact user step and one exact item step of F, in place on the contiguous fp32 tables U and
    V → `population.PopulationFitResult`; F is recorded after every sub-step (`objective_start`: at the tables given)
    and does not increase.  A step with status 2 changes nothing of the rows it names.  The plan of the table (lists,
    counts, coefficients) is made once, before the first sweep."""
    sweeps = int(sweeps)
    if sweeps < 0:
        raise ValueError("sweeps must be >= 0")
    if U is None:
        raise _lib.MfcdError("the exact implicit fit needs U and V on a GPU device (there is no CPU fallback)")
    Ud, Vd, plan = _setup(U, V, data, l2, exclude, normalize, None, row_block, "the exact implicit fit")
    if not (U.is_contiguous() and V.is_contiguous()):
        raise _lib.MfcdError("the exact implicit fit updates contiguous tables in place")
    l2, dev = float(l2), V.device
    history = torch.zeros((sweeps, 2), dtype=torch.float64, device=dev)
    user_status = torch.zeros(plan.n, dtype=torch.int32, device=dev)
    item_status = torch.zeros((), dtype=torch.int32, device=dev)
    start = None

    def penalty(t):
        return 0.5 * l2 * (t.double() ** 2).sum()

    with torch.no_grad():
        for k in range(sweeps):
            step = _user_step(plan, Ud, Vd, l2, gtol, max_newton, None)      # Ud, Vd alias U, V
            if start is None:
                start = step.objective_before.sum() + penalty(V)
            U.copy_(torch.where((step.status != INVALID)[:, None], step.rows, U))
            user_status = step.status
            step = _item_step(plan, Ud, Vd, l2, gtol, max_newton, 25)
            history[k, 0] = step.objective_before + penalty(U)
            V.copy_(step.rows)
            item_status = step.status
            history[k, 1] = step.objective_after + penalty(U)
    out = PopulationFitResult(U, V, history, user_status, item_status)
    out.objective_start = start
    return out
