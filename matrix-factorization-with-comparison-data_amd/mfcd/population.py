"""Exact block steps of the ridge-regularised population objective
    F(U, V) = R(U, V) + (l2 / 2)(|U|^2 + |V|^2),
R the exact all-pairs BTL risk `pairs.population_risk` (mean over users and pairs) or, under a `pairs.PairLaw`,
`pairs.law_risk` (sum of w * loss / sum of w): the objective whose stationary points `pairs.fit_population` / `fit_law`
approach under Adam's coupled weight decay l2.  With V fixed F is strongly convex (modulus l2) and separable in the
users' rows; with U fixed it is strongly convex in V, one problem of m d unknowns because pairs couple the items.

`population_user_step` and `population_item_step` minimise the two blocks by a damped Newton iteration.  The direction
is taken from Jacobi-preconditioned conjugate gradients on products with the block's Hessian  c V^T L(a) V + l2 I  (c
the risk's normaliser, L the row Laplacian of `pairs.pair_hvp_rows`), the preconditioner from the Laplacian's diagonal:
c deg (V o V) + l2.  The step is accepted by the Armijo rule on the objective itself, from `pairs.pair_stats_rows`; a
rejected step leaves the iterate where it was and halves the row's step length for the next iteration, so the objective
never increases; when every row still moving was rejected, the direction is kept and no Hessian product is issued.  All users of a block advance in lockstep through the same kernel calls, each under its own mask.

The d-sized vectors, their dot products and the iterate are f64 torch tensors; scores and kernel inputs are fp32; the
result is rounded to fp32 once.  One device -> host read per Newton iteration: the number of rows still moving.

A row is certified (status 0) when |grad f|_2 <= gtol l2 |u|_inf: by strong convexity it is then within gtol |u|_inf of
its minimiser.  The gradient is known only to the pair kernel's fp32 tolerance, hence gtol = 1e-3 and not an fp64
figure; at small l2 that tolerance, c (2e-5 |g_i| + 2e-6 (m - 1)) |V_i| summed over the items, can exceed gtol l2 |u|_inf,
and the certificate then cannot be reached: the row stops with status 1 and `grad_ratio` says what was reached.

`fit_population_exact` alternates the two steps.  No speed is promised: F is invariant under a joint rescaling of U and
V up to the penalty, so alternation converges linearly and slowly at small l2, as for any alternating scheme.  There is
no CPU form of any of it.

The user step also has a direct form (solver="direct"): the d x d Hessian  c V^T L(a) V + l2 I  of every row is formed by
`pairs.pair_info_rows` (one multi-column kernel call instead of one Hessian-vector call per CG iteration) and the
direction comes from a batched f64 Cholesky solve on the device; the Armijo rule, the certificate and the statuses are
the same.  The item step has no such form: its Hessian is (m d) x (m d)."""
import collections

import torch

from . import _lib
from . import pairs as P
from .rows import RowBlocks, blocks as _blocks

CONVERGED, STOPPED, INVALID = 0, 1, 2
ARMIJO = 1e-4            # sufficient-decrease constant
MIN_STEP = 2.0 ** -12    # a row whose step length falls below this has found no Armijo decrease: it stops
SOLVERS = ("cg", "direct")
DIRECT_BYTES = 64 << 20  # the direct user step keeps a block's [b, d, d] f64 Hessians under this
CG_TOL = 1e-4            # relative residual at which a row's CG freezes: the products carry fp32 noise of about 2e-5


class PopulationStepResult(collections.namedtuple(
        "PopulationStepResult", ("rows", "status", "newton_iters", "cg_iters", "objective_before", "objective_after",
                                 "grad_ratio"))):
    """What the two steps return, on the tables' device.  User step: rows fp32 [k, d], the best-response row of every
    user named, in order; the other fields are [k]: status int32 (0 certified, 1 stopped: iteration cap or no Armijo
    decrease, 2 non-finite score or truth row: the row is NaN), newton_iters / cg_iters int32, objective_before /
    objective_after f64 (the user's c * risk sum + (l2 / 2) |u|^2 at the given and the returned row) and grad_ratio f64 =
    |grad f|_2 / (l2 |u|_inf) at the returned row (status 0 means grad_ratio <= gtol).  Item step: rows is V fp32 [m, d]
    and the other fields are 0-dim, for the one problem over all of V (Frobenius norm, largest entry); status 2 returns V
    unchanged."""


class PopulationFitResult(collections.namedtuple("PopulationFitResult", ("U", "V", "history", "user_status",
                                                                        "item_status"))):
    """What `fit_population_exact` returns: the tables it updated in place; history f64 [sweeps, 2], F after the user
    step and after the item step of each sweep; user_status int32 [k] and item_status (0-dim) of the last sweep.  The
    attribute `objective_start` (0-dim f64, not a field of the tuple) is F at the tables given."""
    objective_start = None


class _Block:
    """A block of users: their law, their truth rows and the pair kernels on them, restricted to the law's columns."""

    def __init__(self, src, law, r0, r1, s):
        self.s, self.m = s, src.m
        self.law = None if law is None else (law.for_rows(src.ids[r0:r1]) if law.per_user() else law)
        self.truth = self.take(src.truth(r0, r1))

    def take(self, rows):
        return rows if self.law is None else self.law.take(rows)

    def back(self, rows):
        return rows if self.law is None else self.law.put_back(rows, self.m)

    def risk(self, A):
        if self.law is None:
            return P.pair_stats_rows(A, self.truth, self.s, "sums")[1][:, 0]
        return P.pair_law_stats_rows(A, self.truth, self.law, self.s)[1][:, 1]

    def grad(self, A):
        if self.law is None:
            return P.pair_grad_rows(A, self.truth, self.s)
        return self.back(P.pair_law_grad_rows(A, self.truth, self.law, self.s))

    def hvp(self, A, Y, deg):
        out = P.pair_hvp_rows(A, Y, deg) if self.law is None else P.pair_law_hvp_rows(A, self.truth, Y, self.law, deg)
        return (self.back(out[0]), self.back(out[1])) if deg else (self.back(out), None)


class _UserProblem:
    """The rows of one block of users as independent problems in u [b, d]: f = c * risk(u V^T) + (l2 / 2) |u|^2."""

    def __init__(self, blk, V, coef, l2):
        self.blk, self.coef, self.l2 = blk, coef, l2
        self.V32, self.Vt, self.V64 = V, V.t(), V.double()
        self.VV = self.V64 * self.V64

    def prepare(self, u):
        return self.blk.take(u.float() @ self.Vt)

    def select(self, ok, new, old):
        return torch.where(ok[:, None], new, old)

    def objective(self, A, u):
        return self.coef * self.blk.risk(A) + 0.5 * self.l2 * (u * u).sum(1)

    def grad(self, A, u):
        return self.coef * (self.blk.grad(A).double() @ self.V64) + self.l2 * u

    def hess(self, A, u, p, deg):
        Q, D = self.blk.hvp(A, self.blk.take(p.float() @ self.Vt), deg)
        out = self.coef * (Q.double() @ self.V64) + self.l2 * p
        return out, (self.coef * (D.double() @ self.VV) + self.l2 if deg else None)

    def direct(self, A, g, active):
        """H p = -g by a Cholesky factorisation of every active row's c V^T L(a) V + l2 I → p (0 where not active).  A
        row whose matrix does not factor (the fp32 noise of the Laplacian against a tiny l2) takes the gradient scaled
        by the matrix's mean diagonal: still a descent direction, and the Armijo rule decides."""
        law = self.blk.law
        H = self.coef * P.pair_info_rows(A, self.V32, self.blk.truth, law, None if law is None else law.columns)
        d = H.shape[1]
        eye = torch.eye(d, dtype=torch.float64, device=H.device)
        H = torch.where(active[:, None, None], H + self.l2 * eye, eye)
        chol, info = torch.linalg.cholesky_ex(H)
        ok = info == 0
        chol = torch.where(ok[:, None, None], chol, eye)
        p = torch.cholesky_solve(-g[:, :, None], chol)[:, :, 0]
        p = torch.where(ok[:, None], p, -g / H.diagonal(dim1=1, dim2=2).mean(1, keepdim=True))
        return torch.where(active[:, None], p, torch.zeros_like(p))


class _ItemProblem:
    """All of V as one problem, v = V flattened [1, m d]: f = c * sum over the users of risk(U v^T) + (l2 / 2) |v|^2.
    Every evaluation walks the users' blocks and forms their scores anew; nothing n x m is kept."""

    def __init__(self, src, law, s, coef, l2):
        self.src, self.law, self.s, self.coef, self.l2 = src, law, s, coef, l2
        self.shape = tuple(src.V.shape)

    def _blocks(self, v):
        Vt = v.reshape(self.shape).float().t()
        for r0, r1 in self.src.blocks():
            blk = _Block(self.src, self.law, r0, r1, self.s)
            Ub = self.src.rows_of(self.src.U, r0, r1)
            yield blk, Ub, blk.take(Ub @ Vt)

    def prepare(self, v):
        return None

    def select(self, ok, new, old):
        return None

    def objective(self, _, v):
        total = torch.zeros((), dtype=torch.float64, device=v.device)
        for blk, _, A in self._blocks(v):
            total += blk.risk(A).sum()
        return (self.coef * total + 0.5 * self.l2 * (v * v).sum()).reshape(1)

    def grad(self, _, v):
        out = torch.zeros(self.shape, dtype=torch.float64, device=v.device)
        for blk, Ub, A in self._blocks(v):
            out.addmm_(blk.grad(A).double().t(), Ub.double())
        return self.coef * out.reshape(1, -1) + self.l2 * v

    def hess(self, _, v, p, deg):
        out = torch.zeros(self.shape, dtype=torch.float64, device=v.device)
        diag = torch.zeros_like(out) if deg else None
        Pt = p.reshape(self.shape).float().t()
        for blk, Ub, A in self._blocks(v):
            Q, D = blk.hvp(A, blk.take(Ub @ Pt), deg)
            U64 = Ub.double()
            out.addmm_(Q.double().t(), U64)
            if deg:
                diag.addmm_(D.double().t(), U64 * U64)
        return self.coef * out.reshape(1, -1) + self.l2 * p, (self.coef * diag.reshape(1, -1) + self.l2 if deg else None)


def _dot(a, b):
    return (a * b).sum(1)


def _cg(prob, state, x, g, active, max_cg):
    """H p = -g for the rows of `active`, in lockstep and without a host read: the exact Cauchy point (its product also
    yields the preconditioner), then `max_cg` preconditioned CG iterations; a row freezes once its residual is below
    CG_TOL |g| → (p, with 0 for rows that are not active; CG iterations per row)."""
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    b = torch.where(active[:, None], -g, zero)
    Hb, M = prob.hess(state, x, b, True)
    bb = _dot(b, b)
    live = active & (bb > 0)
    Hb = torch.where(live[:, None], Hb, zero)
    M = torch.where(live[:, None], M, zero + 1.0)
    a0 = torch.where(live, bb / _dot(b, Hb), zero)
    p = a0[:, None] * b
    r = b - a0[:, None] * Hb
    z = r / M
    q, rz = z, _dot(r, z)
    its = live.to(torch.int32)
    for _ in range(max_cg):
        live = live & (_dot(r, r) > CG_TOL ** 2 * bb)
        q = torch.where(live[:, None], q, zero)
        Hq = torch.where(live[:, None], prob.hess(state, x, q, False)[0], zero)
        qHq = _dot(q, Hq)
        a = torch.where(live & (qHq > 0), rz / qHq, zero)
        p = p + a[:, None] * q
        r = r - a[:, None] * Hq
        z = r / M
        rz_new = _dot(r, z)
        beta = torch.where(live & (rz > 0), rz_new / rz, zero)
        q, rz = z + beta[:, None] * q, rz_new
        its = its + live.to(torch.int32)
    return p, its


def _newton(prob, x, l2, gtol, max_newton, max_cg, solver="cg"):
    """Damped Newton-CG (solver="direct": damped Newton with `prob.direct`'s directions) on the rows of x [b, D] (f64) →
    (x, status, newton_iters, cg_iters, f0, f, grad_ratio)."""
    max_newton = int(max_newton)
    if max_newton < 0:
        raise ValueError("max_newton must be >= 0")
    b, dev = x.shape[0], x.device
    state = prob.prepare(x)
    f = prob.objective(state, x)
    f0 = f.clone()
    invalid = ~torch.isfinite(f)
    active = ~invalid
    done = torch.zeros(b, dtype=torch.bool, device=dev)
    t = torch.ones(b, dtype=torch.float64, device=dev)
    newton = torch.zeros(b, dtype=torch.int32, device=dev)
    cgs = torch.zeros(b, dtype=torch.int32, device=dev)
    moved, p = torch.ones(b, dtype=torch.bool, device=dev), None
    for it in range(max_newton + 1):
        g = prob.grad(state, x)
        gnorm, bound = torch.linalg.vector_norm(g, dim=1), l2 * x.abs().amax(1)
        conv = active & (gnorm <= gtol * bound)
        done, active = done | conv, active & ~conv
        if it == max_newton:
            break
        n_active, n_moved = torch.stack((active.sum(), (active & moved).sum())).tolist()   # the iteration's one host read
        if n_active == 0:
            break
        if (n_moved or p is None) and solver == "direct":
            p, its = prob.direct(state, g, active), torch.zeros_like(cgs)
        elif n_moved or p is None:
            p, its = _cg(prob, state, x, g, active, max_cg)
        else:            # every row still active had its step rejected: x, and with it the direction, is what it was
            p, its = torch.where(active[:, None], p, torch.zeros_like(p)), torch.zeros_like(cgs)
        xt = x + torch.where(active, t, torch.zeros_like(t))[:, None] * p
        st = prob.prepare(xt)
        ft = prob.objective(st, xt)
        ok = active & (ft <= f + ARMIJO * t * _dot(g, p))         # a NaN trial is a rejected one
        x, f, state = torch.where(ok[:, None], xt, x), torch.where(ok, ft, f), prob.select(ok, st, state)
        newton, cgs = newton + active.to(torch.int32), cgs + its
        t = torch.where(ok, torch.clamp(2.0 * t, max=1.0), 0.5 * t)
        active, moved = active & (t >= MIN_STEP), ok
    status = torch.full((b,), STOPPED, dtype=torch.int32, device=dev)
    status = torch.where(done, torch.zeros_like(status), status)
    status = torch.where(invalid, torch.full_like(status, INVALID), status)
    return x, status, newton, cgs, f0, f, gnorm / bound


def _setup(U, V, X, s, l2, law, users, row_block, who):
    """The checks the two steps share → (RowBlocks, the law or None for the plain risk, the risk's normaliser c)."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (U, V)):
        raise _lib.MfcdError(f"{who} needs U and V on a GPU device (there is no CPU fallback)")
    if U.dtype != torch.float32 or V.dtype != torch.float32:
        raise _lib.MfcdError(f"{who} takes float32 factor tables")
    if not float(l2) > 0.0:
        raise ValueError("l2 must be > 0: the block problems are strongly convex only with the ridge")
    U, V = U.detach().contiguous(), V.detach().contiguous()
    if law is None or law.trivial:
        src = RowBlocks(U, V, X, users, row_block, who)
        if src.m < 2:
            raise ValueError("the population risk needs at least two items (m >= 2)")
        if src.k == 0:
            raise ValueError("the population risk needs at least one user")
        return src, None, 1.0 / (src.k * (src.m * (src.m - 1) // 2))
    src = P._law_src(U, V, X, users, row_block, law, who)
    if src.k == 0:
        raise ValueError("the population risk needs at least one user")
    total = float(P.law_weight_total(src, law, s))                # a function of X alone: the one host wait of the set-up
    if not total > 0:
        raise ValueError("the law gives no pair of any user a weight: there is no risk to descend")
    return src, law, 1.0 / total


def population_user_step(U, V, X, s, l2, law=None, users=None, gtol=1e-3, max_newton=20, row_block=2048, max_cg=None,
                         solver="cg"):
    """fp32 tables U [n, d], V [m, d] on a GPU, X dense or a FactoredMatrix, l2 > 0 → PopulationStepResult: with V fixed,
    for every user named (None: every user; the law's users under a law) the minimiser over the user's row u of
        f(u) = c * (risk sum of u V^T against the user's truth row) + (l2 / 2) |u|^2,
    c = 1 / (users x pairs) for the plain risk and 1 / (sum of W over the users named) under a law — the part of F that
    holds the row — started at the row of U, `row_block` users at a time.  Every row named is a problem of its own (a user
    named twice is solved twice, from the same start).  max_cg: CG iterations per Newton step, all of them
    issued for the whole block since nothing reads the device inside a solve (None: min(d, 64)).  A
    user with a non-finite score or truth row gets status 2 and a NaN row, and under a law stays out of c (see
    `pairs.law_weight_total`: `pairs.law_risk` itself is NaN for such an input, so there is nothing else to agree
    with); the other users' problems are those of a call that does not name that user.  The inputs are not modified.
    solver="direct": every Newton direction from the row's d x d Hessian (`pairs.pair_info_rows`, d <= 256: ValueError
    beyond) and a batched f64 Cholesky solve instead of CG; `cg_iters` is 0, `max_cg` is not used, and the row block is
    shrunk so that a block's matrices stay under 64 MiB.  Rule, certificate and statuses are the same."""
    _check_solver(solver, U.shape[1] if torch.is_tensor(U) and U.dim() == 2 else 0)
    src, law, coef = _setup(U, V, X, s, l2, law, users, row_block, "the population user step")
    return _user_step(src, law, coef, s, l2, gtol, max_newton, max_cg, solver)


def _check_solver(solver, d):
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "direct" and d > P.INFO_MAX_D:
        raise ValueError(f"the direct user step forms d x d matrices for d <= {P.INFO_MAX_D}, got d = {d}")


def _user_step(src, law, coef, s, l2, gtol, max_newton, max_cg, solver="cg"):
    d = src.U.shape[1]
    _check_solver(solver, d)
    max_cg = min(d, 64) if max_cg is None else int(max_cg)
    row_block = src.row_block if solver == "cg" else min(src.row_block, max(1, DIRECT_BYTES // (8 * d * d)))
    parts = []
    for r0, r1 in _blocks(src.k, row_block):
        prob = _UserProblem(_Block(src, law, r0, r1, float(s)), src.V, coef, float(l2))
        parts.append(_newton(prob, src.rows_of(src.U, r0, r1).double(), float(l2), float(gtol), max_newton, max_cg,
                             solver))
    x, status, newton, cgs, f0, f, ratio = (torch.cat(t) for t in zip(*parts))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=src.dev)
    rows = torch.where((status == INVALID)[:, None], nan, x).float()
    return PopulationStepResult(rows, status, newton, cgs, f0, f, ratio)


def population_item_step(U, V, X, s, l2, law=None, gtol=1e-3, max_newton=20, row_block=2048, max_cg=25):
    """`population_user_step`'s twin: with U fixed, the minimiser over all of V of
        f(V) = c * (sum over the users of the risk sum of U[u] V^T) + (l2 / 2) |V|^2
    — the part of F that holds V, one problem of m d unknowns — started at V, over every user (the law's users under a
    law) → PopulationStepResult with rows = V [m, d] and 0-dim fields: certified when |grad f|_F <= gtol l2 max |V|.
    A non-finite score or truth row anywhere gives status 2 and V unchanged.  The inputs are not modified."""
    src, law, coef = _setup(U, V, X, s, l2, law, None, row_block, "the population item step")
    return _item_step(src, law, coef, s, l2, gtol, max_newton, max_cg)


def _item_step(src, law, coef, s, l2, gtol, max_newton, max_cg):
    prob = _ItemProblem(src, law, float(s), coef, float(l2))
    x, status, newton, cgs, f0, f, ratio = _newton(prob, src.V.double().reshape(1, -1), float(l2), float(gtol), max_newton,
                                                   int(max_cg))
    rows = torch.where(status == INVALID, src.V.reshape(1, -1), x.float()).reshape(src.V.shape)
    return PopulationStepResult(rows, status[0], newton[0], cgs[0], f0[0], f[0], ratio[0])


def fit_population_exact(U, V, X, s, l2, sweeps, law=None, gtol=1e-3, max_newton=20, row_block=2048, user_solver="cg"):
    """`sweeps` sweeps of one exact user step and one exact item step of F, in place on the fp32 tables U and V →
    PopulationFitResult; F is recorded after every sub-step and does not increase.  Under a law that names its users the
    rows of the other users are left as they are (only the penalty holds them).  A step with status 2 changes nothing.
    The set-up (checks, row blocks, a law's weight total and its one host wait) is done once, before the first sweep.
    user_solver: the `solver` of the user steps ("cg" or "direct", see `population_user_step`)."""
    _check_solver(user_solver, U.shape[1] if torch.is_tensor(U) and U.dim() == 2 else 0)
    sweeps = int(sweeps)
    if sweeps < 0:
        raise ValueError("sweeps must be >= 0")
    src, law, coef = _setup(U, V, X, s, l2, law, None, row_block, "the exact population fit")
    if not (U.is_contiguous() and V.is_contiguous()):
        raise _lib.MfcdError("the exact population fit updates contiguous tables in place")
    l2 = float(l2)
    history = torch.zeros((sweeps, 2), dtype=torch.float64, device=src.dev)
    user_status = torch.zeros(src.k, dtype=torch.int32, device=src.dev)
    item_status = torch.zeros((), dtype=torch.int32, device=src.dev)
    start = None

    def penalty(t):
        return 0.5 * l2 * (t.double() ** 2).sum()

    with torch.no_grad():
        for k in range(sweeps):
            step = _user_step(src, law, coef, s, l2, gtol, max_newton, None, user_solver)   # src reads U and V in place
            if start is None:
                start = step.objective_before.sum() + penalty(V) + (0.0 if src.whole else penalty(U) - penalty(U[src.ids]))
            good = (step.status != INVALID)[:, None]
            if src.whole:
                U.copy_(torch.where(good, step.rows, U))
            else:
                U[src.ids] = torch.where(good, step.rows, U[src.ids])
            user_status = step.status
            step = _item_step(src, law, coef, s, l2, gtol, max_newton, 25)
            history[k, 0] = step.objective_before + penalty(U)
            V.copy_(step.rows)
            item_status = step.status
            history[k, 1] = step.objective_after + penalty(U)
    out = PopulationFitResult(U, V, history, user_status, item_status)
    out.objective_start = start
    return out
