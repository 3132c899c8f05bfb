"""Training and scoring on implicit feedback (include/mfcd.h: mfcd_implicit_rows): a user has observed items P_u —
clicks, purchases, "rated at all" — and the model is asked to put every one of them before every item the user has not
observed, exactly, over all L_u (m - L_u) such pairs and without forming anything n x m:

    R_u(a) = sum over i in P_u \\ E_u, j in N_u of softplus(a_j - a_i),   a = U[u] . V^T,   N_u = [0, m) \\ (P_u u E_u)

E_u is an optional exclusion list, as in `ranking.rank_entries`.  This is BPR with the sampling removed, and the logistic
surrogate of the per-user AUC that `ranking.ranking_metrics` reports.

`implicit_rows` is the kernel call (per-row counts, risk sums and the gradient with respect to the score row),
`implicit_hvp_rows` its second-order twin (include/mfcd.h: mfcd_implicit_hvp_rows) and `implicit_hvp` the product of the
risk's Hessian with a direction in the tables (the exact block steps on it are mfcd/implicit_exact.py), `implicit_risk`
the risk of a model as a differentiable scalar, `implicit_metrics` the exact per-user AUC and log-likelihood,
`fit_implicit` the fused loop of block sweeps and one dense Adam step.  The matrix is a dense fp32 GPU tensor, a
`generation_data.FactoredMatrix` or a pair (A, B) of GPU tensors, as for `ranking.rank_entries`.  There is no CPU form of
any of it."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .ranking import _csr
from .topk import _resolve

CHUNK = 2048        # columns per workgroup of the column pass (csrc/implicit.hip: kImpChunk, mfcd_implicit_chunk())
TILE = 256          # observed columns per LDS tile (csrc/implicit.hip: kImpTile, mfcd_implicit_tile())
_SLAB_BYTES = 128 << 20   # the score slab's bound (csrc/scores_common.h: kSlabBytes): a g block stays within it
_NORMALIZE = ("pairs", "user")

ImplicitRows = namedtuple("ImplicitRows", "counts sums status g")
ImplicitRows.__doc__ = """Device tensors of `implicit_rows`: counts int64 [rows, 4] (pos, neg, inverted, tied), sums f64
[rows] or None, status int32 [rows], g fp32 [rows, m] or None."""


def _launch(Xd, A, B, n, m, d, dev, ids, nrows, p_off, p_items, entries, e_off, e_items, excl_entries, coef, counts, sums,
            g, status):
    """One mfcd_implicit_rows call on checked device tensors; sums None: the prepare pass alone."""
    L = _lib.load()
    ws = None
    if sums is not None:
        nbytes = L.mfcd_implicit_rows_workspace_bytes(nrows, m, 0 if Xd is not None else d)
        if nbytes == 0:
            raise _lib.MfcdError(f"implicit_rows: sizes out of range (rows {nrows}, m {m}, d {d})")
        ws = _lib.workspace(nbytes, dev)
    _lib.check(L.mfcd_implicit_rows(Xd.data_ptr() if Xd is not None else None, Xd.stride(0) if Xd is not None else 0,
                                    _lib.ptr(A), _lib.ptr(B), d, _lib.ptr(ids), nrows, n, m, _lib.ptr(p_off),
                                    _lib.ptr(p_items) if entries else None, entries, _lib.ptr(e_off), _lib.ptr(e_items),
                                    excl_entries, _lib.ptr(coef), _lib.ptr(counts) if nrows else None, _lib.ptr(sums),
                                    _lib.ptr(g), g.stride(0) if g is not None else m,
                                    _lib.ptr(status) if nrows else None, _lib.ptr(ws), ws.numel() if ws is not None else 0,
                                    _lib.stream_ptr(dev)))


def _lists(positives, exclude, ids64, nrows, n, m, dev):
    """The two CSR lists of a call → (p_off, p_items, entries, e_off, e_items, excl_entries)."""
    p_off, p_items = _csr(positives, ids64, nrows, n, m, dev, "positives")
    e_off = e_items = None
    excl_entries = 0
    if exclude is not None:
        e_off, e_items = _csr(exclude, ids64, nrows, n, m, dev, "exclude")
        excl_entries = e_items.numel()
        if excl_entries == 0:
            e_items = torch.zeros(1, dtype=torch.int32, device=dev)
    return p_off, p_items, p_items.numel(), e_off, e_items, excl_entries


def _request(positives, exclude, rows, coef, n, m, dev, who):
    """What the row entries share → (ids int32 or None, the number of requested rows, the two lists, coef checked)."""
    if rows is None:
        ids64, ids, nrows = None, None, n
    else:
        ids64 = torch.as_tensor(rows).reshape(-1).to(device=dev, dtype=torch.int64)
        ids, nrows = ids64.to(torch.int32).contiguous(), ids64.numel()
    lists = _lists(positives, exclude, ids64, nrows, n, m, dev)
    if coef is not None:
        if not torch.is_tensor(coef) or not coef.is_cuda or coef.dtype != torch.float32:
            raise _lib.MfcdError(f"{who} needs coef as a float32 GPU tensor (there is no CPU fallback)")
        if coef.numel() != nrows:
            raise ValueError(f"{coef.numel()} coefficients for {nrows} requested rows")
        coef = coef.reshape(-1).contiguous()
    return ids, nrows, lists, coef


def implicit_rows(X, positives, exclude=None, rows=None, grad=False, coef=None, prepare_only=False):
    """→ `ImplicitRows`: per requested row the counts, the risk sum R and, with grad=True, the gradient of coef R with
    respect to the score row.

    X          dense fp32 GPU tensor [n, m], a FactoredMatrix, or a pair (A, B) of GPU tensors (X = A @ B.T)
    positives  the observed items: a `ratings.RatingsData` on the device, or a ready CSR pair (offsets int64
               [len(rows) + 1], items int32) of device tensors; strictly ascending within a row (a RatingsData's are)
    exclude    None, or the barred columns of every row in the same two forms, strictly ascending within a row
    rows       None (every row) or row numbers, any order, repeats allowed; a CSR pair is indexed by position in `rows`
    grad       also return g fp32 [rows, m]: a negative column j gets coef sum_i sigmoid(a_j - a_i), a positive column i
               gets -coef sum_j sigmoid(a_j - a_i), a barred column 0
    coef       None (1), or one fp32 factor per requested row
    prepare_only  only status and the counts pos, neg (inverted and tied 0) — no score is read; sums is None

    counts: pos = the row's observed items that are not barred, neg = the items that are neither observed nor barred,
    inverted = the (positive, negative) pairs whose negative precedes the positive in `topk_rows`' `best` order (score,
    then column number), tied = the pairs with equal scores.  A row with an invalid list or row number has status 2,
    counts -1, sum NaN and a NaN gradient row; a row with an inf or NaN score at a column that is not barred has status
    0, sum NaN and a NaN gradient row.  Deterministic: two calls are bit-equal."""
    Xd, A, B, n, m, d, dev = _resolve(X, None)
    ids, nrows, lists, coef = _request(positives, exclude, rows, coef, n, m, dev, "implicit_rows")
    counts = torch.empty((nrows, 4), dtype=torch.int64, device=dev)
    status = torch.empty(nrows, dtype=torch.int32, device=dev)
    if prepare_only:
        if grad:
            raise ValueError("prepare_only returns no gradient")
        _launch(None, None, None, n, m, 0, dev, ids, nrows, *lists, None, counts, None, None, status)
        return ImplicitRows(counts, None, status, None)
    sums = torch.empty(nrows, dtype=torch.float64, device=dev)
    g = torch.empty((nrows, m), dtype=torch.float32, device=dev) if grad else None
    _launch(Xd, A, B, n, m, d, dev, ids, nrows, *lists, coef, counts, sums, g, status)
    return ImplicitRows(counts, sums, status, g)


def _launch_hvp(Xd, Yd, A, B, Ay, By, n, m, d, dev, ids, nrows, p_off, p_items, entries, e_off, e_items, excl_entries, coef,
                q, deg, status):
    """One mfcd_implicit_hvp_rows call on checked device tensors: dense (Xd, Yd) or by factors (A, B, Ay, By)."""
    L = _lib.load()
    dense = Xd is not None
    nbytes = L.mfcd_implicit_hvp_rows_workspace_bytes(nrows, m, 0 if dense else d)
    if nbytes == 0:
        raise _lib.MfcdError(f"implicit_hvp_rows: sizes out of range (rows {nrows}, m {m}, d {d})")
    ws = _lib.workspace(nbytes, dev)
    _lib.check(L.mfcd_implicit_hvp_rows(Xd.data_ptr() if dense else None, Xd.stride(0) if dense else 0,
                                        Yd.data_ptr() if dense else None, Yd.stride(0) if dense else 0,
                                        _lib.ptr(A), _lib.ptr(B), _lib.ptr(Ay), _lib.ptr(By), d, _lib.ptr(ids), nrows, n, m,
                                        _lib.ptr(p_off), _lib.ptr(p_items) if entries else None, entries, _lib.ptr(e_off),
                                        _lib.ptr(e_items), excl_entries, _lib.ptr(coef), _lib.ptr(q) if nrows else None,
                                        q.stride(0), _lib.ptr(deg), deg.stride(0) if deg is not None else m,
                                        _lib.ptr(status) if nrows else None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))


def _shape(X):
    """(n, m, d) of a dense matrix (d = 0) or of a factor pair, whatever its device; None where `_resolve` is to refuse."""
    if torch.is_tensor(X):
        return (X.shape[0], X.shape[1], 0) if X.dim() == 2 else None
    A, B = (X.A, X.B) if _lib.is_factored(X) else X if isinstance(X, (tuple, list)) and len(X) == 2 else (None, None)
    ok = torch.is_tensor(A) and torch.is_tensor(B) and A.dim() == 2 and B.dim() == 2
    return (A.shape[0], B.shape[0], A.shape[1]) if ok else None


def implicit_hvp_rows(X, Y, positives, exclude=None, rows=None, coef=None, deg=False):
    """→ (q, deg or None, status): the Hessian of coef R of `implicit_rows` with respect to the score row, applied to
    the direction rows Y — per requested row, with w_ij = sigmoid'(a_j - a_i) over its (observed, unobserved) pairs,
    q_i = coef sum_j w_ij (y_i - y_j) for an observed column, q_j = coef sum_i w_ij (y_j - y_i) for an unobserved one and 0
    for a barred one: a bipartite weighted Laplacian.  deg=True also returns its diagonal, coef sum w over the column's
    partners (the Jacobi preconditioner).

    X, Y       the scores and the direction: both dense fp32 GPU tensors [n, m], or both factors — a FactoredMatrix or a
               pair (A, B) of GPU tensors — of one width d (a user step passes the same B twice, an item step the same A)
    positives, exclude, rows, coef   as `implicit_rows` takes them

    q and deg are fp32 [rows, m], status int32 [rows].  A constant direction row, and a row with pos neg = 0, give exactly
    +0.  A row with an invalid list or row number has status 2 and NaN rows; a row with an inf or NaN score or direction
    at a column that is not barred has status 0 and NaN rows.  Deterministic: two calls are bit-equal, and q does not
    depend on `deg`."""
    if torch.is_tensor(X) != torch.is_tensor(Y):
        raise ValueError("the scores and the direction must both be dense or both be factor pairs")
    sx, sy = _shape(X), _shape(Y)
    if sx is not None and sy is not None and sx != sy:         # a shape `_shape` cannot read is `_resolve`'s to refuse
        raise ValueError(f"scores of shape [n, m, d] = {list(sx)} and a direction of shape {list(sy)}")
    Xd, A, B, n, m, d, dev = _resolve(X, None)
    Yd, Ay, By, _, _, _, _ = _resolve(Y, None)
    ids, nrows, lists, coef = _request(positives, exclude, rows, coef, n, m, dev, "implicit_hvp_rows")
    q = torch.empty((nrows, m), dtype=torch.float32, device=dev)
    dg = torch.empty((nrows, m), dtype=torch.float32, device=dev) if deg else None
    status = torch.empty(nrows, dtype=torch.int32, device=dev)
    _launch_hvp(Xd, Yd, A, B, Ay, By, n, m, d, dev, ids, nrows, *lists, coef, q, dg, status)
    return q, dg, status


def _tables(U, V, who):
    for name, t in (("U", U), ("V", V)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.MfcdError(f"{who} needs {name} as a float32 GPU tensor (there is no CPU fallback)")
    if U.dim() != 2 or V.dim() != 2 or U.shape[1] != V.shape[1]:
        raise ValueError(f"tables of shapes {tuple(U.shape)}, {tuple(V.shape)}")
    return U.detach().contiguous(), V.detach().contiguous()


def _check_normalize(normalize):
    if normalize not in _NORMALIZE:
        raise ValueError(f"normalize must be one of {_NORMALIZE}, got {normalize!r}")


def default_row_block(n, m):
    """Users per block of a sweep: the g block [row_block, m] stays within the score slab's byte bound (whole blocks of
    128 rows, at least one)."""
    return int(min(max(n, 1), max(128, _SLAB_BYTES // (4 * m) // 128 * 128)))


class _Plan:
    """What a sweep over a table needs and what does not change between sweeps: the two lists, the users' pos and neg
    (one prepare pass), the normaliser as a per-user coefficient — all on the device — and the scratch of a block.  The
    one host read is the check that the table has a pair at all."""

    def __init__(self, n, m, dev, data, exclude, normalize, row_block):
        _check_normalize(normalize)
        self.n, self.m, self.dev = n, m, dev
        self.lists = _lists(data, exclude, None, n, n, m, dev)
        self.ids = torch.arange(n, dtype=torch.int32, device=dev)
        self.counts = torch.empty((n, 4), dtype=torch.int64, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        _launch(None, None, None, n, m, 0, dev, None, n, *self.lists, None, self.counts, None, None, self.status)
        pn = (self.counts[:, 0] * self.counts[:, 1]).clamp_(min=0).double()      # status 2: -1 x -1
        has = (pn > 0) & (self.status == 0)
        pn = torch.where(has, pn, torch.zeros_like(pn))
        if normalize == "pairs":
            total = pn.sum()
            coef = torch.where(has, 1.0 / total, torch.zeros_like(pn))
        else:
            total = has.sum().double()
            coef = torch.where(has, 1.0 / (total * pn.clamp(min=1.0)), torch.zeros_like(pn))
        if float(total) <= 0:                                                    # the plan's one host read
            raise ValueError("the table holds no (observed, unobserved) pair of one user's items")
        self.coef64, self.coef = coef, coef.float()
        self.row_block = default_row_block(n, m) if row_block is None else int(row_block)
        if self.row_block < 1:
            raise ValueError("row_block must be >= 1")
        self.sums = torch.empty(n, dtype=torch.float64, device=dev)
        self.g = None

    def sweep(self, U, V, grad):
        """One pass over the users in row blocks → (risk f64 0-dim, dU, dV) (the gradients None without `grad`): per
        block one kernel call, then dU[block] = g V and dV += g^T U[block] by library GEMMs.  No host read."""
        n, m, d, rb = self.n, self.m, U.shape[1], self.row_block
        p_off, p_items, entries, e_off, e_items, excl_entries = self.lists
        dU = dV = None
        if grad:
            dU, dV = torch.empty_like(U), torch.zeros_like(V)
            if self.g is None:
                self.g = torch.empty((min(rb, n), m), dtype=torch.float32, device=self.dev)
        for u0 in range(0, n, rb):
            u1 = min(n, u0 + rb)
            g = self.g[:u1 - u0] if grad else None
            _launch(None, U, V, n, m, d, self.dev, self.ids[u0:u1], u1 - u0, p_off[u0:u1 + 1], p_items, entries,
                    e_off[u0:u1 + 1] if e_off is not None else None, e_items, excl_entries, self.coef[u0:u1],
                    self.counts[u0:u1], self.sums[u0:u1], g, self.status[u0:u1])
            if grad:
                torch.mm(g, V, out=dU[u0:u1])
                dV.addmm_(g.t(), U[u0:u1])
        # a user without a pair has sum 0 and coefficient 0; a NaN sum stays NaN
        return (self.sums * self.coef64).sum(), dU, dV

    def hvp_sweep(self, U, V, dU, dV, gauss_newton):
        """One pass over the users in row blocks → (HU, HV) f64: per block the Laplacian applied to the two parts of
        the score-space direction dU[b] V^T + U[b] dV^T (two kernel calls whose results add: the operator is linear),
        carried back by library GEMMs; the exact form adds the gradient block's bilinear terms g dV and g^T dU."""
        n, m, d, rb = self.n, self.m, U.shape[1], self.row_block
        p_off, p_items, entries, e_off, e_items, excl_entries = self.lists
        V64, dV64 = V.double(), dV.double()
        HU = torch.empty((n, d), dtype=torch.float64, device=self.dev)
        HV = torch.zeros((m, d), dtype=torch.float64, device=self.dev)
        q = torch.empty((2, min(rb, n), m), dtype=torch.float32, device=self.dev)
        for u0 in range(0, n, rb):
            u1 = min(n, u0 + rb)
            lists = (p_off[u0:u1 + 1], p_items, entries, e_off[u0:u1 + 1] if e_off is not None else None, e_items,
                     excl_entries)
            for k, (Ay, By) in enumerate(((dU, V), (U, dV))):
                _launch_hvp(None, None, U, V, Ay, By, n, m, d, self.dev, self.ids[u0:u1], u1 - u0, *lists,
                            self.coef[u0:u1], q[k, :u1 - u0], None, self.status[u0:u1])
            Q = q[0, :u1 - u0].double() + q[1, :u1 - u0].double()
            U64 = U[u0:u1].double()
            torch.mm(Q, V64, out=HU[u0:u1])
            HV.addmm_(Q.t(), U64)
            if not gauss_newton:
                g = q[0, :u1 - u0]
                _launch(None, U, V, n, m, d, self.dev, self.ids[u0:u1], u1 - u0, *lists, self.coef[u0:u1],
                        self.counts[u0:u1], self.sums[u0:u1], g, self.status[u0:u1])
                G = g.double()
                HU[u0:u1].addmm_(G, dV64)
                HV.addmm_(G.t(), dU[u0:u1].double())
        return HU, HV


class _ImplicitRisk(torch.autograd.Function):
    """The normalised risk as a function of the factor tables.  With a gradient required, forward computes the value and
    both table gradients in one sweep; backward only scales them."""

    @staticmethod
    def forward(ctx, U, V, plan, need):
        Ud, Vd = U.detach().contiguous(), V.detach().contiguous()
        risk, dU, dV = plan.sweep(Ud, Vd, need)
        if need:
            ctx.save_for_backward(dU, dV)
        return risk.float()

    @staticmethod
    def backward(ctx, grad_out):
        dU, dV = ctx.saved_tensors
        s = grad_out.float()
        return dU * s, dV * s, None, None


def implicit_risk(U, V, data, exclude=None, normalize="pairs", row_block=None):
    """The exact observed-versus-unobserved logistic risk of the model U V^T on a table of observed items: over every
    user u, every observed item i that is not barred and every item j that is neither observed nor barred,
    softplus(a_j - a_i) = -log sigmoid(a_i - a_j).
      normalize="pairs"  sum_u R_u / sum_u pos_u neg_u: the global normalisation of `ratings.ratings_risk`
      normalize="user"   the mean over the users with pos neg > 0 of R_u / (pos_u neg_u): the surrogate of the `auc` key
                         of `ranking.ranking_metrics`
    data, exclude: a `ratings.RatingsData` on the device or a CSR pair (offsets int64 [n + 1], items int32) over all
    users.  Nothing n x m is formed: the users go through in blocks of `row_block` rows (None: the g block stays within
    the score slab's 128 MiB).  → 0-dim fp32 device tensor, differentiable with respect to fp32 U and V.  A table with
    no (observed, unobserved) pair: ValueError."""
    _check_normalize(normalize)
    _tables(U, V, "the implicit risk")
    plan = _Plan(U.shape[0], V.shape[0], U.device, data, exclude, normalize, row_block)
    need = torch.is_grad_enabled() and (U.requires_grad or V.requires_grad)
    return _ImplicitRisk.apply(U, V, plan, need)


def implicit_hvp(U, V, dU, dV, data, exclude=None, normalize="pairs", row_block=None, gauss_newton=False):
    """→ (HU, HV), f64 device tensors shaped like U and V: the Hessian of `implicit_risk(U, V, data, exclude, normalize)`
    with respect to the two tables, applied to the direction (dU, dV) — one sweep over the users in blocks of `row_block`
    rows (mfcd_implicit_hvp_rows on the score-space direction dU V^T + U dV^T, library GEMMs back to the tables), nothing
    n x m formed.  gauss_newton=True leaves out the bilinear cross term (the gradient block times the other table's
    direction), as `ratings.ratings_hvp` does: that form is positive semi-definite."""
    if all(torch.is_tensor(t) for t in (U, V, dU, dV)) and (dU.shape != U.shape or dV.shape != V.shape):
        raise ValueError(f"directions of shapes {tuple(dU.shape)}, {tuple(dV.shape)} for tables of shapes "
                         f"{tuple(U.shape)}, {tuple(V.shape)}")
    U, V = _tables(U, V, "the implicit Hessian-vector product")
    dU, dV = _tables(dU, dV, "the implicit Hessian-vector product")
    plan = _Plan(U.shape[0], V.shape[0], U.device, data, exclude, normalize, row_block)
    return plan.hvp_sweep(U, V, dU, dV, bool(gauss_newton))


def metrics_from_counts(counts, sums, status, tied_before=None):
    """The formulas of `implicit_metrics` on host arrays: counts int64 [rows, 4], sums f64 [rows], status int32 [rows];
    tied_before int64 [rows]: the tied pairs that `inverted` holds (None: no pair is tied)."""
    c, h, st = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64), np.asarray(status)
    pn = np.where(st == 0, c[:, 0] * c[:, 1], 0).astype(np.float64)
    ok = pn > 0
    low = np.zeros(c.shape[0], dtype=np.int64) if tied_before is None else np.asarray(tied_before, dtype=np.int64)
    per = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        per["auc"] = np.where(ok, 1.0 - c[:, 2] / pn, np.nan)
        per["auc_midrank"] = np.where(ok, 1.0 - ((c[:, 2] - low) + 0.5 * c[:, 3]) / pn, np.nan)
        per["log_likelihood"] = np.where(ok, -h / pn, np.nan)
    out = {}
    for name, v in per.items():
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    out["users"] = int(ok.sum())
    out["pairs"] = int(pn.sum())
    for k, name in enumerate(("pos", "neg", "inverted", "tied")):
        out[name + "_per_user"] = c[:, k].copy()
    return out


def implicit_metrics(U_or_X, V, data, exclude=None):
    """Exact metrics of a model on a table of observed items (typically a held-out split, with the training split as
    `exclude`), in the convention of `ratings.ratings_metrics`.  U_or_X, V: the factor tables, or (V None) a dense GPU
    tensor, a FactoredMatrix or a pair (A, B).  Per user with pos neg > 0, in f64:
      auc             1 - inverted / (pos neg): the share of (observed, unobserved) pairs the model orders correctly in the
                      order (score, then item number) — the `auc` of `ranking.ranking_metrics` on the same lists
      auc_midrank     a tied pair counts as half an error wherever it stands: 1 - (strictly inverted + tied / 2) / (pos
                      neg).  `inverted` holds the tied pairs whose unobserved item has the smaller number; when a pair is
                      tied at all, a second call on the negated scores tells how many those are (inverted + inverted' =
                      pos neg - tied + 2 of them).  NaN for a user with a NaN score and a tie.
      log_likelihood  -R_u / (pos neg), natural log
    Every key is the mean over the users where it is defined (0.0 if there are none), every key with the suffix
    `_per_user` a float64 numpy array (NaN for a user without a pair); pos, neg, inverted, tied `_per_user` are the int64
    counts, `users` and `pairs` their totals."""
    Xd, A, B, n, m, d, dev = _resolve(U_or_X if V is None else (U_or_X, V), None)
    res = implicit_rows(Xd if Xd is not None else (A, B), data, exclude)
    c, h, st = res.counts.cpu().numpy(), res.sums.cpu().numpy(), res.status.cpu().numpy()
    low = None
    if (c[:, 3] > 0).any():
        c2 = implicit_rows(-Xd if Xd is not None else (-A, B), data, exclude).counts.cpu().numpy()
        low = np.where(st == 0, (c[:, 2] + c2[:, 2] - c[:, 0] * c[:, 1] + c[:, 3]) // 2, 0)
    out = metrics_from_counts(c, h, st, low)
    if low is not None:
        out["auc_midrank_per_user"][np.isnan(h) & (c[:, 3] > 0)] = np.nan
        good = out["auc_midrank_per_user"][~np.isnan(out["auc_midrank_per_user"])]
        out["auc_midrank"] = float(good.mean()) if good.size else 0.0
    return out


def fit_implicit(binding, data, steps, log_every=0, exclude=None, normalize="pairs", row_block=None):
    """`ratings.fit_ratings` on `implicit_risk`: `steps` steps of Adam, fused — per step one sweep over the row blocks
    (mfcd_implicit_rows with the gradient, two library GEMMs per block) and one mfcd_adam_dense on the caller's
    torch.optim.Adam state, which stays valid (binding: an engine.AdamBinding, or a (model, optimizer) pair; fp32 tables
    only).  Nothing waits for the device inside the loop; the risks are logged on the device and read once → (steps
    taken, risks) as `fit_ratings` returns them."""
    from . import engine
    _check_normalize(normalize)
    if not isinstance(binding, engine.AdamBinding):
        binding = engine.AdamBinding(*binding)
    for name, t in zip(("model.U", "model.V"), binding.tensors()[:2]):
        engine._require_cuda_param(t, name)                    # fp32 only: bf16 tables are refused here
    L = _lib.load()
    U, V, mU, vU, mV, vV = binding.tensors()
    n, m, d, dev = U.shape[0], V.shape[0], U.shape[1], U.device
    plan = _Plan(n, m, dev, data, exclude, normalize, row_block)
    steps, k = int(steps), int(log_every)
    at = ([t for t in range(0, steps, k)] + [steps]) if k > 0 else []
    log = torch.zeros(max(len(at), 1), dtype=torch.float64, device=dev)
    state = [_lib.ptr(t) for t in (U, V, mU, vU, mV, vV)]
    lr, b1, b2, eps, wd = binding.hyper()
    stream = _lib.stream_ptr(dev)
    try:
        for t in range(steps):
            risk, gU, gV = plan.sweep(U, V, True)
            if k > 0 and t % k == 0:
                log[t // k] = risk
            _lib.check(L.mfcd_adam_dense(*state, _lib.ptr(gU), _lib.ptr(gV), binding.step + 1, n, m, d, lr, b1, b2, eps, wd,
                                         stream))
            binding.advance(1, defer=True)
    finally:
        binding.flush()         # an interrupt must not leave the moments ahead of the optimizer's `step` tensors
    if k <= 0:
        return [], []
    log[len(at) - 1] = plan.sweep(U, V, False)[0]
    return at, log[:len(at)].cpu().tolist()                # the one device->host transfer of the run
