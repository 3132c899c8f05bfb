"""The all-pairs BTL machinery on observed ratings (include/mfcd.h: mfcd_pair_ragged_stats, mfcd_pair_ragged_grad,
mfcd_ragged_dot, mfcd_ragged_gather_sum): a user has a value for some of the items only, and everything is taken over
the L_u (L_u - 1) / 2 pairs among the items that user rated, exactly and without forming a pair.

`RatingsData` holds a ratings table on one device in the kernels' CSR layout, with the by-item transposition and the tile
and segment offsets the entries need; every host read happens there, once per dataset.  `ragged_scores`,
`pair_ragged_stats`, `pair_ragged_grad` and `ragged_gather_sum` are the kernel calls.  `ratings_risk` is the exact BTL
risk of a model on the table as a differentiable scalar, `ratings_metrics` the exact held-out metrics, `fit_ratings` the
fused loop of scores, gradient, two gather-sums and one dense Adam step.  `pair_ragged_hvp` (mfcd_pair_ragged_hvp) is the
curvature of the same risk in score space and `ratings_hvp` its product with a direction of both tables; the exact block
steps built on it are mfcd/ratings_exact.py's.  There is no CPU form of any of it."""
import numpy as np
import torch

from . import _lib
from . import pairs as P

_SIDES = ("user", "item")


def _host(t, dtype):
    return np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).reshape(-1), dtype=dtype)


def _prefix(counts):
    out = np.zeros(counts.size + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def _ceil_prefix(off, unit):
    return _prefix((np.diff(off) + unit - 1) // unit)


class RatingsData:
    """A ratings table of n users and m items on one device, sorted by (user, item).  users, items, values: host arrays
    or tensors of one length (a repeated (user, item) pair: ValueError; an index outside [0, n) / [0, m): IndexError).
    Tensors (built on the CPU; `.to(device)` moves them):
      row_off int64 [n + 1], item int32, user int32, value fp32 [entries]      the CSR layout by user
      tile_off int64 [n + 1], n_tiles       prefix sum of ceil(L_u / mfcd_pair_ragged_tile())
      seg_off int64 [n + 1], n_seg          prefix sum of ceil(L_u / mfcd_ragged_segment())
      col_off int64 [m + 1], col_user int32, col_perm int64 [entries]          the transposition: position p of the
                                            by-(item, user) order is CSR entry col_perm[p], of user col_user[p]
      col_seg_off int64 [m + 1], col_n_seg  the items' segments
    Python ints: entries, pairs = sum of L_u (L_u - 1) / 2, tied_pairs = those of them with equal values (-0.0 equals
    +0.0).  lengths: the users' L_u as a host int64 array; user_pairs, user_tied_pairs: the two counts per user, host
    int64 [n] (`user_support`)."""

    _TENSORS = ("row_off", "item", "user", "value", "tile_off", "seg_off", "col_off", "col_user", "col_perm", "col_seg_off")

    def __init__(self, users, items, values, n, m):
        u, i, v = _host(users, np.int64), _host(items, np.int64), _host(values, np.float32)
        if not u.size == i.size == v.size:
            raise ValueError("users, items and values must have one length")
        n, m = int(n), int(m)
        if n < 0 or m < 0 or n >= 1 << 31 or m >= 1 << 31:
            raise ValueError("n and m must lie in [0, 2^31)")
        if u.size and (u.min() < 0 or u.max() >= n or i.min() < 0 or i.max() >= m):
            raise IndexError(f"a rating names a user outside [0, {n}) or an item outside [0, {m})")
        order = np.lexsort((i, u))
        u, i, v = u[order], i[order], v[order]
        if u.size > 1 and ((u[1:] == u[:-1]) & (i[1:] == i[:-1])).any():
            raise ValueError("a (user, item) pair is rated more than once")
        L = _lib.load()
        tile, seg = L.mfcd_pair_ragged_tile(), L.mfcd_ragged_segment()
        lengths = np.bincount(u, minlength=n).astype(np.int64)
        row_off = _prefix(lengths)
        perm = np.lexsort((u, i)).astype(np.int64)
        col_off = _prefix(np.bincount(i, minlength=m).astype(np.int64))
        host = dict(row_off=row_off, item=i.astype(np.int32), user=u.astype(np.int32), value=v,
                    tile_off=_ceil_prefix(row_off, tile), seg_off=_ceil_prefix(row_off, seg), col_off=col_off,
                    col_user=u[perm].astype(np.int32), col_perm=perm, col_seg_off=_ceil_prefix(col_off, seg))
        for k, a in host.items():
            setattr(self, k, torch.from_numpy(a))
        self.n, self.m, self.entries, self.lengths = n, m, int(u.size), lengths
        self.n_tiles, self.n_seg, self.col_n_seg = (int(host[k][-1]) for k in ("tile_off", "seg_off", "col_seg_off"))
        self.pairs = int((lengths * (lengths - 1) // 2).sum())
        by_value = np.lexsort((v + np.float32(0.0), u))                     # -0.0 + 0.0 = +0.0
        su, sv = u[by_value], v[by_value] + np.float32(0.0)
        start = np.flatnonzero(np.concatenate(([True], (su[1:] != su[:-1]) | (sv[1:] != sv[:-1])))) if u.size else su
        runs = np.diff(np.concatenate((start, [u.size]))).astype(np.int64)
        self.tied_pairs = int((runs * (runs - 1) // 2).sum())
        self.user_pairs = lengths * (lengths - 1) // 2
        self.user_tied_pairs = np.bincount(su[start], weights=runs * (runs - 1) // 2, minlength=n).astype(np.int64)

    def user_support(self, skip_ties=False):
        """`support` per user: host int64 [n].  A user whose support is 0 has a risk that is identically 0."""
        return self.user_pairs - self.user_tied_pairs if skip_ties else self.user_pairs

    @property
    def device(self):
        return self.row_off.device

    def to(self, device):
        """The same table on `device` (self if it is there already)."""
        device = torch.device(device)
        if device == self.device:
            return self
        out = object.__new__(RatingsData)
        out.__dict__.update(self.__dict__)
        for k in self._TENSORS:
            setattr(out, k, getattr(self, k).to(device))
        return out

    def support(self, skip_ties=False):
        """The pairs the risk is taken over: all of them, or those with different values."""
        return self.pairs - self.tied_pairs if skip_ties else self.pairs

    def split(self, fractions, seed=0):
        """Partitions every user's entries at random into len(fractions) parts of about fractions[k] of them (fractions
        >= 0 summing to 1; a user's parts end at floor(cumulative fraction x L_u)) → one RatingsData per fraction, on this
        device, together covering every entry exactly once.  The draw comes from a private numpy Generator(seed)."""
        f = np.asarray(fractions, dtype=np.float64)
        if f.ndim != 1 or f.size == 0 or (f < 0).any() or abs(f.sum() - 1.0) > 1e-9:
            raise ValueError("fractions must be non-negative and sum to 1")
        u, i, v = self.user.cpu().numpy().astype(np.int64), self.item.cpu().numpy(), self.value.cpu().numpy()
        keys = np.random.default_rng(seed).random(self.entries)
        order = np.lexsort((keys, u))                                       # every user's entries in a random order
        su = u[order]
        rank = np.arange(self.entries, dtype=np.int64) - self.row_off.cpu().numpy()[su]
        ends = np.floor(np.cumsum(f)[None, :] * self.lengths[su][:, None] + 1e-9).astype(np.int64)
        ends[:, -1] = self.lengths[su]
        part = (rank[:, None] >= ends).sum(1)
        out = []
        for k in range(f.size):
            sel = order[part == k]
            out.append(RatingsData(u[sel], i[sel], v[sel], self.n, self.m).to(self.device))
        return out


def _need(t, dtype, who, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        raise _lib.MfcdError(f"{who} needs {what} as a {dtype} GPU tensor (there is no CPU fallback)")
    return t.contiguous()


def _need_data(data, who):
    if not data.row_off.is_cuda:
        raise _lib.MfcdError(f"{who} needs the ratings on a GPU device: data.to(device) (there is no CPU fallback)")


def ragged_scores(U, V, data):
    """fp32 GPU tables U [n, d], V [m, d] (d <= 256) → (a fp32 [entries], status int32 [n]): a_e = U[user_e] . V[item_e],
    the model's scores of the table's entries (mfcd_ragged_dot)."""
    U, V = _need(U, torch.float32, "ragged_scores", "U"), _need(V, torch.float32, "ragged_scores", "V")
    _need_data(data, "ragged_scores")
    if U.dim() != 2 or V.dim() != 2 or U.shape[1] != V.shape[1] or U.shape[0] != data.n or V.shape[0] != data.m:
        raise ValueError(f"tables of shapes {tuple(U.shape)}, {tuple(V.shape)} for ratings of {data.n} users, {data.m} items")
    a = torch.empty(data.entries, dtype=torch.float32, device=U.device)
    status = torch.zeros(data.n, dtype=torch.int32, device=U.device)
    _lib.check(_lib.load().mfcd_ragged_dot(_lib.ptr(U), data.n, _lib.ptr(V), data.m, U.shape[1], data.entries,
                                           _lib.ptr(data.row_off), data.n, _lib.ptr(data.item), _lib.ptr(a),
                                           _lib.ptr(status), _lib.stream_ptr(U.device)))
    return a, status


def pair_ragged_stats(a, data, scale=1.0, what="both", skip_ties=False):
    """Scores a fp32 [entries] on the GPU against data.value → (counts int64 [n, 4] or None, sums f64 [n, 4] or None,
    status int32 [n]) per user, as `pairs.pair_stats_rows` defines them over the user's own entries
    (mfcd_pair_ragged_stats).  skip_ties: pairs with equal values leave the sums.  Deterministic."""
    if what not in P._WHAT:
        raise ValueError(f"what must be one of {sorted(P._WHAT)}, got {what!r}")
    w = P._WHAT[what]
    a = _need(a, torch.float32, "pair_ragged_stats", "the scores")
    _need_data(data, "pair_ragged_stats")
    if a.numel() != data.entries:
        raise ValueError(f"{a.numel()} scores for {data.entries} ratings")
    L, dev, n = _lib.load(), a.device, data.n
    counts = torch.empty((n, 4), dtype=torch.int64, device=dev) if w & 1 else None
    sums = torch.empty((n, 4), dtype=torch.float64, device=dev) if w & 2 else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_pair_ragged_workspace_bytes(n, data.n_tiles), dev)
    _lib.check(L.mfcd_pair_ragged_stats(_lib.ptr(a), _lib.ptr(data.value), data.entries, _lib.ptr(data.row_off), n,
                                        _lib.ptr(data.tile_off), data.n_tiles, float(scale), int(bool(skip_ties)), w,
                                        _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr(dev)))
    return counts, sums, status


def pair_ragged_grad(a, data, scale=1.0, skip_ties=False):
    """Scores a fp32 [entries] on the GPU → (g fp32 [entries], status int32 [n]): the gradient of the users' `risk` sums
    of `pair_ragged_stats` with respect to the scores (mfcd_pair_ragged_grad).  Deterministic."""
    a = _need(a, torch.float32, "pair_ragged_grad", "the scores")
    _need_data(data, "pair_ragged_grad")
    if a.numel() != data.entries:
        raise ValueError(f"{a.numel()} scores for {data.entries} ratings")
    g = torch.empty_like(a)
    status = torch.zeros(data.n, dtype=torch.int32, device=a.device)
    _lib.check(_lib.load().mfcd_pair_ragged_grad(_lib.ptr(a), _lib.ptr(data.value), data.entries, _lib.ptr(data.row_off),
                                                 data.n, _lib.ptr(data.tile_off), data.n_tiles, float(scale),
                                                 int(bool(skip_ties)), _lib.ptr(g), _lib.ptr(status),
                                                 _lib.stream_ptr(a.device)))
    return g, status


def pair_ragged_hvp(a, y, data, skip_ties=False, deg=False):
    """Scores a and a score-space vector y, fp32 [entries] on the GPU → (q fp32 [entries], status int32 [n]), or with
    deg=True (q, deg, status): the Hessian of the users' `risk` sums of `pair_ragged_stats` with respect to the scores,
    applied to y, and its diagonal — every user's row Laplacian, `pairs.pair_hvp_rows` over the user's own entries
    (mfcd_pair_ragged_hvp).  Neither the scale nor the values enter, except that skip_ties drops the pairs with equal
    values.  Deterministic."""
    a = _need(a, torch.float32, "pair_ragged_hvp", "the scores")
    y = _need(y, torch.float32, "pair_ragged_hvp", "the vector")
    _need_data(data, "pair_ragged_hvp")
    if a.numel() != data.entries or y.numel() != data.entries:
        raise ValueError(f"{a.numel()} scores and a vector of {y.numel()} for {data.entries} ratings")
    q = torch.empty_like(a)
    d = torch.empty_like(a) if deg else None
    status = torch.zeros(data.n, dtype=torch.int32, device=a.device)
    _lib.check(_lib.load().mfcd_pair_ragged_hvp(_lib.ptr(a), _lib.ptr(data.value), _lib.ptr(y), data.entries,
                                                _lib.ptr(data.row_off), data.n, _lib.ptr(data.tile_off), data.n_tiles,
                                                int(bool(skip_ties)), _lib.ptr(q), _lib.ptr(d), _lib.ptr(status),
                                                _lib.stream_ptr(a.device)))
    return (q, d, status) if deg else (q, status)


def ragged_gather_sum(coef, data, table, side):
    """coef fp32 [entries] (in CSR order) and an fp32 GPU table → (out fp32, status int32) (mfcd_ragged_gather_sum):
    side="user": table is V [m, d], out[u] = sum over u's entries of coef_e V[item_e], [n, d];
    side="item": table is U [n, d], out[i] = sum over the entries of item i of coef_e U[user_e], [m, d]."""
    if side not in _SIDES:
        raise ValueError(f"side must be one of {_SIDES}, got {side!r}")
    coef = _need(coef, torch.float32, "ragged_gather_sum", "coef")
    table = _need(table, torch.float32, "ragged_gather_sum", "the table")
    _need_data(data, "ragged_gather_sum")
    by_user = side == "user"
    rows, t_rows = (data.n, data.m) if by_user else (data.m, data.n)
    if table.dim() != 2 or table.shape[0] != t_rows or coef.numel() != data.entries:
        raise ValueError(f"a table of shape {tuple(table.shape)} and {coef.numel()} coefficients for side {side!r}")
    row_off, idx, perm, seg_off, n_seg = (data.row_off, data.item, None, data.seg_off, data.n_seg) if by_user else \
        (data.col_off, data.col_user, data.col_perm, data.col_seg_off, data.col_n_seg)
    L, dev, d = _lib.load(), table.device, table.shape[1]
    out = torch.empty((rows, d), dtype=torch.float32, device=dev)
    status = torch.zeros(rows, dtype=torch.int32, device=dev)
    need = L.mfcd_ragged_gather_sum_workspace_bytes(rows, d, n_seg)
    if need == 0:
        raise _lib.MfcdError(f"a table of {d} columns is outside the gather-sum's range [1, 256]")
    ws = _lib.workspace(need, dev)
    _lib.check(L.mfcd_ragged_gather_sum(_lib.ptr(table), t_rows, d, data.entries, _lib.ptr(row_off), rows, _lib.ptr(idx),
                                        _lib.ptr(coef), _lib.ptr(perm), _lib.ptr(seg_off), n_seg, _lib.ptr(out),
                                        _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return out, status


def _support(data, skip_ties):
    total = data.support(skip_ties)
    if total <= 0:
        raise ValueError("the ratings hold no pair of one user's items" + (" with different values" if skip_ties else ""))
    return total


def _table_grads(g, data, U, V):
    return ragged_gather_sum(g, data, V, "user")[0], ragged_gather_sum(g, data, U, "item")[0]


class _RatingsRisk(torch.autograd.Function):
    """sum over the users of the risk sums / sum over the users of the supports, as a function of the factor tables.
    Backward is `pair_ragged_grad` on the scores kept from forward, then one `ragged_gather_sum` per table."""

    @staticmethod
    def forward(ctx, U, V, data, s, skip_ties, total):
        a = ragged_scores(U, V, data)[0]
        risk = pair_ragged_stats(a, data, s, "sums", skip_ties)[1][:, 0].sum()
        ctx.save_for_backward(U, V, a)
        ctx.data, ctx.s, ctx.skip_ties, ctx.total = data, s, skip_ties, total
        return (risk / total).float()

    @staticmethod
    def backward(ctx, grad_out):
        U, V, a = ctx.saved_tensors
        g = pair_ragged_grad(a, ctx.data, ctx.s, ctx.skip_ties)[0].mul_(grad_out.float() / ctx.total)
        dU, dV = _table_grads(g, ctx.data, U, V)
        return dU, dV, None, None, None, None


def ratings_risk(U, V, data, s=1.0, skip_ties=False):
    """The exact BTL risk of the model U V^T on a ratings table: over every user and every pair of items that user
    rated, the sum of q (-log p) + (1 - q)(-log(1 - p)), p = sigmoid(a_k - a_l), q = sigmoid(s (x_k - x_l)), divided
    by the number of those pairs (skip_ties: the pairs with different values only) — a global normalisation, as
    `pairs.law_risk`: what comparisons drawn uniformly from the pairs the table implies estimate.  → 0-dim fp32 device
    tensor, differentiable with respect to fp32 U and V.  A table without such a pair: ValueError."""
    for name, t in (("U", U), ("V", V)):
        _need(t, torch.float32, "the ratings risk", name)
    _need_data(data, "the ratings risk")
    return _RatingsRisk.apply(U, V, data, float(s), bool(skip_ties), _support(data, skip_ties))


def ratings_hvp(U, V, dU, dV, data, s=1.0, skip_ties=False, gauss_newton=False):
    """The Hessian of `ratings_risk` with respect to both tables, applied to a direction (dU, dV) of their shapes → (HU,
    HV) fp32, as `pairs.population_hvp` on a ratings table: with dA = dU[user] . V[item] + U[user] . dV[item] over the
    entries, q = `pair_ragged_hvp`(a, dA), g = `pair_ragged_grad`(a) and c = 1 / data.support(skip_ties),
        HU = c [gather_sum(q, V) + gather_sum(g, dV)] by user,   HV = c [gather_sum(q, U) + gather_sum(g, dU)] by item.
    gauss_newton=True drops the two g terms: the positive semi-definite part.  fp32 GPU tensors; nothing is modified."""
    tables = [_need(t, torch.float32, "the ratings Hessian-vector product", name)
              for name, t in (("U", U), ("V", V), ("dU", dU), ("dV", dV))]
    _need_data(data, "the ratings Hessian-vector product")
    U, V, dU, dV = (t.detach() for t in tables)
    if dU.shape != U.shape or dV.shape != V.shape:
        raise ValueError(f"a direction of shapes {tuple(dU.shape)}, {tuple(dV.shape)} for tables {tuple(U.shape)}, "
                         f"{tuple(V.shape)}")
    c = 1.0 / _support(data, skip_ties)
    a = ragged_scores(U, V, data)[0]
    dA = ragged_scores(dU, V, data)[0].add_(ragged_scores(U, dV, data)[0])
    q = pair_ragged_hvp(a, dA, data, skip_ties)[0]
    HU, HV = _table_grads(q, data, U, V)
    if not gauss_newton:
        g = pair_ragged_grad(a, data, s, skip_ties)[0]
        gU, gV = _table_grads(g, data, dU, dV)
        HU, HV = HU.add_(gU), HV.add_(gV)
    return HU.mul_(c), HV.mul_(c)


def ratings_metrics(U, V, data, s=1.0, skip_ties=False):
    """`pairs.pairwise_metrics` on a ratings table (typically a held-out split): the keys of `pairs._KEYS`, each from
    `pairs.pairwise_from_counts`' formulas with the user's own n0 = L_u (L_u - 1) / 2 (skip_ties: the four likelihood /
    accuracy values over the user's n0 - Tx pairs with different values), and every key with the suffix `_per_user`
    (float64 numpy, NaN where undefined: a user without a pair).  The plain key is the mean over the users where it is
    defined (0.0 if there are none)."""
    a = ragged_scores(U.detach(), V.detach(), data)[0]
    counts, sums, _ = pair_ragged_stats(a, data, s, "both", skip_ties)
    c, h = counts.cpu().numpy(), sums.cpu().numpy()                  # the call's one device -> host transfer
    per = P.pairwise_from_counts(c, None, data.lengths)             # n0 per row: the formulas take it elementwise
    n0 = data.lengths * (data.lengths - 1) // 2
    support = (n0 - np.where(c[:, 3] >= 0, c[:, 3], 0) if skip_ties else n0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (name, sign) in enumerate((("expected_log_likelihood", -1.0), ("bayes_log_likelihood", -1.0),
                                          ("expected_accuracy", 1.0), ("bayes_accuracy", 1.0))):
            per[name] = np.where(support > 0, sign * h[:, k] / support, np.nan)
    out = {}
    for name in P._KEYS:
        v = per[name]
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    return out


def fit_ratings(binding, data, s, steps, log_every=0, skip_ties=False):
    """`pairs.fit_population` on `ratings_risk`: `steps` steps of Adam, fused — per step the entries' scores
    (mfcd_ragged_dot), `pair_ragged_grad`, the two gather-sums into dense gradients and one mfcd_adam_dense on the
    caller's torch.optim.Adam state, which stays valid (binding: an engine.AdamBinding, or a (model, optimizer) pair;
    fp32 tables only).  Nothing waits for the device inside the loop; the risks are logged on the device and read once
    → (steps taken, risks) as `fit_population` returns them."""
    from . import engine
    if not isinstance(binding, engine.AdamBinding):
        binding = engine.AdamBinding(*binding)
    for name, t in zip(("model.U", "model.V"), binding.tensors()[:2]):
        engine._require_cuda_param(t, name)                    # fp32 only: bf16 tables are refused here
    _need_data(data, "the ratings fit")
    L = _lib.load()
    U, V, mU, vU, mV, vV = binding.tensors()
    n, m, d, dev = U.shape[0], V.shape[0], U.shape[1], U.device
    inv = 1.0 / _support(data, skip_ties)
    steps, k = int(steps), int(log_every)
    at = ([t for t in range(0, steps, k)] + [steps]) if k > 0 else []
    log = torch.zeros(max(len(at), 1), dtype=torch.float64, device=dev)
    state = [_lib.ptr(t) for t in (U, V, mU, vU, mV, vV)]
    lr, b1, b2, eps, wd = binding.hyper()
    stream = _lib.stream_ptr(dev)

    def risk_into(slot, a):
        slot += pair_ragged_stats(a, data, s, "sums", skip_ties)[1][:, 0].sum()

    try:
        for t in range(steps):
            a = ragged_scores(U, V, data)[0]
            if k > 0 and t % k == 0:
                risk_into(log[t // k], a)
            gU, gV = _table_grads(pair_ragged_grad(a, data, s, skip_ties)[0].mul_(inv), data, U, V)
            _lib.check(L.mfcd_adam_dense(*state, _lib.ptr(gU), _lib.ptr(gV), binding.step + 1, n, m, d, lr, b1, b2, eps, wd,
                                         stream))
            binding.advance(1, defer=True)
    finally:
        binding.flush()         # an interrupt must not leave the moments ahead of the optimizer's `step` tensors
    if k <= 0:
        return [], []
    risk_into(log[len(at) - 1], ragged_scores(U, V, data)[0])
    return at, (log[:len(at)] * inv).cpu().tolist()       # the one device->host transfer of the run
