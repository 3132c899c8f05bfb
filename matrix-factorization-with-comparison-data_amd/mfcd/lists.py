"""Ranked lists under the Plackett–Luce model (include/mfcd.h: mfcd_list_pl): a user orders the L items shown, or
names the best `depth` of them, and the likelihood is a sequence of softmax choices out of what remains — "picked i out
of the slate S" is depth 1, the BTL triplet a list of two.

`RankedLists` holds the lists on one device in the kernels' CSR layout, sorted by (user, position), with the by-item
transposition and the tile and segment offsets the entries need; every host read happens there, once per dataset.
`list_scores` and `pl_rows` are the kernel calls, `pl_risk` the mean negative log-likelihood per choice as a
differentiable scalar, `pl_metrics` the held-out metrics, `fit_lists` the fused loop of scores, list kernel, two
gather-sums and one dense Adam step, `sample_rankings` an exact Plackett–Luce draw from a dense truth.  `pl_hvp_rows` is
the loss's Hessian in the scores applied to a vector, with its diagonal (mfcd_list_pl_hvp), `pl_hvp` the Hessian of
`pl_risk` in both tables applied to a direction; mfcd/lists_exact.py builds the exact block steps on them.  The scores, the
gather-sums and the Kendall counts are ratings.py's entries (mfcd_ragged_dot, mfcd_ragged_gather_sum,
mfcd_pair_ragged_stats) on this layout.  There is no CPU form of the kernel calls."""
import numpy as np
import torch

from . import _lib
from . import pairs as P
from .ratings import _ceil_prefix, _host, _need, _prefix, ragged_gather_sum, ragged_scores

_WHAT = {"loss": 1, "grad": 2, "both": 3}


class RankedLists:
    """Ranked lists of n users over m items on one device.  users, items, positions: host arrays or tensors of one
    length; a user's entries are ordered by position (any integers: only their order counts), best first.  A repeated
    (user, item) or (user, position): ValueError; an index outside [0, n) / [0, m): IndexError.  depth: None (every list
    fully ranked), an int K (every user's best min(K, L_u) are ranked, the rest is an unordered tail: shown, not ranked)
    or one int per user in [0, L_u].
    Tensors (built on the CPU; `.to(device)` moves them):
      row_off int64 [n + 1], item int32, user int32, position int64 [entries]  the CSR layout by user, in rank order
      depth int32 [n]                       the users' ranked positions
      tile_off int64 [n + 1], n_tiles       prefix sum of ceil(L_u / mfcd_list_pl_tile())
      seg_off, n_seg, col_off, col_user, col_perm, col_seg_off, col_n_seg      as ratings.RatingsData builds them
      rank_off int64 [n + 1], rank_idx int64, rank_value fp32 [sum of depth], rank_tile_off int64 [n + 1], rank_n_tiles
                                            the ranked entries alone, as a layout of mfcd_pair_ragged_stats: the CSR
                                            entry of each and minus its rank in the list (exact in fp32)
    Python ints: entries, stages = sum over the users of min(depth_u, L_u - 1), the choices the lists record.  lengths,
    user_depth, user_stages: the users' L_u, depth and stages as host int64 arrays."""

    _TENSORS = ("row_off", "item", "user", "position", "depth", "tile_off", "seg_off", "col_off", "col_user", "col_perm",
                "col_seg_off", "rank_off", "rank_idx", "rank_value", "rank_tile_off")

    def __init__(self, users, items, positions, n, m, depth=None):
        u, i, p = _host(users, np.int64), _host(items, np.int64), _host(positions, np.int64)
        if not u.size == i.size == p.size:
            raise ValueError("users, items and positions must have one length")
        n, m = int(n), int(m)
        if n < 0 or m < 0 or n >= 1 << 31 or m >= 1 << 31:
            raise ValueError("n and m must lie in [0, 2^31)")
        if u.size and (u.min() < 0 or u.max() >= n or i.min() < 0 or i.max() >= m):
            raise IndexError(f"a list names a user outside [0, {n}) or an item outside [0, {m})")
        by_item = np.lexsort((i, u))
        if u.size > 1 and ((u[by_item][1:] == u[by_item][:-1]) & (i[by_item][1:] == i[by_item][:-1])).any():
            raise ValueError("a (user, item) pair is listed more than once")
        order = np.lexsort((p, u))
        u, i, p = u[order], i[order], p[order]
        if u.size > 1 and ((u[1:] == u[:-1]) & (p[1:] == p[:-1])).any():
            raise ValueError("a (user, position) pair is listed more than once")
        L = _lib.load()
        tile, seg, pair_tile = L.mfcd_list_pl_tile(), L.mfcd_ragged_segment(), L.mfcd_pair_ragged_tile()
        lengths = np.bincount(u, minlength=n).astype(np.int64)
        if depth is None:
            dep = lengths.copy()
        elif np.ndim(depth) == 0:
            if int(depth) < 0:
                raise ValueError("depth must be >= 0")
            dep = np.minimum(lengths, int(depth))
        else:
            dep = _host(depth, np.int64)
            if dep.size != n or (dep < 0).any() or (dep > lengths).any():
                raise ValueError("a depth per user must lie in [0, L_u]")
        row_off = _prefix(lengths)
        perm = np.lexsort((u, i)).astype(np.int64)
        col_off = _prefix(np.bincount(i, minlength=m).astype(np.int64))
        rank = np.arange(u.size, dtype=np.int64) - row_off[u]              # an entry's rank in its list, from 0
        ranked = np.flatnonzero(rank < dep[u]).astype(np.int64)
        rank_off = _prefix(dep)
        host = dict(row_off=row_off, item=i.astype(np.int32), user=u.astype(np.int32), position=p,
                    depth=dep.astype(np.int32), tile_off=_ceil_prefix(row_off, tile), seg_off=_ceil_prefix(row_off, seg),
                    col_off=col_off, col_user=u[perm].astype(np.int32), col_perm=perm,
                    col_seg_off=_ceil_prefix(col_off, seg), rank_off=rank_off, rank_idx=ranked,
                    rank_value=(-rank[ranked]).astype(np.float32), rank_tile_off=_ceil_prefix(rank_off, pair_tile))
        for k, a in host.items():
            setattr(self, k, torch.from_numpy(a))
        self.n, self.m, self.entries, self.lengths = n, m, int(u.size), lengths
        self.n_tiles, self.n_seg, self.col_n_seg, self.rank_n_tiles = (
            int(host[k][-1]) for k in ("tile_off", "seg_off", "col_seg_off", "rank_tile_off"))
        self.user_depth = dep
        self.user_stages = np.maximum(np.minimum(dep, lengths - 1), 0)
        self.stages = int(self.user_stages.sum())

    @property
    def device(self):
        return self.row_off.device

    def to(self, device):
        """The same lists on `device` (self if they are there already)."""
        device = torch.device(device)
        if device == self.device:
            return self
        out = object.__new__(RankedLists)
        out.__dict__.update(self.__dict__)
        for k in self._TENSORS:
            setattr(out, k, getattr(self, k).to(device))
        return out

    def split(self, fractions, seed=0):
        """Partitions every user's entries at random into len(fractions) parts of about fractions[k] of them (fractions
        >= 0 summing to 1; a user's parts end at floor(cumulative fraction x L_u)) → one RankedLists per fraction, on
        this device, together covering every entry exactly once.  A part keeps its entries' positions, so their relative
        order, and ranks those of them the list ranked: a part of a fully ranked list is fully ranked (the restriction of
        a Plackett–Luce ranking to a subset is a Plackett–Luce ranking of the subset).  The draw comes from a private
        numpy Generator(seed)."""
        f = np.asarray(fractions, dtype=np.float64)
        if f.ndim != 1 or f.size == 0 or (f < 0).any() or abs(f.sum() - 1.0) > 1e-9:
            raise ValueError("fractions must be non-negative and sum to 1")
        u, i = self.user.cpu().numpy().astype(np.int64), self.item.cpu().numpy()
        p, off, dep = self.position.cpu().numpy(), self.row_off.cpu().numpy(), self.depth.cpu().numpy().astype(np.int64)
        keys = np.random.default_rng(seed).random(self.entries)
        order = np.lexsort((keys, u))                                       # every user's entries in a random order
        su = u[order]
        rank = np.arange(self.entries, dtype=np.int64) - off[su]
        ends = np.floor(np.cumsum(f)[None, :] * self.lengths[su][:, None] + 1e-9).astype(np.int64)
        ends[:, -1] = self.lengths[su]
        part = (rank[:, None] >= ends).sum(1)
        was_ranked = np.arange(self.entries, dtype=np.int64) - off[u] < dep[u]
        out = []
        for k in range(f.size):
            sel = order[part == k]
            d_k = np.bincount(u[sel], weights=was_ranked[sel], minlength=self.n).astype(np.int64)
            out.append(RankedLists(u[sel], i[sel], p[sel], self.n, self.m, d_k).to(self.device))
        return out


def _need_lists(lists, who):
    if not lists.row_off.is_cuda:
        raise _lib.MfcdError(f"{who} needs the lists on a GPU device: lists.to(device) (there is no CPU fallback)")


def list_scores(U, V, lists):
    """fp32 GPU tables U [n, d], V [m, d] (d <= 256) → (a fp32 [entries], status int32 [n]): a_e = U[user_e] . V[item_e],
    the model's scores of the lists' entries in rank order (mfcd_ragged_dot)."""
    return ragged_scores(U, V, lists)


def pl_rows(a, lists, what="both"):
    """Scores a fp32 [entries] on the GPU, in the lists' order → (loss f64 [n] or None, counts int64 [n, 2] or None,
    g fp32 [entries] or None, status int32 [n]) (mfcd_list_pl): per user the negative log-likelihood of the list's
    stages, (stages, hits) and the loss's gradient in the scores.  what: "loss" (loss and counts), "grad" or "both".
    Deterministic."""
    if what not in _WHAT:
        raise ValueError(f"what must be one of {sorted(_WHAT)}, got {what!r}")
    w = _WHAT[what]
    a = _need(a, torch.float32, "pl_rows", "the scores")
    _need_lists(lists, "pl_rows")
    if a.numel() != lists.entries:
        raise ValueError(f"{a.numel()} scores for {lists.entries} list entries")
    L, dev, n = _lib.load(), a.device, lists.n
    loss = torch.empty(n, dtype=torch.float64, device=dev) if w & 1 else None
    counts = torch.empty((n, 2), dtype=torch.int64, device=dev) if w & 1 else None
    g = torch.empty_like(a) if w & 2 else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_list_pl_workspace_bytes(n, lists.n_tiles), dev)
    _lib.check(L.mfcd_list_pl(_lib.ptr(a), lists.entries, _lib.ptr(lists.row_off), _lib.ptr(lists.depth), n,
                              _lib.ptr(lists.tile_off), lists.n_tiles, w, _lib.ptr(loss), _lib.ptr(counts), _lib.ptr(g),
                              _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return loss, counts, g, status


def pl_hvp_rows(a, y, lists, deg=False):
    """Scores a and a score-space vector y, fp32 [entries] on the GPU, in the lists' order → (q fp32 [entries], status
    int32 [n]), or with deg=True (q, deg, status): the Hessian of the users' list losses of `pl_rows` with respect to the
    scores, applied to y, and its diagonal (mfcd_list_pl_hvp) — per user the sum over the stages of diag(p_k) - p_k p_k^T,
    p_k the softmax of the scores that remain at stage k.  A user with a non-finite score or entry of y gets NaN.
    Deterministic; q does not depend on `deg`, deg does not depend on y."""
    a = _need(a, torch.float32, "pl_hvp_rows", "the scores")
    y = _need(y, torch.float32, "pl_hvp_rows", "the vector")
    _need_lists(lists, "pl_hvp_rows")
    if a.numel() != lists.entries or y.numel() != lists.entries:
        raise ValueError(f"{a.numel()} scores and a vector of {y.numel()} for {lists.entries} list entries")
    L, dev, n = _lib.load(), a.device, lists.n
    q = torch.empty_like(a)
    d = torch.empty_like(a) if deg else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_list_pl_hvp_workspace_bytes(n, lists.n_tiles), dev)
    _lib.check(L.mfcd_list_pl_hvp(_lib.ptr(a), _lib.ptr(y), lists.entries, _lib.ptr(lists.row_off), _lib.ptr(lists.depth), n,
                                  _lib.ptr(lists.tile_off), lists.n_tiles, _lib.ptr(q), _lib.ptr(d), _lib.ptr(status),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return (q, d, status) if deg else (q, status)


def _stages(lists):
    if lists.stages <= 0:
        raise ValueError("the lists record no choice: no user has two entries and a ranked position")
    return lists.stages


def _table_grads(g, lists, U, V):
    return ragged_gather_sum(g, lists, V, "user")[0], ragged_gather_sum(g, lists, U, "item")[0]


class _PlRisk(torch.autograd.Function):
    """sum over the users of the list losses / sum over the users of the stages, as a function of the factor tables.
    Backward is the kernel's g (formed in forward where a gradient is asked for: the loss does not depend on it),
    scaled, then one `ragged_gather_sum` per table."""

    @staticmethod
    def forward(ctx, U, V, lists, total):
        a = list_scores(U, V, lists)[0]
        grad = any(ctx.needs_input_grad[:2])
        loss, _, g, _ = pl_rows(a, lists, "both" if grad else "loss")
        ctx.save_for_backward(U, V, g)
        ctx.lists, ctx.total = lists, total
        return (loss.sum() / total).float()

    @staticmethod
    def backward(ctx, grad_out):
        U, V, g = ctx.saved_tensors
        dU, dV = _table_grads(g * (grad_out.float() / ctx.total), ctx.lists, U, V)
        return dU, dV, None, None


def pl_risk(U, V, lists):
    """The Plackett–Luce risk of the model U V^T on ranked lists: the sum over the users of the negative log-likelihood
    of the list's stages, divided by the number of stages of all users — the mean negative log-likelihood per choice, a
    global normalisation as `ratings.ratings_risk`.  → 0-dim fp32 device tensor, differentiable with respect to fp32 U
    and V.  Lists without a stage: ValueError."""
    for name, t in (("U", U), ("V", V)):
        _need(t, torch.float32, "the list risk", name)
    _need_lists(lists, "the list risk")
    return _PlRisk.apply(U, V, lists, _stages(lists))


def pl_hvp(U, V, dU, dV, lists, gauss_newton=False):
    """The Hessian of `pl_risk` with respect to both tables, applied to a direction (dU, dV) of their shapes → (HU, HV)
    fp32, as `ratings.ratings_hvp` on ranked lists: with dA = dU[user] . V[item] + U[user] . dV[item] over the entries,
    q = `pl_hvp_rows`(a, dA), g = `pl_rows`(a, "grad") and c = 1 / lists.stages,
        HU = c [gather_sum(q, V) + gather_sum(g, dV)] by user,   HV = c [gather_sum(q, U) + gather_sum(g, dU)] by item.
    gauss_newton=True drops the two g terms: the positive semi-definite part.  fp32 GPU tensors; nothing is modified."""
    tables = [_need(t, torch.float32, "the list Hessian-vector product", name)
              for name, t in (("U", U), ("V", V), ("dU", dU), ("dV", dV))]
    _need_lists(lists, "the list Hessian-vector product")
    U, V, dU, dV = (t.detach() for t in tables)
    if dU.shape != U.shape or dV.shape != V.shape:
        raise ValueError(f"a direction of shapes {tuple(dU.shape)}, {tuple(dV.shape)} for tables {tuple(U.shape)}, "
                         f"{tuple(V.shape)}")
    c = 1.0 / _stages(lists)
    a = list_scores(U, V, lists)[0]
    dA = list_scores(dU, V, lists)[0].add_(list_scores(U, dV, lists)[0])
    q = pl_hvp_rows(a, dA, lists)[0]
    HU, HV = _table_grads(q, lists, U, V)
    if not gauss_newton:
        g = pl_rows(a, lists, "grad")[2]
        gU, gV = _table_grads(g, lists, dU, dV)
        HU, HV = HU.add_(gU), HV.add_(gV)
    return HU.mul_(c), HV.mul_(c)


_KEYS = ("choice_log_likelihood", "choice_accuracy", "uniform_log_likelihood", "kendall_tau")


def pl_metrics(U, V, lists):
    """The model's metrics on ranked lists (typically a held-out split), per user and as the mean over the users where
    the value is defined (0.0 if there are none); every key also with the suffix `_per_user` (float64 numpy, NaN where
    undefined: a user without a stage):
      choice_log_likelihood    -loss / stages: the mean log-likelihood of the user's recorded choices
      choice_accuracy          hits / stages: the share of them the model would have made (ties count)
      uniform_log_likelihood   the same of the model with equal scores, -sum over the stages of log(L - k) / stages
      kendall_tau              tau-b of the scores against the order among the list's ranked entries
                               (mfcd_pair_ragged_stats on them, value = minus the rank); NaN below two ranked entries
    One device → host transfer."""
    U, V = _need(U, torch.float32, "pl_metrics", "U").detach(), _need(V, torch.float32, "pl_metrics", "V").detach()
    _need_lists(lists, "pl_metrics")
    a = list_scores(U, V, lists)[0]
    loss, counts, _, _ = pl_rows(a, lists, "loss")
    L, dev, n = _lib.load(), a.device, lists.n
    kc = torch.empty((n, 4), dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ranked = a[lists.rank_idx]
    ws = _lib.workspace(L.mfcd_pair_ragged_workspace_bytes(n, lists.rank_n_tiles), dev)
    _lib.check(L.mfcd_pair_ragged_stats(_lib.ptr(ranked), _lib.ptr(lists.rank_value), ranked.numel(),
                                        _lib.ptr(lists.rank_off), n, _lib.ptr(lists.rank_tile_off), lists.rank_n_tiles,
                                        1.0, 0, 1, _lib.ptr(kc), None, _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr(dev)))
    # every count is below 2^53: exact in f64, and the call's one device -> host transfer
    h = torch.cat((loss[:, None], counts.double(), kc.double()), 1).cpu().numpy()
    st = lists.user_stages.astype(np.float64)
    log_fact = np.concatenate(([0.0], np.cumsum(np.log(np.arange(1, max(int(lists.lengths.max(initial=0)), 1) + 1.0)))))
    uniform = log_fact[lists.lengths] - log_fact[lists.lengths - lists.user_stages]
    per = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        has = (st > 0) & (h[:, 1] >= 0)
        per["choice_log_likelihood"] = np.where(has, -h[:, 0] / st, np.nan)
        per["choice_accuracy"] = np.where(has, h[:, 2] / st, np.nan)
        per["uniform_log_likelihood"] = np.where(st > 0, -uniform / st, np.nan)
    per["kendall_tau"] = P.pairwise_from_counts(h[:, 3:7].astype(np.int64), None, lists.user_depth)["kendall_tau"]
    out = {}
    for name in _KEYS:
        v = per[name]
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    return out


def fit_lists(binding, lists, steps, log_every=0):
    """`ratings.fit_ratings` on `pl_risk`: `steps` steps of Adam, fused — per step the entries' scores (mfcd_ragged_dot),
    the list kernel's g (mfcd_list_pl), the two gather-sums into dense gradients and one mfcd_adam_dense on the caller's
    torch.optim.Adam state, which stays valid (binding: an engine.AdamBinding, or a (model, optimizer) pair; fp32 tables
    only).  Nothing waits for the device inside the loop; the risks are logged on the device and read once → (steps
    taken, risks) as `fit_ratings` returns them."""
    from . import engine
    if not isinstance(binding, engine.AdamBinding):
        binding = engine.AdamBinding(*binding)
    for name, t in zip(("model.U", "model.V"), binding.tensors()[:2]):
        engine._require_cuda_param(t, name)                    # fp32 only: bf16 tables are refused here
    _need_lists(lists, "the list fit")
    L = _lib.load()
    U, V, mU, vU, mV, vV = binding.tensors()
    n, m, d, dev = U.shape[0], V.shape[0], U.shape[1], U.device
    inv = 1.0 / _stages(lists)
    steps, k = int(steps), int(log_every)
    at = ([t for t in range(0, steps, k)] + [steps]) if k > 0 else []
    log = torch.zeros(max(len(at), 1), dtype=torch.float64, device=dev)
    state = [_lib.ptr(t) for t in (U, V, mU, vU, mV, vV)]
    lr, b1, b2, eps, wd = binding.hyper()
    stream = _lib.stream_ptr(dev)
    try:
        for t in range(steps):
            a = list_scores(U, V, lists)[0]
            logged = k > 0 and t % k == 0
            loss, _, g, _ = pl_rows(a, lists, "both" if logged else "grad")
            if logged:
                log[t // k] += loss.sum()
            gU, gV = _table_grads(g.mul_(inv), lists, U, V)
            _lib.check(L.mfcd_adam_dense(*state, _lib.ptr(gU), _lib.ptr(gV), binding.step + 1, n, m, d, lr, b1, b2, eps, wd,
                                         stream))
            binding.advance(1, defer=True)
    finally:
        binding.flush()         # an interrupt must not leave the moments ahead of the optimizer's `step` tensors
    if k <= 0:
        return [], []
    log[len(at) - 1] += pl_rows(list_scores(U, V, lists)[0], lists, "loss")[0].sum()
    return at, (log[:len(at)] * inv).cpu().tolist()       # the one device->host transfer of the run


def sample_rankings(X, length, depth=None, s=1.0, seed=0, users=None):
    """Ranked lists drawn from a dense truth X [n, m] → RankedLists on X's device.  Every user (users=None: all rows of X;
    else the given user ids) is shown `length` items, a uniform draw without replacement, and orders them by
    s x + Gumbel noise: an exact Plackett–Luce draw with scores s x (s = inf: the noiseless order, ties by item).  depth
    as `RankedLists` takes it.  Plain torch on X's device, f64 keys from a private torch.Generator(seed): the global RNG
    states are not touched."""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError("sample_rankings takes a dense [n, m] tensor")
    n, m = X.shape
    length, s = int(length), float(s)
    if not 0 <= length <= m:
        raise ValueError(f"length must lie in [0, {m}]")
    if not s >= 0.0:
        raise ValueError("s must be >= 0")
    dev = X.device
    rows = torch.arange(n, device=dev) if users is None else torch.as_tensor(users, dtype=torch.int64, device=dev).reshape(-1)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    shown = torch.rand((rows.numel(), m), generator=gen, device=dev).topk(length, dim=1).indices.sort(dim=1).values
    x = X.detach()[rows[:, None], shown].double()
    if np.isinf(s):
        key = x
    else:
        unif = torch.rand(x.shape, generator=gen, device=dev, dtype=torch.float64).clamp_min(1e-300)
        key = s * x - torch.log(-torch.log(unif))
    order = key.argsort(dim=1, descending=True, stable=True)
    items = shown.gather(1, order)
    positions = torch.arange(length, device=dev).expand_as(items)
    return RankedLists(rows[:, None].expand_as(items), items, positions, n, m, depth).to(dev)
