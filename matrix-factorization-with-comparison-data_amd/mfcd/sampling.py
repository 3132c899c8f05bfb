"""Triplet sampling on the device (include/mfcd.h: mfcd_sample_triplets).

Host side of csrc/sampler.hip: turns a strategy name of the reference (`get_triplets_from_X`, structure.py:533-588)
into a `mfcd_sampler` law, runs blocks of attempts until the request is met or the strategy's attempt budget is spent
(the budgets of the reference: margin 5 000 000 in blocks of 500, top_k 3x, svd 5x the request; the others unbounded),
and returns the triplets in attempt order as a device tensor.  Opt-in (`structure.set_sampler_device`): the default
host samplers consume torch's / numpy's generators draw for draw like the reference; this path has its own Philox
stream (one int64 seed taken from torch's global generator per request), so it is reproducible under
`torch.manual_seed` but distributionally — not bitwise — equal to a reference run.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import cluster as _cluster
from . import topk as _topk
from .rows import resolve

LAW_UNIFORM, LAW_ITEM_CDF, LAW_LISTS, LAW_GROUPS = 0, 1, 2, 3
DEVICE_STRATEGIES = ("random", "margin", "popularity", "variance", "proximity", "top_k", "svd", "cluster")


def _on(X, device):
    """X on the device in the form the kernels read: contiguous, a dense X in fp32, factors as they are kept."""
    X = resolve(X, device)
    return X.map(torch.Tensor.contiguous) if X.factored else X.map(lambda t: t.float().contiguous())


class _Law:
    """A filled mfcd_sampler plus the tensors its pointers refer to (kept alive with it)."""

    def __init__(self, n, m, device):
        self.n, self.m, self.device = int(n), int(m), device
        self.c = _lib.Sampler()
        self.c.law, self.c.n, self.c.m = LAW_UNIFORM, int(n), int(m)
        self.keep = []
        self.budget = None           # attempt budget of the strategy (None: until the request is met)
        self.block_multiple = 1      # the margin strategy counts attempts in blocks of 500
        self.report = lambda got, attempts: None   # the strategy's message for a short result (the reference's own)

    def hold(self, t):
        self.keep.append(t)
        return _lib.ptr(t)


def group_tables(labels, k):
    """The tables of the groups law from one label per item → (members int32 [m]: the item ids grouped by label,
    ascending inside a group; offsets int32 [k + 1] into them), on the labels' device.  ValueError for a label outside
    [0, k) and for a group without items (numpy's choice on an empty array raises there, generation_data.py:242)."""
    lab = torch.as_tensor(labels).reshape(-1).long()
    k = int(k)
    if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= k):
        raise ValueError(f"label outside [0, {k})")
    counts = torch.bincount(lab, minlength=k)
    if k < 1 or int(counts.min()) == 0:
        raise ValueError(f"cluster {int(counts.argmin()) if k >= 1 else 0} of {k} has no items: 'a' cannot be empty")
    members = torch.sort(lab, stable=True)[1].to(torch.int32).contiguous()
    offsets = torch.zeros(k + 1, dtype=torch.int32, device=lab.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return members, offsets


def item_probs(X, strategy, device, popularity_method="zipf", alpha=1.5):
    """The item probabilities p [m] (float64 numpy) of `popularity` (generation_data.py:110-119) and `variance`
    (generation_data.py:90-91)."""
    import generation_data as _gd
    if strategy == "popularity":
        return _gd._popularity_probs(X.shape[1], popularity_method, alpha)
    var = _gd._factored_column_variances(X).numpy() if _lib.is_factored(X) else \
        torch.var(_on(X, device).dense, dim=0).double().cpu().numpy()
    probs = var / var.sum()
    if not np.isfinite(probs).all() or (probs < 0).any():          # e.g. one user: the unbiased variance is NaN
        raise RuntimeError("probability tensor contains either `inf`, `nan` or element < 0")   # as torch.multinomial (ref:95)
    return probs


def item_lists(X, strategy, k, device):
    """The per-user item lists of `proximity` (k best and k worst) and `top_k` (k best) → (k, best int32 [n, k],
    worst int32 [n, k] or None), on the device.  A factored X never becomes dense: its lists come from mfcd_topk_rows
    over the factors (one call, all n rows)."""
    import generation_data as _gd
    m = X.shape[1]
    Xd = _on(X, device)
    fac, Xd = ((Xd.A, Xd.B), None) if Xd.factored else (None, Xd.dense)
    if strategy == "proximity":
        kk = int(_gd._proximity_k(m, k))
        if fac:
            best, worst = _topk.topk_rows(fac, kk, ends="both")
        else:
            best = torch.topk(Xd, k=kk, dim=1)[1].to(torch.int32).contiguous()
            worst = torch.topk(-Xd, k=kk, dim=1)[1].to(torch.int32).contiguous()
        return kk, best, worst
    kk = int(_gd._top_k_k(m, k))
    if fac:
        best = _topk.topk_rows(fac, kk, ends="best")
    else:
        best = torch.topk(Xd, k=kk, dim=1)[1].to(torch.int32).contiguous()
    return kk, best, None


def cluster_labels(X, n_clusters, seed, device):
    """The item clusters of `cluster` (generation_data.py:229-239) → (k, labels int32 [m] on the device)."""
    kk = int(n_clusters)
    if kk < 2:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")   # numpy's (ref:241)
    return kk, _cluster.kmeans(_cluster.item_points(X, device), kk, (int(seed) ^ 0x6B6D65616E73) & (2 ** 63 - 1))[0]


def build_law(X, num_triplets, strategy, device, popularity_method="zipf", alpha=1.5, k=None, max_attempts=5_000_000,
              n_clusters=10, seed=0):
    """The reference's per-strategy set-up (everything in front of its attempt loop, as generation_data defines it) → a
    device law.  `seed`: the request's seed, for a set-up that draws (the k-means++ of `cluster`)."""
    import generation_data as _gd
    n, m = X.shape
    law = _Law(n, m, device)
    c = law.c
    if strategy == "random":
        return law
    if strategy == "margin":
        c.use_margin = 1
        c.margin = float(_gd._margin_threshold(X, num_triplets))
        Xd = _on(X, device)
        if Xd.factored:
            c.A, c.B, c.dx = law.hold(Xd.A), law.hold(Xd.B), Xd.d
        else:
            c.X = law.hold(Xd.dense)
        law.budget, law.block_multiple = int(max_attempts), 500
        law.report = lambda got, attempts: _gd._report_short_margin(X, got, num_triplets, c.margin, attempts)
        return law
    if strategy in ("popularity", "variance"):
        probs = item_probs(X, strategy, device, popularity_method, alpha)
        c.pair_rule = 0 if strategy == "popularity" else 1
        cdf = np.cumsum(probs)
        cdf /= cdf[-1]
        c.law = LAW_ITEM_CDF
        c.cdf = law.hold(torch.from_numpy(cdf).to(device))
        return law
    if strategy in ("proximity", "top_k"):
        kk, best, worst = item_lists(X, strategy, k, device)
        if strategy == "proximity":
            c.list_i, c.list_j, c.pair_rule = law.hold(best), law.hold(worst), 0
        else:
            c.list_i = c.list_j = law.hold(best)
            c.pair_rule = 1
            law.budget = 3 * int(num_triplets)
            law.report = lambda got, attempts: _gd._report_short(got, num_triplets, f", k={kk}")
        c.law, c.k, c.list_row_stride = LAW_LISTS, kk, kk
        return law
    if strategy == "svd":
        top_users, top_items = _gd._svd_top_sets(X, num_triplets)
        items = torch.from_numpy(top_items.astype(np.int32)).to(device)
        c.law, c.k, c.list_row_stride, c.pair_rule = LAW_LISTS, int(items.numel()), 0, 1
        c.list_i = c.list_j = law.hold(items)
        c.users, c.n_users = law.hold(torch.from_numpy(top_users.astype(np.int32)).to(device)), int(top_users.size)
        law.budget = 5 * int(num_triplets)
        law.report = lambda got, attempts: _gd._report_short(got, num_triplets)
        return law
    if strategy == "cluster":                                           # generation_data.py:229-239
        kk, labels = cluster_labels(X, n_clusters, seed, device)
        members, offsets = group_tables(labels, kk)
        c.law, c.k, c.list_row_stride = LAW_GROUPS, kk, int(members.numel())
        c.list_i, c.list_j = law.hold(members), law.hold(offsets)
        return law
    raise ValueError(f"no device law for triplet sampling strategy: {strategy}")


def triplet_keys(rows, m):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return (rows[:, 0] * m + rows[:, 1]) * m + rows[:, 2]


def run_law(law, num_triplets, exclude=None, seed=0):
    """Blocks of attempts until `num_triplets` are kept or the budget is spent → (int32 [T, 3] device tensor in attempt
    order, attempts consumed)."""
    L = _lib.load()
    device, m = law.device, law.m
    want = int(num_triplets)
    out = torch.empty((max(want, 0), 3), dtype=torch.int32, device=device)
    if want <= 0:
        return out, 0
    if isinstance(exclude, torch.Tensor):          # int [E, 3] device triplets (what an earlier request returned)
        e = exclude.to(device=device, dtype=torch.int64).reshape(-1, 3)
        barred = ((e[:, 0] * m + e[:, 1]) * m + e[:, 2]).contiguous()
    else:
        barred = torch.from_numpy(triplet_keys(sorted(exclude), m)).to(device) if exclude else \
            torch.empty(0, dtype=torch.int64, device=device)
    have = attempts = idle = 0
    stream = _lib.stream_ptr(device)
    while have < want and (law.budget is None or attempts < law.budget):
        need = want - have
        A = max(65536, need + need // 4)
        if law.budget is not None:
            A = min(A, law.budget - attempts)
        A = -(-A // law.block_multiple) * law.block_multiple
        ws_bytes = L.mfcd_sample_workspace_bytes(A, barred.numel())
        if ws_bytes == 0:
            raise _lib.MfcdError("triplet request too large for one sampling block")
        ws = _lib.workspace(ws_bytes, device)
        keys = torch.empty(need, dtype=torch.int64, device=device)
        counts = torch.zeros(2, dtype=torch.int64, device=device)
        part = out[have:]
        _lib.check(L.mfcd_sample_triplets(ctypes.byref(law.c), _lib.ptr(barred) if barred.numel() else None,
                                          barred.numel(), attempts, A, int(seed) & 0xFFFFFFFFFFFFFFFF, need,
                                          _lib.ptr(part), _lib.ptr(keys), _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
                                          stream))
        got, used = (int(v) for v in counts.tolist())
        used = -(-used // law.block_multiple) * law.block_multiple
        attempts += used
        have += got
        if got:
            barred = torch.cat((barred, keys[:got]))
        idle = 0 if got else idle + 1
        if idle >= 16 and law.budget is None:      # the reference's loop would spin forever: nothing left to draw
            raise ValueError(f"cannot draw {want} distinct triplets with this strategy: {have} found, none in the "
                             f"last {idle} blocks of attempts")
    return out[:have], attempts


def sample_triplets(X, num_triplets, strategy="random", exclude=None, device=None, seed=None, **kw):
    """Device form of `get_triplets_from_X` → int32 [T, 3] device tensor (T <= num_triplets), attempt order."""
    if device is None:
        device = X.device if torch.is_tensor(X) and X.is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.MfcdError("device triplet sampling needs a GPU device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
    law = build_law(X, int(num_triplets), strategy, device, seed=seed, **kw)
    trip, attempts = run_law(law, num_triplets, exclude, seed)
    law.report(trip.shape[0], attempts)
    return trip
