"""Full-catalogue ranking metrics on the device (include/mfcd.h: mfcd_rank_entries).

`rank_entries` gives, for every listed (row, column) of a score matrix, the position the column has in the row's ordered
list of admissible columns — `topk.topk_rows`' `best` order, with the same exclusion lists — without sorting a row and
without forming anything n x m.  `ranking_metrics` turns the ranks of a held-out ratings split, with the training split
barred, into recall@k, precision@k, hit@k, NDCG@k, MRR, mean rank and AUC per user.  The matrix is a dense fp32 GPU tensor,
a `generation_data.FactoredMatrix` or a pair (A, B) of GPU tensors, as for `topk_rows`.  There is no CPU form.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .topk import _resolve

EntryRanks = namedtuple("EntryRanks", "rank ties admissible status score")
EntryRanks.__doc__ = """Device tensors of `rank_entries`: rank, ties int32 [entries], admissible, status int32 [rows], score
fp32 [entries] or None."""


def _csr(src, ids64, nrows, n, m, dev, what):
    """A `RatingsData` on the device or a ready CSR pair → (offsets int64 [nrows + 1], items int32), indexed by requested
    row.  A RatingsData is indexed by user: with `ids64` its rows are gathered (the items stay ascending per row)."""
    if isinstance(src, (tuple, list)) and len(src) == 2:
        off, items = src
        for t, dt in ((off, torch.int64), (items, torch.int32)):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt:
                raise _lib.MfcdError(f"rank_entries needs {what} as (offsets int64, items int32) GPU tensors "
                                     "(there is no CPU fallback)")
        if off.dim() != 1 or off.numel() != nrows + 1:
            raise ValueError(f"{what}: {off.numel()} offsets for {nrows} requested rows")
        return off.to(dev).contiguous(), items.to(dev).reshape(-1).contiguous()
    if not hasattr(src, "row_off") or not hasattr(src, "item"):
        raise TypeError(f"{what} must be a RatingsData or a CSR pair (offsets, items)")
    if not src.row_off.is_cuda:
        raise _lib.MfcdError(f"rank_entries needs {what} on a GPU device: data.to(device) (there is no CPU fallback)")
    if src.n != n or src.m != m:
        raise ValueError(f"{what} of {src.n} users and {src.m} items for a matrix of shape [{n}, {m}]")
    return _gather_rows(src.row_off.to(dev), src.item.to(dev), ids64, nrows, n)


def _gather_rows(off, items, ids64, nrows, n):
    """The CSR rows `ids64` of a table of n rows, in that order (None: the table as it is)."""
    if ids64 is None:
        return off, items
    if nrows and (int(ids64.min()) < 0 or int(ids64.max()) >= n):
        raise IndexError(f"row number out of range for a table of {n} users")
    dev = off.device
    lens = off[ids64 + 1] - off[ids64]
    out = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
    out[1:] = torch.cumsum(lens, 0)
    total = int(out[-1])
    src_pos = torch.repeat_interleave(off[ids64] - out[:-1], lens) + torch.arange(total, device=dev)
    return out, items[src_pos].contiguous()


def rank_entries(X, targets, exclude=None, rows=None, scores=False):
    """→ `EntryRanks`: for every target, the number of admissible columns of its row that precede it.

    X        dense fp32 GPU tensor [n, m], a FactoredMatrix, or a pair (A, B) of GPU tensors (X = A @ B.T)
    targets  the entries to rank: a `ratings.RatingsData` on the device (its row_off / item are used as they are), or a
             ready CSR pair (offsets int64 [len(rows) + 1], items int32) of device tensors, any order within a row
    exclude  None, or the barred columns of every row in the same two forms; strictly ascending within a row (a
             RatingsData's are)
    rows     None (every row) or row numbers, any order, repeats allowed; a CSR pair is indexed by position in `rows`
    scores   also return the fp32 score of every entry, the number that was compared

    Order: `topk_rows`' `best` — descending score, -0.0 equal to +0.0, NaN above +inf, equal scores by ascending column.
    rank is the position the column has in `topk_rows(X, k, exclude=...)`'s list, ties the number of other admissible
    columns with an equal score.  An entry whose own column is barred has rank -1 and ties -1.  A row with an invalid
    list, target or row number has status 2, admissible -1 and rank -1, ties -1, score NaN for its entries; the other
    rows are unaffected.  Deterministic: every count is an integer."""
    Xd, A, B, n, m, d, dev = _resolve(X, None)
    L = _lib.load()
    if rows is None:
        ids64, ids, nrows = None, None, n
    else:
        ids64 = torch.as_tensor(rows).reshape(-1).to(device=dev, dtype=torch.int64)
        ids, nrows = ids64.to(torch.int32).contiguous(), ids64.numel()
    t_off, t_items = _csr(targets, ids64, nrows, n, m, dev, "targets")
    entries = t_items.numel()
    e_off = e_items = None
    excl_entries = 0
    if exclude is not None:
        e_off, e_items = _csr(exclude, ids64, nrows, n, m, dev, "exclude")
        excl_entries = e_items.numel()
        if excl_entries == 0:
            e_items = torch.zeros(1, dtype=torch.int32, device=dev)
    # entries outside every row's slice are not written by the kernel
    rank = torch.full((entries,), -1, dtype=torch.int32, device=dev)
    ties = torch.full((entries,), -1, dtype=torch.int32, device=dev)
    score = torch.full((entries,), float("nan"), dtype=torch.float32, device=dev) if scores else None
    admissible = torch.empty(nrows, dtype=torch.int32, device=dev)
    status = torch.empty(nrows, dtype=torch.int32, device=dev)
    ws = None
    if Xd is None:
        nbytes = L.mfcd_rank_entries_workspace_bytes(nrows, m, d, entries)
        if nbytes == 0:
            raise _lib.MfcdError(f"rank_entries: sizes out of range (rows {nrows}, m {m}, d {d})")
        ws = _lib.workspace(nbytes, dev)
    _lib.check(L.mfcd_rank_entries(Xd.data_ptr() if Xd is not None else None, Xd.stride(0) if Xd is not None else 0,
                                   _lib.ptr(A), _lib.ptr(B), d, _lib.ptr(ids), nrows, n, m, _lib.ptr(t_off),
                                   _lib.ptr(t_items) if entries else None, entries, _lib.ptr(e_off), _lib.ptr(e_items),
                                   excl_entries, _lib.ptr(rank) if entries else None,
                                   _lib.ptr(ties) if entries else None, _lib.ptr(score) if entries else None,
                                   _lib.ptr(admissible) if nrows else None, _lib.ptr(status) if nrows else None,
                                   _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr(dev)))
    return EntryRanks(rank, ties, admissible, status, score)


def metrics_from_ranks(off, rank, admissible, status, ks=(10,)):
    """The metric formulas of `ranking_metrics` on host arrays: off int64 [rows + 1], rank int32 [entries] (-1: dropped),
    admissible and status int32 [rows].  Every sum is f64 in a fixed order (np.bincount adds its weights in array order,
    the entries sorted by (row, rank)), so equal ranks give equal bits."""
    off, rank = np.asarray(off, dtype=np.int64), np.asarray(rank, dtype=np.int64)
    admissible, status = np.asarray(admissible, dtype=np.int64), np.asarray(status, dtype=np.int64)
    n = off.size - 1
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError("every k must be >= 1")
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(off)) if n else np.zeros(0, dtype=np.int64)
    rank = rank[off[0]:off[-1]] if n else rank[:0]
    invalid = status[row_of] != 0
    keep = (rank >= 0) & ~invalid
    ue, rk = row_of[keep], rank[keep]
    order = np.lexsort((rk, ue))
    ue, rk = ue[order], rk[order]
    T = np.bincount(ue, minlength=n).astype(np.int64)
    start = np.cumsum(T) - T
    has = T > 0
    at = np.arange(ue.size, dtype=np.int64)
    first = np.ones(ue.size, dtype=bool)
    first[1:] = (ue[1:] != ue[:-1]) | (rk[1:] != rk[:-1])
    pos = np.maximum.accumulate(np.where(first, at, 0)) - start[ue]   # the row's targets with a smaller rank
    Tf = T.astype(np.float64)
    per = {}

    def per_user(weights):
        return np.bincount(ue, weights=weights, minlength=n).astype(np.float64)

    with np.errstate(invalid="ignore", divide="ignore"):
        min_rank = np.full(n, np.nan)
        min_rank[has] = rk[start[has]]
        gain = 1.0 / np.log2(rk.astype(np.float64) + 2.0)
        ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(max(ks), dtype=np.float64) + 2.0))))
        for k in ks:
            hits = per_user((rk < k).astype(np.float64))
            per[f"recall@{k}"] = np.where(has, hits / Tf, np.nan)
            per[f"precision@{k}"] = np.where(has, hits / k, np.nan)
            per[f"hit@{k}"] = np.where(has, (min_rank < k).astype(np.float64), np.nan)
            per[f"ndcg@{k}"] = np.where(has, per_user(np.where(rk < k, gain, 0.0)) / ideal[np.minimum(T, k)], np.nan)
        per["mrr"] = 1.0 / (min_rank + 1.0)
        per["mean_rank"] = np.where(has, per_user(rk.astype(np.float64)) / Tf, np.nan)
        N = (admissible - T).astype(np.float64)
        per["auc"] = np.where(has & (N > 0), 1.0 - per_user((rk - pos).astype(np.float64)) / (Tf * N), np.nan)
    out = {}
    for name, v in per.items():
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    out["users"] = int(has.sum())
    out["targets"] = int(keep.sum())
    out["dropped_barred"] = int(((rank < 0) & ~invalid).sum())
    out["dropped_invalid"] = int(invalid.sum())
    return out


def ranking_metrics(X, test, train=None, ks=(10,), min_value=None, users=None):
    """Ranking metrics of the score matrix X on a held-out ratings table over the FULL catalogue: every user's targets —
    `test`'s entries, or those with value >= `min_value` — are ranked among all items that are not in `train` (the
    exclusion list; None: nothing is barred).  Relevance is binary; test entries below `min_value` are not targets and
    stay ordinary candidates.  test, train: `ratings.RatingsData` on the device.  users: None = every user, else user
    numbers, returned in that order.

    Per user with T >= 1 targets, from the ranks (`rank_entries`) in f64:
      recall@k     #{rank < k} / T                  precision@k  #{rank < k} / k
      hit@k        [min rank < k]                   mrr          1 / (min rank + 1)
      ndcg@k       sum over rank < k of 1 / log2(rank + 2), divided by the same sum over ranks 0 .. min(T, k) - 1
      mean_rank    the mean of the user's target ranks
      auc          1 - sum_e (rank_e - pos_e) / (T N): pos_e = the user's other targets ranked before e, N = admissible
                   - T the items that are neither barred nor targets; NaN when N = 0.  The share of (target, other item)
                   pairs the model orders correctly in the composite order (score, then item number): an item tied with
                   a target counts as before or after it by its number, with NO half credit for ties — `rank_entries`
                   returns `ties` for callers who want mid-ranks.
    Returns a dict: every key is the mean over the users where it is defined (0.0 if there are none), every key with the
    suffix `_per_user` a float64 numpy array holding NaN for users without a target; `users` counts the users with a
    target and `targets` their entries; targets that are barred themselves (`dropped_barred`) and the entries of rows
    with status 2 (`dropped_invalid`) leave T.  Deterministic."""
    Xd, A, B, n, m, d, dev = _resolve(X, None)
    if not hasattr(test, "row_off") or not test.row_off.is_cuda:
        raise _lib.MfcdError("ranking_metrics needs the held-out ratings as a RatingsData on a GPU device (no CPU fallback)")
    ids64 = None if users is None else torch.as_tensor(users).reshape(-1).to(device=dev, dtype=torch.int64)
    nrows = n if ids64 is None else ids64.numel()
    if min_value is None:
        t_off, t_items = _csr(test, ids64, nrows, n, m, dev, "test")
    else:
        if test.n != n or test.m != m:
            raise ValueError(f"test of {test.n} users and {test.m} items for a matrix of shape [{n}, {m}]")
        keep = test.value.to(dev) >= float(min_value)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(torch.bincount(test.user.to(dev)[keep].long(), minlength=n), 0)
        t_off, t_items = _gather_rows(off, test.item.to(dev)[keep].contiguous(), ids64, nrows, n)
    exclude = None if train is None else _csr(train, ids64, nrows, n, m, dev, "train")
    res = rank_entries(Xd if Xd is not None else (A, B), (t_off, t_items), exclude, rows=ids64)
    return metrics_from_ranks(t_off.cpu().numpy(), res.rank.cpu().numpy(), res.admissible.cpu().numpy(),
                              res.status.cpu().numpy(), ks)
