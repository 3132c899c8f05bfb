"""A numpy model of mfcd_rank_entries (include/mfcd.h) and of mfcd/ranking.py's metric formulas, written from the
definitions: the ranks come from one stable argsort of a row's admissible columns on (key, column), the metrics from plain
loops.  `by_definition` is a second, independent form of the ranks (an O(T m) double loop on float comparisons) that the
CPU tests hold the model to."""
import math

import numpy as np


def best_keys(scores):
    """mfcd_topk_rows' `best` key of fp32 scores: ~sortable_key(x), -0.0 as +0.0, NaN -> 0 (above +inf)."""
    x = np.array(scores, dtype=np.float32).reshape(-1)   # a copy
    nan = np.isnan(x)
    x[x == 0.0] = 0.0
    u = x.view(np.uint32)
    s = np.where(u >> np.uint32(31) != 0, ~u, u ^ np.uint32(0x80000000))
    return np.where(nan, np.uint32(0), ~s).astype(np.uint32)


def csr(lists):
    """[[items of row 0], ...] → (offsets int64, items int32)."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    items = np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in lists]) if lists else np.zeros(0)
    return off, items.astype(np.int32)


def rank_entries(S, t_off, t_items, e_off=None, e_items=None, row_ids=None):
    """S: [n, m] scores (cast to fp32).  → (rank, ties int64 [entries], admissible int64 [rows]) for valid inputs."""
    S = np.asarray(S, dtype=np.float32)
    m = S.shape[1]
    rows = len(t_off) - 1
    rank = np.full(len(t_items), -1, dtype=np.int64)
    ties = np.full(len(t_items), -1, dtype=np.int64)
    admissible = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        row = S[r if row_ids is None else row_ids[r]]
        barred = np.zeros(m, dtype=bool)
        if e_off is not None:
            barred[e_items[e_off[r]:e_off[r + 1]]] = True
        cols = np.flatnonzero(~barred)                       # ascending
        keys = best_keys(row)
        order = cols[np.argsort(keys[cols], kind="stable")]  # stable: equal keys stay in ascending column order
        place = np.full(m, -1, dtype=np.int64)
        place[order] = np.arange(order.size)
        admissible[r] = cols.size
        for e in range(t_off[r], t_off[r + 1]):
            t = t_items[e]
            if not barred[t]:
                rank[e] = place[t]
                ties[e] = int((keys[cols] == keys[t]).sum()) - 1
    return rank, ties, admissible


def _precedes(sc, c, st, t):
    if math.isnan(sc) or math.isnan(st):
        return c < t if math.isnan(sc) and math.isnan(st) else math.isnan(sc)
    return sc > st or (sc == st and c < t)


def _same_key(sc, st):
    return (math.isnan(sc) and math.isnan(st)) or sc == st


def by_definition(S, t_off, t_items, e_off=None, e_items=None):
    """The same outputs from the definition itself: for every target, a loop over the row's columns."""
    S = np.asarray(S, dtype=np.float32)
    n, m = S.shape
    rank, ties, admissible = [], [], []
    for r in range(n):
        barred = set() if e_off is None else set(int(c) for c in e_items[e_off[r]:e_off[r + 1]])
        admissible.append(m - len(barred))
        for e in range(t_off[r], t_off[r + 1]):
            t = int(t_items[e])
            if t in barred:
                rank.append(-1)
                ties.append(-1)
                continue
            before = equal = 0
            for c in range(m):
                if c == t or c in barred:
                    continue
                before += _precedes(float(S[r, c]), c, float(S[r, t]), t)
                equal += _same_key(float(S[r, c]), float(S[r, t]))
            rank.append(before)
            ties.append(equal)
    return np.array(rank, dtype=np.int64), np.array(ties, dtype=np.int64), np.array(admissible, dtype=np.int64)


def metrics(off, rank, admissible, status=None, ks=(10,)):
    """mfcd/ranking.py's dict from per-entry ranks, in plain loops (f64)."""
    n = len(off) - 1
    names = [f"{a}@{k}" for k in ks for a in ("recall", "precision", "hit", "ndcg")] + ["mrr", "mean_rank", "auc"]
    per = {name: np.full(n, np.nan) for name in names}
    users = targets = barred = invalid = 0
    for u in range(n):
        mine = [int(x) for x in rank[off[u]:off[u + 1]]]
        if status is not None and status[u] != 0:
            invalid += len(mine)
            continue
        barred += sum(x < 0 for x in mine)
        ranks = sorted(x for x in mine if x >= 0)
        T = len(ranks)
        if T == 0:
            continue
        users += 1
        targets += T
        for k in ks:
            hits = sum(x < k for x in ranks)
            per[f"recall@{k}"][u] = hits / T
            per[f"precision@{k}"][u] = hits / k
            per[f"hit@{k}"][u] = float(ranks[0] < k)
            dcg = sum(1.0 / math.log2(x + 2) for x in ranks if x < k)
            per[f"ndcg@{k}"][u] = dcg / sum(1.0 / math.log2(i + 2) for i in range(min(T, k)))
        per["mrr"][u] = 1.0 / (ranks[0] + 1)
        per["mean_rank"][u] = sum(ranks) / T
        N = int(admissible[u]) - T
        if N > 0:
            wrong = sum(x - sum(y < x for y in ranks) for x in ranks)   # other items ahead of each target
            per["auc"][u] = 1.0 - wrong / (T * N)
    out = {}
    for name, v in per.items():
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    out.update(users=users, targets=targets, dropped_barred=barred, dropped_invalid=invalid)
    return out
