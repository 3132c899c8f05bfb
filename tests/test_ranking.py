"""mfcd_rank_entries on the device against the numpy model of tests/rank_entries_model.py (exact: every output is an
integer count, and every score of these inputs is exact in fp32 unless a test says otherwise), against mfcd_topk_rows
(an identity: both entries compare the numbers one score kernel writes), and mfcd/ranking.py's metrics end to end."""
import numpy as np
import pytest
import torch

import rank_entries_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev_csr(off, items):
    return (torch.from_numpy(np.asarray(off, dtype=np.int64)).to(DEV),
            torch.from_numpy(np.asarray(items, dtype=np.int32)).to(DEV))


def _lists(rng, n, m, max_t=40):
    """Per row 0 .. max_t targets in any order, repeats possible, and 0 .. m / 2 barred columns, ascending."""
    targets = [rng.integers(0, m, rng.integers(0, max_t + 1)).tolist() for _ in range(n)]
    barred = [np.sort(rng.choice(m, rng.integers(0, m // 2 + 1), replace=False)).tolist() for _ in range(n)]
    return targets, barred


def _call(X, targets, barred=None, rows=None, scores=True):
    from mfcd import ranking
    res = ranking.rank_entries(X, _dev_csr(*RM.csr(targets)), None if barred is None else _dev_csr(*RM.csr(barred)),
                               rows=rows, scores=scores)
    torch.cuda.synchronize()
    return res


def _host(res):
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_against_model(S, res, targets, barred, row_ids=None):
    """S: the fp32 scores the device compares, [n, m] on the host."""
    rank, ties, adm, status, score = _host(res)
    t_off, t_items = RM.csr(targets)
    e = (None, None) if barred is None else RM.csr(barred)
    w_rank, w_ties, w_adm = RM.rank_entries(S, t_off, t_items, *e, row_ids=row_ids)
    assert rank.dtype == np.int32 and ties.dtype == np.int32 and adm.dtype == np.int32 and status.dtype == np.int32
    assert (status == 0).all()
    assert adm.tolist() == w_adm.tolist()
    assert rank.tolist() == w_rank.tolist()
    assert ties.tolist() == w_ties.tolist()
    if score is not None and t_items.size:
        rows = np.repeat(np.arange(len(targets)), np.diff(t_off))
        if row_ids is not None:
            rows = np.asarray(row_ids)[rows]
        assert _same_bits(score, np.ascontiguousarray(S[rows, t_items], dtype=np.float32))


@pytest.mark.parametrize("n,m", [(7, 1), (5, 100), (300, 1000), (3, 70001)])
def test_dense_mode_equals_the_model(n, m):
    rng = np.random.default_rng(100 + m)
    S = rng.integers(-2, 3, (n, m)).astype(np.float32)                 # ties everywhere
    targets, barred = _lists(rng, n, m)
    X = torch.from_numpy(S).to(DEV)
    _check_against_model(S, _call(X, targets, barred), targets, barred)
    _check_against_model(S, _call(X, targets), targets, None)          # nothing barred: both pointers NULL
    if m == 1000:                                                      # a row stride beyond m
        wide = torch.full((n, m + 24), 9.0, device=DEV)
        wide[:, :m] = X
        _check_against_model(S, _call(wide[:, :m], targets, barred), targets, barred)


def test_dense_mode_with_special_values():
    rng = np.random.default_rng(7)
    n, m = 40, 333
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 1e-45, -1e-45, 3.5], dtype=np.float32)
    S = pool[rng.integers(0, pool.size, (n, m))]
    S[0], S[1], S[2, :] = np.nan, 0.0, np.inf
    S[1, ::2] = -0.0
    targets, barred = _lists(rng, n, m)
    targets[0], targets[1] = list(range(0, m, 7)), list(range(0, m, 5))
    X = torch.from_numpy(S).to(DEV)
    _check_against_model(S, _call(X, targets, barred), targets, barred)


def _int_factors(rng, n, m, d):
    A = rng.integers(-3, 4, (n, d)).astype(np.float32)
    B = rng.integers(-3, 4, (m, d)).astype(np.float32)
    S = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32)      # |score| <= 9 d: exact in fp32
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), S


@pytest.mark.parametrize("d", [2, 3, 64, 100, 256])
def test_factor_mode_with_integer_factors_is_exact(d):
    rng = np.random.default_rng(200 + d)
    n, m = 257, 1000
    A, B, S = _int_factors(rng, n, m, d)
    targets, barred = _lists(rng, n, m)
    _check_against_model(S, _call((A, B), targets, barred), targets, barred)


@pytest.mark.parametrize("d", [64, 100])
def test_factor_mode_is_topk_rows_list_position(d):
    """An identity, not an approximation: the entry's rank is the place of the column in mfcd_topk_rows' list under the
    same exclusion lists, and its score is the value there bit for bit — for every target, no case left out."""
    from mfcd import topk
    rng = np.random.default_rng(300 + d)
    n, m = 300, 1000
    A = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(DEV)
    targets, barred = _lists(rng, n, m)
    res = _call((A, B), targets, barred)
    rank, ties, adm, status, score = _host(res)
    assert (status == 0).all() and adm.tolist() == [m - len(b) for b in barred]
    k = int(min(adm.min(), 900))
    idx, val = topk.topk_rows((A, B), k, exclude=_dev_csr(*RM.csr(barred)), values=True)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    t_off, t_items = RM.csr(targets)
    seen_inside = seen_beyond = seen_barred = 0
    for r in range(n):
        listed = set(idx[r].tolist())
        for e in range(t_off[r], t_off[r + 1]):
            t = int(t_items[e])
            if t in barred[r]:
                assert rank[e] == -1 and ties[e] == -1 and t not in listed
                seen_barred += 1
            elif rank[e] < k:
                assert idx[r, rank[e]] == t
                assert score[e:e + 1].tobytes() == val[r, rank[e]:rank[e] + 1].tobytes()
                seen_inside += 1
            else:
                assert rank[e] < adm[r] and t not in listed
                seen_beyond += 1
    assert seen_inside > 1000 and seen_beyond > 20 and seen_barred > 100


@pytest.mark.parametrize("mode", ["dense", "factor"])
def test_ragged_edges(mode):
    rng = np.random.default_rng(41)
    m, d = 1000, 3
    counts = [0, 1, 255, 256, 257, 600, 1, 1, 5]
    n = len(counts)
    A, B, S = _int_factors(rng, n, m, d)
    X = torch.from_numpy(S).to(DEV) if mode == "dense" else (A, B)
    targets = [rng.integers(0, m, c).tolist() for c in counts]
    barred = [np.sort(rng.choice(m, rng.integers(0, m // 2), replace=False)).tolist() for _ in range(n)]
    targets[6], barred[6] = [417], [c for c in range(m) if c != 417]          # nothing else is admissible
    targets[7], barred[7] = [barred[7][3] if len(barred[7]) > 3 else 5], sorted(set(barred[7]) | {5})   # its target is barred
    res = _call(X, targets, barred)
    _check_against_model(S, res, targets, barred)
    rank, ties, adm, status, score = _host(res)
    t_off, _ = RM.csr(targets)
    assert rank[t_off[6]] == 0 and ties[t_off[6]] == 0 and adm[6] == 1
    assert rank[t_off[7]] == -1 and ties[t_off[7]] == -1
    assert adm[0] == m - len(barred[0])                                        # a row without targets is still answered
    # a shuffled subset of the rows with a repeat
    ids = [5, 2, 7, 2, 0, 8, 4]
    sub = _call(X, [targets[i] for i in ids], [barred[i] for i in ids], rows=ids)
    _check_against_model(S, sub, [targets[i] for i in ids], [barred[i] for i in ids], row_ids=ids)
    s_rank, s_ties, s_adm, s_status, s_score = _host(sub)
    s_off, _ = RM.csr([targets[i] for i in ids])
    for p, i in enumerate(ids):
        a, b = slice(s_off[p], s_off[p + 1]), slice(t_off[i], t_off[i + 1])
        assert _same_bits(s_rank[a], rank[b]) and _same_bits(s_ties[a], ties[b]) and _same_bits(s_score[a], score[b])
        assert s_adm[p] == adm[i]
    # no targets at all: admissible and status are still written
    empty = _call(X, [[] for _ in range(n)], barred)
    assert empty.rank.numel() == 0 and empty.admissible.cpu().tolist() == adm.tolist() and (empty.status == 0).all()


def test_slab_boundary():
    """500 rows of m = 70 001 at d = 2: 479 rows of 70 016 floats fit 128 MiB and the slab takes whole blocks of 128 rows
    of them, 384, so rows 384 .. 499 go through a second slab.  Rows on both sides of the boundary equal a call on those
    rows alone (one slab, other positions) and the model."""
    from mfcd import _lib
    rng = np.random.default_rng(5)
    n, m, d = 500, 70001, 2
    A, B, _ = _int_factors(rng, n, 1, d)
    Bh = rng.integers(-3, 4, (m, d)).astype(np.float32)
    B = torch.from_numpy(Bh).to(DEV)
    slab_rows = _lib.load().mfcd_rank_entries_workspace_bytes(n, m, d, 3 * n) // (70016 * 4)
    assert slab_rows == 384
    targets = [rng.integers(0, m, 3).tolist() for _ in range(n)]
    barred = [np.sort(rng.choice(m, 50, replace=False)).tolist() for _ in range(n)]
    full = _call((A, B), targets, barred)
    rank, ties, adm, status, score = _host(full)
    assert (status == 0).all() and (adm == m - 50).all()
    ids = list(range(slab_rows - 4, slab_rows + 4)) + [0, n - 1]
    alone = _call((A, B), [targets[i] for i in ids], [barred[i] for i in ids], rows=ids)
    S = (A.cpu().numpy().astype(np.float64)[ids] @ Bh.astype(np.float64).T).astype(np.float32)
    _check_against_model(S, alone, [targets[i] for i in ids], [barred[i] for i in ids], row_ids=list(range(len(ids))))
    a_rank, a_ties, a_adm, _, a_score = _host(alone)
    for p, i in enumerate(ids):
        a, b = slice(3 * p, 3 * p + 3), slice(3 * i, 3 * i + 3)
        assert _same_bits(a_rank[a], rank[b]) and _same_bits(a_ties[a], ties[b]) and _same_bits(a_score[a], score[b])


BAD = ["target_eq_m", "target_negative", "barred_not_ascending", "barred_repeated", "barred_out_of_range",
       "barred_negative", "row_id_eq_n", "row_id_negative", "target_offsets_decrease", "barred_offsets_decrease"]


@pytest.mark.parametrize("mode", ["dense", "factor"])
@pytest.mark.parametrize("kind", BAD)
def test_an_invalid_row_is_marked_and_the_others_are_untouched(kind, mode):
    from mfcd import ranking
    rng = np.random.default_rng(9)
    n, m, d = 6, 50, 3
    A, B, S = _int_factors(rng, n, m, d)
    X = torch.from_numpy(S).to(DEV) if mode == "dense" else (A, B)
    ids = [4, 0, 5, 1, 3]
    targets = [rng.integers(0, m, 6).tolist() for _ in ids]
    barred = [np.sort(rng.choice(m, 9, replace=False)).tolist() for _ in ids]
    good = _host(_call(X, targets, barred, rows=ids))
    assert (good[3] == 0).all()

    at = len(ids) if kind.endswith("offsets_decrease") else 2         # where the bad row goes (see below)
    b_id, b_t, b_e = 2, [3, 9, 9, 40], [1, 7, 20, 33]
    if kind == "target_eq_m":
        b_t = [3, m, 9]
    elif kind == "target_negative":
        b_t = [3, 9, -1]
    elif kind == "barred_not_ascending":
        b_e = [1, 20, 7, 33]
    elif kind == "barred_repeated":
        b_e = [1, 7, 7, 33]
    elif kind == "barred_out_of_range":
        b_e = [1, 7, 20, m]
    elif kind == "barred_negative":
        b_e = [-4, 7, 20, 33]
    elif kind == "row_id_eq_n":
        b_id = n
    elif kind == "row_id_negative":
        b_id = -1
    ids2, t2, e2 = list(ids), list(targets), list(barred)
    ids2.insert(at, b_id), t2.insert(at, b_t), e2.insert(at, b_e)
    (t_off, t_items), (e_off, e_items) = RM.csr(t2), RM.csr(e2)
    # A row whose offsets decrease shares off[r + 1] with the next row's start, so it is put last: a list that ends
    # before it starts.
    if kind == "target_offsets_decrease":
        t_off[-1] = t_off[-2] - 2
    elif kind == "barred_offsets_decrease":
        e_off[-1] = e_off[-2] - 1
    res = ranking.rank_entries(X, _dev_csr(t_off, t_items), _dev_csr(e_off, e_items), rows=ids2, scores=True)
    torch.cuda.synchronize()
    rank, ties, adm, status, score = _host(res)
    assert status.tolist() == [2 if p == at else 0 for p in range(len(ids2))]
    assert adm[at] == -1
    if kind != "target_offsets_decrease":                              # else the row has no slice to mark
        sl = slice(t_off[at], t_off[at + 1])
        assert (rank[sl] == -1).all() and (ties[sl] == -1).all() and np.isnan(score[sl]).all() and rank[sl].size == len(b_t)
    g_off, _ = RM.csr(targets)
    for p in range(len(ids)):                                          # the other rows: bit-equal to the call without it
        q = p if p < at else p + 1
        a, b = slice(t_off[q], t_off[q] + 6), slice(g_off[p], g_off[p + 1])
        assert _same_bits(rank[a], good[0][b]) and _same_bits(ties[a], good[1][b]) and _same_bits(score[a], good[4][b])
        assert adm[q] == good[2][p]


def test_two_calls_are_bit_equal_and_the_score_is_optional():
    rng = np.random.default_rng(77)
    n, m, d = 300, 5000, 64                                            # two column chunks per row
    A = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(DEV)
    targets, barred = _lists(rng, n, m, max_t=300)
    first, second, bare = _host(_call((A, B), targets, barred)), _host(_call((A, B), targets, barred)), \
        _host(_call((A, B), targets, barred, scores=False))
    for a, b in zip(first, second):
        assert _same_bits(a, b)
    assert bare[4] is None
    for a, b in zip(first[:4], bare[:4]):
        assert _same_bits(a, b)
    X = A @ B.t()                                                      # the dense mode on any scores agrees with the model
    dense = _call(X, targets, barred)
    _check_against_model(X.cpu().numpy(), dense, targets, barred)


def _ratings_case():
    import structure as St
    from mfcd.ratings import RatingsData
    rng = np.random.default_rng(3)
    n, m, d = 60, 200, 3
    keep = rng.random((n, m)) < 0.3
    keep[7] = False                                                    # a user without ratings
    users, items = np.nonzero(keep)
    values = rng.integers(1, 6, users.size).astype(np.float32)
    data = RatingsData(users, items, values, n, m).to(DEV)
    train, test = data.split([0.8, 0.2], seed=1)
    model = St.MatrixFactorization(n, m, d)
    U, V = rng.integers(-3, 4, (n, d)).astype(np.float32), rng.integers(-3, 4, (m, d)).astype(np.float32)
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(U))
        model.V.copy_(torch.from_numpy(V))
    S = (U.astype(np.float64) @ V.astype(np.float64).T).astype(np.float32)
    return St, model.to(DEV), S, train, test


def _model_metrics(S, test, train, ks, min_value=None, users=None):
    n = S.shape[0]
    off, item, value = (t.cpu().numpy() for t in (test.row_off, test.item, test.value))
    users = list(range(n)) if users is None else list(users)
    targets = [[int(i) for i, v in zip(item[off[u]:off[u + 1]], value[off[u]:off[u + 1]])
                if min_value is None or v >= min_value] for u in users]
    e_off, e_item = train.row_off.cpu().numpy(), train.item.cpu().numpy()
    barred = [e_item[e_off[u]:e_off[u + 1]].tolist() for u in users]
    t_off, t_items = RM.csr(targets)
    rank, _, adm = RM.rank_entries(S, t_off, t_items, *RM.csr(barred), row_ids=users)
    return RM.metrics(t_off, rank, adm, None, ks), targets


def _assert_dicts_agree(got, want):
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        g = got[key]
        if key.endswith("_per_user"):
            assert g.dtype == np.float64 and (np.isnan(g) == np.isnan(w)).all(), key
            assert not (~np.isnan(w)).any() or np.nanmax(np.abs(g - w)) <= 1e-12, key
        else:
            assert abs(g - w) <= 1e-12, key


def test_ranking_metrics_end_to_end():
    St, model, S, train, test = _ratings_case()
    ks = (10, 3)
    got = St.compute_ranking_metrics(model, test, train, ks=ks)
    want, targets = _model_metrics(S, test, train, ks)
    _assert_dicts_agree(got, want)
    assert got["users"] == sum(len(t) > 0 for t in targets) < S.shape[0] and got["dropped_barred"] == 0
    assert 0.0 < got["auc"] < 1.0 and np.isnan(got["auc_per_user"][7])
    # recall@10 is what recommend_items, with the training items left out, recovers of the held-out items
    pairs = torch.stack((train.user.long(), train.item.long()), 1)
    top = St.recommend_items(model, k=10, exclude=pairs).cpu().numpy()
    for u, t in enumerate(targets):
        if t:
            assert got["recall@10_per_user"][u] == len(set(top[u].tolist()) & set(t)) / len(t)
    # a dense X in the model's place, a relevance threshold, a subset of the users in their order
    users = [9, 7, 30, 9, 0]
    got = St.compute_ranking_metrics(torch.from_numpy(S).to(DEV), test, train, ks=(5,), min_value=4.0, users=users)
    want, _ = _model_metrics(S, test, train, (5,), 4.0, users)
    _assert_dicts_agree(got, want)
    assert got["mrr_per_user"].shape == (5,) and got["mrr_per_user"][0] == got["mrr_per_user"][3]
    # without a training table nothing is barred; a target that is barred itself leaves T and is counted
    got = St.compute_ranking_metrics(model, test, None)
    rank, _, adm = RM.rank_entries(S, test.row_off.cpu().numpy(), test.item.cpu().numpy())
    _assert_dicts_agree(got, RM.metrics(test.row_off.cpu().numpy(), rank, adm, None, (10,)))
    got = St.compute_ranking_metrics(model, test, test)
    assert got["users"] == 0 and got["targets"] == 0 and got["dropped_barred"] == test.entries and got["mrr"] == 0.0
