"""GPU tests of the implicit-feedback risk kernel and of what is built on it (include/mfcd.h: mfcd_implicit_rows;
mfcd/implicit.py: implicit_rows, implicit_risk, implicit_metrics, fit_implicit; structure.implicit_risk,
train_model_implicit, compute_implicit_metrics) against the float64 model of tests/implicit_model.py.

Shapes: with C = implicit.CHUNK columns per workgroup of the column pass and T = implicit.TILE positives per tile,
m in {1, 2, 63, 64, 65, C-1, C, C+1, 2C+3} and, per m, one row for every L in {0, 1, 2, 63, 64, 65, T-1, T, T+1, m-1, m}
clipped to m: an empty side, a single pair, the wave boundary, a partly filled and an exactly full tile of positives and
chunk of columns, a second chunk of one column, three chunks with a short last one, neg = 1 and neg = 0.  Values lie in
[-3, 3], except one row with scores in {-60, 0, 60} (differences of 120: exp underflows, nothing may overflow).

Integer outputs are exact.  Float outputs are compared on the mean term — sums / (pos neg), g_j / pos for a negative,
g_i / neg for a positive — at rtol 2e-5, atol 2e-6, the project's fp32 pair tolerance.  Its derivation in the docstring of
tests/test_pair_grad.py carries over: the per-pair arithmetic is the same (the difference, one v_exp_f32, one reciprocal,
one v_log_f32, the selects) and so are the fp32 runs of at most 64 terms before an f64 sum: about 10 * 2^-24 absolute per
term and 33 * 2^-24 relative from a run, 6e-7 + 2e-6 |mean term|.  The reference of every shape is computed once per
module and shared."""
import functools

import numpy as np
import pytest
import torch

import implicit_model as IM
import rank_entries_model as RM

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
VARIANTS = ("none", "barred", "overlap")


def _CT():
    from mfcd import implicit
    return implicit.CHUNK, implicit.TILE


def _ms():
    C, _ = _CT()
    return [1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]


def _Ls(m):
    _, T = _CT()
    return sorted({min(L, m) for L in (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, m - 1, m)})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _lists(m, variant):
    """One row per L, then the row of extreme scores (L about m / 3) → (pos lists, barred lists)."""
    rng = np.random.default_rng(1000 * m + VARIANTS.index(variant))
    pos, excl = [], []
    for L in _Ls(m) + [max(m // 3, min(m, 1))]:
        p = np.sort(rng.choice(m, L, replace=False))
        if variant == "none":
            e = np.zeros(0, dtype=np.int64)
        elif variant == "barred":
            rest = np.setdiff1d(np.arange(m), p)
            e = np.sort(rng.choice(rest, min(rest.size, max(1, m // 5)), replace=False)) if rest.size else rest
        else:
            e = np.sort(rng.choice(m, max(1, m // 4), replace=False))
            if L:
                e = np.union1d(e, p[:1 + L // 3])        # barred positives, for certain
        pos.append(p)
        excl.append(e)
    return pos, excl


@functools.lru_cache(maxsize=None)
def _scores(m):
    rng = np.random.default_rng(77 + m)
    rows = len(_Ls(m)) + 1
    S = rng.uniform(-3.0, 3.0, (rows, m)).astype(np.float32)
    S[-1] = rng.choice(np.array([-60.0, 0.0, 60.0], dtype=np.float32), m)
    return S


@functools.lru_cache(maxsize=None)
def _want(m, variant):
    """The model of the dense case (m, variant), computed once."""
    pos, excl = _lists(m, variant)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    return IM.rows(_scores(m), po, pi, None if variant == "none" else eo, ei)


def _dev_lists(m, variant, dev, sel=None):
    pos, excl = _lists(m, variant)
    if sel is not None:
        pos, excl = [pos[k] for k in sel], [excl[k] for k in sel]
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    P = (torch.from_numpy(po).to(dev), torch.from_numpy(pi).to(dev))
    E = None if variant == "none" else (torch.from_numpy(eo).to(dev), torch.from_numpy(ei).to(dev))
    return P, E


def _compare(res, want, tag, coef=None):
    """Device outputs against the model's (counts, sums, g): integers exactly, floats on the mean term."""
    wc, ws, wg = want
    counts, sums, g = res.counts.cpu().numpy(), res.sums.cpu().numpy(), res.g.cpu().numpy().astype(np.float64)
    assert (res.status.cpu().numpy() == 0).all(), tag
    assert np.array_equal(counts, wc), (tag, counts, wc)
    pos, neg = wc[:, 0].astype(np.float64), wc[:, 1].astype(np.float64)
    pn = np.maximum(pos * neg, 1.0)
    err = np.abs(sums / pn - ws / pn)
    print(f"{tag}: worst mean-term error of the sums {np.nanmax(err):.3e}")
    np.testing.assert_allclose(sums / pn, ws / pn, rtol=RTOL, atol=ATOL, err_msg=tag)
    assert np.all(sums[pos * neg == 0] == 0.0), tag
    c = np.ones(len(pn)) if coef is None else np.asarray(coef, dtype=np.float64)
    # a negative column is divided by pos, a positive one by neg; barred columns are 0 in both
    div = np.where(wg > 0, pos[:, None], np.where(wg < 0, neg[:, None], 1.0)) * np.abs(c)[:, None]
    div = np.maximum(div, 1e-300)
    print(f"{tag}: worst mean-term error of g {np.abs(g / div - wg / div).max():.3e}")
    np.testing.assert_allclose(g / div, wg / div, rtol=RTOL, atol=ATOL, err_msg=tag)
    assert np.all(g[wg == 0] == 0.0), tag


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", _ms())
def test_dense_rows_match_the_f64_model(dev, m, variant):
    from mfcd import implicit
    X = torch.from_numpy(_scores(m)).to(dev)
    P, E = _dev_lists(m, variant, dev)
    res = implicit.implicit_rows(X, P, E, grad=True)
    _compare(res, _want(m, variant), f"dense m={m} {variant}")
    # a statistics-only call and the prepare pass alone return the same numbers
    stats = implicit.implicit_rows(X, P, E)
    assert stats.g is None and torch.equal(stats.counts, res.counts) and torch.equal(stats.sums, res.sums)
    prep = implicit.implicit_rows(X, P, E, prepare_only=True)
    assert prep.sums is None and torch.equal(prep.counts[:, :2], res.counts[:, :2]) and int(prep.counts[:, 2:].abs().sum()) == 0
    if variant == "overlap":
        pos, excl = _lists(m, variant)
        assert any(np.intersect1d(p, e).size for p, e in zip(pos, excl)) or m == 1


@pytest.mark.parametrize("d", [1, 2, 33])
@pytest.mark.parametrize("m", _ms())
def test_factor_mode_with_exact_scores_matches_the_f64_model(dev, m, d):
    """Factors on the grid of halves: every product and every partial sum is exact in fp32, so the device's scores are
    the model's whatever the order of the MFMA sums."""
    from mfcd import implicit
    rng = np.random.default_rng(31 * m + d)
    variant = VARIANTS[(m + d) % 3]
    rows = len(_Ls(m)) + 1
    n = rows + 3
    hi = 3 if d == 1 else 1
    A = (rng.integers(-2, 3, (n, d)) * 0.5).astype(np.float32)
    B = (rng.integers(-2 * hi, 2 * hi + 1, (m, d)) * 0.5).astype(np.float32)
    ids = rng.permutation(n)[:rows]
    S = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32)
    pos, excl = _lists(m, variant)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    want = IM.rows(S, po, pi, None if variant == "none" else eo, ei, row_ids=ids)
    P, E = _dev_lists(m, variant, dev)
    res = implicit.implicit_rows((torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)), P, E, rows=ids, grad=True)
    _compare(res, want, f"factored m={m} d={d} {variant}")


def _device_scores(A, B, rows, m, dev):
    """The scores the device forms for the requested rows: what mfcd_rank_entries reports for every column."""
    from mfcd import ranking
    nrows = len(rows)
    off = torch.arange(nrows + 1, dtype=torch.int64, device=dev) * m
    items = torch.arange(m, dtype=torch.int32, device=dev).repeat(nrows)
    res = ranking.rank_entries((A, B), (off, items), rows=rows, scores=True)
    return res.score.reshape(nrows, m).cpu().numpy()


@pytest.mark.parametrize("m,d", [(65, 33), (2049, 2), (4099, 33)])
def test_factor_mode_with_random_factors_matches_the_model_on_the_devices_scores(dev, m, d):
    from mfcd import implicit
    assert m in _ms()
    rng = np.random.default_rng(5 * m + d)
    rows = len(_Ls(m)) + 1
    n = rows + 2
    A = torch.from_numpy((rng.standard_normal((n, d)) * (1.5 / np.sqrt(d))).astype(np.float32)).to(dev)
    B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(dev)
    ids = rng.permutation(n)[:rows]
    S = _device_scores(A, B, ids, m, dev)
    pos, excl = _lists(m, "overlap")
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    P, E = _dev_lists(m, "overlap", dev)
    res = implicit.implicit_rows((A, B), P, E, rows=ids, grad=True)
    _compare(res, IM.rows(S, po, pi, eo, ei), f"random factors m={m} d={d}")


def test_rows_with_repeats_in_any_order_and_coef(dev):
    from mfcd import implicit
    C, _ = _CT()
    m = C + 1
    rng = np.random.default_rng(3)
    S = _scores(m)
    X = torch.from_numpy(S).to(dev)
    n = S.shape[0]
    ids = np.concatenate((rng.permutation(n), [2, 2, n - 1, 0]))
    coef = rng.uniform(0.5, 2.0, ids.size).astype(np.float32)
    for variant in ("none", "overlap"):
        pos, excl = _lists(m, variant)
        (po, pi), (eo, ei) = RM.csr([pos[k] for k in ids]), RM.csr([excl[k] for k in ids])
        want = IM.rows(S, po, pi, None if variant == "none" else eo, ei, row_ids=ids, coef=coef)
        P, E = _dev_lists(m, variant, dev, sel=ids)
        res = implicit.implicit_rows(X, P, E, rows=ids, grad=True, coef=torch.from_numpy(coef).to(dev))
        _compare(res, want, f"rows+coef {variant}", coef=coef)
        # a RatingsData is indexed by user: its rows are gathered
        if variant == "none":
            from mfcd.ratings import RatingsData
            u = np.concatenate([np.full(len(p), k) for k, p in enumerate(pos)])
            data = RatingsData(u, np.concatenate(pos), np.ones(u.size), n, m).to(dev)
            again = implicit.implicit_rows(X, data, rows=ids, grad=True, coef=torch.from_numpy(coef).to(dev))
            assert _same(again, res)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def _same(a, b, rows_a=None, rows_b=None):
    """Bit equality of two results (NaN included) on the given row positions."""
    for x, y in zip(a, b):
        if x is None or y is None:
            if x is not y:
                return False
            continue
        x = x if rows_a is None else x[rows_a]
        y = y if rows_b is None else y[rows_b]
        if not torch.equal(_bits(x), _bits(y)):
            return False
    return True


def test_identity_with_the_ranking_entry(dev):
    """Random fp32 factors, which are not exact: `inverted` is the sum of (rank - pos) of mfcd_rank_entries on the same
    targets and barred lists, exactly, and the AUC is `ranking_metrics`' to 1e-12 with NaN in the same places."""
    from mfcd import implicit, ranking
    from mfcd.ratings import RatingsData
    C, _ = _CT()
    for m, d in ((65, 3), (C + 1, 17)):
        rng = np.random.default_rng(m)
        pos, excl = _lists(m, "overlap")
        n = len(pos)
        A = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(dev)
        P, E = _dev_lists(m, "overlap", dev)
        res = implicit.implicit_rows((A, B), P, E)
        ranks = ranking.rank_entries((A, B), P, E)
        rk, off = ranks.rank.cpu().numpy().astype(np.int64), P[0].cpu().numpy()
        inverted = res.counts[:, 2].cpu().numpy()
        for u in range(n):
            r = np.sort(rk[off[u]:off[u + 1]])
            r = r[r >= 0]
            assert inverted[u] == int((r - np.arange(r.size)).sum()), (m, u)
        users = lambda ls: np.concatenate([np.full(len(x), k) for k, x in enumerate(ls)])    # noqa: E731
        test = RatingsData(users(pos), np.concatenate(pos), np.ones(sum(map(len, pos))), n, m).to(dev)
        train = RatingsData(users(excl), np.concatenate(excl), np.ones(sum(map(len, excl))), n, m).to(dev)
        want = ranking.ranking_metrics((A, B), test, train)["auc_per_user"]
        got = implicit.implicit_metrics(A, B, test, train)
        assert np.array_equal(np.isnan(got["auc_per_user"]), np.isnan(want)) and np.isnan(want).any()
        np.testing.assert_allclose(got["auc_per_user"], want, rtol=0, atol=1e-12, equal_nan=True)
        assert np.all(got["auc_midrank_per_user"][~np.isnan(want)] >= got["auc_per_user"][~np.isnan(want)] - 1e-15)


def test_metrics_with_ties_give_half_credit(dev):
    from mfcd import implicit
    m = 65
    rng = np.random.default_rng(9)
    S = rng.integers(-1, 2, (len(_Ls(m)) + 1, m)).astype(np.float32)
    pos, excl = _lists(m, "overlap")
    P, E = _dev_lists(m, "overlap", dev)
    got = implicit.implicit_metrics(torch.from_numpy(S).to(dev), None, P, E)
    for u in range(S.shape[0]):
        Pu, Nu = IM.classes(m, pos[u], excl[u])
        if Pu.size * Nu.size == 0:
            assert np.isnan(got["auc_midrank_per_user"][u]) and np.isnan(got["auc_per_user"][u])
            continue
        a = S[u].astype(np.float64)
        v = a[Nu][None, :] - a[Pu][:, None]
        want = 1.0 - ((v > 0).sum() + 0.5 * (v == 0).sum()) / v.size
        assert abs(got["auc_midrank_per_user"][u] - want) < 1e-12, u
        assert got["tied_per_user"][u] == (v == 0).sum()
        assert abs(got["log_likelihood_per_user"][u] + IM.softplus(v).sum() / v.size) < 1e-5


def test_calls_are_bit_equal_and_rows_do_not_depend_on_their_neighbours(dev):
    from mfcd import implicit
    C, _ = _CT()
    m = 2 * C + 3
    rng = np.random.default_rng(8)
    d, pos_excl = 5, _lists(m, "overlap")
    n = len(pos_excl[0])
    A = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(dev)
    X = (A @ B.t()).contiguous()
    for M in ((A, B), X):
        P, E = _dev_lists(m, "overlap", dev)
        one = implicit.implicit_rows(M, P, E, grad=True)
        two = implicit.implicit_rows(M, P, E, grad=True)
        assert _same(one, two)
        perm = rng.permutation(n)
        Pp, Ep = _dev_lists(m, "overlap", dev, sel=perm)
        moved = implicit.implicit_rows(M, Pp, Ep, rows=perm, grad=True)
        assert _same(moved, one, None, torch.from_numpy(perm).to(dev))
        keep = np.array([n - 2, 3])
        Pk, Ek = _dev_lists(m, "overlap", dev, sel=keep)
        alone = implicit.implicit_rows(M, Pk, Ek, rows=keep, grad=True)
        assert _same(alone, one, None, torch.from_numpy(keep).to(dev))
        # next to an invalid row (an item >= m is refused before anything is gathered)
        bad_items = torch.cat((Pk[1], torch.tensor([m], dtype=torch.int32, device=dev)))
        bad_off = torch.cat((Pk[0], Pk[0][-1:] + 1))
        bad_E = (torch.cat((Ek[0], Ek[0][-1:])), Ek[1])
        mixed = implicit.implicit_rows(M, (bad_off, bad_items), bad_E, rows=np.append(keep, 0), grad=True)
        assert mixed.status.tolist() == [0, 0, 2]
        assert _same(ImplicitPart(mixed, slice(0, 2)), alone)


def ImplicitPart(res, sl):
    return tuple(None if t is None else t[sl] for t in res)


def test_invalid_rows_get_status_2_and_nothing_else_changes(dev):
    from mfcd import implicit
    m, n = 70, 6
    rng = np.random.default_rng(12)
    X = torch.from_numpy(rng.uniform(-3, 3, (n, m)).astype(np.float32)).to(dev)
    good = [np.sort(rng.choice(m, 7, replace=False)) for _ in range(8)]
    barred = [np.sort(rng.choice(m, 5, replace=False)) for _ in range(8)]
    pos = [g.copy() for g in good]
    exc = [b.copy() for b in barred]
    pos[1][3] = m                                       # an item >= m
    pos[2][[2, 3]] = pos[2][[3, 2]]                     # not ascending
    exc[4][[0, 1]] = exc[4][[1, 0]]                     # a barred list that is not ascending
    exc[5][4] = -1                                      # a negative barred item
    pos[6][1] = pos[6][0]                               # a repeat: not strictly ascending
    ids = np.array([0, 1, 2, n + 3, 4, 5, 1, -1])       # rows 3 and 7: a row id outside [0, n)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(exc)
    dv = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    res = implicit.implicit_rows(X, (dv(po), dv(pi)), (dv(eo), dv(ei)), rows=ids, grad=True)
    assert res.status.tolist() == [0, 2, 2, 2, 2, 2, 2, 2]
    assert (res.counts[1:] == -1).all() and torch.isnan(res.sums[1:]).all() and torch.isnan(res.g[1:]).all()
    alone = implicit.implicit_rows(X, (dv(po[:2]), dv(pi[:7])), (dv(eo[:2]), dv(ei[:5])), rows=ids[:1], grad=True)
    assert _same(ImplicitPart(res, slice(0, 1)), alone) and not torch.isnan(res.g[0]).any()
    # offsets: a row that ends before it starts, and one that ends beyond the entries; the rows around them are valid
    po2 = po.copy()
    po2[1:] = [7, 14, 10, 14, 21, 28, 35, 99]           # row 2: [14, 10); row 7: [35, 99) of 56 entries; row 3: a tail
    ok_ids = np.array([0, 1, 2, 3, 4, 5, 0, 1])
    pos_ok = np.concatenate(good)
    res2 = implicit.implicit_rows(X, (dv(po2), dv(pos_ok.astype(np.int32))), None, rows=ok_ids, grad=True)
    assert res2.status.tolist() == [0, 0, 2, 0, 0, 0, 0, 2]
    assert (res2.counts[[2, 7]] == -1).all() and torch.isnan(res2.sums[[2, 7]]).all() and torch.isnan(res2.g[[2, 7]]).all()
    for r in (0, 1, 3, 4, 5, 6):
        b, e = po2[r], po2[r + 1]
        c, s, g = IM.row(X[ok_ids[r]].cpu().numpy(), pos_ok[b:e])
        assert res2.counts[r].tolist() == c.tolist()
        np.testing.assert_allclose(float(res2.sums[r]) / (c[0] * c[1]), s / (c[0] * c[1]), rtol=RTOL, atol=ATOL)
    prep = implicit.implicit_rows(X, (dv(po), dv(pi)), (dv(eo), dv(ei)), rows=ids, prepare_only=True)
    assert prep.status.tolist() == res.status.tolist() and torch.equal(prep.counts[:, :2], res.counts[:, :2])


def test_non_finite_scores_follow_the_pair_gradients_rule(dev):
    from mfcd import implicit
    m, n = 2 * _CT()[0] + 3, 5
    rng = np.random.default_rng(13)
    S = rng.uniform(-3, 3, (n, m)).astype(np.float32)
    pos = [np.sort(rng.choice(m, 40, replace=False)) for _ in range(n)]
    exc = [np.sort(rng.choice(m, 30, replace=False)) for _ in range(n)]
    free = [np.setdiff1d(np.arange(m), np.union1d(p, e)) for p, e in zip(pos, exc)]
    S[0, free[0][-1]] = np.nan                          # at a negative of the last chunk
    S[1, np.setdiff1d(pos[1], exc[1])[0]] = np.inf      # at a positive
    S[2, free[2][5]] = -np.inf
    S[3, exc[3]] = np.nan                               # only at barred columns: an ordinary row
    S[3, exc[3][::2]] = np.inf
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(exc)
    dv = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    res = implicit.implicit_rows(dv(S), (dv(po), dv(pi)), (dv(eo), dv(ei)), grad=True)
    wc, ws, wg = IM.rows(S, po, pi, eo, ei)
    assert res.status.tolist() == [0] * n
    assert np.array_equal(res.counts.cpu().numpy(), wc)             # the key order: NaN above +inf
    assert torch.isnan(res.sums[:3]).all() and torch.isnan(res.g[:3]).all() and np.isnan(ws[:3]).all()
    assert not torch.isnan(res.sums[3:]).any() and not torch.isnan(res.g[3:]).any()
    ordinary = ImplicitPart(res, slice(3, 5))
    _compare(implicit.ImplicitRows(*ordinary), (wc[3:], ws[3:], wg[3:]), "NaN at barred columns only")


def _table(m, n, rng, dev):
    """A small table of observed items with an empty user, a full user and a barred list that overlaps."""
    from mfcd.ratings import RatingsData
    pos = [np.sort(rng.choice(m, int(rng.integers(1, m // 2)), replace=False)) for _ in range(n)]
    pos[1], pos[2] = np.zeros(0, dtype=np.int64), np.arange(m)
    exc = [np.sort(rng.choice(m, int(rng.integers(0, m // 4)), replace=False)) for _ in range(n)]
    users = lambda ls: np.concatenate([np.full(len(x), k) for k, x in enumerate(ls)])    # noqa: E731
    data = RatingsData(users(pos), np.concatenate(pos), np.ones(sum(map(len, pos))), n, m).to(dev)
    excl = RatingsData(users(exc), np.concatenate(exc), np.ones(sum(map(len, exc))), n, m).to(dev)
    return RM.csr(pos), RM.csr(exc), data, excl


@pytest.mark.parametrize("normalize", ["pairs", "user"])
def test_table_gradients_are_the_gemms_of_the_devices_g(dev, normalize):
    """`implicit_risk(...).backward()` over three row blocks: U.grad and V.grad against the f64 GEMMs of the device's own g
    (pinned by the tests above) within the worst-case fp32 dot-product bound, the value against the model's."""
    from mfcd import implicit
    m, n, d, rb = 130, 12, 7, 5
    rng = np.random.default_rng(21)
    (po, pi), (eo, ei), data, excl = _table(m, n, rng, dev)
    U = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32) * 0.6).to(dev).requires_grad_()
    V = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(dev).requires_grad_()
    risk = implicit.implicit_risk(U, V, data, excl, normalize, row_block=rb)
    assert risk.dim() == 0 and risk.dtype == torch.float32 and risk.requires_grad
    risk.backward()
    plan = implicit._Plan(n, m, dev, data, excl, normalize, rb)
    res = implicit.implicit_rows((U.detach(), V.detach()), data, excl, grad=True, coef=plan.coef)
    g, Ud, Vd = res.g.double(), U.detach().double(), V.detach().double()
    eps = 2.0 ** -24
    errU = (U.grad.double() - g @ Vd).abs()
    errV = (V.grad.double() - g.t() @ Ud).abs()
    boundU, boundV = (m + d) * eps * (g.abs() @ Vd.abs()), (n + d) * eps * (g.abs().t() @ Ud.abs())
    print(f"{normalize}: worst error / bound of U.grad {float((errU / boundU.clamp(min=1e-300)).max()):.3f}, "
          f"of V.grad {float((errV / boundV.clamp(min=1e-300)).max()):.3f}")
    assert bool((errU <= boundU).all()) and bool((errV <= boundV).all())
    assert bool((U.grad[1] == 0).all()) and bool((U.grad[2] == 0).all())          # users without a pair
    S = _device_scores(U.detach(), V.detach(), np.arange(n), m, dev)
    wc, ws, _ = IM.rows(S, po, pi, eo, ei)
    want = float((ws * IM.coefficients(wc, normalize)).sum())
    print(f"{normalize}: risk {float(risk.detach()):.8f}, model {want:.8f}")
    np.testing.assert_allclose(float(risk.detach()), want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(plan.coef64.cpu().numpy(), IM.coefficients(wc, normalize), rtol=1e-15, atol=0)
    # one block or three: the same value bit for bit (a row's sum does not depend on its block)
    with torch.no_grad():
        assert torch.equal(implicit.implicit_risk(U, V, data, excl, normalize), risk)
        assert torch.equal(implicit.implicit_risk(U, V, data, excl, normalize, row_block=rb), risk)
    # a table without a pair
    from mfcd.ratings import RatingsData
    full = RatingsData(np.repeat(np.arange(n), m), np.tile(np.arange(m), n), np.ones(n * m), n, m).to(dev)
    with pytest.raises(ValueError):
        implicit.implicit_risk(U, V, full, None, normalize)


def _model(S, n, m, d, seed, dev):
    torch.manual_seed(seed)
    return S.MatrixFactorization(n, m, d).to(dev)


def _twin(S, model, dev):
    twin = S.MatrixFactorization(model.U.shape[0], model.V.shape[0], model.U.shape[1]).to(dev)
    with torch.no_grad():
        twin.U.copy_(model.U)
        twin.V.copy_(model.V)
    return twin


@pytest.mark.parametrize("normalize", ["pairs", "user"])
def test_fit_implicit_is_backward_plus_adam_and_logs_the_models_risks(dev, normalize):
    import structure as S
    from mfcd import _lib, implicit
    n, m, d, lr, rb = 9, 65, 3, 0.05, 4
    rng = np.random.default_rng(33)
    (po, pi), (eo, ei), data, excl = _table(m, n, rng, dev)
    model = _model(S, n, m, d, 5, dev)
    twin = _twin(S, model, dev)
    U0, V0 = model.U.detach().cpu().numpy().astype(np.float64), model.V.detach().cpu().numpy().astype(np.float64)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    steps, risks = implicit.fit_implicit((model, opt), data, 3, log_every=1, exclude=excl, normalize=normalize, row_block=rb)
    assert steps == [0, 1, 2, 3] and all(isinstance(r, float) for r in risks)
    assert float(opt.state[model.U]["step"]) == 3 == float(opt.state[model.V]["step"])
    topt = torch.optim.Adam(twin.parameters(), lr=lr)
    seen = []
    for _ in range(3):
        topt.zero_grad()
        risk = implicit.implicit_risk(twin.U, twin.V, data, excl, normalize, row_block=rb)
        seen.append(float(risk.detach()))
        risk.backward()
        topt.step()
    with torch.no_grad():
        seen.append(float(implicit.implicit_risk(twin.U, twin.V, data, excl, normalize, row_block=rb)))
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(model.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(risks, seen, rtol=1e-5, atol=0)
    _, _, want = IM.adam_fit(U0, V0, po, pi, 3, lr, eo, ei, normalize)
    print(f"{normalize}: logged risks {risks}, f64 model {want}")
    np.testing.assert_allclose(risks, want, rtol=RTOL, atol=ATOL)
    # the optimizer's state stays valid: one more torch step on both moves them alike
    for mdl, o in ((model, opt), (twin, topt)):
        o.zero_grad()
        implicit.implicit_risk(mdl.U, mdl.V, data, excl, normalize, row_block=rb).backward()
        o.step()
    assert float(opt.state[model.U]["step"]) == 4
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    # the structure-level entry: Adam takes the fused loop, any other optimiser the backward loop
    a, b = _twin(S, twin, dev), _twin(S, twin, dev)
    oa = torch.optim.Adam(a.parameters(), lr=lr)
    ob = torch.optim.Adam(b.parameters(), lr=lr)
    sa, ra = S.train_model_implicit(a, data, oa, dev, num_steps=2, log_every=1, exclude=excl, normalize=normalize)
    sb, rb_ = implicit.fit_implicit((b, ob), data, 2, 1, excl, normalize)
    assert sa == sb == [0, 1, 2] and ra == rb_ and torch.equal(a.U, b.U) and not a.training
    sgd_model, sgd_twin = _twin(S, twin, dev), _twin(S, twin, dev)
    sgd = torch.optim.SGD(sgd_model.parameters(), lr=0.1)
    steps, risks = S.train_model_implicit(sgd_model, data, sgd, dev, num_steps=2, log_every=1, exclude=excl, normalize=normalize)
    for _ in range(2):
        sgd_twin.zero_grad()
        S.implicit_risk(sgd_twin, data, excl, normalize).backward()
        with torch.no_grad():
            sgd_twin.U -= 0.1 * sgd_twin.U.grad
            sgd_twin.V -= 0.1 * sgd_twin.V.grad
    assert steps == [0, 1, 2] and len(risks) == 3
    np.testing.assert_allclose(sgd_model.U.detach().cpu().numpy(), sgd_twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    bf = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        implicit.fit_implicit((bf, torch.optim.Adam(bf.parameters(), lr=lr)), data, 2)
    with pytest.raises(_lib.MfcdError):
        S.implicit_risk(bf, data)


def test_min_value_and_the_structure_metrics(dev):
    import structure as S
    from mfcd import implicit
    from mfcd.ratings import RatingsData
    n, m, d = 8, 40, 3
    rng = np.random.default_rng(4)
    keep = rng.random((n, m)) < 0.4
    u, i = np.nonzero(keep)
    v = rng.integers(1, 6, u.size).astype(np.float32)
    data = RatingsData(u, i, v, n, m).to(dev)
    model = _model(S, n, m, d, 6, dev)
    liked = RatingsData(u[v >= 4], i[v >= 4], v[v >= 4], n, m).to(dev)
    got = S.compute_implicit_metrics(model, data, min_value=4.0)
    want = implicit.implicit_metrics(model.U.data, model.V.data, liked)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k
    with torch.no_grad():
        assert torch.equal(S.implicit_risk(model, data, min_value=4.0), implicit.implicit_risk(model.U, model.V, liked))
    with torch.no_grad():
        per_user = float(S.implicit_risk(model, data, normalize="user", min_value=4.0))
    np.testing.assert_allclose(got["log_likelihood"], -per_user, rtol=1e-6)


def test_end_to_end_training_on_implicit_feedback_improves_the_held_out_auc(dev):
    """Rank-2 truth, 60 x 60; the observed items are every user's top 30 %, each kept with probability 0.7; split 80 / 20;
    300 fused steps of Adam at lr 0.05.  Relative comparisons only (on the CPU in f64 the held-out AUC went from about 0.5
    to about 0.93)."""
    import structure as S
    from mfcd.ratings import RatingsData
    n = m = 60
    g = torch.Generator().manual_seed(11)
    X = (torch.randn(n, 2, generator=g) @ torch.randn(m, 2, generator=g).t()).numpy()
    top = X >= np.quantile(X, 0.7, axis=1, keepdims=True)
    keep = top & (np.random.default_rng(0).random((n, m)) < 0.7)
    u, i = np.nonzero(keep)
    data = RatingsData(u, i, np.ones(u.size), n, m).to(dev)
    train, test = data.split((0.8, 0.2), seed=0)
    model = _model(S, n, m, 2, 1011, dev)
    before = S.compute_ranking_metrics(model, test, train)
    own_before = S.compute_implicit_metrics(model, test, train)
    with torch.no_grad():
        risk_before = float(S.implicit_risk(model, train))
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    steps, risks = S.train_model_implicit(model, train, opt, dev, num_steps=300, log_every=100)
    after = S.compute_ranking_metrics(model, test, train)
    own_after = S.compute_implicit_metrics(model, test, train)
    print(f"training risk {risk_before:.5f} -> {risks[-1]:.5f}; held-out auc {before['auc']:.4f} -> {after['auc']:.4f} "
          f"(implicit_metrics {own_before['auc']:.4f} -> {own_after['auc']:.4f})")
    assert steps == [0, 100, 200, 300]
    np.testing.assert_allclose(risks[0], risk_before, rtol=RTOL, atol=ATOL)
    assert risks[-1] < risks[0]
    assert after["auc"] > before["auc"]
    assert abs(own_after["auc"] - after["auc"]) < 1e-12 and abs(own_before["auc"] - before["auc"]) < 1e-12
