"""GPU tests of the ragged pair kernels, the two table kernels and the ratings fit built on them (include/mfcd.h:
mfcd_pair_ragged_stats, mfcd_pair_ragged_grad, mfcd_ragged_dot, mfcd_ragged_gather_sum; mfcd/ratings.py;
structure.observe_ratings, ratings_risk, train_model_ratings, compute_ratings_metrics) against the float64 model of
tests/ratings_model.py.

Shapes: with T = mfcd_pair_ragged_tile() entries per workgroup tile, one call holds rows of lengths
{0, 1, 2, 63, 64, 65, T-1, T, T+1, 2T+3, 4T+1} in a shuffled order, for each of nine kinds of value rows: the eight of
test_pair_grad.py's `case_rows` (no ties, heavy ties in a / in x / in both, a constant row, +-0, denormals, the spread
{-60, 0, 60} at scale 1 only) and integer ratings 1..5.  They reach the empty row, a single pair, the wave boundary, a
partly filled and an exactly full tile, a second tile of one entry and several J tiles with a short last one.

Tolerances: the per-pair arithmetic is pairs_common.h's, the functions the dense kernels run, and an accumulator still adds
at most 64 fp32 terms before it is widened, so the roundings counted in test_pair_grad.py's docstring carry over: rtol
2e-5, atol 2e-6 on the mean term (sums / support, g_e / (L - 1)).  The references are computed once per module."""
import copy
import functools

import numpy as np
import pytest
import torch

import ratings_model as RM
from test_pair_grad import case_rows

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.25, 4.0)
RTOL, ATOL = 2e-5, 2e-6
KINDS = 9                     # case_rows' eight and the ratings row
SPREAD = 7                    # case_rows' last row: scale 1 only


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tile():
    from mfcd import _lib
    return _lib.load().mfcd_pair_ragged_tile()


def _lengths():
    T = _tile()
    return [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 4 * T + 1]


def _kind_row(kind, L):
    if L == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    if kind < 8:
        A, X = case_rows(L)
        return A[kind], X[kind]
    rng = np.random.default_rng(9000 + L)
    return (rng.permutation(L).astype(np.float64) / L * 6.0 - 3.0).astype(np.float32), rng.integers(1, 6, L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(scale):
    """The (a, x) rows of one call in a shuffled order → (list of (kind, L, a, x))."""
    rows = [(k, L) + _kind_row(k, L) for k in range(KINDS) if scale == 1.0 or k != SPREAD for L in _lengths()]
    order = np.random.default_rng(77).permutation(len(rows))
    return [rows[i] for i in order]


def build(rows, dev):
    """RatingsData and the score tensor of a list of (a, x) rows: row r rates items 0..L_r - 1."""
    from mfcd import ratings
    lens = np.array([len(a) for a, _ in rows], dtype=np.int64)
    users = np.repeat(np.arange(len(rows)), lens)
    items = np.concatenate([np.arange(L) for L in lens]) if len(rows) else np.zeros(0, np.int64)
    a = np.concatenate([a for a, _ in rows]).astype(np.float32)
    x = np.concatenate([x for _, x in rows]).astype(np.float32)
    data = ratings.RatingsData(users, items, x, len(rows), max(int(lens.max()), 1)).to(dev)
    assert data.value.cpu().numpy().tobytes() == x.tobytes()
    return data, torch.from_numpy(a).to(dev), a, x


@functools.lru_cache(maxsize=None)
def reference(scale, skip):
    rows = case(scale)
    a = np.concatenate([r[2] for r in rows])
    x = np.concatenate([r[3] for r in rows])
    row_off = np.concatenate(([0], np.cumsum([len(r[2]) for r in rows])))
    counts, sums, support = RM.stats(a, x, row_off, scale, skip)
    return row_off, counts, sums, support, RM.grad(a, x, row_off, scale, skip)


def run_stats(a, data, scale=1.0, what="both", skip=False):
    from mfcd import ratings
    counts, sums, status = ratings.pair_ragged_stats(a, data, scale, what, skip)
    return (None if counts is None else counts.cpu().numpy(), None if sums is None else sums.cpu().numpy(),
            status.cpu().numpy())


def run_grad(a, data, scale=1.0, skip=False):
    from mfcd import ratings
    g, status = ratings.pair_ragged_grad(a, data, scale, skip)
    assert g.dtype == torch.float32 and g.shape == a.shape
    return g.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("scale", SCALES)
def test_counts_sums_and_gradient_match_the_f64_model(dev, scale, skip):
    rows = case(scale)
    data, a_dev, _, _ = build([(r[2], r[3]) for r in rows], dev)
    row_off, ref_counts, ref_sums, support, ref_g = reference(scale, skip)
    counts, sums, status = run_stats(a_dev, data, scale, "both", skip)
    assert (status == 0).all()
    assert counts.dtype == np.int64 and (counts == ref_counts).all()                 # as integers
    assert np.isfinite(sums).all()
    live = support > 0
    assert (sums[~live] == 0.0).all() and not np.signbit(sums[~live]).any()          # no pair: +0
    mean, want = sums[live] / support[live, None], ref_sums[live] / support[live, None]
    err = np.abs(mean - want)
    print(f"scale {scale} skip {skip}: sums max error / bound {(err / (ATOL + RTOL * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(mean, want, rtol=RTOL, atol=ATOL)
    g, gstatus = run_grad(a_dev, data, scale, skip)
    assert (gstatus == 0).all() and np.isfinite(g).all()
    for r, sl in enumerate(RM.rows_of(row_off)):
        L = sl.stop - sl.start
        if L == 1:
            assert g[sl].tobytes() == np.zeros(1, np.float32).tobytes()               # exactly +0
        elif L > 1:
            got, ref = g[sl].astype(np.float64) / (L - 1), ref_g[sl] / (L - 1)
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"row {r}: kind {rows[r][0]}, L = {L}")


def test_counts_equal_the_dense_kernel_on_every_length(dev):
    """Each length run as its own dense call (no padding at all): the same integers."""
    from mfcd import pairs
    rows = case(1.0)
    data, a_dev, _, _ = build([(r[2], r[3]) for r in rows], dev)
    counts, _, _ = run_stats(a_dev, data, 1.0, "counts")
    for L in _lengths():
        if L == 0:
            assert all((counts[r] == 0).all() for r, row in enumerate(rows) if row[1] == 0)
            continue
        ids = [r for r, row in enumerate(rows) if row[1] == L]
        A = torch.from_numpy(np.stack([rows[r][2] for r in ids])).to(dev)
        X = torch.from_numpy(np.stack([rows[r][3] for r in ids])).to(dev)
        dense = pairs.pair_stats_rows(A, X, 1.0, "counts")[0].cpu().numpy()
        assert (counts[ids] == dense).all(), L


def test_rows_are_independent_of_their_place_and_calls_are_bit_equal(dev):
    rows = [(r[2], r[3]) for r in case(4.0)]
    data, a_dev, _, _ = build(rows, dev)
    row_off = data.row_off.cpu().numpy()
    for skip in (False, True):
        counts, sums, _ = run_stats(a_dev, data, 4.0, "both", skip)
        g, _ = run_grad(a_dev, data, 4.0, skip)
        c2, s2, _ = run_stats(a_dev, data, 4.0, "both", skip)
        assert counts.tobytes() == c2.tobytes() and sums.tobytes() == s2.tobytes()
        assert run_grad(a_dev, data, 4.0, skip)[0].tobytes() == g.tobytes()
        c1, none, _ = run_stats(a_dev, data, 4.0, "counts", skip)
        assert none is None and c1.tobytes() == counts.tobytes()
        none, s1, _ = run_stats(a_dev, data, 4.0, "sums", skip)
        assert none is None and s1.tobytes() == sums.tobytes()
        perm = np.random.default_rng(3).permutation(len(rows))
        pdata, pa, _, _ = build([rows[i] for i in perm], dev)
        pc, ps, _ = run_stats(pa, pdata, 4.0, "both", skip)
        pg, _ = run_grad(pa, pdata, 4.0, skip)
        poff = pdata.row_off.cpu().numpy()
        for k, i in enumerate(perm):
            assert pc[k].tobytes() == counts[i].tobytes() and ps[k].tobytes() == sums[i].tobytes(), (k, i)
            assert pg[poff[k]:poff[k + 1]].tobytes() == g[row_off[i]:row_off[i + 1]].tobytes(), (k, i)


def _plain_rows(lens, seed):
    rng = np.random.default_rng(seed)
    return [((rng.permutation(L).astype(np.float64) / max(L, 1) * 6.0 - 3.0).astype(np.float32),
             rng.integers(1, 6, L).astype(np.float32)) for L in lens]


def test_a_non_finite_row_follows_the_rules_and_its_neighbours_are_untouched(dev):
    T = _tile()
    rows = _plain_rows([T + 37, 40, T + 37, 2 * T + 5, 70, 3], 5)
    data, a_dev, a, x = build(rows, dev)
    off = data.row_off.cpu().numpy()
    c0, s0, _ = run_stats(a_dev, data)
    g0, _ = run_grad(a_dev, data)
    a, x = a.copy(), x.copy()
    a[off[0] + 3] = np.inf                     # first tile: the second tile's workgroup must see it
    a[off[2] + T + 30] = np.nan                # second tile: the first tile's workgroup must see it
    x[off[3] + 2 * T + 4] = -np.inf            # the last entry of a row
    x[off[4] + 1] = np.nan
    bad = build([(a[s], x[s]) for s in RM.rows_of(off)], dev)
    c, s, status = run_stats(bad[1], bad[0])
    g, gstatus = run_grad(bad[1], bad[0])
    assert (status == 0).all() and (gstatus == 0).all()
    assert np.isnan(s[[0, 2, 3, 4]]).all() and (c[[2, 4]] == -1).all() and (c[[0, 3]] >= 0).all()
    ref = RM.stats(a.astype(np.float64), x.astype(np.float64), off, 1.0)[0]
    assert (c == ref).all()
    for r in (0, 2, 3, 4):
        assert np.isnan(g[off[r]:off[r + 1]]).all()
    for r in (1, 5):
        assert c[r].tobytes() == c0[r].tobytes() and s[r].tobytes() == s0[r].tobytes()
        assert g[off[r]:off[r + 1]].tobytes() == g0[off[r]:off[r + 1]].tobytes()


def test_invalid_rows_get_status_2_and_nothing_else_changes(dev):
    """Offsets that decrease or run past `entries`, and an index out of range: the bad values are only compared, so
    nothing outside the buffers is read; the row is marked and the other rows keep their bytes."""
    from mfcd import _lib, ratings
    rows = _plain_rows([300, 10, 20, 5], 8)
    data, a_dev, _, _ = build(rows, dev)
    off = data.row_off.cpu().numpy()                      # 0, 300, 310, 330, 335
    c0, s0, st0 = run_stats(a_dev, data)
    g0, _ = run_grad(a_dev, data)
    assert (st0 == 0).all()
    for name, edit, bad_rows in (("decreasing", {2: 290}, [1]), ("past entries", {4: 336}, [3]),
                                 ("negative", {0: -1}, [0]), ("tile count", {2: 600}, [1, 2])):
        broken = copy.copy(data)
        ro = off.copy()
        for k, v in edit.items():
            ro[k] = v
        broken.row_off = torch.from_numpy(ro).to(dev)
        c, s, status = run_stats(a_dev, broken)
        g = torch.full_like(a_dev, -123.0)
        gstatus = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().mfcd_pair_ragged_grad(a_dev.data_ptr(), data.value.data_ptr(), data.entries,
                                                     broken.row_off.data_ptr(), 4, data.tile_off.data_ptr(), data.n_tiles,
                                                     1.0, 0, g.data_ptr(), gstatus.data_ptr(), _lib.stream_ptr(dev)))
        g, gstatus = g.cpu().numpy(), gstatus.cpu().numpy()
        want = [2 if r in bad_rows else 0 for r in range(4)]
        assert status.tolist() == want and gstatus.tolist() == want, name
        written = np.zeros(data.entries, dtype=bool)
        for r in range(4):
            if r in bad_rows:
                assert (c[r] == -1).all() and np.isnan(s[r]).all(), (name, r)
            else:
                written[ro[r]:ro[r + 1]] = True
                if ro[r] == off[r] and ro[r + 1] == off[r + 1]:
                    assert c[r].tobytes() == c0[r].tobytes() and s[r].tobytes() == s0[r].tobytes(), (name, r)
                    assert g[off[r]:off[r + 1]].tobytes() == g0[off[r]:off[r + 1]].tobytes(), (name, r)
        assert (g[~written] == -123.0).all(), name                           # no entry of a bad row is written
    # an index out of range: the dot and both gather-sums
    U = torch.randn(4, 3, device=dev)
    V = torch.randn(data.m, 3, device=dev)
    base, st = ratings.ragged_scores(U, V, data)
    assert (st == 0).all()
    coef = torch.randn(data.entries, device=dev)
    out0, _ = ratings.ragged_gather_sum(coef, data, V, "user")
    col0, _ = ratings.ragged_gather_sum(coef, data, U, "item")
    for value in (data.m, -1, 2 ** 31 - 1):
        broken = copy.copy(data)
        broken.item = data.item.clone()
        broken.item[off[2] + 7] = value
        got, st = ratings.ragged_scores(U, V, broken)
        assert st.tolist() == [0, 0, 2, 0] and torch.isnan(got[off[2]:off[3]]).all()
        keep = np.r_[0:off[2], off[3]:off[4]]
        assert got.cpu().numpy()[keep].tobytes() == base.cpu().numpy()[keep].tobytes()
        out, st = ratings.ragged_gather_sum(coef, broken, V, "user")
        assert st.tolist() == [0, 0, 2, 0] and torch.isnan(out[2]).all()
        assert out[[0, 1, 3]].cpu().numpy().tobytes() == out0[[0, 1, 3]].cpu().numpy().tobytes()
    broken = copy.copy(data)
    broken.col_perm = data.col_perm.clone()
    col_off = data.col_off.cpu().numpy()
    broken.col_perm[col_off[5] + 1] = data.entries                        # item 5 is rated by rows 0, 1, 2
    out, st = ratings.ragged_gather_sum(coef, broken, U, "item")
    st = st.cpu().numpy()
    assert st[5] == 2 and (np.delete(st, 5) == 0).all() and torch.isnan(out[5]).all()
    rest = np.delete(np.arange(data.m), 5)
    assert out.cpu().numpy()[rest].tobytes() == col0.cpu().numpy()[rest].tobytes()
    broken.col_user = data.col_user.clone()
    broken.col_user[col_off[7]] = 4                                         # a user past U's rows
    out, st = ratings.ragged_gather_sum(coef, broken, U, "item")
    assert st.cpu().numpy()[[5, 7]].tolist() == [2, 2] and torch.isnan(out[[5, 7]]).all()


@functools.lru_cache(maxsize=None)
def gather_problem():
    """n = 900 users, m = 12 items; item 0 is rated by every user (a row of the item side longer than three segments),
    the rest with probability 0.3."""
    rng = np.random.default_rng(21)
    keep = rng.random((900, 12)) < 0.3
    keep[:, 0] = True
    users, items = np.nonzero(keep)
    return users, items, rng.normal(size=users.size).astype(np.float32)


@pytest.mark.parametrize("d", [1, 2, 3, 64, 65, 256])
def test_ragged_dot_matches_the_model(dev, d):
    from mfcd import ratings
    users, items, values = gather_problem()
    data = ratings.RatingsData(users, items, values, 900, 12).to(dev)
    g = torch.Generator().manual_seed(d)
    U, V = torch.randn(900, d, generator=g), torch.randn(12, d, generator=g)
    a, status = ratings.ragged_scores(U.to(dev), V.to(dev), data)
    assert (status == 0).all() and a.dtype == torch.float32
    ref, mag = RM.dot(U.numpy(), V.numpy(), data.row_off.cpu().numpy(), data.item.cpu().numpy().astype(np.int64))
    err = np.abs(a.cpu().numpy().astype(np.float64) - ref)
    bound = d * 2.0 ** -23 * mag
    print(f"d = {d}: max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    again, _ = ratings.ragged_scores(U.to(dev), V.to(dev), data)
    assert again.cpu().numpy().tobytes() == a.cpu().numpy().tobytes()


@pytest.mark.parametrize("d", [1, 2, 64, 65, 256])
def test_ragged_gather_sum_matches_the_model_on_both_sides(dev, d):
    """Bound 2^-24 |ref| + L 2^-52 sum |terms|: the products are exact in f64, the order is fixed, one rounding to fp32."""
    from mfcd import _lib, ratings
    users, items, values = gather_problem()
    seg = _lib.load().mfcd_ragged_segment()
    g = torch.Generator().manual_seed(100 + d)
    coef = torch.randn(users.size, generator=g)
    for n, m, us, it in ((900, 12, users, items), (12, 900, items, users)):      # and transposed: a long user row
        data = ratings.RatingsData(us, it, values, n, m).to(dev)
        assert max(np.diff(data.col_off.cpu().numpy()).max(), data.lengths.max()) > 3 * seg
        U, V = torch.randn(n, d, generator=g), torch.randn(m, d, generator=g)
        h = {k: getattr(data, k).cpu().numpy() for k in ("row_off", "item", "col_off", "col_user", "col_perm")}
        for side, table, ro, idx, perm in (("user", V, h["row_off"], h["item"], None),
                                           ("item", U, h["col_off"], h["col_user"], h["col_perm"])):
            out, status = ratings.ragged_gather_sum(coef.to(dev), data, table.to(dev), side)
            assert (status == 0).all() and out.dtype == torch.float32 and tuple(out.shape) == (len(ro) - 1, d)
            ref, mag = RM.gather_sum(table.numpy(), ro, idx.astype(np.int64), coef.numpy(), perm)
            L = np.diff(ro)[:, None]
            bound = 2.0 ** -24 * np.abs(ref) + L * 2.0 ** -52 * mag
            err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
            assert (err <= bound).all(), (n, side, float((err - bound).max()))
            again, _ = ratings.ragged_gather_sum(coef.to(dev), data, table.to(dev), side)
            assert again.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
            empty = np.flatnonzero(np.diff(ro) == 0)
            assert out.cpu().numpy()[empty].tobytes() == np.zeros((empty.size, d), np.float32).tobytes()


def _problem(n, m, d, seed, dev):
    import generation_data as gd
    import structure as S
    g = torch.Generator().manual_seed(seed)
    F = gd.FactoredMatrix(torch.randn(n, 2, generator=g), torch.randn(m, 2, generator=g))
    torch.manual_seed(seed + 1000)              # not the truth's stream: at d = 2 the model would start at the truth
    model = S.MatrixFactorization(n, m, d).to(dev)
    return S, model, F.dense(dev)


def _twin(S, model, dev):
    twin = S.MatrixFactorization(model.U.shape[0], model.V.shape[0], model.U.shape[1]).to(dev)
    with torch.no_grad():
        twin.U.copy_(model.U)
        twin.V.copy_(model.V)
    return twin


def test_fully_observed_ratings_are_the_population_risk(dev):
    """p = 1 through RatingsData: value and gradients of `ratings_risk` against `population_risk` at the module
    tolerance, the counts against `pair_stats_rows` exactly, the metrics against `compute_pairwise_metrics`."""
    from mfcd import pairs, ratings
    T = _tile()
    n, m, d, s = 5, T + 9, 3, 0.7
    S, model, Xd = _problem(n, m, d, 21, dev)
    data = S.observe_ratings(Xd, 1.0)
    assert data.device == Xd.device and data.entries == n * m and data.pairs == n * (m * (m - 1) // 2)
    risk = S.ratings_risk(model, data, s)
    assert risk.dim() == 0 and risk.is_cuda and risk.dtype == torch.float32 and risk.requires_grad
    risk.backward()
    gU, gV = model.U.grad.clone(), model.V.grad.clone()
    model.zero_grad()
    want = S.population_risk(model, Xd, s)
    want.backward()
    np.testing.assert_allclose(float(risk.detach()), float(want.detach()), rtol=RTOL, atol=ATOL)
    for name, got, ref in (("U", gU, model.U.grad), ("V", gV, model.V.grad)):
        err = (got - ref).abs().max().item()
        print(f"d{name}: max |grad| {ref.abs().max().item():.3e}, max abs difference {err:.3e}")
        np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=name)
    a, _ = ratings.ragged_scores(model.U.data, model.V.data, data)
    counts = ratings.pair_ragged_stats(a, data, s, "counts")[0]
    dense = pairs.pair_stats_rows(a.reshape(n, m), Xd, s, "counts")[0]
    assert torch.equal(counts, dense)
    # the likelihood / accuracy keys against the dense path (its scores come from a GEMM: tolerance, not bits); the two
    # keys made of counts against the dense counts of the same scores, where a rounding cannot flip a pair
    got, ref = S.compute_ratings_metrics(model, data, s), S.compute_pairwise_metrics(model, Xd, s)
    assert set(got) == set(ref)
    ref.update({k + "_per_user": v for k, v in pairs.pairwise_from_counts(dense, None, m).items()})
    for key in pairs._KEYS:
        np.testing.assert_allclose(got[key + "_per_user"], ref[key + "_per_user"], rtol=RTOL, atol=ATOL, err_msg=key)
        np.testing.assert_allclose(got[key], ref[key + "_per_user"].mean(), rtol=RTOL, atol=ATOL, err_msg=key)


def test_metrics_and_risk_on_a_sparse_table_match_the_model(dev):
    """Users with 0, 1 and more ratings, quantised to three levels: per-user metrics (NaN without a pair, out of the
    means), the global risk and its table gradients against the f64 model, with and without skip-ties."""
    import pairs_model as M
    n, m, d, s = 7, 40, 2, 1.3
    S, model, Xd = _problem(n, m, d, 5, dev)
    full = S.observe_ratings(Xd, 0.5, levels=3, seed=1)
    users, items, values = full.user.cpu().numpy(), full.item.cpu().numpy(), full.value.cpu().numpy()
    keep = (users != 2) & ((users != 4) | (items == items[users == 4][0]))          # user 2: none, user 4: one rating
    from mfcd import ratings
    data = ratings.RatingsData(users[keep], items[keep], values[keep], n, m).to(dev)
    assert data.lengths[2] == 0 and data.lengths[4] == 1
    U, V = model.U.detach().cpu().numpy().astype(np.float64), model.V.detach().cpu().numpy().astype(np.float64)
    ro, item, x = data.row_off.cpu().numpy(), data.item.cpu().numpy().astype(np.int64), data.value.cpu().numpy()
    for skip in (False, True):
        model.zero_grad()
        risk = S.ratings_risk(model, data, s, skip)
        np.testing.assert_allclose(float(risk.detach()), RM.ratings_risk(U, V, ro, item, x, s, skip), rtol=RTOL, atol=ATOL)
        risk.backward()
        dU, dV, g = RM.ratings_grad(U, V, ro, item, x, s, skip)
        # g's bound carried through the sums, as test_pair_grad.py's check_tables: per entry RTOL |g_e| + ATOL (L - 1)
        c = 1.0 / data.support(skip)
        eb = RTOL * np.abs(g) + ATOL * np.repeat(np.maximum(data.lengths - 1, 0), data.lengths)
        boundU = c * RM.gather_sum(np.abs(V), ro, item, eb)[0] + 2.0 ** -23 * np.abs(dU)
        boundV = c * RM.gather_sum(np.abs(U), data.col_off.cpu().numpy(), data.col_user.cpu().numpy().astype(np.int64), eb,
                                   data.col_perm.cpu().numpy())[0] + 2.0 ** -23 * np.abs(dV)
        for name, got, ref, bound in (("U", model.U.grad, dU, boundU), ("V", model.V.grad, dV, boundV)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert (err <= bound).all(), (skip, name, float(err.max()))
        got = S.compute_ratings_metrics(model, data, s, skip)
        a = RM.dot(U, V, ro, item)[0]
        counts, sums, support = RM.stats(a, x.astype(np.float64), ro, s, skip)
        for u in range(n):
            L = int(data.lengths[u])
            tau, acc = M.tau_b(list(counts[u]), L), M.pairwise_accuracy(list(counts[u]), L)
            for key, ref in (("kendall_tau", tau), ("pairwise_accuracy", acc),
                             ("expected_log_likelihood", -sums[u, 0] / support[u] if support[u] else np.nan),
                             ("bayes_log_likelihood", -sums[u, 1] / support[u] if support[u] else np.nan),
                             ("expected_accuracy", sums[u, 2] / support[u] if support[u] else np.nan),
                             ("bayes_accuracy", sums[u, 3] / support[u] if support[u] else np.nan)):
                v = got[key + "_per_user"][u]
                if np.isnan(ref):
                    assert np.isnan(v), (skip, u, key)
                else:
                    np.testing.assert_allclose(v, ref, rtol=RTOL, atol=ATOL, err_msg=f"{skip} {u} {key}")
        assert np.isnan(got["kendall_tau_per_user"][[2, 4]]).all()
        for key in ("kendall_tau", "expected_accuracy"):
            per = got[key + "_per_user"]
            np.testing.assert_allclose(got[key], per[~np.isnan(per)].mean(), rtol=1e-12)
    empty = ratings.RatingsData([0, 1], [0, 1], [1.0, 2.0], n, m).to(dev)
    with pytest.raises(ValueError):
        S.ratings_risk(model, empty, s)


def test_fit_ratings_is_backward_plus_adam_and_logs_the_models_risks(dev):
    from mfcd import _lib, ratings
    n, m, d, s, lr = 9, 65, 3, 0.7, 0.05
    S, model, Xd = _problem(n, m, d, 33, dev)
    data = S.observe_ratings(Xd, 0.6, seed=4)
    twin = _twin(S, model, dev)
    U0, V0 = model.U.detach().cpu().numpy().astype(np.float64), model.V.detach().cpu().numpy().astype(np.float64)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    steps, risks = S.train_model_ratings(model, data, s, opt, dev, num_steps=3, log_every=1)
    assert steps == [0, 1, 2, 3] and not model.training and all(isinstance(r, float) for r in risks)
    assert float(opt.state[model.U]["step"]) == 3 == float(opt.state[model.V]["step"])
    topt = torch.optim.Adam(twin.parameters(), lr=lr)
    seen = []
    for _ in range(3):
        topt.zero_grad()
        risk = S.ratings_risk(twin, data, s)
        seen.append(float(risk.detach()))
        risk.backward()
        topt.step()
    with torch.no_grad():
        seen.append(float(S.ratings_risk(twin, data, s)))
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(model.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(risks, seen, rtol=1e-5, atol=0)
    ro, item, x = data.row_off.cpu().numpy(), data.item.cpu().numpy().astype(np.int64), data.value.cpu().numpy()
    _, _, at, want = RM.fit(U0, V0, ro, item, x, s, 3, lr, log_every=1)
    assert at == steps
    print(f"logged risks {risks}, f64 model {want}")
    np.testing.assert_allclose(risks, want, rtol=RTOL, atol=ATOL)
    # any other optimiser takes backward: the same loop by hand
    sgd_model, sgd_twin = _twin(S, twin, dev), _twin(S, twin, dev)
    sgd = torch.optim.SGD(sgd_model.parameters(), lr=0.1)
    steps, risks = S.train_model_ratings(sgd_model, data, s, sgd, dev, num_steps=2, log_every=1, skip_ties=True)
    for _ in range(2):
        sgd_twin.zero_grad()
        S.ratings_risk(sgd_twin, data, s, True).backward()
        with torch.no_grad():
            sgd_twin.U -= 0.1 * sgd_twin.U.grad
            sgd_twin.V -= 0.1 * sgd_twin.V.grad
    assert steps == [0, 1, 2]
    np.testing.assert_allclose(sgd_model.U.detach().cpu().numpy(), sgd_twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    bf = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        ratings.fit_ratings((bf, torch.optim.Adam(bf.parameters(), lr=lr)), data, s, 2)
    with pytest.raises(_lib.MfcdError):
        S.ratings_risk(bf, data)


def test_end_to_end_training_on_observed_ratings_improves_the_held_out_ranking(dev):
    """Rank-2 X, 60 x 60, half of it observed, split 80 / 20, 300 fused steps: relative comparisons only."""
    S, model, Xd = _problem(60, 60, 2, 11, dev)
    data = S.observe_ratings(Xd, 0.5, seed=0)
    train, test = data.split((0.8, 0.2), seed=0)
    assert train.entries + test.entries == data.entries and train.device == Xd.device
    before = S.compute_ratings_metrics(model, test, 1.0)
    with torch.no_grad():
        risk_before = float(S.ratings_risk(model, train, 1.0))
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    steps, risks = S.train_model_ratings(model, train, 1.0, opt, dev, num_steps=300, log_every=100)
    after = S.compute_ratings_metrics(model, test, 1.0)
    print(f"training risk {risk_before:.5f} -> {risks[-1]:.5f}; held-out tau-b {before['kendall_tau']:.4f} -> "
          f"{after['kendall_tau']:.4f}, pairwise accuracy {before['pairwise_accuracy']:.4f} -> {after['pairwise_accuracy']:.4f}")
    assert steps == [0, 100, 200, 300]
    np.testing.assert_allclose(risks[0], risk_before, rtol=RTOL, atol=ATOL)
    assert risks[-1] < risk_before
    assert after["kendall_tau"] > before["kendall_tau"]
