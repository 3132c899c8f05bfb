"""GPU tests of the ranked-list machinery (include/mfcd.h: mfcd_list_pl; mfcd/lists.py; structure.rankings_risk,
train_model_rankings, compute_rankings_metrics): the kernel against the numpy f64 model (tests/list_pl_model.py) on the
same fp32 scores over every length and depth at which it takes another path and on the scores that break the naive form;
bit-equality, independence of a row's place and the `what` halves; non-finite and invalid rows; lists of two against the
ratings risk; autograd, the fused fit, the metrics and an end-to-end fit."""
import functools

import numpy as np
import pytest
import torch

import list_pl_model as LM

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6       # test_ratings.py's, for the same kind of comparison
KINDS = ("normal", "equal", "down200", "down3000", "up200", "up3000", "peak", "huge")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tile():
    from mfcd import _lib
    return _lib.load().mfcd_list_pl_tile()


def _scores(kind, L, rng):
    if kind == "equal":
        return np.full(L, 0.25, dtype=np.float32)
    if kind in ("down200", "down3000", "up200", "up3000"):     # strictly monotone: the steps are far above an fp32 ulp
        a = np.linspace(float(kind.lstrip("downup")), 0.0, L).astype(np.float32)
        assert L < 2 or (np.diff(a) < 0).all()
        return a if kind.startswith("down") else a[::-1].copy()
    a = rng.standard_normal(L).astype(np.float32)
    if kind == "peak":
        a *= np.float32(0.1)
        if L:
            a[L // 2] += np.float32(10.0)
    if kind == "huge" and L >= 2:
        # neighbours whose difference overflows fp32.  At the head of the list, where the f64 model is still the truth: it
        # folds (max, sum) into one f64, so after k entries that a 3e38 follows it has lost log k beside the 3e38
        # (test_a_huge_score_in_mid_list holds the kernel to the closed form there)
        a[0], a[1] = np.float32(3e38), np.float32(-3e38)
    return a


def _offsets(lens, unit):
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(lens))), np.concatenate(([0], np.cumsum((lens + unit - 1) // unit)))


@functools.lru_cache(maxsize=None)
def case():
    """Every length with every depth that applies and every kind of scores → (rows [(scores, depth, kind)], model)."""
    T = _tile()
    rng = np.random.default_rng(0)
    rows = []
    for L in (0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 70001):
        for depth in sorted({d for d in (0, 1, 2, L - 1, L, T, T + 1) if 0 <= d <= L}):
            for kind in KINDS:
                rows.append((_scores(kind, L, rng), depth, kind))
    a = np.concatenate([r[0] for r in rows])
    off, _ = _offsets([r[0].size for r in rows], T)
    depth = np.array([r[1] for r in rows], dtype=np.int32)
    return rows, a, off, depth, LM.rows(a, off, depth)


def run(dev, a, off, depth, what=3, tile_off=None, n_tiles=None, entries=None, g_fill=None):
    """One call of the entry on host arrays → (loss, counts, g, status) as numpy (None where not asked for)."""
    from mfcd import _lib
    L = _lib.load()
    off = np.asarray(off, dtype=np.int64)
    rows = off.size - 1
    if tile_off is None:
        tile_off = _offsets(np.diff(off), _tile())[1]
    n_tiles = int(tile_off[-1]) if n_tiles is None else n_tiles
    entries = int(np.asarray(a).size) if entries is None else entries
    a_d = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    off_d, tile_d = torch.from_numpy(off).to(dev), torch.from_numpy(np.asarray(tile_off, dtype=np.int64)).to(dev)
    depth_d = None if depth is None else torch.from_numpy(np.asarray(depth, dtype=np.int32)).to(dev)
    loss = torch.full((rows,), -7.0, dtype=torch.float64, device=dev) if what & 1 else None
    counts = torch.full((rows, 2), -7, dtype=torch.int64, device=dev) if what & 1 else None
    g = None
    if what & 2:
        g = torch.empty(max(entries, 1), dtype=torch.float32, device=dev)
        g.fill_(float("nan") if g_fill is None else g_fill)
    status = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_list_pl_workspace_bytes(rows, n_tiles), dev)
    _lib.check(L.mfcd_list_pl(_lib.ptr(a_d), entries, _lib.ptr(off_d), _lib.ptr(depth_d), rows, _lib.ptr(tile_d), n_tiles,
                              what, _lib.ptr(loss), _lib.ptr(counts), _lib.ptr(g), _lib.ptr(status), _lib.ptr(ws),
                              ws.numel(), _lib.stream_ptr(dev)))
    host = lambda t: None if t is None else t.cpu().numpy()    # noqa: E731
    return host(loss), host(counts), None if g is None else host(g)[:entries], host(status)


@functools.lru_cache(maxsize=None)
def case_outputs():
    rows, a, off, depth, _ = case()
    return run(torch.device("cuda:0"), a, off, depth)


def test_loss_counts_and_gradient_match_the_f64_model(dev):
    rows, a, off, depth, (want_loss, want_counts, want_g) = case()
    loss, counts, g, status = case_outputs()
    assert (status == 0).all()
    assert np.array_equal(counts, want_counts)
    worst = {}
    for r, (scores, d, kind) in enumerate(rows):
        L, b, e = scores.size, off[r], off[r + 1]
        stages = LM.stages_of(L, d)
        assert counts[r, 0] == stages
        np.testing.assert_allclose(loss[r], want_loss[r], rtol=RTOL, atol=ATOL, err_msg=f"loss {kind} L={L} depth={d}")
        np.testing.assert_allclose(g[b:e], want_g[b:e], rtol=RTOL, atol=ATOL, err_msg=f"g {kind} L={L} depth={d}")
        assert abs(g[b:e].astype(np.float64).sum()) <= ATOL * max(L, 1), (kind, L, d)
        if stages == 0:
            assert loss[r].tobytes() == np.float64(0.0).tobytes() and counts[r, 1] == 0
            assert g[b:e].tobytes() == np.zeros(L, np.float32).tobytes()             # +0, not -0
            continue
        if kind in ("equal", "down200", "down3000"):
            assert counts[r, 1] == stages, (kind, L, d)
        if kind in ("up200", "up3000"):
            assert counts[r, 1] == 0, (kind, L, d)
        if kind == "equal":
            np.testing.assert_allclose(loss[r], LM.uniform_loss(L, d), rtol=1e-10)    # L 2^-53 = 8e-12 at the worst
        # in units of 2^-24 |g|, where <= 1 is a correctly rounded g; over |g| >= 1e-3 only: the model forms a + N at the
        # size of the scores, so below that its own error (an ulp of 3000 is 4.5e-13) is not small beside 2^-24 |g|
        big = np.abs(want_g[b:e]) >= 1e-3
        ulps = np.abs(g[b:e] - want_g[b:e])[big] / (np.abs(want_g[b:e][big]) * 2.0 ** -24)
        worst[kind] = max(worst.get(kind, 0.0), float(ulps.max(initial=0.0)))
    up = [r for r, (s, d, kind) in enumerate(rows) if kind == "up3000" and s.size == 3 * _tile() + 5 and d == s.size]
    assert g[off[up[0]]:off[up[0] + 1]].max() > 30.0 and want_loss[up[0]] > 1e6    # far from the softmax's [0, 1]
    print("largest |g - model| in units of 2^-24 |g|, by kind:", {k: round(v, 3) for k, v in worst.items()})


def test_a_huge_score_in_mid_list(dev):
    """3e38 at rank j, -3e38 after it, small scores around: every stage up to j would have picked entry j with
    probability 1 - O(exp(-3e38)), so g_j = (stages up to j) - [j is a stage], g_l = -[l is a stage] before it, and from
    j + 1 on the list is the softmax chain of its own tail; the sum over the row is 0 and the loss is (the j stages
    before it) x 3e38 + the tail's.  One tile and three."""
    T = _tile()
    rng = np.random.default_rng(4)
    rows, want = [], []
    for L, j, depth in ((40, 13, 40), (40, 13, 9), (3 * T + 5, T + 3, 3 * T + 5), (3 * T + 5, 2 * T, T + 1)):
        a = rng.standard_normal(L).astype(np.float32)
        a[j], a[j + 1] = np.float32(3e38), np.float32(-3e38)
        stages = LM.stages_of(L, depth)
        tail_loss, _, _, tail_g = LM.row(a[j + 1:], max(depth - j - 1, 0))
        g = np.concatenate((-(np.arange(j) < stages).astype(np.float64), [min(j + 1, stages) - float(j < stages)], tail_g))
        rows.append((a, depth))
        want.append((min(j, stages) * float(np.float32(3e38)) + tail_loss, g))
    off, _ = _offsets([a.size for a, _ in rows], T)
    loss, counts, g, status = run(dev, np.concatenate([a for a, _ in rows]), off, [d for _, d in rows])
    assert (status == 0).all()
    for r, (want_loss, want_g) in enumerate(want):
        got = g[off[r]:off[r + 1]]
        np.testing.assert_allclose(loss[r], want_loss, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got, want_g, rtol=RTOL, atol=ATOL)
        assert abs(got.astype(np.float64).sum()) <= ATOL * got.size


def test_the_naive_form_loses_the_confident_rows():
    """What the test above would not forgive: exp(a - max) and a plain suffix sum, in fp32 and over 3000 in f64."""
    for spread, dtype in ((200.0, np.float32), (3000.0, np.float64)):
        a = np.linspace(spread, 0.0, 300).astype(np.float32)
        e = np.exp((a - a.max()).astype(dtype))
        suffix = np.cumsum(e[::-1], dtype=dtype)[::-1]
        assert (suffix[-100:] == 0).any() or not np.isfinite(np.log(suffix[:-1]) - np.log(e[:-1])).all()


def test_calls_are_bit_equal_rows_independent_of_their_place_and_what_halves_match(dev):
    rows, a, off, depth, _ = case()
    loss, counts, g, _ = case_outputs()
    again = run(dev, a, off, depth)
    assert again[0].tobytes() == loss.tobytes() and again[1].tobytes() == counts.tobytes()
    assert again[2].tobytes() == g.tobytes()
    half1, half2 = run(dev, a, off, depth, what=1), run(dev, a, off, depth, what=2)
    assert half1[0].tobytes() == loss.tobytes() and half1[1].tobytes() == counts.tobytes() and half1[2] is None
    assert half2[2].tobytes() == g.tobytes() and half2[0] is None and (half2[3] == 0).all()
    # a sample of the rows, permuted and embedded between other rows
    rng = np.random.default_rng(1)
    long_rows = [r for r in range(len(rows)) if rows[r][0].size == 70001]
    pick = list(rng.permutation([r for r in range(len(rows)) if r not in long_rows])[:150]) + long_rows[:2]
    pick = [int(r) for r in rng.permutation(pick)]
    filler = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(0, 600, len(pick) + 1)]
    parts, lens, deps, where = [], [], [], {}
    for k, r in enumerate(pick):
        parts.append(filler[k])
        lens.append(filler[k].size)
        deps.append(filler[k].size // 2)
        where[r] = len(lens)
        parts.append(rows[r][0])
        lens.append(rows[r][0].size)
        deps.append(rows[r][1])
    parts.append(filler[-1])
    lens.append(filler[-1].size)
    deps.append(filler[-1].size)
    off2, _ = _offsets(lens, _tile())
    loss2, counts2, g2, status2 = run(dev, np.concatenate(parts), off2, deps)
    assert (status2 == 0).all()
    for r, q in where.items():
        assert loss2[q].tobytes() == loss[r].tobytes() and counts2[q].tobytes() == counts[r].tobytes(), rows[r][1:]
        assert g2[off2[q]:off2[q + 1]].tobytes() == g[off[r]:off[r + 1]].tobytes(), rows[r][1:]
    # depth = NULL is every row fully ranked
    full = [r for r in range(len(rows)) if rows[r][1] == rows[r][0].size and rows[r][0].size < 1000]
    offf, _ = _offsets([rows[r][0].size for r in full], _tile())
    lossf, countsf, gf, _ = run(dev, np.concatenate([rows[r][0] for r in full]), offf, None)
    for q, r in enumerate(full):
        assert lossf[q].tobytes() == loss[r].tobytes() and countsf[q].tobytes() == counts[r].tobytes()
        assert gf[offf[q]:offf[q + 1]].tobytes() == g[off[r]:off[r + 1]].tobytes()


LENS = [300, 10, 600, 5, 20]                      # offsets 0, 300, 310, 910, 915, 935; tiles 2, 1, 3, 1, 1


def _plain():
    rng = np.random.default_rng(8)
    a = rng.standard_normal(sum(LENS)).astype(np.float32)
    off, tile_off = _offsets(LENS, _tile())
    depth = np.array([300, 4, 599, 5, 0], dtype=np.int32)
    return a, off, tile_off, depth


def test_a_non_finite_row_gets_nan_and_its_neighbours_are_untouched(dev):
    a, off, tile_off, depth = _plain()
    loss0, counts0, g0, st0 = run(dev, a, off, depth)
    assert (st0 == 0).all() and np.isfinite(loss0).all() and np.isfinite(g0).all()
    for value, rows_hit, at in ((np.nan, [2], [off[2] + 599]), (np.inf, [1], [off[1]]), (-np.inf, [0, 3], [5, off[3] + 2]),
                                (np.nan, [2], [off[2] + 300]), (np.inf, [4], [off[4] + 7])):     # row 4 has depth 0
        b = a.copy()
        b[at] = value
        for what in (3, 1, 2):
            loss, counts, g, status = run(dev, b, off, depth, what=what)
            assert (status == 0).all()
            for r in range(5):
                sl = slice(off[r], off[r + 1])
                if r in rows_hit:
                    assert loss is None or (np.isnan(loss[r]) and (counts[r] == -1).all()), (value, r)
                    assert g is None or np.isnan(g[sl]).all(), (value, r)
                else:
                    assert loss is None or (loss[r].tobytes() == loss0[r].tobytes() and
                                            counts[r].tobytes() == counts0[r].tobytes()), (value, r)
                    assert g is None or g[sl].tobytes() == g0[sl].tobytes(), (value, r)


def test_invalid_rows_get_status_2_and_nothing_of_them_is_written(dev):
    """Offsets that decrease or run past `entries`, a depth outside [0, L], a wrong tile count: the bad values are only
    compared, so nothing outside the buffers is read; the row is marked and the other rows keep their bytes."""
    a, off, tile_off, depth = _plain()
    loss0, counts0, g0, _ = run(dev, a, off, depth)
    cases = (("decreasing", {2: 290}, {}, {}, [1]), ("past entries", {5: 936}, {}, {}, [4]),
             ("negative", {0: -1}, {}, {}, [0]), ("tile count", {2: 700}, {}, {}, [1, 2]),
             ("depth < 0", {}, {1: -1}, {}, [1]), ("depth > L", {}, {3: 6}, {}, [3]),
             ("depth > L, long", {}, {2: 601}, {}, [2]), ("tile offsets", {}, {}, {3: 7}, [2, 3]),
             ("tiles past n_tiles", {}, {}, {5: 9}, [4]))
    for name, edit_off, edit_depth, edit_tiles, bad_rows in cases:
        ro, dp, to = off.copy(), depth.copy(), tile_off.copy()
        for k, v in edit_off.items():
            ro[k] = v
        for k, v in edit_depth.items():
            dp[k] = v
        for k, v in edit_tiles.items():
            to[k] = v
        loss, counts, g, status = run(dev, a, ro, dp, tile_off=to, n_tiles=int(tile_off[-1]), g_fill=-123.0)
        assert status.tolist() == [2 if r in bad_rows else 0 for r in range(5)], name
        owners = np.zeros(a.size, dtype=np.int64)         # "decreasing" makes row 2 start inside row 0: two writers there
        for r in range(5):
            if r not in bad_rows:
                owners[ro[r]:ro[r + 1]] += 1
        for r in range(5):
            if r in bad_rows:
                assert np.isnan(loss[r]) and (counts[r] == -1).all(), (name, r)
            elif ro[r] == off[r] and ro[r + 1] == off[r + 1]:
                assert loss[r].tobytes() == loss0[r].tobytes() and counts[r].tobytes() == counts0[r].tobytes(), (name, r)
                mine = np.arange(off[r], off[r + 1])[owners[off[r]:off[r + 1]] == 1]
                assert g[mine].tobytes() == g0[mine].tobytes(), (name, r)
        assert (g[owners == 0] == -123.0).all(), name                        # no entry of a bad row is written
        only_g = run(dev, a, ro, dp, what=2, tile_off=to, n_tiles=int(tile_off[-1]), g_fill=-123.0)
        assert only_g[2][owners < 2].tobytes() == g[owners < 2].tobytes() and only_g[3].tolist() == status.tolist(), name


def _problem(n, m, d, seed, dev):
    """A rank-2 truth (f64 product rounded to fp32 once, on the host) and a model that does not start at it."""
    import structure as S
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(n, 2, generator=g), torch.randn(m, 2, generator=g)
    torch.manual_seed(seed + 1000)
    return S, S.MatrixFactorization(n, m, d).to(dev), (A.double() @ B.double().t()).float()


def _twin(S, model, dev):
    twin = S.MatrixFactorization(model.U.shape[0], model.V.shape[0], model.U.shape[1]).to(dev)
    with torch.no_grad():
        twin.U.copy_(model.U)
        twin.V.copy_(model.V)
    return twin


def _ragged_lists(n, m, low, high, seed, dev, depths=False):
    from mfcd.lists import RankedLists
    rng = np.random.default_rng(seed)
    users, items, positions, depth = [], [], [], []
    for u in range(n):
        L = int(rng.integers(low, high + 1))
        users += [u] * L
        items += rng.choice(m, L, replace=False).tolist()
        positions += list(range(L))
        depth.append(int(rng.integers(0, L + 1)) if depths and u % 2 else L)
    return RankedLists(users, items, positions, n, m, depth).to(dev)


def test_lists_of_two_are_the_btl_pair(dev):
    """A list of two with depth 1 is the comparison "the first beats the second": `ratings_risk` with values (1, 0) at
    s = 64, whose label is 1 to 1e-28."""
    from mfcd.lists import RankedLists
    from mfcd.ratings import RatingsData
    n, m, d = 70, 30, 3
    S, model, _ = _problem(n, m, d, 3, dev)
    rng = np.random.default_rng(2)
    pairs = np.array([rng.choice(m, 2, replace=False) for _ in range(n)])
    users = np.repeat(np.arange(n), 2)
    lists = RankedLists(users, pairs.reshape(-1), np.tile([0, 1], n), n, m, depth=1).to(dev)
    data = RatingsData(users, pairs.reshape(-1), np.tile([1.0, 0.0], n), n, m).to(dev)
    assert lists.stages == n == data.pairs
    risk = S.rankings_risk(model, lists)
    assert risk.dim() == 0 and risk.is_cuda and risk.dtype == torch.float32 and risk.requires_grad
    risk.backward()
    gU, gV = model.U.grad.clone(), model.V.grad.clone()
    model.zero_grad()
    want = S.ratings_risk(model, data, 64.0)
    want.backward()
    np.testing.assert_allclose(float(risk.detach()), float(want.detach()), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gU.cpu().numpy(), model.U.grad.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV.cpu().numpy(), model.V.grad.cpu().numpy(), rtol=RTOL, atol=ATOL)
    full = RankedLists(users, pairs.reshape(-1), np.tile([0, 1], n), n, m).to(dev)      # depth 2 is one stage too
    with torch.no_grad():
        assert float(S.rankings_risk(model, full)) == float(risk.detach())


@pytest.mark.parametrize("d", [2, 16])
def test_the_risk_and_its_table_gradients_match_the_model(dev, d):
    from mfcd import lists as ML
    n, m = 12, 40
    S, model, _ = _problem(n, m, d, 5 + d, dev)
    lists = _ragged_lists(n, m, 3, 40, 9, dev, depths=True)
    risk = ML.pl_risk(model.U, model.V, lists)
    risk.backward()
    a, status = ML.list_scores(model.U.data, model.V.data, lists)
    assert (status == 0).all()
    off, item, user = lists.row_off.cpu().numpy(), lists.item.cpu().numpy().astype(np.int64), lists.user.cpu().numpy()
    U, V = model.U.detach().cpu().numpy().astype(np.float64), model.V.detach().cpu().numpy().astype(np.float64)
    # d products rounded to fp32 and d - 1 fp32 additions of them
    assert (np.abs(a.cpu().numpy() - (U[user] * V[item]).sum(1)) <= d * 2.0 ** -23 * np.abs(U[user] * V[item]).sum(1)).all()
    loss, counts, g = LM.rows(a.cpu().numpy(), off, lists.depth.cpu().numpy())          # the model on the same fp32 scores
    assert counts[:, 0].sum() == lists.stages and np.array_equal(counts[:, 0], lists.user_stages)
    c = 1.0 / lists.stages
    np.testing.assert_allclose(float(risk.detach()), loss.sum() * c, rtol=RTOL, atol=ATOL)
    # g's bound carried through the sums: per entry RTOL |g_e| + ATOL, then the fp32 roundings of c g and of the sum
    eb = RTOL * np.abs(g) + ATOL + 2.0 ** -22 * np.abs(g)
    for name, got, idx, table, into in (("U", model.U.grad, user, V[item], np.zeros_like(U)),
                                        ("V", model.V.grad, item, U[user], np.zeros_like(V))):
        want, bound = into.copy(), into.copy()
        np.add.at(want, idx, c * g[:, None] * table)
        np.add.at(bound, idx, c * eb[:, None] * np.abs(table))
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"d{name}: max |grad| {np.abs(want).max():.3e}, max abs difference {err.max():.3e}")
        assert (err <= bound + 1e-12).all(), (name, float(err.max()))
    with torch.no_grad():
        quiet = ML.pl_risk(model.U, model.V, lists)
    assert not quiet.requires_grad and float(quiet) == float(risk.detach())
    empty = ML.RankedLists([0, 1, 1], [0, 1, 2], [0, 0, 1], n, m, depth=[1, 0] + [0] * (n - 2)).to(dev)
    with pytest.raises(ValueError):
        ML.pl_risk(model.U, model.V, empty)


def test_fit_lists_is_backward_plus_adam(dev):
    from mfcd import _lib, lists as ML
    n, m, d, lr = 9, 65, 3, 0.05
    S, model, _ = _problem(n, m, d, 33, dev)
    lists = _ragged_lists(n, m, 0, 65, 4, dev, depths=True)
    twin = _twin(S, model, dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    steps, risks = S.train_model_rankings(model, lists, opt, dev, num_steps=5, log_every=1)
    assert steps == [0, 1, 2, 3, 4, 5] and not model.training and all(isinstance(r, float) for r in risks)
    assert float(opt.state[model.U]["step"]) == 5 == float(opt.state[model.V]["step"])
    topt = torch.optim.Adam(twin.parameters(), lr=lr)
    seen = []

    def twin_step():
        topt.zero_grad()
        risk = S.rankings_risk(twin, lists)
        seen.append(float(risk.detach()))
        risk.backward()
        topt.step()

    for _ in range(5):
        twin_step()
    with torch.no_grad():
        seen.append(float(S.rankings_risk(twin, lists)))
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(model.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(risks, seen, rtol=1e-5, atol=0)
    # the optimizer's state is usable afterwards: a sixth step by backward on both
    opt.zero_grad()
    S.rankings_risk(model, lists).backward()
    opt.step()
    twin_step()
    assert float(opt.state[model.U]["step"]) == 6
    # an Adam step is at most about lr long and the two forms round it differently: two fp32 roundings of lr a step, which
    # a relative bound does not grant an element that has come close to 0
    slack = 6 * lr * 2.0 ** -22
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=slack)
    np.testing.assert_allclose(model.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=slack)
    # without logging nothing is read back; any other optimiser takes backward: the same loop by hand
    assert ML.fit_lists((model, opt), lists, 2) == ([], []) and float(opt.state[model.U]["step"]) == 8
    sgd_model, sgd_twin = _twin(S, twin, dev), _twin(S, twin, dev)
    sgd = torch.optim.SGD(sgd_model.parameters(), lr=0.1)
    steps, risks = S.train_model_rankings(sgd_model, lists, sgd, dev, num_steps=2, log_every=1)
    for _ in range(2):
        sgd_twin.zero_grad()
        S.rankings_risk(sgd_twin, lists).backward()
        with torch.no_grad():
            sgd_twin.U -= 0.1 * sgd_twin.U.grad
            sgd_twin.V -= 0.1 * sgd_twin.V.grad
    assert steps == [0, 1, 2]
    np.testing.assert_allclose(sgd_model.U.detach().cpu().numpy(), sgd_twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    bf = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        ML.fit_lists((bf, torch.optim.Adam(bf.parameters(), lr=lr)), lists, 2)
    with pytest.raises(_lib.MfcdError):
        S.rankings_risk(bf, lists)


def test_metrics_match_the_model_and_scipy(dev):
    from scipy.stats import kendalltau
    from mfcd import lists as ML
    n, m, d = 14, 300, 4
    S, model, _ = _problem(n, m, d, 17, dev)
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 2, 3, 300, 257, 40, 40, 17, 5, 64, 65, 9]
    deps = [0, 1, 1, 2, 0, 300, 1, 2, 40, 16, 5, 63, 3, 1]
    users, items, positions = [], [], []
    for u, L in enumerate(lens):
        users += [u] * L
        items += rng.choice(m, L, replace=False).tolist()
        positions += list(range(L))
    lists = ML.RankedLists(users, items, positions, n, m, deps).to(dev)
    got = S.compute_rankings_metrics(model, lists)
    assert set(got) == {k + suffix for k in ML._KEYS for suffix in ("", "_per_user")}
    a = ML.list_scores(model.U.data, model.V.data, lists)[0].cpu().numpy()
    off = lists.row_off.cpu().numpy()
    for u, (L, dep) in enumerate(zip(lens, deps)):
        loss, stages, hits, _ = LM.row(a[off[u]:off[u + 1]], dep)
        want = {"choice_log_likelihood": -loss / stages if stages else np.nan,
                "choice_accuracy": hits / stages if stages else np.nan,
                "uniform_log_likelihood": -LM.uniform_loss(L, dep) / stages if stages else np.nan,
                "kendall_tau": kendalltau(a[off[u]:off[u] + dep], -np.arange(dep)).statistic if dep >= 2 else np.nan}
        for key, ref in want.items():
            v = got[key + "_per_user"][u]
            if np.isnan(ref):
                assert np.isnan(v), (u, key)
            else:
                np.testing.assert_allclose(v, ref, rtol=RTOL, atol=ATOL, err_msg=f"{u} {key}")
    for key in ML._KEYS:
        per = got[key + "_per_user"]
        assert per.shape == (n,) and per.dtype == np.float64
        np.testing.assert_allclose(got[key], per[~np.isnan(per)].mean(), rtol=1e-12)
    assert np.isnan(got["choice_accuracy_per_user"][[0, 1, 4]]).all() and not np.isnan(got["choice_accuracy_per_user"][2])


def test_end_to_end_training_on_ranked_lists_improves_the_held_out_choices(dev):
    """Rank-2 X, 60 x 60, lists of 20 drawn at s = 4 on the host (the same lists wherever this runs), split 80 / 20, 300
    fused Adam steps at lr = 0.1 (at 0.05 an f64 fit is still on its first plateau after 300 steps).  The thresholds come
    from the f64 CPU twin of the same fit (torch autograd on torch.logcumsumexp over the padded lists, f64 tables from the
    same start), which goes
        held-out choice log-likelihood  -1.2813 -> -0.6328   (uniform: -1.0594)
        held-out mean Kendall tau        0.0000 ->  0.7722
        training risk                    2.2903 ->  0.8198
    and each threshold grants half of the twin's improvement: fp32 tables and another summation order move a 300-step
    trajectory."""
    from mfcd.lists import sample_rankings
    S, model, X = _problem(60, 60, 2, 11, dev)
    lists = sample_rankings(X, 20, s=4.0, seed=0).to(dev)
    train, test = lists.split((0.8, 0.2), seed=0)
    assert (train.entries, test.entries, train.stages, test.stages) == (960, 240, 900, 180) and train.device.type == "cuda"
    before = S.compute_rankings_metrics(model, test)
    with torch.no_grad():
        risk_before = float(S.rankings_risk(model, train))
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    steps, risks = S.train_model_rankings(model, train, opt, dev, num_steps=300, log_every=100)
    after = S.compute_rankings_metrics(model, test)
    print(f"training risk {risk_before:.5f} -> {risks[-1]:.5f}; held-out choice log-likelihood "
          f"{before['choice_log_likelihood']:.4f} -> {after['choice_log_likelihood']:.4f} (uniform "
          f"{after['uniform_log_likelihood']:.4f}), tau {before['kendall_tau']:.4f} -> {after['kendall_tau']:.4f}, "
          f"choice accuracy {before['choice_accuracy']:.4f} -> {after['choice_accuracy']:.4f}")
    assert steps == [0, 100, 200, 300]
    np.testing.assert_allclose(risks[0], risk_before, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(before["choice_log_likelihood"], -1.2813, atol=2e-4)     # the twin's start
    np.testing.assert_allclose(after["uniform_log_likelihood"], -1.0594, atol=2e-4)
    assert risks[-1] < risk_before - 0.5 * (2.2903 - 0.8198)
    assert after["choice_log_likelihood"] > after["uniform_log_likelihood"]
    assert after["choice_log_likelihood"] > before["choice_log_likelihood"] + 0.5 * (1.2813 - 0.6328)
    assert after["kendall_tau"] > before["kendall_tau"] + 0.5 * 0.7722
