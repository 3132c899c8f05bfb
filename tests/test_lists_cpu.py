"""CPU-only checks of the ranked-list machinery (include/mfcd.h: mfcd_list_pl; mfcd/lists.py; structure.observe_rankings,
load_rankings, rankings_risk, train_model_rankings, compute_rankings_metrics): the numpy model the GPU tests compare with
(tests/list_pl_model.py) is a probability over the orders, its gradient is the central difference's and sums to 0; the
entries are declared and bound, bad arguments are refused before the device is touched, there is no CPU fallback;
`RankedLists` sorts, validates, transposes and splits; `sample_rankings` draws from the Plackett–Luce law."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import list_pl_model as LM
from conftest import ROOT

NAME = "mfcd_list_pl"


def _brute(a, depth=None):
    """The definitions, term by term: O(L^2), no scan."""
    a = np.asarray(a, dtype=np.float64)
    L = a.size
    stages = LM.stages_of(L, depth)
    lse = np.array([np.logaddexp.reduce(a[k:]) for k in range(L)])
    loss = sum(lse[k] - a[k] for k in range(stages))
    g = np.array([sum(np.exp(a[l] - lse[k]) for k in range(min(l + 1, stages))) - (l < stages) for l in range(L)])
    hits = sum(int(a[k] >= a[k:].max()) for k in range(stages))
    return loss, stages, hits, g


def test_the_model_is_a_probability_over_the_orders():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(5) * 2.0
    total = sum(np.exp(-LM.row(a[list(p)])[0]) for p in itertools.permutations(range(5)))
    assert abs(total - 1.0) < 1e-13
    top2 = 0.0
    for i, j in itertools.permutations(range(5), 2):
        rest = [k for k in range(5) if k not in (i, j)]
        top2 += np.exp(-LM.row(a[[i, j] + rest], depth=2)[0])
    assert abs(top2 - 1.0) < 1e-13
    first = sum(np.exp(-LM.row(a[[i] + [k for k in range(5) if k != i]], depth=1)[0]) for i in range(5))
    assert abs(first - 1.0) < 1e-13


@pytest.mark.parametrize("L,depth", [(2, None), (7, None), (7, 3), (7, 6), (7, 7), (40, 1), (40, 25)])
def test_the_models_gradient(L, depth):
    rng = np.random.default_rng(L + (depth or 0))
    a = rng.standard_normal(L) * 1.5
    loss, stages, hits, g = LM.row(a, depth)
    bl, bs, bh, bg = _brute(a, depth)
    assert abs(loss - bl) < 1e-12 and stages == bs and hits == bh
    np.testing.assert_allclose(g, bg, rtol=0, atol=1e-13)
    assert abs(g.sum()) < 1e-14 * L
    h = 1e-5
    for l in range(L):
        e = np.zeros(L)
        e[l] = h
        fd = (LM.row(a + e, depth)[0] - LM.row(a - e, depth)[0]) / (2 * h)
        assert abs(fd - g[l]) < 1e-8


def test_the_model_on_equal_far_and_degenerate_rows():
    for L, depth in ((1, None), (2, None), (9, None), (9, 4), (300, 299)):
        loss, stages, hits, g = LM.row(np.full(L, 0.25), depth)
        assert abs(loss - LM.uniform_loss(L, depth)) < 1e-12 * max(L, 1) and hits == stages == LM.stages_of(L, depth)
        want = sum(np.log(L - k) for k in range(stages))
        assert abs(LM.uniform_loss(L, depth) - want) < 1e-10
    assert LM.row([], None) [:3] == (0.0, 0, 0) and LM.row([3.0], None)[:3] == (0.0, 0, 0)
    assert LM.row([1.0, 2.0, 3.0], 0)[:3] == (0.0, 0, 0) and not LM.row([1.0, 2.0, 3.0], 0)[3].any()
    assert np.isnan(LM.row([1.0, np.inf], None)[0]) and LM.row([1.0, np.nan, 2.0], None)[1:3] == (-1, -1)
    # a confident model: exp(a - max) underflows from the 750th entry on, the scans do not care
    for spread in (200.0, 3000.0):
        down = np.linspace(spread, 0.0, 300)
        loss, stages, hits, g = LM.row(down)
        # a + N is formed at magnitude `spread` (ulp(3000) = 4.5e-13) and sum |g| is about 4: a few roundings of it
        assert hits == stages == 299 and np.isfinite(loss) and 0.0 < loss < 300 and abs(g.sum()) < 1e-11
        bl, _, _, bg = _brute(down)
        assert abs(loss - bl) < 1e-9 and np.abs(g - bg).max() < 1e-12
        loss, stages, hits, g = LM.row(down[::-1].copy())
        assert hits == 0 and abs(g.sum()) < 1e-9 and g.max() > 1.0
        assert abs(loss - _brute(down[::-1])[0]) < 1e-9 * loss
    # a list of two is the BTL pair
    loss, _, _, g = LM.row([0.3, -1.1], 1)
    assert abs(loss - np.log1p(np.exp(-1.4))) < 1e-15 and abs(g[0] + 1 / (1 + np.exp(1.4))) < 1e-15


def test_the_entries_are_declared_and_bound():
    from mfcd import _lib, lists
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 15
    assert len(re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1).split(",")) == 15
    assert len(_lib.SIGNATURES[NAME + "_workspace_bytes"][1]) == 2
    assert len(re.search(r"\b%s_workspace_bytes\(([^)]*)\);" % NAME, header).group(1).split(",")) == 2
    assert re.search(r"\bint %s_tile\(void\);" % NAME, header)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4
    assert hasattr(L, NAME) and hasattr(L, NAME + "_workspace_bytes") and hasattr(L, NAME + "_tile")
    assert L.mfcd_list_pl_tile() == 256
    csrc = os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc")
    src = open(os.path.join(csrc, "list_pl.hip")).read()
    assert "__global__" in src and "atomicAdd" not in src
    assert "list_pl.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "mfcd_list_pl(" in inspect.getsource(lists.pl_rows)


def test_the_workspace_is_88_bytes_a_tile_and_4_a_row():
    from mfcd import _lib
    ws = _lib.load().mfcd_list_pl_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256    # noqa: E731
    assert ws(0, 0) == 512 and ws(1, 1) == 512
    assert ws(1000, 5000) == up(5000 * 88) + up(4000)
    assert ws(3, 1 << 40) == up((1 << 40) * 88) + 256
    assert ws(-1, 4) == 0 and ws(4, -1) == 0 and ws(4, (1 << 40) + 1) == 0


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
A, OFF, DEPTH, TOFF, LOSS, CNT, G, ST, WS = (k << 20 for k in range(1, 10))


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    need = L.mfcd_list_pl_workspace_bytes(4, 6)

    def call(a=A, entries=100, row_off=OFF, depth=DEPTH, rows=4, tile_off=TOFF, n_tiles=6, what=3, loss=LOSS, counts=CNT,
             g=G, status=ST, workspace=WS, workspace_bytes=need):
        return L.mfcd_list_pl(a, entries, row_off, depth, rows, tile_off, n_tiles, what, loss, counts, g, status, workspace,
                              workspace_bytes, None)

    assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(n_tiles=-1) == -1
    assert call(n_tiles=(1 << 40) + 1, workspace_bytes=1 << 62) == -1
    assert call(row_off=None) == -1 and call(tile_off=None) == -1 and call(status=None) == -1 and call(a=None) == -1
    assert call(what=0) == -1 and call(what=4) == -1 and call(what=-1) == -1
    assert call(loss=None) == -1 and call(counts=None) == -1 and call(what=1, loss=None) == -1
    assert call(what=1, counts=None) == -1 and call(g=None) == -1 and call(what=2, g=None) == -1
    assert call(g=A) == -1 and call(what=2, g=A) == -1
    assert call(workspace=None) == -1
    assert call(workspace_bytes=need - 1) == -2 and call(workspace_bytes=0) == -2
    # nothing to launch: what an output the call does not ask for holds is not looked at
    assert call(rows=0) == 0 and call(rows=0, entries=0, a=None, g=None, what=2, workspace=None, workspace_bytes=0) == 0
    assert call(rows=0, what=1, g=None) == 0 and call(rows=0, what=2, loss=None, counts=None) == 0
    assert call(rows=0, depth=None) == 0


def _example():
    #          user 2: items 5 > 1 > 7        user 0: items 3 > 4          user 3: item 2
    users = [2, 0, 2, 2, 0, 3]
    items = [1, 4, 5, 7, 3, 2]
    positions = [20, 9, 10, 30, 2, 0]
    return users, items, positions


def test_ranked_lists_sort_validate_and_transpose():
    from mfcd.lists import RankedLists
    users, items, positions = _example()
    R = RankedLists(users, items, positions, 4, 8)
    assert R.entries == 6 and R.n == 4 and R.m == 8 and R.stages == 1 + 2 and R.device.type == "cpu"
    assert R.row_off.tolist() == [0, 2, 2, 5, 6] and R.item.tolist() == [3, 4, 5, 1, 7, 2]
    assert R.user.tolist() == [0, 0, 2, 2, 2, 3] and R.position.tolist() == [2, 9, 10, 20, 30, 0]
    assert R.depth.tolist() == [2, 0, 3, 1] and R.depth.dtype == torch.int32 and R.item.dtype == torch.int32
    assert R.lengths.tolist() == [2, 0, 3, 1] and R.user_stages.tolist() == [1, 0, 2, 0]
    assert R.tile_off.tolist() == [0, 1, 1, 2, 3] and R.n_tiles == 3 and R.seg_off.tolist() == [0, 1, 1, 2, 3]
    # the transposition: position p of the by-(item, user) order is CSR entry col_perm[p], of user col_user[p]
    assert R.col_off.tolist() == [0, 0, 1, 2, 3, 4, 5, 5, 6] and R.col_perm.tolist() == [3, 5, 0, 1, 2, 4]
    assert R.col_user.tolist() == [2, 3, 0, 0, 2, 2] and R.col_seg_off.tolist() == [0, 0, 1, 2, 3, 4, 5, 5, 6]
    assert R.item[R.col_perm].tolist() == sorted(R.item.tolist())
    # the ranked entries as a layout of the pair statistics
    assert R.rank_off.tolist() == [0, 2, 2, 5, 6] and R.rank_idx.tolist() == [0, 1, 2, 3, 4, 5]
    assert R.rank_value.tolist() == [0.0, -1.0, 0.0, -1.0, -2.0, 0.0]
    K = RankedLists(users, items, positions, 4, 8, depth=1)
    assert K.depth.tolist() == [1, 0, 1, 1] and K.stages == 2 and K.rank_idx.tolist() == [0, 2, 5]
    assert K.rank_off.tolist() == [0, 1, 1, 2, 3] and K.item.tolist() == R.item.tolist()
    D = RankedLists(users, items, positions, 4, 8, depth=[2, 0, 0, 1])
    assert D.user_stages.tolist() == [1, 0, 0, 0] and D.stages == 1
    T = RankedLists(torch.tensor(users), torch.tensor(items), torch.tensor(positions), 4, 8)
    assert T.item.tolist() == R.item.tolist() and T.to("cpu") is T
    E = RankedLists([], [], [], 3, 2)
    assert E.entries == 0 and E.stages == 0 and E.row_off.tolist() == [0, 0, 0, 0] and E.n_tiles == 0
    with pytest.raises(ValueError):
        RankedLists([0, 0], [1, 1], [0, 1], 2, 3)                        # an item twice in a list
    with pytest.raises(ValueError):
        RankedLists([0, 0], [1, 2], [5, 5], 2, 3)                        # a position twice in a list
    with pytest.raises(ValueError):
        RankedLists([0, 0], [1, 2], [5], 2, 3)
    with pytest.raises(ValueError):
        RankedLists(users, items, positions, 4, 8, depth=[3, 0, 3, 1])   # deeper than the list
    with pytest.raises(ValueError):
        RankedLists(users, items, positions, 4, 8, depth=-1)
    for bad_u, bad_i in (([4], [0]), ([-1], [0]), ([0], [8]), ([0], [-1])):
        with pytest.raises(IndexError):
            RankedLists(bad_u, bad_i, [0], 4, 8)


def test_split_covers_every_entry_once_and_keeps_the_order():
    from mfcd.lists import RankedLists
    rng = np.random.default_rng(3)
    n, m = 30, 50
    users, items, positions = [], [], []
    for u in range(n):
        L = int(rng.integers(0, 41))
        users += [u] * L
        items += rng.choice(m, L, replace=False).tolist()
        positions += (rng.permutation(L) * 3).tolist()
    R = RankedLists(users, items, positions, n, m)
    parts = R.split([0.8, 0.2], seed=5)
    assert [p.n for p in parts] == [n, n] and sum(p.entries for p in parts) == R.entries
    seen = sorted((int(u), int(i), int(p)) for part in parts for u, i, p in zip(part.user, part.item, part.position))
    assert seen == sorted(zip(users, items, positions))
    for part in parts:
        assert (part.depth.numpy() == part.lengths).all()               # a part of a fully ranked list is fully ranked
        for u in range(n):
            b, e = int(part.row_off[u]), int(part.row_off[u + 1])
            pos = part.position[b:e].tolist()
            assert pos == sorted(pos)
            full = R.item[int(R.row_off[u]):int(R.row_off[u + 1])].tolist()
            mine = part.item[b:e].tolist()
            assert mine == [i for i in full if i in set(mine)]           # the list's order, restricted
    assert (parts[1].lengths == R.lengths - np.floor(0.8 * R.lengths + 1e-9).astype(np.int64)).all()
    again = R.split([0.8, 0.2], seed=5)
    assert all(torch.equal(x.item, y.item) for x, y in zip(parts, again))
    assert not torch.equal(R.split([0.8, 0.2], seed=6)[0].item, parts[0].item)
    # a top-K list: a part ranks those of its entries the list ranked
    K = RankedLists(users, items, positions, n, m, depth=5)
    for part in K.split([0.5, 0.5], seed=1):
        for u in range(n):
            top = set(K.item[int(K.row_off[u]):int(K.row_off[u]) + int(K.depth[u])].tolist())
            b, e, d = int(part.row_off[u]), int(part.row_off[u + 1]), int(part.depth[u])
            assert set(part.item[b:b + d].tolist()) == top & set(part.item[b:e].tolist())
    with pytest.raises(ValueError):
        R.split([0.5, 0.6])


def test_sample_rankings_without_noise_is_the_exact_order():
    from mfcd.lists import sample_rankings
    gen = torch.Generator().manual_seed(1)
    X = torch.randn(20, 30, generator=gen)
    state = torch.get_rng_state()
    np_state = np.random.get_state()[1].copy()
    R = sample_rankings(X, 12, s=float("inf"), seed=4)
    assert torch.equal(torch.get_rng_state(), state) and (np.random.get_state()[1] == np_state).all()
    assert R.entries == 20 * 12 and (R.lengths == 12).all() and R.stages == 20 * 11
    shown = set()
    for u in range(20):
        it = R.item[12 * u:12 * u + 12].long()
        x = X[u, it]
        assert (x[:-1] >= x[1:]).all() and len(set(it.tolist())) == 12
        shown.add(tuple(sorted(it.tolist())))
    assert len(shown) > 15                                               # the users see different slates
    same = sample_rankings(X, 12, s=float("inf"), seed=4)
    assert torch.equal(same.item, R.item)
    assert not torch.equal(sample_rankings(X, 12, s=float("inf"), seed=5).item, R.item)
    top = sample_rankings(X, 12, depth=3, s=2.0, seed=4, users=[3, 7])
    assert top.depth.tolist() == [0, 0, 0, 3, 0, 0, 0, 3] + [0] * 12 and top.entries == 24 and top.stages == 6
    full = sample_rankings(X, 30, s=float("inf"))
    assert all(torch.equal(full.item[30 * u:30 * u + 30].long(), X[u].argsort(descending=True, stable=True)) for u in range(20))


def test_sample_rankings_draws_from_the_plackett_luce_law():
    from mfcd.lists import sample_rankings
    x = np.array([0.4, -0.3, 1.1])
    s, users = 1.5, 60000
    R = sample_rankings(torch.tensor(x, dtype=torch.float32).expand(users, 3), 3, s=s, seed=7)
    order = R.item.reshape(users, 3).numpy()
    w = np.exp(s * x.astype(np.float32).astype(np.float64))
    chi2 = 0.0
    for p in itertools.permutations(range(3)):
        prob = w[p[0]] / w.sum() * w[p[1]] / (w[p[1]] + w[p[2]])
        seen = int((order == np.array(p)).all(1).sum())
        chi2 += (seen - users * prob) ** 2 / (users * prob)
    assert chi2 < 35.89                                                  # the 1 - 1e-6 quantile of chi^2 with 5 degrees


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, lists
    R = lists.RankedLists(*_example(), 4, 8)
    U, V = torch.randn(4, 2), torch.randn(8, 2)
    model = St.MatrixFactorization(4, 8, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    for call in (lambda: lists.list_scores(U, V, R), lambda: lists.pl_rows(torch.randn(6), R),
                 lambda: lists.pl_risk(U, V, R), lambda: lists.pl_metrics(U, V, R),
                 lambda: lists.fit_lists((model, opt), R, 2)):
        with pytest.raises(_lib.MfcdError):
            call()
    for call in (lambda: St.rankings_risk(model, R), lambda: St.compute_rankings_metrics(model, R),
                 lambda: St.train_model_rankings(model, R, opt, "cpu", num_steps=1)):
        with pytest.raises(RuntimeError):
            call()
    fit = inspect.getsource(lists.fit_lists)
    assert "pl_rows(" in fit and "mfcd_adam_dense(" in fit and "logcumsumexp" not in inspect.getsource(lists)


def test_load_rankings_and_public_signatures(tmp_path):
    import structure as St
    from mfcd import lists
    path = tmp_path / "lists.txt"
    path.write_text("10 7 2\n10 5 1\n30 7 1\n30 9 3\n30 5 2\n")
    R, user_ids, item_ids = St.load_rankings(str(path))
    assert user_ids.tolist() == [10, 30] and item_ids.tolist() == [5, 7, 9]
    assert R.row_off.tolist() == [0, 2, 5] and R.item.tolist() == [0, 1, 1, 0, 2] and R.stages == 3

    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(lists.RankedLists.__init__)[1:] == [("users", E), ("items", E), ("positions", E), ("n", E), ("m", E),
                                                   ("depth", None)]
    assert sig(lists.pl_rows) == [("a", E), ("lists", E), ("what", "both")]
    assert sig(lists.pl_risk) == [("U", E), ("V", E), ("lists", E)] == sig(lists.pl_metrics) == sig(lists.list_scores)
    assert sig(lists.fit_lists) == [("binding", E), ("lists", E), ("steps", E), ("log_every", 0)]
    assert sig(lists.sample_rankings) == [("X", E), ("length", E), ("depth", None), ("s", 1.0), ("seed", 0), ("users", None)]
    assert sig(St.observe_rankings) == [("X", E), ("length", E), ("depth", None), ("s", 1.0), ("seed", 0)]
    assert sig(St.load_rankings)[:1] == [("path", E)]
    assert sig(St.rankings_risk) == [("model", E), ("lists", E)] == sig(St.compute_rankings_metrics)
    assert sig(St.train_model_rankings) == [("model", E), ("lists", E), ("optimizer", E), ("device", E), ("num_steps", 1000),
                                            ("log_every", 100)]
    for fn in (St.observe_rankings, St.load_rankings, St.rankings_risk, St.train_model_rankings, St.compute_rankings_metrics):
        assert "Extension (not in the reference)" in fn.__doc__ and "Not part of the result dict / .pkl" in fn.__doc__
    for bad in (lambda: lists.sample_rankings(torch.zeros(3), 1), lambda: lists.sample_rankings(torch.zeros(3, 4), 5),
                lambda: lists.sample_rankings(torch.zeros(3, 4), 2, s=-1.0)):
        with pytest.raises(ValueError):
            bad()
