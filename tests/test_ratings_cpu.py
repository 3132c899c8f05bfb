"""CPU-only checks of the ragged entries and what is built on them (include/mfcd.h: mfcd_pair_ragged_stats,
mfcd_pair_ragged_grad, mfcd_ragged_dot, mfcd_ragged_gather_sum; mfcd/ratings.py; structure.observe_ratings, load_ratings,
ratings_risk, train_model_ratings, compute_ratings_metrics): the entries are declared and bound, bad arguments are refused
before the device is touched, there is no CPU fallback, the host side of RatingsData is right, and the CPU model the GPU
tests compare with (tests/ratings_model.py) is consistent with itself."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ratings_model as RM
from conftest import ROOT

ENTRIES = {"mfcd_pair_ragged_tile": 0, "mfcd_pair_ragged_workspace_bytes": 2, "mfcd_pair_ragged_stats": 16,
           "mfcd_pair_ragged_grad": 12, "mfcd_ragged_dot": 12, "mfcd_ragged_segment": 0,
           "mfcd_ragged_gather_sum_workspace_bytes": 3, "mfcd_ragged_gather_sum": 16}


def test_ragged_entries_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\b%s\(([^)]*)\);" % name, header).group(1)
        assert (0 if decl.strip() == "void" else len(decl.split(","))) == nargs, name
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header) and re.search(r"#define MFCD_RAGGED_SKIP_TIES 1\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4
    assert L.mfcd_pair_ragged_tile() == 256 and L.mfcd_ragged_segment() == 256
    makefile = open(os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc", "Makefile")).read()
    assert " pair_ragged.hip" in makefile and " ragged.hip" in makefile


P, Q, R, S, T, W = 4096, 8192, 12288, 16384, 20480, 24576   # non-null addresses that are never dereferenced


def test_pair_ragged_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()

    def stats(a=P, x=Q, entries=8, row_off=R, rows=2, tile_off=S, n_tiles=2, scale=1.0, flags=0, what=3, counts=T, sums=W,
              status=T + 4096, ws=W + 4096, ws_bytes=1 << 20):
        return L.mfcd_pair_ragged_stats(a, x, entries, row_off, rows, tile_off, n_tiles, scale, flags, what, counts, sums,
                                        status, ws, ws_bytes, None)

    def grad(a=P, x=Q, entries=8, row_off=R, rows=2, tile_off=S, n_tiles=2, scale=1.0, flags=0, g=T, status=W):
        return L.mfcd_pair_ragged_grad(a, x, entries, row_off, rows, tile_off, n_tiles, scale, flags, g, status, None)

    for call in (stats, grad):
        assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(n_tiles=-1) == -1
        assert call(a=None) == -1 and call(x=None) == -1 and call(row_off=None) == -1 and call(tile_off=None) == -1
        assert call(status=None) == -1
        assert call(scale=float("inf")) == -1 and call(scale=float("nan")) == -1 and call(scale=1e300) == -1
        assert call(flags=2) == -1 and call(flags=-1) == -1
        assert call(rows=0) == 0                        # nothing to do, nothing launched
        assert call(rows=0, flags=2) == -1              # and a bad call stays bad with no rows
    assert stats(what=0) == -1 and stats(what=4) == -1
    assert stats(counts=None) == -1 and stats(sums=None) == -1
    assert stats(what=1, sums=None, rows=0) == 0 and stats(what=2, counts=None, rows=0) == 0
    assert stats(ws=None) == -1 and stats(ws_bytes=16) == -2
    assert grad(g=None) == -1 and grad(g=P) == -1 and grad(g=Q) == -1     # g missing, g == a, g == x
    assert L.mfcd_pair_ragged_workspace_bytes(2, 3) == 256 and L.mfcd_pair_ragged_workspace_bytes(-1, 3) == 0
    assert L.mfcd_pair_ragged_workspace_bytes(2, 1000) == -(-80 * 1000 // 256) * 256


def test_table_kernels_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()

    def dot(Rt=P, n_r=4, C=Q, n_c=5, d=3, entries=8, row_off=R, rows=4, idx=S, a=T, status=W):
        return L.mfcd_ragged_dot(Rt, n_r, C, n_c, d, entries, row_off, rows, idx, a, status, None)

    assert dot(Rt=None) == -1 and dot(C=None) == -1 and dot(row_off=None) == -1 and dot(idx=None) == -1
    assert dot(a=None) == -1 and dot(status=None) == -1
    assert dot(d=0) == -1 and dot(d=257) == -1 and dot(n_r=0) == -1 and dot(n_c=0) == -1 and dot(entries=-1) == -1
    assert dot(rows=-1) == -1 and dot(rows=5) == -1          # more rows than R has
    assert dot(a=P) == -1 and dot(a=Q) == -1
    assert dot(rows=0) == 0 and dot(rows=0, d=0) == -1

    def gs(Tt=P, t_rows=5, d=3, entries=8, row_off=R, rows=4, idx=S, coef=Q, perm=None, seg_off=T, n_seg=4, out=W,
           status=W + 4096, ws=W + 8192, ws_bytes=1 << 20):
        return L.mfcd_ragged_gather_sum(Tt, t_rows, d, entries, row_off, rows, idx, coef, perm, seg_off, n_seg, out, status,
                                        ws, ws_bytes, None)

    assert gs(Tt=None) == -1 and gs(row_off=None) == -1 and gs(idx=None) == -1 and gs(coef=None) == -1
    assert gs(seg_off=None) == -1 and gs(out=None) == -1 and gs(status=None) == -1
    assert gs(d=0) == -1 and gs(d=257) == -1 and gs(t_rows=0) == -1 and gs(entries=-1) == -1 and gs(rows=-1) == -1
    assert gs(n_seg=-1) == -1 and gs(n_seg=(1 << 31) + 1) == -1
    assert gs(out=P) == -1 and gs(out=Q) == -1               # out == T, out == coef
    assert gs(ws=None) == -1 and gs(ws_bytes=16) == -2
    assert gs(rows=0) == 0 and gs(rows=0, d=0) == -1
    assert L.mfcd_ragged_gather_sum_workspace_bytes(4, 3, 4) == 256 + 256 + 256
    assert L.mfcd_ragged_gather_sum_workspace_bytes(4, 257, 4) == 0


def _small_data():
    from mfcd import ratings
    users = [2, 0, 2, 0, 3, 2]
    items = [1, 4, 0, 2, 3, 3]
    values = [5.0, 1.0, 3.0, 1.0, 2.0, 3.0]
    return ratings.RatingsData(users, items, values, 4, 5)


def test_ratings_have_no_cpu_fallback():
    import structure as S
    from mfcd import _lib, ratings
    data = _small_data()
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    a = torch.randn(data.entries)
    for call in (lambda: ratings.ragged_scores(U, V, data), lambda: ratings.pair_ragged_stats(a, data),
                 lambda: ratings.pair_ragged_grad(a, data), lambda: ratings.ragged_gather_sum(a, data, V, "user"),
                 lambda: ratings.ratings_risk(U, V, data), lambda: ratings.pair_ragged_grad(a.double(), data)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = S.MatrixFactorization(4, 5, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    with pytest.raises(_lib.MfcdError):
        ratings.fit_ratings((model, opt), data, 1.0, 2)
    with pytest.raises(RuntimeError):
        S.ratings_risk(model, data)
    with pytest.raises(RuntimeError):
        S.compute_ratings_metrics(model, data)
    with pytest.raises(RuntimeError):
        S.train_model_ratings(model, data, 1.0, opt, "cpu", num_steps=2)


def test_ratings_public_signatures():
    import structure as S
    from mfcd import ratings

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(ratings.RatingsData.__init__)[1:] == ["users", "items", "values", "n", "m"]
    assert names(ratings.ragged_scores) == ["U", "V", "data"]
    assert names(ratings.pair_ragged_stats) == ["a", "data", "scale", "what", "skip_ties"]
    assert defaults(ratings.pair_ragged_stats) == {"scale": 1.0, "what": "both", "skip_ties": False}
    assert names(ratings.pair_ragged_grad) == ["a", "data", "scale", "skip_ties"]
    assert defaults(ratings.pair_ragged_grad) == {"scale": 1.0, "skip_ties": False}
    assert names(ratings.ragged_gather_sum) == ["coef", "data", "table", "side"]
    assert names(ratings.ratings_risk) == ["U", "V", "data", "s", "skip_ties"]
    assert names(ratings.ratings_metrics) == ["U", "V", "data", "s", "skip_ties"]
    assert names(ratings.fit_ratings) == ["binding", "data", "s", "steps", "log_every", "skip_ties"]
    assert defaults(ratings.fit_ratings) == {"log_every": 0, "skip_ties": False}
    assert names(S.observe_ratings) == ["X", "p", "levels", "seed"] and defaults(S.observe_ratings) == {"levels": None, "seed": 0}
    assert names(S.load_ratings) == ["path", "sep"] and defaults(S.load_ratings) == {"sep": None}
    assert names(S.ratings_risk) == ["model", "data", "s", "skip_ties"]
    assert names(S.train_model_ratings) == ["model", "data", "s", "optimizer", "device", "num_steps", "log_every", "skip_ties"]
    assert defaults(S.train_model_ratings) == {"num_steps": 1000, "log_every": 100, "skip_ties": False}
    assert names(S.compute_ratings_metrics) == ["model", "data", "s", "skip_ties"]
    for fn in (S.observe_ratings, S.load_ratings, S.ratings_risk, S.train_model_ratings, S.compute_ratings_metrics):
        assert fn.__doc__.startswith("Extension (not in the reference)")
    assert not any("rating" in k for k in S._RESULT_KEYS)


@pytest.mark.parametrize("skip_ties", [False, True])
@pytest.mark.parametrize("scale", [0.7, 4.0])
def test_model_gradient_is_the_derivative_of_the_models_risk(scale, skip_ties):
    """Central differences of the model's risk in f64, h = 1e-6, bound 1e-6, as test_pair_grad_cpu.py argues it
    (truncation ~1e-12, rounding of the difference ~1e-7 at 37 entries).  x holds ratings 1..5, so ties are heavy."""
    m, h = 37, 1e-6
    rng = np.random.default_rng(41)
    a, x = rng.uniform(-3, 3, m), rng.integers(1, 6, m).astype(np.float64)
    g = RM.row_grad(a, x, scale, skip_ties)
    fd = np.empty(m)
    for i in range(m):
        e = np.zeros(m)
        e[i] = h
        fd[i] = (RM.row_sums(a + e, x, scale, skip_ties)[0] - RM.row_sums(a - e, x, scale, skip_ties)[0]) / (2 * h)
    print(f"scale {scale} skip_ties {skip_ties}: max |g - central difference| = {np.abs(g - fd).max():.2e}")
    assert np.abs(g - fd).max() <= 1e-6
    assert abs(g.sum()) <= 1e-12 * m * m
    # the skip-ties forms against the definition written out over the pairs with different values
    i, j = np.triu_indices(m, k=1)
    keep = x[i] != x[j]
    assert RM.row_support(x, True) == int(keep.sum()) and RM.row_support(x, False) == m * (m - 1) // 2
    t = scale * (x[i] - x[j])
    direct = (RM.M.softplus(a[i] - a[j]) - RM.M.sigmoid(t) * (a[i] - a[j]))[keep].sum()
    np.testing.assert_allclose(RM.row_sums(a, x, scale, True)[0], direct, rtol=1e-12)
    assert np.isnan(RM.row_grad([1.0, np.inf, 0.0], [0.0, 1.0, 1.0], scale, skip_ties)).all()
    assert RM.row_grad([1.5], [0.5], scale, skip_ties).tolist() == [0.0]


def test_model_table_gradients_dot_and_gather_sum():
    rng = np.random.default_rng(5)
    data = _small_data()
    row_off, item, value = data.row_off.numpy(), data.item.numpy().astype(np.int64), data.value.numpy()
    U, V = rng.normal(size=(4, 2)), rng.normal(size=(5, 2))
    for skip in (False, True):
        dU, dV, g = RM.ratings_grad(U, V, row_off, item, value, 0.7, skip)
        h = 1e-6
        for Tb, dT in ((U, dU), (V, dV)):
            for idx in [(0, 0), (2, 1), (Tb.shape[0] - 1, 1)]:
                Pl, Mi = Tb.copy(), Tb.copy()
                Pl[idx] += h
                Mi[idx] -= h
                args = ((Pl, V), (Mi, V)) if Tb is U else ((U, Pl), (U, Mi))
                fd = (RM.ratings_risk(*args[0], row_off, item, value, 0.7, skip) -
                      RM.ratings_risk(*args[1], row_off, item, value, 0.7, skip)) / (2 * h)
                assert abs(fd - dT[idx]) <= 1e-8, (skip, idx, fd, dT[idx])
        # the item side through the transposition is the same dV
        dV2, _ = RM.gather_sum(U, data.col_off.numpy(), data.col_user.numpy().astype(np.int64), g, data.col_perm.numpy())
        c = 1.0 / data.support(skip)
        np.testing.assert_allclose(c * dV2, dV, rtol=1e-12, atol=1e-15)
    a, mag = RM.dot(U, V, row_off, item)
    np.testing.assert_allclose(a, (U[data.user.numpy()] * V[item]).sum(1), rtol=1e-14)
    assert (mag >= np.abs(a)).all()


def test_ratings_data_on_the_host():
    from mfcd import _lib, ratings
    L = _lib.load()
    tile, seg = L.mfcd_pair_ragged_tile(), L.mfcd_ragged_segment()
    rng = np.random.default_rng(7)
    n, m = 9, 700
    lengths = np.array([0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 3, 5, 0])
    users = np.repeat(np.arange(n), lengths)
    items = np.concatenate([rng.permutation(m)[:k] for k in lengths])
    values = rng.integers(1, 6, users.size).astype(np.float32)
    shuffle = rng.permutation(users.size)
    data = ratings.RatingsData(torch.from_numpy(users[shuffle]), items[shuffle], values[shuffle], n, m)
    u, i, v = data.user.numpy(), data.item.numpy(), data.value.numpy()
    assert data.n == n and data.m == m and data.entries == users.size
    assert data.user.dtype == torch.int32 and data.item.dtype == torch.int32 and data.value.dtype == torch.float32
    assert data.row_off.dtype == torch.int64 and data.col_off.dtype == torch.int64 and data.col_perm.dtype == torch.int64
    key = u.astype(np.int64) * m + i
    assert (np.diff(key) > 0).all()                            # sorted by (user, item), no repeat
    want = {(a, b): c for a, b, c in zip(users, items, values)}
    assert {(a, b): c for a, b, c in zip(u, i, v)} == want
    assert data.row_off.numpy().tolist() == np.concatenate(([0], np.cumsum(lengths))).tolist()
    assert data.lengths.tolist() == lengths.tolist()
    assert data.pairs == int((lengths * (lengths - 1) // 2).sum())
    assert data.tied_pairs == sum(int((v[s][:, None] == v[s][None, :]).sum() - (s.stop - s.start)) // 2
                                  for s in RM.rows_of(data.row_off.numpy()))
    assert data.support(False) == data.pairs and data.support(True) == data.pairs - data.tied_pairs
    assert data.tile_off.numpy().tolist() == np.concatenate(([0], np.cumsum([-(-k // tile) for k in lengths]))).tolist()
    assert data.seg_off.numpy().tolist() == np.concatenate(([0], np.cumsum([-(-k // seg) for k in lengths]))).tolist()
    assert data.n_tiles == int(data.tile_off[-1]) and data.n_seg == int(data.seg_off[-1])
    # the transposition: position p of the by-(item, user) order is CSR entry col_perm[p]
    perm, col_off, col_user = data.col_perm.numpy(), data.col_off.numpy(), data.col_user.numpy()
    assert sorted(perm.tolist()) == list(range(data.entries))
    assert (col_user == u[perm]).all()
    col_item = np.repeat(np.arange(m), np.diff(col_off))
    assert (col_item == i[perm]).all()
    assert (np.diff(col_item.astype(np.int64) * n + col_user) > 0).all()
    per_item = np.bincount(items, minlength=m)
    assert np.diff(col_off).tolist() == per_item.tolist()
    assert data.col_seg_off.numpy().tolist() == np.concatenate(([0], np.cumsum(-(-per_item // seg)))).tolist()
    assert data.col_n_seg == int(data.col_seg_off[-1])
    assert data.to("cpu") is data and data.device.type == "cpu"
    # errors
    with pytest.raises(ValueError):
        ratings.RatingsData([0, 1, 0], [2, 2, 2], [1.0, 2.0, 3.0], 2, 3)
    with pytest.raises(IndexError):
        ratings.RatingsData([0, 2], [0, 1], [1.0, 2.0], 2, 3)
    with pytest.raises(IndexError):
        ratings.RatingsData([0, 1], [0, 3], [1.0, 2.0], 2, 3)
    with pytest.raises(IndexError):
        ratings.RatingsData([0, -1], [0, 1], [1.0, 2.0], 2, 3)
    with pytest.raises(ValueError):
        ratings.RatingsData([0, 1], [0], [1.0, 2.0], 2, 3)
    zeros = ratings.RatingsData([0, 0, 0], [0, 1, 2], [0.0, -0.0, 1.0], 1, 3)
    assert zeros.pairs == 3 and zeros.tied_pairs == 1           # -0.0 equals +0.0
    empty = ratings.RatingsData([], [], [], 3, 4)
    assert empty.entries == 0 and empty.pairs == 0 and empty.n_tiles == 0 and empty.row_off.tolist() == [0, 0, 0, 0]


def test_split_covers_every_entry_once_and_is_reproducible():
    from mfcd import ratings
    rng = np.random.default_rng(11)
    n, m = 30, 50
    keep = rng.random((n, m)) < 0.4
    users, items = np.nonzero(keep)
    data = ratings.RatingsData(users, items, rng.normal(size=users.size), n, m)
    state = np.random.get_state()
    parts = data.split((0.8, 0.2), seed=3)
    again = data.split((0.8, 0.2), seed=3)
    other = data.split((0.8, 0.2), seed=4)
    after = np.random.get_state()
    assert state[0] == after[0] and (state[1] == after[1]).all() and state[2:] == after[2:]   # the global RNG is not used
    assert len(parts) == 2 and all(p.n == n and p.m == m for p in parts)

    def entries(d):
        return list(zip(d.user.tolist(), d.item.tolist(), d.value.tolist()))

    assert sorted(entries(parts[0]) + entries(parts[1])) == entries(data)
    assert entries(parts[0]) == entries(again[0]) and entries(parts[1]) == entries(again[1])
    assert entries(parts[0]) != entries(other[0])
    assert (parts[0].lengths == np.floor(0.8 * data.lengths + 1e-9).astype(np.int64)).all()
    assert (parts[0].lengths + parts[1].lengths == data.lengths).all()
    three = data.split((0.5, 0.25, 0.25), seed=0)
    assert sorted(sum((entries(p) for p in three), [])) == entries(data)
    with pytest.raises(ValueError):
        data.split((0.5, 0.4))


def test_observe_ratings_is_private_reproducible_and_quantised():
    import structure as S
    gen = torch.Generator().manual_seed(9)
    X = torch.randn(40, 60, generator=gen)
    torch.manual_seed(123)
    np.random.seed(123)
    t_state, n_state = torch.get_rng_state(), np.random.get_state()
    data = S.observe_ratings(X, 0.5, seed=2)
    again = S.observe_ratings(X, 0.5, seed=2)
    other = S.observe_ratings(X, 0.5, seed=3)
    levels = S.observe_ratings(X, 0.5, levels=5, seed=2)
    assert torch.equal(torch.get_rng_state(), t_state)
    n_after = np.random.get_state()
    assert n_state[0] == n_after[0] and (n_state[1] == n_after[1]).all() and n_state[2:] == n_after[2:]
    assert data.n == 40 and data.m == 60 and 0.4 * 2400 < data.entries < 0.6 * 2400
    assert torch.equal(data.user, again.user) and torch.equal(data.item, again.item) and torch.equal(data.value, again.value)
    assert not (data.entries == other.entries and torch.equal(data.item, other.item))
    assert torch.equal(data.value, X[data.user.long(), data.item.long()])
    assert torch.equal(levels.user, data.user) and torch.equal(levels.item, data.item)
    assert sorted(set(levels.value.tolist())) == [1.0, 2.0, 3.0, 4.0, 5.0]          # exactly k distinct values
    order = np.argsort(data.value.numpy(), kind="stable")
    assert (np.diff(levels.value.numpy()[order]) >= 0).all()                        # monotone in the kept value
    counts = np.bincount(levels.value.numpy().astype(np.int64))[1:]
    assert counts.max() - counts.min() <= 2                                         # cut at the quantiles
    full = S.observe_ratings(X, 1.0)
    assert full.entries == 2400 and torch.equal(full.value.reshape(40, 60), X)
    assert S.observe_ratings(X, 0.0).entries == 0


def test_load_ratings_reads_a_text_table(tmp_path):
    import structure as S
    path = tmp_path / "u.data"
    path.write_text("196\t242\t3\t881250949\n186\t302\t3\t891717742\n22\t377\t1\t878887116\n196\t302\t5\t0\n22\t242\t4\t1\n")
    data, user_ids, item_ids = S.load_ratings(str(path))
    assert user_ids.tolist() == [22, 186, 196] and item_ids.tolist() == [242, 302, 377]
    assert data.n == 3 and data.m == 3 and data.entries == 5 and data.device.type == "cpu"
    got = {(int(user_ids[u]), int(item_ids[i])): v for u, i, v in zip(data.user.tolist(), data.item.tolist(), data.value.tolist())}
    assert got == {(196, 242): 3.0, (186, 302): 3.0, (22, 377): 1.0, (196, 302): 5.0, (22, 242): 4.0}
    comma = tmp_path / "r.csv"
    comma.write_text("7,9,2.5\n7,8,0.5\n")
    data, user_ids, item_ids = S.load_ratings(str(comma), sep=",")
    assert user_ids.tolist() == [7] and item_ids.tolist() == [8, 9] and data.value.tolist() == [0.5, 2.5]
