"""GPU tests of the per-user D-optimal comparison design (mfcd/design.py: user_design, informative_pairs;
structure.optimal_design, strategy_efficiency, informative_pairs) against brute force in float64 (tests/design_model.py).

Problems: (n = 6, m = 40, d = 3), (n = 4, m = T + 5, d = 2) with T = pairs.BEST_TILE, and (n = 3, m = 65, d = 8); item
vectors standard normal, truth 1.5 N(0, 1), s = 1, max_iter = 300, gtol = 1e-3.  The fits are made once per module.

The KKT check is brute force over all pairs at the returned `info`: max_p g_p <= tr(P M) + gtol d + bound.  The bound is
what the kernel's fp32 arg-max can miss: the design takes the pair the kernel names and re-evaluates it in f64, and the
kernel's choice is within 2 max E of the best (tests/test_pair_best.py), E the kernel's tolerance on the table
G = (B - mean) L it was given."""
import functools

import numpy as np
import pytest
import torch

import design_model as DM
import pair_best_model as BM
import pair_law_model as LM

pytestmark = pytest.mark.gpu

GTOL, MAX_ITER = 1e-3, 300


def _tile():
    from mfcd import pairs
    return pairs.BEST_TILE


CASES = {"m40_d3": (6, 40, 3), "tile_d2": (4, _tile() + 5, 2), "m65_d8": (3, 65, 8)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def problem(name, offset=0.0):
    n, m, d = CASES[name]
    rng = np.random.default_rng(900 + m + d)
    V = (rng.standard_normal((m, d)) + offset).astype(np.float32)
    X = (1.5 * rng.standard_normal((n, m))).astype(np.float32)
    return V, X


_fits = {}


def fit(dev, name, offset=0.0, **kw):
    """(UserDesign on the host as numpy, the device's start measure [n, d, d])."""
    from mfcd import design, pairs
    key = (name, offset, tuple(sorted(kw.items())))
    if key not in _fits:
        V, X = problem(name, offset)
        U = torch.zeros((X.shape[0], V.shape[1]), device=dev)
        Vd, Xd = torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev)
        res = design.user_design(U, Vd, Xd, 1.0, max_iter=MAX_ITER, gtol=GTOL, **kw)
        start = pairs.user_information(U, Vd, Xd, 1.0, at="truth")
        _fits[key] = (design.UserDesign(*(t.cpu().numpy() for t in res)), (start.info / start.weight[:, None, None]).cpu().numpy())
    return _fits[key]


def kernel_slack(a, B, info, M0=0.0):
    """2 max E of the kernel's table at P = (M0 + info)^-1."""
    C = M0 + info
    L = np.linalg.inv(np.linalg.cholesky(C)).T
    G = ((B - B.mean(axis=0)) @ L).astype(np.float32)
    return 2.0 * BM.scores(a, G)[1].max()


@pytest.mark.parametrize("name", list(CASES))
def test_design_is_certified_and_consistent(dev, name):
    n, m, d = CASES[name]
    V, X = problem(name)
    res, start = fit(dev, name)
    assert res.pairs.dtype == np.int32 and res.pairs.shape[:1] == (n,) and res.pairs.shape[2] == 2
    assert res.weights.shape == res.pairs.shape[:2] and res.info.shape == (n, d, d)
    print(f"{name}: iters {res.iters.tolist()}, gap {res.gap.tolist()}, atoms {(res.weights > 0).sum(1).tolist()}, "
          f"rest {res.rest.tolist()}, uniform D-efficiency {np.exp((res.logdet_start - res.logdet) / d).tolist()}")
    assert (res.status == 0).all() and (res.gap <= GTOL * d).all() and (res.iters <= MAX_ITER).all()
    B = V.astype(np.float64)
    for u in range(n):
        a = X[u].astype(np.float64)
        w, pr = res.weights[u], res.pairs[u]
        held = w > 0
        assert (w >= 0).all() and res.rest[u] >= 0 and abs(w.sum() + res.rest[u] - 1.0) <= 1e-12
        assert (pr[held, 0] < pr[held, 1]).all() and (pr[held] >= 0).all() and (pr[~held] == -1).all()
        assert len({tuple(p) for p in pr[held]}) == held.sum()
        S, D, adm, _ = DM.pair_terms(a, B)
        info = res.rest[u] * start[u]
        for (i, j), wq in zip(pr[held], w[held]):
            info = info + wq * S[i, j] * np.outer(D[i, j], D[i, j])
        assert np.abs(res.info[u] - info).max() <= 1e-12 * np.abs(info).max()
        g, tr = DM.kkt(a, B, res.info[u])
        slack = kernel_slack(a, B, res.info[u])
        assert g <= tr + GTOL * d + slack, f"user {u}: KKT gap {g - tr:.3e}, allowed {GTOL * d + slack:.3e}"
        assert abs((g - tr) - res.gap[u]) <= slack + 1e-9
        assert res.logdet[u] >= res.logdet_start[u]
        assert abs(res.logdet[u] - np.linalg.slogdet(res.info[u])[1]) <= 1e-9
        assert abs(res.logdet_start[u] - np.linalg.slogdet(start[u])[1]) <= 1e-9


def test_the_design_centres_the_table(dev):
    """An item table offset by 1000 (rounded to fp32: the entries sit on a grid of 6e-5) is certified by the same brute
    force on the offset table: without the f64 centring the fp32 table G would carry the offset into the kernel's
    cancellation and the arg-max would be noise."""
    name = "m40_d3"
    n, m, d = CASES[name]
    V, X = problem(name, 1000.0)
    assert np.abs(V).min() > 990
    res, _ = fit(dev, name, 1000.0)
    assert (res.status == 0).all()
    B = V.astype(np.float64)
    for u in range(n):
        a = X[u].astype(np.float64)
        g, tr = DM.kkt(a, B, res.info[u])
        assert g <= tr + GTOL * d + kernel_slack(a, B, res.info[u])


def test_one_dimension_takes_the_single_best_pair_exactly(dev):
    from mfcd import design
    rng = np.random.default_rng(77)
    n, m = 3, 30
    V = rng.standard_normal((m, 1)).astype(np.float32)
    X = (1.5 * rng.standard_normal((n, m))).astype(np.float32)
    res = design.user_design(torch.zeros((n, 1), device=dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev), 1.0,
                             max_iter=1)
    assert res.status.tolist() == [0] * n and res.iters.tolist() == [1] * n
    assert res.weights.cpu().tolist() == [[1.0]] * n and res.rest.cpu().tolist() == [0.0] * n
    for u in range(n):
        S64, E, adm = BM.scores(X[u], V)
        top = np.sort(S64[np.triu_indices(m, 1)])[-2:]
        assert top[1] - top[0] > 2 * E.max()                   # the data leave the fp32 kernel no doubt
        i, j = np.unravel_index(S64.argmax(), S64.shape)
        assert res.pairs[u, 0].cpu().tolist() == [min(i, j), max(i, j)]


def test_under_a_margin_law_every_atom_is_admissible(dev):
    from mfcd import design, pairs
    V, X = problem("m40_d3")
    n, m, d = CASES["m40_d3"]
    law = pairs.PairLaw(margin=1.25, device=dev)
    res = design.user_design(torch.zeros((n, d), device=dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev), 1.0, law,
                             max_iter=MAX_ITER)
    pr, w = res.pairs.cpu().numpy(), res.weights.cpu().numpy()
    assert (res.status.cpu().numpy() == 0).all() and ((w > 0).sum(1) >= 1).all()
    free, _ = fit(dev, "m40_d3")
    for u in range(n):
        wl = LM.weights(X[u], margin=1.25)
        assert all(wl[i, j] > 0 for i, j in pr[u][w[u] > 0])
        g, tr = DM.kkt(X[u].astype(np.float64), V.astype(np.float64), res.info[u].cpu().numpy(), wl)
        assert g <= tr + GTOL * d + kernel_slack(X[u].astype(np.float64), V.astype(np.float64), res.info[u].cpu().numpy())
        assert float(res.logdet[u]) <= free.logdet[u] + free.gap[u]      # fewer pairs cannot do better


def test_a_rank_deficient_table_needs_a_prior(dev):
    from mfcd import design
    rng = np.random.default_rng(12)
    n, m, d = 3, 40, 3
    V = rng.standard_normal((m, d)).astype(np.float32)
    V[:, 2] = 0.0
    X = (1.5 * rng.standard_normal((n, m))).astype(np.float32)
    U, Vd, Xd = torch.zeros((n, d), device=dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev)
    bare = design.user_design(U, Vd, Xd, 1.0, max_iter=MAX_ITER)
    assert bare.status.tolist() == [2] * n and bool(torch.isnan(bare.info).all()) and bool(torch.isnan(bare.gap).all())
    assert bare.iters.tolist() == [0] * n and bool((bare.pairs == -1).all()) and bool(torch.isnan(bare.logdet).all())
    mixed = design.user_design(U, Vd, Xd, 1.0, prior=0.1, max_iter=MAX_ITER)
    assert mixed.status.tolist() == [0] * n and bool((mixed.gap <= GTOL * d).all())
    tau = torch.eye(d, dtype=torch.float64, device=dev).expand(n, d, d) * 0.1
    same = design.user_design(U, Vd, Xd, 1.0, prior=tau, max_iter=MAX_ITER)
    assert torch.equal(same.info, mixed.info) and torch.equal(same.pairs, mixed.pairs)
    B = V.astype(np.float64)
    for u in range(n):
        g, tr = DM.kkt(X[u].astype(np.float64), B, mixed.info[u].cpu().numpy(), None, 0.1)
        assert g <= tr + GTOL * d + kernel_slack(X[u].astype(np.float64), B, mixed.info[u].cpu().numpy(), 0.1 * np.eye(d))
    stopped = design.user_design(U, Vd, Xd, 1.0, prior=0.1, gtol=1e-9, max_iter=3)      # max_iter reached: the gap is reported
    assert stopped.status.tolist() == [1] * n and stopped.iters.tolist() == [3] * n and bool((stopped.gap > 1e-9 * d).all())


def test_no_strategy_beats_the_design(dev):
    import structure as S
    V, X = problem("m40_d3")
    n, m, d = CASES["m40_d3"]
    Vd, Xd = torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev)
    strategies = ("random", "popularity", "top_k")
    eff = S.strategy_efficiency(Vd, Xd, 1.0, 500, strategies=strategies)
    assert set(eff) == set(strategies) | {"gap"} and all(v.shape == (n,) and v.dtype == np.float64 for v in eff.values())
    best = S.optimal_design(Vd, Xd, 1.0)
    assert np.array_equal(eff["gap"], best.gap.cpu().numpy())
    cap = np.exp(eff["gap"] / d)
    print({k: np.round(v, 3).tolist() for k, v in eff.items()})
    for name in strategies:
        v = eff[name]
        assert (np.isnan(v) | (v <= cap * (1 + 1e-12))).all(), name
    assert np.isfinite(eff["random"]).all() and (eff["random"] > 0.02).all() and (eff["random"] < 0.9).all()
    np.testing.assert_allclose(eff["random"], torch.exp((best.logdet_start - best.logdet) / d).cpu().numpy(), rtol=1e-9)


def test_informative_pairs_are_the_top_of_best_val(dev):
    import structure as S
    from mfcd import pairs
    rng = np.random.default_rng(31)
    n, m, d, k = 5, _tile() + 9, 4, 7
    model = S.MatrixFactorization(n, m, d).to(dev)
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)))
        model.V.copy_(torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)))
    X = torch.from_numpy(rng.standard_normal((n, m)).astype(np.float32)).to(dev)
    i, j, score = S.informative_pairs(model, X, k, prior=0.5)
    assert i.dtype == torch.int32 and j.dtype == torch.int32 and score.dtype == torch.float32
    assert tuple(i.shape) == tuple(j.shape) == tuple(score.shape) == (n, k)
    U, V = model.U.data, model.V.data
    H = pairs.user_information(U, V, X, 1.0, at="model").info
    C = H + 0.5 * torch.eye(d, dtype=torch.float64, device=dev)
    eye = torch.eye(d, dtype=torch.float64, device=dev).expand(n, d, d)
    L = torch.linalg.solve_triangular(torch.linalg.cholesky_ex(C)[0], eye, upper=False).transpose(1, 2)       # P = L L^T
    V64 = V.double()
    val, arg = pairs.pair_best_rows(U @ V.t(), torch.matmul(V64 - V64.mean(0, keepdim=True), L).float(), X)
    want = torch.topk(val, k, dim=1)[0]
    assert torch.equal(score, want)                             # the same values, best first
    assert torch.equal(val.gather(1, i.long()), score) and torch.equal(arg.gather(1, i.long()), j)
    assert all(len(set(row)) == k for row in i.cpu().tolist())
