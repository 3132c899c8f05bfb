"""GPU tests of the pair-law kernels and of what is built on them (include/mfcd.h: mfcd_pair_law_stats_rows,
mfcd_pair_law_grad_rows; mfcd/pairs.py: PairLaw, strategy_law, pair_law_stats_rows, pair_law_grad_rows,
law_risk, law_metrics, fit_law; structure.sampling_law, law_risk, train_model_law, compute_law_metrics) against the
float64 model of tests/pair_law_model.py.

Rows: the eight kinds of tests/test_pair_grad.py (ties in a, in x, in both, a constant row, +-0, denormals, and a spread
of 120 at scale 1 only).  Shapes: with T = pairs.TILE, m in {1, 2, 65, T-1, T+1, 2T+3} reaches the empty sum, a single
pair, more than one wave, a partly filled tile, a second tile of one column and three tiles with a short last one.

Tolerances: the project's fp32-loss tolerance rtol 2e-5 / atol 2e-6 (tests/test_pairs.py), on each sum divided by the
model's W and on g_i / W_i with W_i the weight total of item i.  It carries over from the unweighted kernels because
every term of the sums is non-negative and the weight enters by one fma: the error of a weighted sum is bounded by the
same relative error on sum of w |term|, whatever the range of the weights; the weight itself is three fp32 roundings
(1.8e-7).  W is exact without alpha / beta (a sum of 0s and 1s in runs of 64) and held to rtol 2e-5 with them."""
import concurrent.futures
import functools

import numpy as np
import pytest
import torch

import pair_grad_model as GM
import pair_law_model as LM
from test_pair_grad import FIT, _distinct, _model_at, _problem, case_rows, rows_for

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.25, 4.0)
RTOL, ATOL = 2e-5, 2e-6
KINDS = ("weights", "margin_half", "margin_zero", "shared_labels", "row_labels", "all")


def _tile():
    from mfcd import pairs
    return pairs.TILE


def _ms():
    T = _tile()
    return [1, 2, 65, T - 1, T + 1, 2 * T + 3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def log_uniform_weights(m, rng):
    """Log-uniform in [1e-6, 1], a tenth of the entries exactly 0."""
    v = 10.0 ** rng.uniform(-6.0, 0.0, m)
    v[rng.random(m) < 0.1] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def law_parts(kind, m, rows=8):
    """The law `kind` for rows of m columns as plain numpy keyword arguments of PairLaw, and whether x goes on the grid."""
    rng = np.random.default_rng(7000 + m)
    kw = {}
    if kind in ("weights", "all"):
        kw["alpha"], kw["beta"] = log_uniform_weights(m, rng), log_uniform_weights(m, rng)
    if kind in ("margin_half", "all"):
        kw["margin"] = 0.5                                  # x on multiples of 0.25: the <= edge is met exactly
    if kind == "margin_zero":
        kw["margin"] = 0.0                                  # only ties in x count
    if kind == "shared_labels":
        kw["labels"] = rng.integers(0, 3, m)
    if kind in ("row_labels", "all"):
        kw["labels"] = rng.integers(0, 3, (rows, m))
    return kw, "margin" in kw


def grid(X):
    return (np.round(X * 4.0) / 4.0).astype(np.float32)


def make_law(dev, kw, rows=None):
    from mfcd import pairs
    kw = dict(kw)
    if rows is not None and "labels" in kw and np.ndim(kw["labels"]) == 2:
        kw["labels"] = kw["labels"][rows]
    return pairs.PairLaw(device=dev, **kw)


def spec_of(law):
    """The law as the model's dict: what the device holds (alpha and beta after the host's scaling)."""
    host = lambda t: None if t is None else t.cpu().numpy()
    return dict(alpha=host(law.alpha), beta=host(law.beta), labels=host(law.labels), margin=law.margin,
                columns=host(law.columns), users=host(law.users))


def run(dev, A, X, law, scale=1.0):
    from mfcd import pairs
    Ad, Xd = torch.from_numpy(np.ascontiguousarray(A)).to(dev), torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    support, sums = pairs.pair_law_stats_rows(Ad, Xd, law, scale)
    G = pairs.pair_law_grad_rows(Ad, Xd, law, scale)
    assert support.dtype == torch.int64 and sums.dtype == torch.float64 and G.dtype == torch.float32
    assert tuple(support.shape) == A.shape[:1] and tuple(sums.shape) == (A.shape[0], 5) and tuple(G.shape) == A.shape
    return support.cpu().numpy(), sums.cpu().numpy(), G.cpu().numpy()


def model(A, X, spec, scale):
    """(support [rows], sums [rows, 5], G [rows, m], Wi [rows, m]) of the f64 model; the rows on a few threads (numpy
    releases the lock inside its loops)."""
    lab = spec.get("labels")

    def one(r):
        w = LM.weights(X[r], spec.get("alpha"), spec.get("beta"), spec.get("margin"),
                       None if lab is None else lab[r] if lab.ndim == 2 else lab)
        return LM.law_row(A[r], X[r], scale, w) + (w.sum(axis=1),)

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        out = list(pool.map(one, range(len(A))))
    return tuple(np.stack([o[q] for o in out]) for q in range(4))


def check(got, want, weighted, what):
    support, sums, G = got
    w_support, w_sums, w_G, Wi = want
    assert (support == w_support).all(), what
    W = w_sums[:, 0]
    if weighted:
        np.testing.assert_allclose(sums[:, 0], W, rtol=RTOL, atol=0, err_msg=what)
    else:
        assert (sums[:, 0] == w_support).all() and (W == w_support).all(), what
    empty = W == 0
    assert sums[empty].tobytes() == np.zeros_like(sums[empty]).tobytes(), what          # exactly +0
    live = ~empty
    mean, w_mean = sums[live, 1:] / W[live, None], w_sums[live, 1:] / W[live, None]
    dead = Wi == 0
    assert G[dead].tobytes() == np.zeros_like(G[dead]).tobytes(), what                  # exactly +0
    g, w_g = G[~dead].astype(np.float64) / Wi[~dead], w_G[~dead] / Wi[~dead]
    for name, a, b in (("sums / W", mean, w_mean), ("g_i / W_i", g, w_g)):
        if a.size:
            err = np.abs(a - b)
            print(f"{what}: {name}: max abs error {err.max():.3e}, max error / bound "
                  f"{(err / (ATOL + RTOL * np.abs(b))).max():.3f}")
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", _ms())
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_the_f64_model(dev, kind, m, scale):
    A, X = rows_for(m, scale)
    kw, on_grid = law_parts(kind, m)
    if on_grid:
        X = grid(X)
    law = make_law(dev, kw, slice(0, A.shape[0]))
    got = run(dev, A, X, law, scale)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    check(got, model(A, X, spec_of(law), scale), "alpha" in kw, f"{kind} m={m} scale={scale}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. degenerate and equal forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [65, _ms()[-1]])
def test_laws_without_any_pair_give_exact_zeros(dev, m):
    A, X = case_rows(m)
    rng = np.random.default_rng(m)
    Xd = np.stack([_distinct(m, rng) for _ in range(A.shape[0])])          # no two x of a row are equal
    weights = dict(alpha=log_uniform_weights(m, rng), beta=log_uniform_weights(m, rng))
    for what, x, kw in (("margin 0 on distinct x", Xd, dict(margin=0.0)),
                        ("margin 0 on distinct x, weighted", Xd, dict(margin=0.0, **weights)),
                        ("labels all equal", X, dict(labels=np.full(m, 5))),
                        ("labels all equal, weighted", X, dict(labels=np.full(m, 5), **weights))):
        support, sums, G = run(dev, A, x, make_law(dev, kw), 1.0)
        assert (support == 0).all(), what
        assert sums.tobytes() == np.zeros_like(sums).tobytes(), what
        assert G.tobytes() == np.zeros_like(G).tobytes(), what


@pytest.mark.parametrize("m", [65, _ms()[-1]])
def test_distinct_labels_are_bit_equal_to_no_labels(dev, m):
    A, X = case_rows(m)
    kw, _ = law_parts("weights", m)
    for base in (kw, dict(margin=0.5), dict(margin=0.5, **kw), {}):
        x = grid(X) if "margin" in base else X
        plain = run(dev, A, x, make_law(dev, base), 4.0)
        labelled = run(dev, A, x, make_law(dev, dict(labels=np.arange(m)[::-1].copy(), **base)), 4.0)
        for a, b in zip(plain, labelled):
            assert a.tobytes() == b.tobytes(), sorted(base)


@pytest.mark.parametrize("m", [2, 65, _ms()[-1]])
def test_the_empty_law_is_the_unweighted_kernels(dev, m):
    from mfcd import pairs
    A, X = case_rows(m)
    Ad, Xd = torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)
    support, sums, G = run(dev, A, X, pairs.PairLaw(), 1.0)
    n0 = m * (m - 1) // 2
    assert (support == n0).all() and (sums[:, 0] == n0).all()
    plain = pairs.pair_stats_rows(Ad, Xd, 1.0, "sums")[1].cpu().numpy()
    np.testing.assert_allclose(sums[:, 1:] / n0, plain / n0, rtol=RTOL, atol=ATOL)
    plain_G = pairs.pair_grad_rows(Ad, Xd, 1.0).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(G / (m - 1), plain_G / (m - 1), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("m", [65, _tile() + 1])
def test_a_column_without_weight_is_a_deleted_column(dev, m):
    A, X = case_rows(m)
    kw, _ = law_parts("weights", m)
    dead = m // 3
    alpha, beta = kw["alpha"].copy(), kw["beta"].copy()
    alpha[dead] = beta[dead] = 0.0
    if alpha.argmax() == dead or beta.argmax() == dead:
        pytest.fail("the deleted column holds the largest weight: pick another column")
    keep = np.arange(m) != dead
    full = run(dev, A, X, make_law(dev, dict(alpha=alpha, beta=beta)), 0.25)
    less = run(dev, A[:, keep], X[:, keep], make_law(dev, dict(alpha=alpha[keep], beta=beta[keep])), 0.25)
    assert (full[0] == less[0]).all()
    assert (full[2][:, dead].view(np.uint32) == 0).all()                          # exactly +0
    W = less[1][:, :1]
    np.testing.assert_allclose(full[1][:, 0], less[1][:, 0], rtol=RTOL, atol=0)
    np.testing.assert_allclose(full[1][:, 1:] / W, less[1][:, 1:] / W, rtol=RTOL, atol=ATOL)
    spec = dict(alpha=alpha[keep].astype(np.float32), beta=beta[keep].astype(np.float32))
    Wi = np.stack([LM.weights(x, spec["alpha"], spec["beta"]).sum(1) for x in X[:, keep]]) / (alpha.max() * beta.max())
    live = Wi > 0
    np.testing.assert_allclose(full[2][:, keep][live] / Wi[live], less[2][live] / Wi[live], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism and layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [65, _ms()[-1]])
def test_two_calls_rows_alone_and_strided_views_are_bit_equal(dev, m):
    import ctypes
    from mfcd import _lib, pairs
    A, X = case_rows(m)
    X = grid(X)
    rows = A.shape[0]
    kw, _ = law_parts("all", m)
    law = make_law(dev, kw)
    base = run(dev, A, X, law, 4.0)
    again = run(dev, A, X, law, 4.0)
    for a, b in zip(base, again):
        assert a.tobytes() == b.tobytes()
    for r in range(rows):                                      # a row does not depend on its neighbours
        alone = run(dev, A[r:r + 1], X[r:r + 1], make_law(dev, kw, slice(r, r + 1)), 4.0)
        for a, b in zip(base, alone):
            assert a[r:r + 1].tobytes() == b.tobytes(), r
    Ad, Xd = torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)
    wideA = torch.full((rows, m + 5), 7.0, device=dev)
    wideX = torch.full((rows, m + 9), -7.0, device=dev)
    wideA[:, 2:2 + m], wideX[:, 6:6 + m] = Ad, Xd
    va, vx = wideA[:, 2:2 + m], wideX[:, 6:6 + m]
    assert va.stride(0) == m + 5 and not va.is_contiguous()
    support, sums = pairs.pair_law_stats_rows(va, vx, law, 4.0)
    assert support.cpu().numpy().tobytes() == base[0].tobytes() and sums.cpu().numpy().tobytes() == base[1].tobytes()
    assert pairs.pair_law_grad_rows(va, vx, law, 4.0).cpu().numpy().tobytes() == base[2].tobytes()
    # ldg > m and a label stride > m through the C entry: the same bits, and the padding columns of G are left alone
    ldg, stride = m + 7, m + 3
    wideG = torch.full((rows, ldg), -123.0, device=dev)
    wideL = torch.full((rows, stride), 1, dtype=torch.int32, device=dev)
    wideL[:, :m] = law.labels
    c = law._c(rows, m)
    c.labels, c.label_stride = wideL.data_ptr(), stride
    _lib.check(_lib.load().mfcd_pair_law_grad_rows(va.data_ptr(), va.stride(0), vx.data_ptr(), vx.stride(0), rows, m, 4.0,
                                                   ctypes.byref(c), wideG.data_ptr(), ldg, _lib.stream_ptr(dev)))
    host = wideG.cpu().numpy()
    assert np.ascontiguousarray(host[:, :m]).tobytes() == base[2].tobytes()
    assert (host[:, m:] == -123.0).all()
    empty = pairs.pair_law_grad_rows(Ad[:0], Xd[:0], make_law(dev, law_parts("weights", m)[0]))
    assert tuple(empty.shape) == (0, m)
    with pytest.raises(ValueError):
        pairs.pair_law_grad_rows(Ad[:, :-1], Xd[:, :-1], law)                  # a law of m columns on m - 1
    with pytest.raises(ValueError):
        pairs.pair_law_stats_rows(Ad[:3], Xd[:3], law)                         # 8 label rows for 3 rows


def test_a_non_finite_row_is_nan_and_its_neighbours_are_untouched(dev):
    T = _tile()
    m = T + 37
    rng = np.random.default_rng(5)
    A = np.stack([_distinct(m, rng) for _ in range(6)])
    X = grid(np.stack([_distinct(m, rng) for _ in range(6)]))
    kw = dict(alpha=log_uniform_weights(m, rng), beta=log_uniform_weights(m, rng), margin=0.5,
              labels=rng.integers(0, 3, (6, m)))
    law = make_law(dev, kw)
    clean = run(dev, A, X, law, 1.0)
    assert np.isfinite(clean[1]).all() and np.isfinite(clean[2]).all()
    A[1, 3] = np.inf                                           # first tile: the second tile's workgroup must see it
    A[3, T + 30] = np.nan                                      # second tile: the first tile's workgroup must see it
    X[4, 2] = -np.inf
    X[5, m - 1] = np.nan                                       # the last column
    got = run(dev, A, X, law, 1.0)
    bad, good = [1, 3, 4, 5], [0, 2]
    assert np.isnan(got[1][bad]).all() and np.isnan(got[2][bad]).all()
    for q in range(3):
        assert got[q][good].tobytes() == clean[q][good].tobytes()
    want = model(A, X, spec_of(law), 1.0)
    assert (got[0] == want[0]).all()                           # the support of a non-finite row is still counted
    assert (got[0][[1, 3]] == clean[0][[1, 3]]).all()          # a bad score changes no weight


# ---------------------------------------------------------------------------------------------------------------------
# 4. population_risk under a law: value and table gradients
# ---------------------------------------------------------------------------------------------------------------------
def check_law_tables(mdl, want, users, n, what):
    """model.U.grad / model.V.grad against the f64 model's, elementwise, under test_pair_grad.check_tables' bound with
    the weight totals in place of the pair counts: the score gradient g_i is held to rtol on |g_i| plus atol W_i (W_i:
    the weight total of item i), the GEMM adds one 2^-24 per term of its inner dimension, and everything is divided by
    the law's total weight W:
      U:  ((2e-5 + m 2^-24) (|G| @ |V|) + 2e-6 (Wi @ |V|)) / W,     V: the mirror image over the chosen users."""
    _, dU, dV, G, Wi, W = want
    U, V = mdl.U.detach().cpu().numpy().astype(np.float64), mdl.V.detach().cpu().numpy().astype(np.float64)
    m, k = V.shape[0], G.shape[0]
    ids = np.asarray(users)
    per_row = ((RTOL + m * 2.0 ** -24) * (np.abs(G) @ np.abs(V)) + ATOL * (Wi @ np.abs(V))) / W
    boundU = np.zeros_like(U)
    np.add.at(boundU, ids, per_row)
    boundV = ((RTOL + k * 2.0 ** -24) * (np.abs(G).T @ np.abs(U[ids])) + ATOL * (Wi.T @ np.abs(U[ids]))) / W
    for name, got, ref, bound in (("U", mdl.U.grad, dU, boundU), ("V", mdl.V.grad, dV, boundV)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        live = bound > 0
        print(f"{what}: d{name} max |grad| {np.abs(ref).max():.3e}, max abs error {err.max():.3e}, "
              f"max error / bound {(err[live] / bound[live]).max():.3f}")
        assert (err <= bound).all(), (what, name)


LAWS = (("margin", {}), ("popularity", {}), ("top_k", dict(k=7)), ("proximity", dict(k=40)), ("cluster", dict(n_clusters=3)))


@pytest.mark.parametrize("strategy,kw", LAWS, ids=[name for name, _ in LAWS])
@pytest.mark.parametrize("shape", ["n5_m65_d3", "n3_mT1_d2"])
def test_population_risk_under_a_law_value_and_gradients(dev, shape, strategy, kw):
    n, m, d = (5, 65, 3) if shape == "n5_m65_d3" else (3, _tile() + 1, 2)
    S, mdl, F, Xd = _problem(n, m, d, 21, dev)
    X32 = Xd.cpu().numpy()
    U, V = mdl.U.detach().cpu().numpy(), mdl.V.detach().cpu().numpy()
    s, nt = 0.7, n * m // 10
    variants = [("all users", Xd, {}, None), ("row_block=2", Xd, {"row_block": 2}, None), ("factored X", F, {}, None)]
    if n == 5:
        variants.append(("users=[4, 0, 4]", Xd, {"users": [4, 0, 4], "row_block": 2}, [4, 0, 4]))
    for what, X, call, users in variants:
        law = S.sampling_law(X, nt, strategy, device=dev, seed=3, **kw)
        if strategy == "proximity" and m == 65:                # the lists overlap: the per-row labels matter
            cols = law.columns.cpu().numpy()
            assert all(len(set(row)) < cols.shape[1] for row in cols)
        want = LM.population(U, V, X32, s, spec_of(law), users)
        assert want[5] > 0
        mdl.zero_grad()
        risk = S.law_risk(mdl, X, law, s, **call)
        assert risk.dim() == 0 and risk.is_cuda and risk.dtype == torch.float32 and risk.requires_grad
        print(f"{shape} {strategy} {what}: risk {float(risk.detach()):.6f}, model {want[0]:.6f}")
        np.testing.assert_allclose(float(risk.detach()), want[0], rtol=RTOL, atol=ATOL, err_msg=what)
        risk.backward()
        check_law_tables(mdl, want, np.arange(n) if users is None else users, n, f"{shape} {strategy} {what}")
        res = S.compute_law_metrics(mdl, X, law, s, **call)
        assert sorted(res) == sorted([k + t for k in ("expected_log_likelihood", "bayes_log_likelihood",
                                                       "expected_accuracy", "bayes_accuracy") for t in ("", "_per_user")])
        np.testing.assert_allclose(-res["expected_log_likelihood"], want[0], rtol=RTOL, atol=ATOL, err_msg=what)
        assert res["expected_accuracy_per_user"].shape == (len(want[3]),)
        assert res["bayes_accuracy"] >= res["expected_accuracy"] - ATOL


def test_a_law_without_weight_gives_nan_and_the_fit_refuses_it(dev):
    from mfcd import pairs
    S, mdl, F, Xd = _problem(5, 65, 3, 21, dev)
    law = pairs.PairLaw(labels=np.zeros(65, dtype=np.int64), device=dev)
    assert np.isnan(float(S.law_risk(mdl, Xd, law, 0.7)))
    assert np.isnan(S.compute_law_metrics(mdl, Xd, law, 0.7)["expected_accuracy"])
    opt = torch.optim.Adam(mdl.parameters(), lr=0.05)
    with pytest.raises(ValueError):
        S.train_model_law(mdl, Xd, 0.7, opt, dev, law, num_steps=2)
    with pytest.raises(IndexError):
        S.law_risk(mdl, Xd, pairs.PairLaw(columns=[0, 65], device=dev), 0.7)
    # the law of `random` is the unweighted path itself
    plain = S.population_risk(mdl, Xd, 0.7)
    assert float(S.law_risk(mdl, Xd, S.sampling_law(Xd, 30, "random"), 0.7)) == float(plain)


# ---------------------------------------------------------------------------------------------------------------------
# 5. strategy_law against the enumerated attempt law of the reference
# ---------------------------------------------------------------------------------------------------------------------
STRATEGIES = ("random", "margin", "popularity", "variance", "top_k", "proximity", "cluster", "svd")


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_strategy_law_is_the_symmetrised_attempt_law(dev, strategy):
    import generation_data as gd
    import structure as S
    n, m, nt = 12, 40, 120
    torch.manual_seed(11)
    np.random.seed(11)
    X = S.generate_X(n, m, 2, "cpu")
    X32 = X.numpy()
    kw = dict(k=25) if strategy == "proximity" else dict(n_clusters=3, seed=5) if strategy == "cluster" else {}
    law = S.sampling_law(X.to(dev), nt, strategy, **kw)
    spec = spec_of(law)
    extra = {}
    if strategy == "popularity":
        extra["probs"] = gd._popularity_probs(m, "zipf", 1.5)
    elif strategy == "variance":
        v = X.double().var(0).numpy()
        extra["probs"] = v / v.sum()
    elif strategy == "top_k":
        extra["k"] = 5                                          # ref:199: min(m, max(5, int(0.1 m)))
    elif strategy == "proximity":
        extra["k"] = 25
    elif strategy == "cluster":
        extra["clusters"] = spec["labels"]
        assert sorted(set(spec["labels"].tolist())) == [0, 1, 2]
    users = np.arange(n)
    if strategy == "svd":
        top_users, top_items = gd._svd_top_sets(X, nt)
        assert sorted(spec["users"].tolist()) == sorted(top_users.tolist()) and len(top_users) == 3
        extra["top_items"], users = top_items, top_users
    else:
        assert spec["users"] is None
    for u in users:
        P = LM.attempt_law(strategy, X32, u, num_triplets=nt, **extra)
        sym = P + P.T
        w = LM.user_matrix(spec, X32, u)
        assert sym.sum() > 0, (strategy, u)
        np.testing.assert_allclose(w / w.sum(), sym / sym.sum(), rtol=1e-6, atol=0, err_msg=f"{strategy} user {u}")


def test_user_similarity_has_no_law(dev):
    import structure as S
    with pytest.raises(ValueError):
        S.sampling_law(torch.randn(12, 40, device=dev), 120, "user_similarity")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the fit under a law
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def law_fit_setup(dev):
    """test_pair_grad's FIT problem under the popularity law, and the f64 model's run from the same start."""
    import structure as S
    np.random.seed(0)
    torch.manual_seed(0)
    X = S.generate_X(FIT["n"], FIT["m"], FIT["d"], "cpu")
    mdl = S.MatrixFactorization(FIT["n"], FIT["m"], FIT["d"])
    U0, V0 = mdl.U.detach().numpy().copy(), mdl.V.detach().numpy().copy()
    law = S.sampling_law(X.to(dev), 100, "popularity")
    spec = spec_of(law)
    X32 = X.numpy()
    _, _, at, risks = LM.fit(U0, V0, X32, FIT["s"], spec, FIT["steps"], FIT["lr"], log_every=FIT["log_every"])
    bayes = LM.bayes_risk(X32, FIT["s"], spec)
    print(f"f64 model under the popularity law: risks {np.round(risks, 7).tolist()}, bayes {bayes:.7f}, "
          f"gap {risks[-1] - bayes:.2e}")
    assert at == [0, 100, 200, 300, 400]
    return S, X.to(dev), X32, U0, V0, law, spec, at, risks, bayes


def test_fused_fit_under_the_popularity_law_reaches_its_bayes_risk(law_fit_setup, dev):
    S, Xd, X32, U0, V0, law, spec, at, ref_risks, bayes = law_fit_setup
    mdl = _model_at(S, U0, V0, dev)
    opt = torch.optim.Adam(mdl.parameters(), lr=FIT["lr"])
    steps, risks = S.train_model_law(mdl, Xd, FIT["s"], opt, dev, law, num_steps=FIT["steps"],
                                     log_every=FIT["log_every"])
    assert not mdl.training and steps == at and len(risks) == len(at)
    res = S.compute_law_metrics(mdl, Xd, law, s=FIT["s"])
    gap = -res["expected_log_likelihood"] - -res["bayes_log_likelihood"]
    print(f"fused fit under the law: logged risks {np.round(risks, 7).tolist()} (model {np.round(ref_risks, 7).tolist()}), "
          f"bayes {-res['bayes_log_likelihood']:.7f} (model {bayes:.7f}), risk - bayes {gap:.3e}")
    np.testing.assert_allclose(risks[0], ref_risks[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(-res["bayes_log_likelihood"], bayes, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(risks[-1], -res["expected_log_likelihood"], rtol=RTOL, atol=ATOL)
    for a, b in zip(risks[:-1], risks[1:]):
        if a > bayes + 1e-3:
            assert b <= a, risks
    assert gap <= 1e-4
    assert float(opt.state[mdl.U]["step"]) == FIT["steps"] == float(opt.state[mdl.V]["step"])


def test_fused_first_step_under_a_law_with_weight_decay_is_the_models_adam_step(law_fit_setup, dev):
    S, Xd, X32, U0, V0, law, spec, _, _, _ = law_fit_setup
    mdl = _model_at(S, U0, V0, dev)
    opt = torch.optim.Adam(mdl.parameters(), lr=FIT["lr"], weight_decay=1e-2)
    steps, risks = S.train_model_law(mdl, Xd, FIT["s"], opt, dev, law, num_steps=1, log_every=1)
    assert steps == [0, 1] and float(opt.state[mdl.U]["step"]) == 1
    Uf, Vf, _, want = LM.fit(U0, V0, X32, FIT["s"], spec, 1, FIT["lr"], weight_decay=1e-2, log_every=1)
    np.testing.assert_allclose(risks, want, rtol=RTOL, atol=ATOL)
    _, dU, dV = LM.population(U0, V0, X32, FIT["s"], spec)[:3]
    for name, got, ref, g in (("U", mdl.U, Uf, dU + 1e-2 * U0), ("V", mdl.V, Vf, dV + 1e-2 * V0)):
        live = np.abs(g) > 1e-6
        assert live.sum() >= live.size // 2, name
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)[live]
        print(f"first step under the law, {name}: {live.sum()} of {live.size} elements compared, max abs error "
              f"{err.max():.2e}")
        assert err.max() <= 1e-6, name


def test_generic_path_under_a_law_is_plain_backward_and_manual_updates(dev):
    S, mdl, F, Xd = _problem(5, 65, 3, 33, dev)
    law = S.sampling_law(Xd, 30, "proximity", k=40)
    twin = _model_at(S, mdl.U.detach().cpu().numpy(), mdl.V.detach().cpu().numpy(), dev)
    opt = torch.optim.SGD(mdl.parameters(), lr=0.1)
    steps, risks = S.train_model_law(mdl, Xd, 0.7, opt, dev, law, num_steps=3, log_every=1)
    assert steps == [0, 1, 2, 3] and not mdl.training
    seen = []
    for _ in range(3):
        twin.zero_grad()
        risk = S.law_risk(twin, Xd, law, 0.7)
        seen.append(float(risk.detach()))
        risk.backward()
        with torch.no_grad():
            twin.U -= 0.1 * twin.U.grad
            twin.V -= 0.1 * twin.V.grad
    with torch.no_grad():
        seen.append(float(S.law_risk(twin, Xd, law, 0.7)))
    np.testing.assert_allclose(mdl.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(mdl.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(risks, seen, rtol=1e-5, atol=0)
    assert risks[3] < risks[0]


def test_an_svd_law_leaves_the_other_users_without_gradient(dev):
    import structure as S
    n, m = 12, 40
    torch.manual_seed(11)
    np.random.seed(11)
    X = S.generate_X(n, m, 2, "cpu").to(dev)
    law = S.sampling_law(X, 120, "svd")
    inside = sorted(law.users.cpu().tolist())
    outside = [u for u in range(n) if u not in inside]
    assert len(inside) == 3
    mdl = S.MatrixFactorization(n, m, 2).to(dev)
    S.law_risk(mdl, X, law, 1.0).backward()
    grad = mdl.U.grad.cpu().numpy()
    assert (grad[outside].view(np.uint32) == 0).all() and (np.abs(grad[inside]).sum(1) > 0).all()
    cols = law.columns.cpu().numpy()
    assert (mdl.V.grad.cpu().numpy()[np.setdiff1d(np.arange(m), cols)] == 0).all()
    # the fused fit: those users move by weight decay alone, and without it stay where they were
    start = mdl.U.detach().clone()
    opt = torch.optim.Adam(mdl.parameters(), lr=0.05)
    S.train_model_law(mdl, X, 1.0, opt, dev, law, num_steps=3, log_every=0)
    assert torch.equal(mdl.U.detach()[outside], start[outside])
    assert not torch.equal(mdl.U.detach()[inside], start[inside])
