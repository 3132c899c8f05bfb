"""GPU tests of the exact all-pairs statistics (include/mfcd.h: mfcd_pair_stats_rows; mfcd/pairs.py;
structure.compute_pairwise_metrics) against the CPU model of tests/pairs_model.py (numpy float64 over np.triu_indices)
and scipy.stats.kendalltau.

Shapes: with T = pairs.TILE columns per workgroup tile, m in {1, 2, 63, 64, 65, T-1, T, T+1, 2T+3} reaches the empty
row, a single pair, the wave boundary, a partly filled / exactly full diagonal tile, a second tile of one column and
three tiles (unmasked tile pairs, a short last tile); m = 5000 with 3 rows adds five tiles.  Values lie in [-3, 3].
Counts must be equal as integers.  The sums are held to the project's fp32-loss tolerance (rtol 2e-5, atol 2e-6 on
sums / n0: the tolerance of smoke() in __graft_entry__.py) at scale 1, 0.25 and 4.  The reference of every shape is
computed once per module and shared."""
import functools

import numpy as np
import pytest
import torch

import pairs_model as M

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.25, 4.0)
RTOL, ATOL = 2e-5, 2e-6


def _tile():
    from mfcd import pairs
    return pairs.TILE


def _ms():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _levels(m, rng, values):
    return np.asarray(values, dtype=np.float32)[rng.integers(0, len(values), m)]


def _distinct(m, rng):
    return (rng.permutation(m).astype(np.float64) / m * 6.0 - 3.0).astype(np.float32)      # spacing 6 / m >> an fp32 ulp


@functools.lru_cache(maxsize=None)
def case_rows(m):
    """(A, X) float32 [rows, m]: the kinds of row the counts can go wrong on.  m = 5000 keeps three of them."""
    rng = np.random.default_rng(1000 + m)
    three = (-1.5, 0.0, 2.25)
    zeros = (-0.0, 0.0, 0.0, -0.0, 1.0, -2.0)
    tiny = np.float32(1e-42)                                   # denormal values whose differences are denormal too
    rows = [
        (_distinct(m, rng), _distinct(m, rng)),                # no ties
        (_levels(m, rng, three), _distinct(m, rng)),           # heavy ties in a
        (_levels(m, rng, three), _levels(m, rng, three)),      # heavy ties in both
    ]
    if m != 5000:
        rows += [
            (_distinct(m, rng), _levels(m, rng, three)),       # heavy ties in x
            (np.full(m, 0.75, dtype=np.float32), _distinct(m, rng)),                  # constant row
            (_levels(m, rng, zeros), _levels(m, rng, zeros)),  # -0.0 equals +0.0
            (rng.integers(-3, 4, m).astype(np.float32) * tiny, rng.integers(-2, 3, m).astype(np.float32) * tiny),
        ]
    A, X = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert np.abs(A).max() <= 3 and np.abs(X).max() <= 3
    return A, X


@functools.lru_cache(maxsize=None)
def ref_counts(m):
    A, X = case_rows(m)
    return np.array([M.pair_counts(a, x) for a, x in zip(A, X)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def ref_sums(m, scale):
    A, X = case_rows(m)
    return np.stack([M.pair_sums(a, x, scale) for a, x in zip(A, X)])


def run(dev, A, X, scale=1.0, what="both"):
    from mfcd import pairs
    c, s = pairs.pair_stats_rows(torch.from_numpy(np.ascontiguousarray(A)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(X)).to(dev), scale, what)
    return (None if c is None else c.cpu().numpy()), (None if s is None else s.cpu().numpy())


def check_sums(got, want, m, what):
    n0 = m * (m - 1) // 2
    if n0 == 0:
        np.testing.assert_array_equal(got, np.zeros_like(got), err_msg=what)      # no pairs: nothing to divide by
        return
    err = np.abs(got / n0 - want / n0)
    print(f"{what}: mean values {np.round((want / n0).mean(0), 4).tolist()}, max abs error {err.max():.3e}, "
          f"max error / bound {(err / (ATOL + RTOL * np.abs(want / n0))).max():.3f}")
    np.testing.assert_allclose(got / n0, want / n0, rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("m", _ms() + [5000])
def test_counts_equal_the_model_and_tau_is_scipys(dev, m):
    from scipy.stats import kendalltau
    from mfcd import pairs
    A, X = case_rows(m)
    counts, sums = run(dev, A, X, 1.0, "counts")
    assert sums is None and counts.dtype == np.int64 and counts.shape == (A.shape[0], 4)
    np.testing.assert_array_equal(counts, ref_counts(m))
    n0 = m * (m - 1) // 2
    assert ((counts[:, 0] + counts[:, 1] + counts[:, 2] <= n0) & (counts >= 0).all(1)).all()
    per = pairs.pairwise_from_counts(counts, None, m)
    for r, (a, x) in enumerate(zip(A, X)):
        if m == 1:
            assert np.isnan(per["kendall_tau"][r]) and np.isnan(per["pairwise_accuracy"][r])
            continue
        want = kendalltau(a.astype(np.float64), x.astype(np.float64)).statistic
        if np.isnan(want):
            assert np.isnan(per["kendall_tau"][r]), (m, r)
        else:
            assert abs(per["kendall_tau"][r] - want) <= 1e-12, (m, r, per["kendall_tau"][r], want)
        acc = M.pairwise_accuracy(ref_counts(m)[r], m)
        assert per["pairwise_accuracy"][r] == acc or (np.isnan(acc) and np.isnan(per["pairwise_accuracy"][r]))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", _ms() + [5000])
def test_sums_match_the_f64_model(dev, m, scale):
    A, X = case_rows(m)
    counts, sums = run(dev, A, X, scale, "sums")
    assert counts is None and sums.dtype == np.float64 and sums.shape == (A.shape[0], 4)
    check_sums(sums, ref_sums(m, scale), m, f"m={m} scale={scale}")


def test_infinities_nans_and_their_neighbours(dev):
    T = _tile()
    m = T + 37
    rng = np.random.default_rng(5)
    A = np.stack([_distinct(m, rng) for _ in range(6)])
    X = np.stack([_levels(m, rng, (-1.0, 0.5, 2.0, 3.0)) for _ in range(6)])
    A[1, [3, T + 5, 700]] = [np.inf, -np.inf, np.inf]          # +-inf compare as numbers: exact counts, NaN sums
    X[1, [0, 9]] = [-np.inf, np.inf]
    A[3, T + 30] = np.nan                                      # a NaN in the scores, in the second tile
    X[4, 2] = np.nan                                           # a NaN in the ground truth
    counts, sums = run(dev, A, X, 1.0, "both")
    want = np.array([M.pair_counts(a, x) for a, x in zip(A, X)], dtype=np.int64)
    np.testing.assert_array_equal(counts, want)
    assert (counts[[3, 4]] == -1).all() and (counts[1] >= 0).all() and counts[1, 2] == 1      # the two +inf tie
    assert np.isnan(sums[[1, 3, 4]]).all() and np.isfinite(sums[[0, 2, 5]]).all()
    good = [0, 2, 5]
    check_sums(sums[good], np.stack([M.pair_sums(A[r], X[r], 1.0) for r in good]), m, "neighbours of bad rows")
    for r in good:                                             # and bit for bit what the row gives on its own
        c1, s1 = run(dev, A[r:r + 1], X[r:r + 1], 1.0, "both")
        assert np.array_equal(c1[0], counts[r]) and s1.tobytes() == sums[r:r + 1].tobytes()


def test_strided_views_and_no_rows(dev):
    from mfcd import pairs
    T = _tile()
    m = T + 1
    A, X = case_rows(m)
    Ad, Xd = torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)
    wideA = torch.full((A.shape[0], m + 5), 7.0, device=dev)
    wideX = torch.full((A.shape[0], m + 9), -7.0, device=dev)
    wideA[:, 2:2 + m], wideX[:, 6:6 + m] = Ad, Xd
    va, vx = wideA[:, 2:2 + m], wideX[:, 6:6 + m]
    assert va.stride(0) == m + 5 and not va.is_contiguous()
    c0, s0 = pairs.pair_stats_rows(Ad, Xd, 0.25)
    c1, s1 = pairs.pair_stats_rows(va, vx, 0.25)
    assert torch.equal(c0, c1) and s0.cpu().numpy().tobytes() == s1.cpu().numpy().tobytes()
    c2, s2 = pairs.pair_stats_rows(Ad[:0], Xd[:0])
    assert c2.shape == (0, 4) and c2.dtype == torch.int64 and s2.shape == (0, 4) and s2.dtype == torch.float64
    with pytest.raises(Exception):
        pairs.pair_stats_rows(Ad, Xd[:, :-1])


@pytest.mark.parametrize("m", [65, _ms()[-1]])
def test_two_calls_and_the_halves_are_bit_equal(dev, m):
    A, X = case_rows(m)
    c3, s3 = run(dev, A, X, 4.0, "both")
    c3b, s3b = run(dev, A, X, 4.0, "both")
    c1, none_s = run(dev, A, X, 4.0, "counts")
    none_c, s2 = run(dev, A, X, 4.0, "sums")
    assert none_s is None and none_c is None
    assert c3.tobytes() == c3b.tobytes() and s3.tobytes() == s3b.tobytes()
    assert c1.tobytes() == c3.tobytes() and s2.tobytes() == s3.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# structure.compute_pairwise_metrics, n = 37, m = 300, d = 8
# ---------------------------------------------------------------------------------------------------------------------
N, MI, D = 37, 300, 8
KEYS = ("kendall_tau", "pairwise_accuracy", "expected_log_likelihood", "bayes_log_likelihood", "expected_accuracy",
        "bayes_accuracy")


@pytest.fixture(scope="module")
def setup(dev):
    import generation_data as gd
    import structure as S
    g = torch.Generator().manual_seed(11)
    FA, FB = torch.randn(N, D, generator=g) / 2, torch.randn(MI, D, generator=g) / 2
    F = gd.FactoredMatrix(FA, FB)
    model = S.MatrixFactorization(N, MI, D).to(dev)
    return S, model, F, F.dense(dev)


def model_rows(scores, truth, s):
    """The six per-user values of the model for given score / truth rows (numpy float32 [k, m])."""
    m = scores.shape[1]
    n0 = m * (m - 1) // 2
    out = {k: [] for k in KEYS}
    for a, x in zip(scores, truth):
        c, t = M.pair_counts(a, x), M.pair_sums(a, x, s)
        out["kendall_tau"].append(M.tau_b(c, m))
        out["pairwise_accuracy"].append(M.pairwise_accuracy(c, m))
        out["expected_log_likelihood"].append(-t[0] / n0)
        out["bayes_log_likelihood"].append(-t[1] / n0)
        out["expected_accuracy"].append(t[2] / n0)
        out["bayes_accuracy"].append(t[3] / n0)
    return {k: np.array(v) for k, v in out.items()}


def check_against_model(res, want):
    for k in KEYS:
        per = res[k + "_per_user"]
        assert isinstance(per, np.ndarray) and per.dtype == np.float64 and per.shape == want[k].shape, k
        if k in ("kendall_tau", "pairwise_accuracy"):
            np.testing.assert_allclose(per, want[k], rtol=0, atol=1e-12, err_msg=k)
        else:
            np.testing.assert_allclose(per, want[k], rtol=RTOL, atol=ATOL, err_msg=k)
        assert isinstance(res[k], float) and res[k] == float(per.mean()), k
    assert set(res) == set(KEYS) | {k + "_per_user" for k in KEYS}


def test_metrics_equal_the_model_on_torchs_product(setup, dev):
    S, model, F, Xd = setup
    res = S.compute_pairwise_metrics(model, Xd, s=0.5)
    scores = (model.U.data @ model.V.data.t()).cpu().numpy()
    check_against_model(res, model_rows(scores, Xd.cpu().numpy(), 0.5))
    # blocks of rows: the same values, each block's product formed as the function forms it
    res16 = S.compute_pairwise_metrics(model, Xd, s=0.5, row_block=16)
    blocked = torch.cat([model.U.data[r0:r0 + 16] @ model.V.data.t() for r0 in range(0, N, 16)]).cpu().numpy()
    check_against_model(res16, model_rows(blocked, Xd.cpu().numpy(), 0.5))


def test_metrics_dense_and_factored_truth_agree(setup, dev):
    S, model, F, Xd = setup
    dense = S.compute_pairwise_metrics(model, Xd, s=2.0)
    fact = S.compute_pairwise_metrics(model, F, s=2.0)
    same_bits = torch.equal(F.A.to(dev) @ F.B.to(dev).t(), Xd)          # the product the factored path forms
    for k in KEYS:
        a, b = dense[k + "_per_user"], fact[k + "_per_user"]
        if same_bits:
            assert a.tobytes() == b.tobytes(), k
        else:
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=k)
    with pytest.raises(ValueError):
        S.compute_pairwise_metrics(model, Xd[:, :-1])


def test_metrics_for_chosen_users_keep_their_order(setup, dev):
    S, model, F, Xd = setup
    sel = [5, 0, 5]
    scores = (model.U.data[sel] @ model.V.data.t()).cpu().numpy()           # the products as the function forms them
    for X, truth in ((Xd, Xd[sel]), (F, F.A.to(dev)[sel] @ F.B.to(dev).t())):
        some = S.compute_pairwise_metrics(model, X, users=sel)
        check_against_model(some, model_rows(scores, truth.cpu().numpy(), 1.0))
        assert all(some[k + "_per_user"][0] == some[k + "_per_user"][2] for k in KEYS)
    every = S.compute_pairwise_metrics(model, Xd)
    assert not np.array_equal(every["kendall_tau_per_user"][[5, 0]], every["kendall_tau_per_user"][[0, 5]])
    np.testing.assert_allclose(some["kendall_tau_per_user"], every["kendall_tau_per_user"][sel], rtol=0, atol=1e-3)
    empty = S.compute_pairwise_metrics(model, Xd, users=[])
    assert all(empty[k] == 0.0 and empty[k + "_per_user"].shape == (0,) for k in KEYS)
    with pytest.raises(IndexError):
        S.compute_pairwise_metrics(model, Xd, users=[N])


def test_metrics_of_the_true_and_the_negated_model(setup, dev):
    S, model, F, Xd = setup
    truth = S.MatrixFactorization(N, MI, D).to(dev)
    with torch.no_grad():
        truth.U.copy_(F.A)
        truth.V.copy_(F.B)
    X = truth.U.data @ truth.V.data.t()                                     # the product the function forms, bit for bit
    res = S.compute_pairwise_metrics(truth, X, s=1.0)
    assert (res["kendall_tau_per_user"] == 1.0).all() and res["kendall_tau"] == 1.0
    assert (res["pairwise_accuracy_per_user"] == 1.0).all() and res["pairwise_accuracy"] == 1.0
    np.testing.assert_allclose(res["expected_log_likelihood_per_user"], res["bayes_log_likelihood_per_user"],
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res["expected_accuracy_per_user"], res["bayes_accuracy_per_user"], rtol=RTOL, atol=ATOL)
    with torch.no_grad():
        truth.U.neg_()
    neg = S.compute_pairwise_metrics(truth, X, s=1.0)
    assert (neg["kendall_tau_per_user"] == -1.0).all() and neg["kendall_tau"] == -1.0
    assert neg["pairwise_accuracy"] == 0.0
    assert neg["expected_log_likelihood"] < res["expected_log_likelihood"] <= 0.0


def test_block_loop_at_a_ragged_last_block_and_a_repeated_user(dev):
    """n = 70, m = 130, d = 8, row_block = 32 (blocks of 32, 32 and 6 rows), users with a repeat.  Exact: every block
    is what `pair_stats_rows` gives for the products formed here as the function forms them, in the order of `users`.
    Across row_block in {32, 70} the score GEMMs may round differently, so that comparison carries the tolerances of
    the tests above: 1e-3 on the two values made of counts (a pair whose order flips moves tau by 2 / n0 = 2.4e-4), the
    module's RTOL / ATOL on the sums.  Dense against factored X: bits where the products are bit-equal, else 1e-6."""
    import generation_data as gd
    import structure as S
    from mfcd import pairs
    n, m, d, rb = 70, 130, 8, 32
    g = torch.Generator().manual_seed(12)
    F = gd.FactoredMatrix(torch.randn(n, d, generator=g) / 2, torch.randn(m, d, generator=g) / 2)
    Xd = F.dense(dev)
    torch.manual_seed(12)
    model = S.MatrixFactorization(n, m, d).to(dev)
    U, V = model.U.data, model.V.data
    users = list(range(n - 1, -1, -1)) + [3, 3]                              # 72 rows: blocks of 32, 32 and 8
    for sel in (None, users):
        ids = torch.arange(n, device=dev) if sel is None else torch.tensor(sel, device=dev)
        for X, truth in ((Xd, lambda i: Xd[i]), (F, lambda i: F.A.to(dev)[i] @ F.B.to(dev).t())):
            res = {b: S.compute_pairwise_metrics(model, X, s=0.5, users=sel, row_block=b) for b in (rb, n)}
            parts = [pairs.pair_stats_rows(U[ids[r0:r0 + rb]] @ V.t(), truth(ids[r0:r0 + rb]), 0.5, "both")
                     for r0 in range(0, len(ids), rb)]
            want = pairs.pairwise_from_counts(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), m)
            want["expected_log_likelihood"], want["bayes_log_likelihood"] = -want.pop("risk"), -want.pop("bayes_risk")
            for k in KEYS:
                assert res[rb][k + "_per_user"].tobytes() == want[k].tobytes(), k
                counted = k in ("kendall_tau", "pairwise_accuracy")
                np.testing.assert_allclose(res[rb][k + "_per_user"], res[n][k + "_per_user"], err_msg=k,
                                           rtol=0 if counted else RTOL, atol=1e-3 if counted else ATOL)
            if sel is not None:
                assert all(res[rb][k + "_per_user"][-1] == res[rb][k + "_per_user"][-2] for k in KEYS)
    dense, fact = (S.compute_pairwise_metrics(model, X, s=0.5, row_block=rb) for X in (Xd, F))
    same_bits = all(torch.equal(F.A.to(dev)[r0:r0 + rb] @ F.B.to(dev).t(), Xd[r0:r0 + rb]) for r0 in range(0, n, rb))
    for k in KEYS:
        a, b = dense[k + "_per_user"], fact[k + "_per_user"]
        if same_bits:
            assert a.tobytes() == b.tobytes(), k
        else:
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=k)
