"""GPU tests of the per-row top-k of a dense or factored score matrix (include/mfcd.h: mfcd_topk_rows, mfcd/topk.py) and of
what is built on it: the `proximity` / `top_k` samplers on a FactoredMatrix, recommend_items, compute_topk_overlap.

Exact cases compare with a stable sort of the row (torch.sort(..., stable=True)): equal scores in ascending column order,
NaN above +inf for `best`, after every number for `worst`.  Real-valued factor cases use bounds that are derived, not
measured: e(r, c) = d * 2^-24 * sum_k |a_k b_k|, the standard bound of an fp32 dot product of length d.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C3 = (16384, 16384, 128)
C4 = (65536, 65536, 64)
C5 = (100000, 20000, 256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def stable_ref(S, k, worst):
    """(indices, values) of the first k entries of the stable sort of every row: descending for best, ascending for worst."""
    v, i = torch.sort(S, dim=1, descending=not worst, stable=True)
    return i[:, :k], v[:, :k]


def check_exact(got, S, k, worst, what):
    idx, val = got
    ri, rv = stable_ref(S, k, worst)
    idx, val = idx.cpu(), val.cpu()
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == ri.shape, what
    bad = (idx.long() != ri).nonzero()
    assert bad.numel() == 0, f"{what}: first index mismatch at {bad[0].tolist()}: got {idx[tuple(bad[0])]}, want {ri[tuple(bad[0])]}"
    torch.testing.assert_close(val, rv.float(), rtol=0, atol=0, equal_nan=True, msg=lambda s: f"{what}: {s}")


def ks_for(m):
    return sorted({k for k in (1, 5, 100, m // 10) if 1 <= k <= m})


def base_factors(n, m, d, seed):
    import generation_data as gd
    return gd.generate_embedding_factors(n, m, d, "cpu", generator=torch.Generator().manual_seed(seed))


def dot_bound(A64, B64, d):
    """e(r, c) = d 2^-24 sum_k |a_k b_k| for every (r, c) of the product."""
    return (A64.abs() @ B64.abs().t()) * (d * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact, dense mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(7, 1), (5, 100), (300, 1000), (64, 20449), (32, 65536), (3, 70001)])
def test_dense_mode_equals_the_stable_sort(dev, n, m):
    from mfcd import topk
    g = torch.Generator().manual_seed(100 + m)
    X = torch.randn(n, m, generator=g)
    Q = torch.randint(0, 16, (n, m), generator=g).float() - 8.0          # 16 distinct values: massive ties
    rows = torch.randperm(n, generator=g)[:max(1, (2 * n) // 3)]
    for name, M in (("random", X), ("quantised", Q)):
        Md = M.to(dev)
        for k in sorted(set(ks_for(m)) | {m if m <= 100 else 1}):
            (b, w) = topk.topk_rows(Md, k, rows=rows, ends="both", values=True)
            check_exact(b, M[rows], k, False, f"{name} {n}x{m} k={k} best")
            check_exact(w, M[rows], k, True, f"{name} {n}x{m} k={k} worst")
        k = ks_for(m)[-1]
        check_exact(topk.topk_rows(Md, k, ends="best", values=True), M, k, False, f"{name} {n}x{m} k={k} all rows")


def test_dense_mode_signed_zeros_infinities_and_nan(dev):
    from mfcd import topk
    g = torch.Generator().manual_seed(5)
    m = 777
    X = torch.randn(6, m, generator=g)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), -0.0, 0.0, float("nan"),
                            float("inf"), float("-inf")])
    X[5, 100:400] = 0.0
    X[5, 150:300:2] = -0.0                                               # a long run of +-0.0: one tie class
    for r in range(6):
        pos = torch.randperm(m, generator=g)[:special.numel() * 3]
        X[r, pos] = special.repeat(3)
    Xd = X.to(dev)
    for k in (1, 4, 9, 77, m - 7, m):
        b, w = topk.topk_rows(Xd, k, ends="both", values=True)
        check_exact(b, X, k, False, f"special k={k} best")
        check_exact(w, X, k, True, f"special k={k} worst")
        if k <= m - 6:
            assert not torch.isnan(w[1]).any(), "NaN returned among the worst although k numbers remain"
    b1 = topk.topk_rows(Xd, 6, ends="best", values=True)
    assert torch.isnan(b1[1][:, :6]).all(), "the six NaN of a row rank above +inf for best"


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact, factor mode: small integer factors, every fp32 partial sum is an exact integer in any order
# ---------------------------------------------------------------------------------------------------------------------
def int_factors(n, m, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (n, d), generator=g).float(), torch.randint(-3, 4, (m, d), generator=g).float())


@pytest.mark.parametrize("d", [2, 3, 64, 100, 256])
@pytest.mark.parametrize("n,m", [(257, 1000), (64, 20449)])
def test_factor_mode_integer_factors_equal_the_stable_sort_of_the_f64_product(dev, n, m, d):
    from mfcd import topk
    A, B = int_factors(n, m, d, 7 * d + m)
    S = A.double() @ B.double().t()
    Ad, Bd = A.to(dev), B.to(dev)
    for k in ks_for(m):
        b, w = topk.topk_rows((Ad, Bd), k, ends="both", values=True)
        check_exact(b, S, k, False, f"int {n}x{m} d={d} k={k} best")
        check_exact(w, S, k, True, f"int {n}x{m} d={d} k={k} worst")
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:n // 2]
    check_exact(topk.topk_rows((Ad, Bd), 5, rows=rows, ends="worst", values=True), S[rows], 5, True, "row subset")


def test_factor_mode_integer_factors_c4_shape_row_subset(dev):
    from mfcd import topk
    n, m, d = C4
    A, B = int_factors(n, m, d, 44)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(2))[:64]
    S = A[rows].double() @ B.double().t()
    k = 6553
    b, w = topk.topk_rows((A.to(dev), B.to(dev)), k, rows=rows, ends="both", values=True)
    check_exact(b, S, k, False, "C4 subset best")
    check_exact(w, S, k, True, "C4 subset worst")


# ---------------------------------------------------------------------------------------------------------------------
# 3. real-valued factor mode: derived bounds against the f64 product
# ---------------------------------------------------------------------------------------------------------------------
def check_bounded(idx, val, S64, E, worst, what):
    """(a) |val - s64[idx]| <= e; (b) values monotone, equal values in ascending column order; (c) no column outside the
    returned set beats the k-th returned one by more than 2 e_max of its row.  All on the device, every row and element."""
    sgn = -1.0 if worst else 1.0
    idx = idx.long()
    s_at = torch.gather(S64, 1, idx)
    e_at = torch.gather(E, 1, idx)
    err = (val.double() - s_at).abs()
    assert bool((err <= e_at).all()), f"{what} (a): max excess {(err - e_at).max().item():.3e}"
    v0, v1 = val[:, :-1] * sgn, val[:, 1:] * sgn
    assert bool((v1 <= v0).all()), f"{what} (b): values not monotone"
    tie = v1 == v0
    assert bool((idx[:, 1:][tie] > idx[:, :-1][tie]).all()), f"{what} (b): equal values not in ascending column order"
    assert bool((torch.sort(idx, dim=1)[0].diff(dim=1) > 0).all()), f"{what}: a column returned twice"
    outside = S64.clone() * sgn
    outside.scatter_(1, idx, float("-inf"))
    kth = s_at[:, -1] * sgn
    emax = E.max(dim=1)[0]
    excess = outside.max(dim=1)[0] - (kth + 2 * emax)
    assert bool((excess <= 0).all()), f"{what} (c): an outside column beats the k-th by {excess.max().item():.3e} beyond 2 e_max"


@pytest.mark.parametrize("shape,nrows,k", [(C3, None, 100), (C5, 256, 2000)])
def test_factor_mode_real_factors_within_derived_bounds(dev, shape, nrows, k):
    from mfcd import topk
    n, m, d = shape
    A, B = base_factors(n, m, d, 11)
    Ad, Bd = A.to(dev), B.to(dev)
    rows = None if nrows is None else torch.randperm(n, generator=torch.Generator().manual_seed(3))[:nrows].to(dev)
    (bi, bv), (wi, wv) = topk.topk_rows((Ad, Bd), k, rows=rows, ends="both", values=True)
    A64, B64 = Ad.double(), Bd.double()
    order = torch.arange(n, device=dev) if rows is None else rows
    for r0 in range(0, order.numel(), 1024):
        sl = slice(r0, min(order.numel(), r0 + 1024))
        a = A64[order[sl]]
        S64, E = a @ B64.t(), dot_bound(a, B64, d)
        check_bounded(bi[sl], bv[sl], S64, E, False, f"{shape} rows {r0}.. best")
        check_bounded(wi[sl], wv[sl], S64, E, True, f"{shape} rows {r0}.. worst")


# ---------------------------------------------------------------------------------------------------------------------
# 4. exclusion
# ---------------------------------------------------------------------------------------------------------------------
def test_exclusion_equals_the_sort_without_the_barred_entries(dev):
    from mfcd import topk
    g = torch.Generator().manual_seed(9)
    n, m, k = 50, 1000, 25
    X = torch.randn(n, m, generator=g)
    pairs = torch.stack((torch.randint(0, n, (4000,), generator=g), torch.randint(0, m, (4000,), generator=g)), 1)
    short = torch.stack((torch.full((m - 3,), 7), torch.randperm(m, generator=g)[:m - 3]), 1)   # row 7 keeps 3 columns
    gone = torch.stack((torch.full((m,), 9), torch.arange(m)), 1)                                # row 9 keeps none
    pairs = torch.cat((pairs, short, gone))
    rows = torch.randperm(n, generator=g)
    Xb, Xw = X.clone(), X.clone()
    Xb[pairs[:, 0], pairs[:, 1]] = float("-inf")
    Xw[pairs[:, 0], pairs[:, 1]] = float("inf")
    left = m - torch.zeros(n, m).index_put_((pairs[:, 0], pairs[:, 1]), torch.tensor(1.0)).sum(1).long()
    for src, what in ((X.to(dev), "dense"), ):
        for excl in (pairs, {tuple(p) for p in pairs.tolist()}):
            (bi, bv), (wi, wv) = topk.topk_rows(src, k, rows=rows, ends="both", exclude=excl, values=True)
            for (gi, gv), ref, worst in (((bi, bv), Xb, False), ((wi, wv), Xw, True)):
                ri, rv = stable_ref(ref[rows], k, worst)
                keep = torch.arange(k).unsqueeze(0) < left[rows].unsqueeze(1)
                ri = torch.where(keep, ri, torch.full_like(ri, -1))
                rv = torch.where(keep, rv, torch.full_like(rv, float("nan")))
                assert torch.equal(gi.cpu().long(), ri), f"{what} worst={worst}"
                torch.testing.assert_close(gv.cpu(), rv, rtol=0, atol=0, equal_nan=True)
    assert left[7] == 3 and left[9] == 0
    # factor mode (integer factors: exact), triplet rows bar both items of their user
    A, B = int_factors(n, m, 5, 3)
    S = A.double() @ B.double().t()
    trip = torch.stack((torch.randint(0, n, (3000,), generator=g), torch.randint(0, m, (3000,), generator=g),
                        torch.randint(0, m, (3000,), generator=g)), 1)
    S[trip[:, 0], trip[:, 1]] = float("-inf")
    S[trip[:, 0], trip[:, 2]] = float("-inf")
    gi, gv = topk.topk_rows((A.to(dev), B.to(dev)), k, rows=rows, ends="best", exclude=trip, values=True)
    check_exact((gi, gv), S[rows], k, False, "factor mode with barred triplets")


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_and_both_ends_equal_the_single_end_calls(dev):
    from mfcd import topk
    n, m, d = C3
    A, B = base_factors(n, m, d, 12)
    F = (A.to(dev), B.to(dev))
    (bi, bv), (wi, wv) = topk.topk_rows(F, 100, ends="both", values=True)
    (bi2, bv2), (wi2, wv2) = topk.topk_rows(F, 100, ends="both", values=True)
    for a, b in ((bi, bi2), (wi, wi2), (bv.view(torch.int32), bv2.view(torch.int32)), (wv.view(torch.int32), wv2.view(torch.int32))):
        assert torch.equal(a, b)
    b1, v1 = topk.topk_rows(F, 100, ends="best", values=True)
    w1, x1 = topk.topk_rows(F, 100, ends="worst", values=True)
    assert torch.equal(b1, bi) and torch.equal(w1, wi)
    assert torch.equal(v1.view(torch.int32), bv.view(torch.int32)) and torch.equal(x1.view(torch.int32), wv.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 6. samplers on a FactoredMatrix
# ---------------------------------------------------------------------------------------------------------------------
# (n, m, d, seed of generate_embedding_factors): seeds chosen by running assert_unambiguous on the CPU first
SAMPLER_FIXTURES = [(200, 1000, 2, 0), (128, 4096, 3, 0)]
K_LIST = 20


def assert_unambiguous(A, B, k):
    """In f64 no two neighbours among any row's top k + 1 and bottom k + 1 scores are closer than 2 e (e of the row's
    largest-bound column): the order of the lists does not depend on how a score is rounded in fp32."""
    A64, B64 = A.double(), B.double()
    S = A64 @ B64.t()
    e = dot_bound(A64, B64, A.shape[1]).max(dim=1)[0]
    v = torch.sort(S, dim=1, descending=True)[0]
    for part, what in ((v[:, :k + 1], "top"), (v[:, -(k + 1):], "bottom")):
        gap = -(part.diff(dim=1))
        bad = int((gap < 2 * e.unsqueeze(1)).sum())
        assert bad == 0, f"{bad} ambiguous neighbour pairs among the {what} {k + 1} scores"
    return S


def sampler_fixture(n, m, d, seed):
    import generation_data as gd
    A, B = base_factors(n, m, d, seed)
    S = assert_unambiguous(A, B, K_LIST)
    return gd.FactoredMatrix(A, B), S


@pytest.mark.parametrize("n,m,d,seed", SAMPLER_FIXTURES)
def test_host_samplers_on_a_factored_matrix_replay_the_dense_run(dev, n, m, d, seed):
    import generation_data as gd
    FX, _ = sampler_fixture(n, m, d, seed)
    Xd = FX.dense()
    for fn in (gd.choose_items_by_proximity, gd.choose_items_top_k):
        out = []
        for X in (FX, Xd):
            torch.manual_seed(21)
            np.random.seed(22)
            got = fn(X, 3000, set(), k=K_LIST)
            out.append((got, torch.get_rng_state(), np.random.get_state()))
        (a, ta, na), (b, tb, nb) = out
        assert len(a) == 3000 and a == b, fn.__name__
        assert torch.equal(ta, tb), f"{fn.__name__}: torch's generator left elsewhere"
        assert na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:], f"{fn.__name__}: numpy's generator left elsewhere"


@pytest.mark.parametrize("n,m,d,seed", SAMPLER_FIXTURES)
def test_device_law_on_a_factored_matrix_equals_the_dense_law(dev, n, m, d, seed):
    from mfcd import sampling
    FX, S = sampler_fixture(n, m, d, seed)
    Xd = FX.dense().to(dev)
    order = torch.sort(S, dim=1, descending=True, stable=True)[1].numpy()
    best, worst = order[:, :K_LIST], order[:, ::-1][:, :K_LIST]
    for strategy, want in (("proximity", 4000), ("top_k", 4000)):
        a = sampling.sample_triplets(FX, want, strategy, None, device=dev, seed=5, k=K_LIST)
        b = sampling.sample_triplets(Xd, want, strategy, None, device=dev, seed=5, k=K_LIST)
        assert a.shape == (want, 3) and torch.equal(a, b), strategy
        r = a.cpu().numpy()
        assert len({tuple(t) for t in r.tolist()}) == want and (r[:, 1] != r[:, 2]).all()
        assert (best[r[:, 0]] == r[:, 1:2]).any(axis=1).all(), f"{strategy}: i outside the user's k best"
        pool_j = worst if strategy == "proximity" else best
        assert (pool_j[r[:, 0]] == r[:, 2:3]).any(axis=1).all(), f"{strategy}: j outside its list"
        short = sampling.sample_triplets(FX, 500, strategy, None, device=dev, seed=5, k=K_LIST)
        assert torch.equal(short, a[:500]), f"{strategy}: a shorter request is a prefix"
        barred = {tuple(t) for t in r[:1500].tolist()}
        more = sampling.sample_triplets(FX, 1000, strategy, barred, device=dev, seed=6, k=K_LIST).cpu().numpy()
        assert more.shape[0] == 1000 and not ({tuple(t) for t in more.tolist()} & barred), f"{strategy}: exclude"


def test_device_top_k_law_at_c4_shape_stays_factored(dev):
    import generation_data as gd
    from mfcd import sampling
    n, m, d = C4
    A, B = base_factors(n, m, d, 13)
    FX = gd.FactoredMatrix(A, B)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    trip = sampling.sample_triplets(FX, 100000, "top_k", None, device=dev, seed=1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    assert peak < 16 * 2 ** 30, f"peak device memory {peak / 2 ** 30:.2f} GiB: as much as the dense matrix"
    r = trip.cpu().numpy()
    assert r.shape == (100000, 3) and r.min() >= 0 and r[:, 0].max() < n and r[:, 1:].max() < m
    assert (r[:, 1] != r[:, 2]).all() and len({tuple(t) for t in r.tolist()}) == r.shape[0]
    # both items among the user's k = 6553 best: checked against the f64 scores of the first 256 triplets' users, the
    # k-th largest f64 score less 2 e_max being the lowest score a member of a valid list can have
    k = min(m, max(5, int(0.1 * m)))
    t = torch.from_numpy(r[:256]).long().to(dev)
    a = A.to(dev).double()[t[:, 0]]
    B64 = B.to(dev).double()
    S64, E = a @ B64.t(), dot_bound(a, B64, d)
    floor = torch.sort(S64, dim=1, descending=True)[0][:, k - 1] - 2 * E.max(dim=1)[0]
    for col in (1, 2):
        assert bool((torch.gather(S64, 1, t[:, col:col + 1]).squeeze(1) >= floor).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. public functions
# ---------------------------------------------------------------------------------------------------------------------
def test_recommend_items_against_the_dense_stable_sort(dev):
    import structure as S
    n, m, d, k = 300, 500, 8, 10
    A, B = int_factors(n, m, d, 17)
    model = S.MatrixFactorization(n, m, d)
    with torch.no_grad():
        model.U.copy_(A * 0.25)                                          # exact in fp32: every score is k / 16
        model.V.copy_(B * 0.25)
    model = model.to(dev)
    P = (A.double() * 0.25) @ (B.double() * 0.25).t()
    got = S.recommend_items(model, k=k)
    assert got.shape == (n, k) and got.dtype == torch.int32 and got.is_cuda
    assert torch.equal(got.cpu().long(), stable_ref(P, k, False)[0])
    users = [5, 299, 0, 5]
    assert torch.equal(S.recommend_items(model, users=users, k=k).cpu().long(), stable_ref(P[users], k, False)[0])
    g = torch.Generator().manual_seed(4)
    shown = {(int(u), int(i), int(j)) for u, i, j in zip(torch.randint(0, n, (5000,), generator=g),
                                                         torch.randint(0, m, (5000,), generator=g),
                                                         torch.randint(0, m, (5000,), generator=g))}
    Pb = P.clone()
    for u, i, j in shown:
        Pb[u, i] = Pb[u, j] = float("-inf")
    got = S.recommend_items(model, k=k, exclude=shown).cpu().long()
    assert torch.equal(got, stable_ref(Pb, k, False)[0])
    seen = {(u, i) for u, i, _ in shown} | {(u, j) for u, _, j in shown}
    assert not any((u, int(i)) in seen for u in range(n) for i in got[u])


def valid_topk_set(idx, S64, emax):
    """Rule (c) of the real-valued test: no column outside the set beats the set's lowest member by more than 2 e_max."""
    idx = idx.long()
    low = torch.gather(S64, 1, idx).min(dim=1)[0]
    outside = S64.clone().scatter_(1, idx, float("-inf"))
    return bool((outside.max(dim=1)[0] <= low + 2 * emax).all())


def test_topk_overlap(dev):
    import generation_data as gd
    import structure as S
    from mfcd import topk
    # the model IS the ground truth: every list is recovered
    A, B = base_factors(400, 700, 6, 19)
    model = S.MatrixFactorization(400, 700, 6)
    with torch.no_grad():
        model.U.copy_(A)
        model.V.copy_(B)
    model = model.to(dev)
    mean, per_user = S.compute_topk_overlap(model, gd.FactoredMatrix(A, B), k=10)
    assert mean == 1.0 and per_user.shape == (400,) and (per_user == 1.0).all()
    # a trained 1000 x 1000 model against its X: equal to a set intersection evaluated in numpy on lists that are valid
    # top-k sets of the f64 scores
    torch.manual_seed(0)
    np.random.seed(0)
    n = m = 1000
    X = S.generate_X(n, m, 2, dev)
    train, val, _ = S.split_dataset_from_triplets(X, 20000)
    model = S.MatrixFactorization(n, m, 2).to(dev)
    S.train_model(model, train, val, torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-5), dev, num_epochs=3)
    k = 10
    mean, per_user = S.compute_topk_overlap(model, X, k=k)
    mine = S.recommend_items(model, k=k)
    theirs = topk.topk_rows(X, k)
    U64, V64 = model.U.data.double(), model.V.data.double()
    assert valid_topk_set(mine, U64 @ V64.t(), dot_bound(U64, V64, 2).max(dim=1)[0])
    assert valid_topk_set(theirs, X.double(), torch.zeros(n, dtype=torch.float64, device=dev))
    a, b = mine.cpu().numpy(), theirs.cpu().numpy()
    want = np.array([len(set(a[u].tolist()) & set(b[u].tolist())) / k for u in range(n)])
    assert np.array_equal(per_user, want) and mean == float(want.mean())
    assert 0.0 <= mean <= 1.0
