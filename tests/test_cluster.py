"""GPU tests of the cluster sampling strategy: the two k-means kernels (include/mfcd.h: mfcd_kmeans_assign,
mfcd_kmeans_update), the host loop around them (mfcd/cluster.py), the groups law of mfcd_sample_triplets and the
public path through structure.py; and of the variance law on a FactoredMatrix.

References are f64 restatements in torch, written here.  The assignment bound is derived, not measured: scores
p . c - |c|^2 / 2 are fp32 dot products of length dim (+ the half norm), so two centres can be confused only when their
f64 squared distances differ by at most 4 (dim + 2) 2^-24 (|p|^2 + 2 max |c|^2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (P, dim, k): ragged P, dim = 1, dim past one stage, k at the limit; from 128 coordinates on, few points take the
# kernel that splits the coordinates over the waves: (300, 1025, 7), and (150, 515, 40) with both centre tiles
SHAPES = [(5, 3, 2), (257, 1, 3), (1000, 70, 20), (300, 1025, 7), (4097, 16, 64), (150, 515, 40)]
PLANTED = [(40, 60, 5), (3, 200, 8), (300, 257, 20)]                                    # (dim, P, k)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _chi2_ok(counts, probs, label, z=5.0):
    """Pearson chi-square of observed counts against a law, accepted within z sigma of its mean (dof, var 2 dof)."""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    keep = probs * counts.sum() >= 5
    c = np.append(counts[keep], counts[~keep].sum())
    q = np.append(probs[keep], probs[~keep].sum())
    c, q = c[q > 0], q[q > 0]
    stat = (((c - q * c.sum()) ** 2) / (q * c.sum())).sum()
    dof = len(c) - 1
    assert stat < dof + z * np.sqrt(2 * dof) + 10, (label, stat, dof)


def _case(P, dim, k, seed):
    """Points, and centres among which the last is a near-duplicate of the first."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(P, dim, generator=g) * 3.0
    C = torch.randn(k, dim, generator=g) * 3.0
    C[k - 1] = C[0] + 1e-6 * torch.randn(dim, generator=g)
    return pts, C


def _dist64(pts, C):
    return ((pts.double()[:, None, :] - C.double()[None, :, :]) ** 2).sum(dim=2)


def _bound(pts, C):
    dim = pts.shape[1]
    return 4 * (dim + 2) * 2.0 ** -24 * ((pts.double() ** 2).sum(1) + 2 * (C.double() ** 2).sum(1).max())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the assignment kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,dim,k", SHAPES)
def test_assign_picks_the_nearest_centre(dev, P, dim, k):
    from mfcd import cluster
    pts, C = _case(P, dim, k, 100 + P)
    D = _dist64(pts, C)
    bound = _bound(pts, C)
    g = torch.Generator().manual_seed(1)
    before = D.argmin(1).int()
    flip = torch.rand(P, generator=g) < 0.3
    before[flip] = (before[flip] + torch.randint(0, k + 1, (int(flip.sum()),), generator=g).int()) % (k + 1) - 1   # -1 .. k-1
    labels = before.to(dev)
    changed = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    out, d2 = cluster.assign(pts.to(dev), C.to(dev), labels, dist2=True, changed=changed)
    assert out is labels and out.dtype == torch.int32 and d2.dtype == torch.float32
    L = out.cpu().long()
    assert int(L.min()) >= 0 and int(L.max()) < k
    chosen = D.gather(1, L[:, None])[:, 0]
    best, arg = D.min(1)
    excess = chosen - best
    print(f"assign {P, dim, k}: max excess / bound = {float((excess / bound).max()):.3g}, labels off the f64 argmin: "
          f"{int((L != arg).sum())}, max |dist2 - D| / bound = {float(((d2.cpu().double() - chosen).abs() / bound).max()):.3g}")
    assert bool((excess <= bound).all())
    second = D.scatter(1, arg[:, None], float("inf")).min(1)[0]
    clear = second - best > bound
    assert bool((L[clear] == arg[clear]).all())
    assert bool(((d2.cpu().double() - chosen).abs() <= bound).all())
    assert int(changed) == int((before.long() != L).sum())
    # labels only (no dist2, no counter): the same labels
    assert torch.equal(cluster.assign(pts.to(dev), C.to(dev)), out)


@pytest.mark.parametrize("P,dim,k", SHAPES)
def test_assign_breaks_exact_ties_by_the_lowest_index(dev, P, dim, k):
    from mfcd import cluster
    g = torch.Generator().manual_seed(200 + P)
    pts = torch.randint(-4, 5, (P, dim), generator=g)
    C = torch.randint(-4, 5, (k, dim), generator=g)
    C[k - 1] = C[0]                                                    # duplicated centres
    if k >= 4:
        C[2] = C[1]
    pts[: min(P, k)] = C[: min(P, k)]                                   # points on centres
    D = ((pts[:, None, :] - C[None, :, :]) ** 2).sum(2)               # int64: exact
    want = (D == D.min(1, keepdim=True)[0]).int().argmax(1)            # the first of the minima
    out, d2 = cluster.assign(pts.float().to(dev), C.float().to(dev), dist2=True)
    assert torch.equal(out.cpu().long(), want)
    assert torch.equal(d2.cpu().double(), D.min(1)[0].double())       # integers: exact


# ---------------------------------------------------------------------------------------------------------------------
# 2. the update kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,dim,k", SHAPES)
def test_update_forms_the_f64_means(dev, P, dim, k):
    from mfcd import cluster
    pts, C = _case(P, dim, k, 300 + P)
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(-1, k + 1, (P,), generator=g).int()         # -1 and k are skipped
    empty = k - 1
    labels[labels == empty] = 0                                        # one cluster without members
    if P >= 3:
        labels[0], labels[1], labels[2] = -1, k, 0
    ok = (labels >= 0) & (labels < k)
    sums = torch.zeros(k, dim, dtype=torch.float64).index_add_(0, labels[ok].long(), pts[ok].double())
    n = torch.bincount(labels[ok].long(), minlength=k)
    dpts, dlab = pts.to(dev), labels.to(dev)
    c1, c2 = C.to(dev).clone(), C.to(dev).clone()
    counts = cluster.update(dpts, dlab, c1)
    counts2 = cluster.update(dpts, dlab, c2)
    assert counts.dtype == torch.int32 and torch.equal(counts.cpu().long(), n) and int(n[empty]) == 0
    assert torch.equal(c1, c2) and torch.equal(counts, counts2)      # no order-dependent sums: bit-equal
    got = c1.cpu()
    assert torch.equal(got[n == 0], C[n == 0])                         # an empty cluster keeps its centre
    mean = sums[n > 0] / n[n > 0, None].double()
    m32 = mean.float().abs()
    ulp = (torch.nextafter(m32, torch.full_like(m32, float("inf"))) - m32).double()
    err = (got[n > 0].double() - mean).abs()
    print(f"update {P, dim, k}: max error {float((err / ulp).max()):.3g} ulp")
    assert bool((err <= ulp).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host loop: Lloyd from given centres, k-means++
# ---------------------------------------------------------------------------------------------------------------------
def _planted(dim, P, k, seed, factored):
    """Items in k groups (group of item p: p % k, shuffled), group centres N(0, 200^2), noise N(0, 1) → (X, groups):
    dense X [dim, P], or a FactoredMatrix [dim, P] with dx = 6 whose item factors are planted."""
    import generation_data as gd
    g = torch.Generator().manual_seed(seed)
    groups = (torch.arange(P) % k)[torch.randperm(P, generator=g)]
    d = 6 if factored else dim
    items = 200.0 * torch.randn(k, d, generator=g)[groups] + torch.randn(P, d, generator=g)
    if factored:
        return gd.FactoredMatrix(torch.randn(dim, 6, generator=g), items), groups
    return items.t().contiguous(), groups


def _same_partition(labels, groups, k):
    pairs = {(int(a), int(b)) for a, b in zip(labels.tolist(), groups.tolist())}
    return len(pairs) == k and len({a for a, _ in pairs}) == k and len({b for _, b in pairs}) == k


def _lloyd64(pts, init, iters):
    """Labels of every iteration of plain Lloyd in f64 (first minimum on ties; an empty cluster keeps its centre)."""
    x, C = pts.double(), init.double().clone()
    out = []
    for _ in range(iters):
        D = ((x[:, None, :] - C[None, :, :]) ** 2).sum(2)
        lab = (D == D.min(1, keepdim=True)[0]).int().argmax(1)
        out.append(lab)
        for c in range(C.shape[0]):
            if bool((lab == c).any()):
                C[c] = x[lab == c].mean(0)
    return out


@pytest.mark.parametrize("factored", [False, True], ids=["dense", "factored"])
@pytest.mark.parametrize("dim,P,k", PLANTED)
def test_kmeans_from_given_centres_follows_lloyd(dev, dim, P, k, factored):
    from mfcd import cluster
    X, groups = _planted(dim, P, k, 400 + P, factored)
    pts = cluster.item_points(X, dev)
    assert pts.shape == (P, 6 if factored else dim) and pts.is_cuda and pts.dtype == torch.float32
    first = torch.tensor([int((groups == c).nonzero()[0]) for c in range(k)])
    init = pts[first.to(dev)].clone()
    labels, centres, n_iter = cluster.kmeans(pts, k, seed=0, init=init)
    assert labels.dtype == torch.int32 and centres.shape == (k, pts.shape[1]) and 2 <= n_iter <= 10
    assert torch.equal(labels.cpu().long(), groups)                    # centre c started inside planted group c
    ref = _lloyd64(pts.cpu(), init.cpu(), n_iter)
    for t in range(1, n_iter + 1):
        lt, _, it = cluster.kmeans(pts, k, seed=0, init=init, max_iter=t)
        assert it == t and torch.equal(lt.cpu().long(), ref[t - 1]), t
    assert torch.equal(init, pts[first.to(dev)])                       # the caller's init is not written to


@pytest.mark.parametrize("dim,P,k", PLANTED)
def test_kmeans_plus_plus_recovers_planted_groups(dev, dim, P, k):
    from mfcd import cluster
    X, groups = _planted(dim, P, k, 500 + P, False)
    pts = cluster.item_points(X.to(dev), dev)
    labels, centres, n_iter = cluster.kmeans(pts, k, seed=1234 + P)
    assert _same_partition(labels.cpu(), groups, k), n_iter
    assert torch.equal(cluster.assign(pts, centres), labels)           # a fixed point
    again = cluster.kmeans(pts, k, seed=1234 + P)
    assert torch.equal(again[0], labels) and torch.equal(again[1], centres)
    with pytest.raises(ValueError):
        cluster.kmeans(pts[: k - 1].contiguous(), k, seed=0)


def test_kmeans_relocates_an_empty_cluster(dev):
    """Three centres of which two coincide: the second never wins a tie, is left empty and takes the farthest point."""
    from mfcd import cluster
    pts = torch.tensor([[0.0], [1.0], [2.0], [100.0], [101.0], [250.0]], device=dev)
    init = torch.tensor([[1.0], [1.0], [100.0]], device=dev)
    labels, centres, n_iter = cluster.kmeans(pts, 3, seed=0, init=init)
    assert labels.tolist() == [0, 0, 0, 2, 2, 1] and centres[:, 0].tolist() == [1.0, 250.0, 100.5]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the groups law, on hand-built tables
# ---------------------------------------------------------------------------------------------------------------------
def test_groups_law_draws_from_two_different_groups(dev):
    from mfcd import sampling
    n, m, k = 6000, 60, 4
    rng = np.random.default_rng(0)
    group_of = np.repeat(np.arange(k), (30, 15, 10, 5))[rng.permutation(m)]
    size = np.bincount(group_of, minlength=k)
    members, offsets = sampling.group_tables(torch.from_numpy(group_of).to(dev), k)
    assert members.is_cuda and offsets.tolist() == [0, 30, 45, 55, 60]

    def draw(want, exclude=None, seed=7):
        law = sampling._Law(n, m, dev)
        c = law.c
        c.law, c.k, c.list_row_stride = sampling.LAW_GROUPS, k, m
        c.list_i, c.list_j = law.hold(members), law.hold(offsets)
        rows = sampling.run_law(law, want, exclude, seed)[0].cpu().numpy()
        assert rows.shape == (want, 3) and len({tuple(r) for r in rows.tolist()}) == want
        assert rows.min() >= 0 and rows[:, 0].max() < n and rows[:, 1:].max() < m
        assert (group_of[rows[:, 1]] != group_of[rows[:, 2]]).all()
        return rows

    r = draw(30000)
    assert np.array_equal(r, draw(30000)) and not np.array_equal(r, draw(30000, seed=8))
    assert np.array_equal(r[:1000], draw(1000))                        # attempt order: a shorter request is a prefix
    barred = {tuple(t) for t in r[:10000].tolist()}
    r2 = draw(20000, exclude=barred)
    assert not ({tuple(t) for t in r2.tolist()} & barred)
    gi, gj = group_of[r[:, 1]], group_of[r[:, 2]]
    pair = np.full((k, k), 1 / (k * (k - 1)))
    np.fill_diagonal(pair, 0.0)
    _chi2_ok(np.bincount(gi * k + gj, minlength=k * k), pair.reshape(-1), "ordered group pair")
    item_law = 1.0 / (k * size[group_of])
    _chi2_ok(np.bincount(r[:, 1], minlength=m), item_law, "groups i")
    _chi2_ok(np.bincount(r[:, 2], minlength=m), item_law, "groups j")
    _chi2_ok(np.bincount(r[:, 0] % 97, minlength=97), np.bincount(np.arange(n) % 97) / n, "groups u")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public path
# ---------------------------------------------------------------------------------------------------------------------
def test_cluster_strategy_feeds_the_reference_pipeline(dev):
    import structure as S
    n, m, k = 200, 60, 10
    X, groups = _planted(n, m, k, 77, False)
    groups = groups.numpy()
    X = X.to(dev)
    S.set_sampler_device(dev)
    S.set_label_device(dev)
    try:
        torch.manual_seed(0)
        tr, va, te = S.split_dataset_from_triplets(X, 2000, strategy="cluster")      # 10 clusters on both paths
        for ld in (tr, va, te):          # triplets, split, labels and records were made in HBM; nothing on the host yet
            assert ld.dataset._mfcd_device_records() is not None and ld.dataset._rows is None
        assert len(tr.dataset) == 1600 and len(va.dataset) == 200 and len(te.dataset) >= 500
        for ld in (tr, va):
            rows = np.asarray(ld.dataset.data)[:, :3].astype(np.int64)
            assert (groups[rows[:, 1]] != groups[rows[:, 2]]).all()
        got = S.get_triplets_from_X(X, 300, strategy="cluster", n_clusters=4)
        assert isinstance(got, set) and len(got) == 300 and all(type(v) is int for t in got for v in t)
        assert all(i != j for _, i, j in got)
    finally:
        S.set_sampler_device(None)
        S.set_label_device(None)


def test_variance_law_takes_a_factored_matrix(dev):
    import generation_data as gd
    from mfcd import sampling
    n, m, dx = 6000, 40, 6
    g = torch.Generator().manual_seed(9)
    FX = gd.FactoredMatrix(torch.randn(n, dx, generator=g), torch.randn(m, dx, generator=g) * torch.linspace(0.3, 2.0, m)[:, None])
    pv = torch.var(FX.A.double() @ FX.B.double().t(), dim=0).numpy()
    pv /= pv.sum()
    r = sampling.sample_triplets(FX, 3000, "variance", None, device=dev, seed=7).cpu().numpy()
    assert r.shape == (3000, 3) and len({tuple(t) for t in r.tolist()}) == 3000 and (r[:, 1] != r[:, 2]).all()
    seq = np.outer(pv, pv) / (1 - pv)[:, None]                         # sequential draw without replacement
    np.fill_diagonal(seq, 0.0)
    _chi2_ok(np.bincount(r[:, 1], minlength=m), seq.sum(axis=1), "factored variance i")
    _chi2_ok(np.bincount(r[:, 2], minlength=m), seq.sum(axis=0), "factored variance j")
