"""GPU tests of the fold-in solve (include/mfcd.h: mfcd_fold_in_users; mfcd/foldin.py; structure.fit_users,
structure.refit_users) against the f64 numpy model of tests/foldin_model.py.

Inputs: m = 97 items, V ~ N(0, 1 / d) in fp32, labels from a hidden u0 ~ N(0, 9 I) per row (foldin_model.make_case).
With T = mfcd_fold_in_chunk(), a call's rows have 0, 1, 3, 50, 1000, T - 1, T, T + 1 and 2 T + 3 comparisons: the empty
row, less than one chunk, exactly one, a second chunk of one comparison, three chunks with a short last one, and a row
of many chunks.

Tolerances: |U_out - u*|_inf <= 2^-22 |u*|_inf — the 2^-24 relative rounding of the fp32 output with a factor 4 of
margin; both solvers stop only after a Newton step below 2^-30 |u|_inf, so what is left of the iteration is far below
the rounding.  The objective: within 1e-9 max(1, f(u*)) — f is second-order in the iterate's error near the minimiser,
and an f64 sum of <= 5000 terms errs around 1e-12."""
import functools

import numpy as np
import pytest
import torch

import foldin_model as FM

pytestmark = pytest.mark.gpu

DS = (1, 2, 7, 16, 64)
L2S = (1e-3, 1.0)
U_TOL = 2.0 ** -22
F_TOL = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def chunk():
    from mfcd import _lib
    return _lib.load().mfcd_fold_in_chunk()


@functools.lru_cache(maxsize=None)
def case(d, labels, start):
    """The inputs of one ragged call; the same for both l2."""
    seed = 1000 * d + 10 * FM.LABELS.index(labels) + int(start)
    return FM.make_case(d, labels, FM.row_lengths(chunk()), seed, start)


@functools.lru_cache(maxsize=None)
def reference(d, l2, labels, start):
    V, rec, off, U0 = case(d, labels, start)
    return FM.solve(V, rec, off, l2, U0)


def run(dev, V, rec, off, l2, U0=None, **kw):
    from mfcd import foldin
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    out = foldin.fold_in_users(to(V), to(rec), to(off), l2, to(U0), **kw)
    return [t.cpu().numpy() for t in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("start", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("labels", FM.LABELS)
@pytest.mark.parametrize("l2", L2S)
@pytest.mark.parametrize("d", DS)
def test_parity_with_the_host_model(dev, d, l2, labels, start):
    V, rec, off, U0 = case(d, labels, start)
    ref = reference(d, l2, labels, start)
    U, f, iters, status = run(dev, V, rec, off, l2, U0)
    assert U.dtype == np.float32 and f.dtype == np.float64 and iters.dtype == np.int32 and status.dtype == np.int32
    worst_u = worst_f = 0.0
    for r, row in enumerate(ref):
        assert row.status == FM.CONVERGED, (r, "the host model did not converge on this input")
        scale = np.abs(row.u).max()
        err = np.abs(U[r].astype(np.float64) - row.u).max()
        ferr = abs(f[r] - row.objective)
        if scale > 0:
            worst_u = max(worst_u, err / (U_TOL * scale))
        worst_f = max(worst_f, ferr / (F_TOL * max(1.0, row.objective)))
        print(f"row {r}: n {off[r + 1] - off[r]} iters {iters[r]} (model {row.iters}, {row.halvings} halvings) "
              f"status {status[r]} |dU| {err:.3e} of |u*| {scale:.3e}, |df| {ferr:.3e} of f {row.objective:.6e}")
    print(f"worst share of the bounds: U {worst_u:.3f}, objective {worst_f:.3f}")
    assert (status == 0).all(), status
    for r, row in enumerate(ref):
        n = off[r + 1] - off[r]
        scale = np.abs(row.u).max()
        if scale == 0.0:
            assert not U[r].any() and bits(U[r]) == bits(np.zeros(d, dtype=np.float32))
        else:
            assert np.abs(U[r].astype(np.float64) - row.u).max() <= U_TOL * scale, r
        assert abs(f[r] - row.objective) <= F_TOL * max(1.0, row.objective), r
        assert (iters[r] >= 1) if n > 0 else (iters[r] == 0 and f[r] == 0.0), r


@pytest.mark.parametrize("d", [2, 64])
def test_two_calls_are_bit_equal_and_rows_permute(dev, d):
    V, rec, off, U0 = case(d, "hard", True)
    first = run(dev, V, rec, off, 1e-3, U0)
    assert same(first, run(dev, V, rec, off, 1e-3, U0))
    rows = len(off) - 1
    perm = np.random.default_rng(3).permutation(rows)
    blocks = [rec[off[r]:off[r + 1]] for r in perm]
    prec = np.concatenate(blocks)
    poff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    moved = run(dev, V, prec, poff, 1e-3, U0[perm])
    assert same([a[perm] for a in first], moved)


def test_many_short_rows_in_one_call_or_two(dev):
    """700 rows of 1 to 12 comparisons, d = 16: more workgroups than CUs; the same rows in two calls of 350."""
    rng = np.random.default_rng(11)
    lengths = rng.integers(1, 13, 700).tolist()
    V, rec, off, U0 = FM.make_case(16, "hard", lengths, seed=77, start=True)
    whole = run(dev, V, rec, off, 1.0, U0)
    assert (whole[3] == 0).all()
    cut = int(off[350])
    a = run(dev, V, rec[:cut], off[:351], 1.0, U0[:350])
    b = run(dev, V, rec[cut:], off[350:] - cut, 1.0, U0[350:])
    assert same(whole, [np.concatenate((x, y)) for x, y in zip(a, b)])


def test_invalid_rows_get_status_two_and_leave_the_others_alone(dev):
    d = 7
    lengths = [5, 20, 0, 64, 9, 70, 31]
    V, rec, off, U0 = FM.make_case(d, "hard", lengths, seed=5, start=True)
    V = V.copy()
    good = [0, 2, 3, 5]
    bad_index, bad_label, bad_table = 1, 4, 6
    rec = rec.copy()
    rec[off[bad_index] + 7, 2] = FM.M_ITEMS                              # an index equal to m
    rec[off[bad_label] + 3, 3] = np.float32(1.5).view(np.int32)          # z = 1.5
    own = int(rec[off[bad_table] + 2, 1])                                # an item that only the third bad row gathers:
    for r in good:                                                       # the good rows use its neighbours instead
        blk = rec[off[r]:off[r + 1], 1:3]
        for c in (0, 1):
            hit = blk[:, c] == own
            blk[hit, c] = np.where((blk[hit, 1 - c] == (own + 1) % FM.M_ITEMS), own + 2, own + 1) % FM.M_ITEMS
        assert not (blk == own).any() and (blk[:, 0] != blk[:, 1]).all()
    V[own, 3] = np.inf
    U, f, iters, status = run(dev, V, rec, off, 1e-3, U0)
    for r in (bad_index, bad_label, bad_table):
        assert status[r] == 2 and np.isnan(U[r]).all() and np.isnan(f[r]) and iters[r] == 0, r
    model = FM.solve(V, rec, off, 1e-3, U0)
    assert [row.status for row in model] == [2 if r in (bad_index, bad_label, bad_table) else 0 for r in range(7)]
    # the other rows are bit-equal to a call without the bad ones
    blocks = [rec[off[r]:off[r + 1]] for r in good]
    goff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    alone = run(dev, V, np.concatenate(blocks), goff, 1e-3, U0[good])
    assert same([a[good] for a in (U, f, iters, status)], alone)
    assert (alone[3] == 0).all()


def test_iteration_cap_stops_with_the_last_accepted_iterate(dev):
    d, l2 = 7, 1e-3
    V, rec, off, U0 = FM.make_case(d, "hard", [50], seed=21, start=True)
    z = rec[:, 3].copy().view(np.float32)
    assert FM.solve(V, rec, off, l2, U0)[0].iters > 1
    U, f, iters, status = run(dev, V, rec, off, l2, U0, max_iter=1)
    start_f = FM.objective(U0[0].astype(np.float64), FM.deltas(V, rec[:, 1], rec[:, 2]), z.astype(np.float64), l2)
    assert status[0] == 1 and iters[0] == 1 and np.isfinite(U[0]).all() and f[0] <= start_f
    one = FM.solve_row(V, rec[:, 1], rec[:, 2], z, l2, U0[0], max_iter=1)
    assert np.abs(U[0].astype(np.float64) - one.u).max() <= U_TOL * np.abs(one.u).max()     # the same single step


def test_public_path(dev):
    import structure as S
    from mfcd import engine, foldin
    torch.manual_seed(3)
    np.random.seed(3)
    n, m, d = 40, FM.M_ITEMS, 2
    X = torch.randn(n, m).to(dev)
    train, _, _ = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    rows = engine.dataset_records(train.dataset)
    N = rows.shape[0]
    # fit_users on the loader against fold_in_users on records grouped by hand
    order = np.argsort(rows[:, 0], kind="stable")
    rec = engine.pack_records(rows[order], n, m)
    off = np.concatenate(([0], np.cumsum(np.bincount(rows[:, 0].astype(np.int64), minlength=n)))).astype(np.int64)
    by_hand = foldin.fold_in_users(model.V.data, torch.from_numpy(rec).to(dev), torch.from_numpy(off).to(dev), 0.5)
    public = S.fit_users(model, train, 0.5)
    assert same([t.cpu().numpy() for t in public], [t.cpu().numpy() for t in by_hand])
    bare = S.fit_users(model.V.data, tuple(torch.from_numpy(rows[:, k].copy()) for k in range(4)), 0.5)
    n_seen = int(rows[:, 0].max()) + 1
    assert tuple(bare.U.shape) == (n_seen, d) and same([t.cpu().numpy() for t in bare],
                                                       [t[:n_seen].cpu().numpy() for t in by_hand])
    # refit_users: the exact U-step on the model's own V, warm-started from model.U
    wd = 1e-5
    before = model.U.data.clone()
    result, at_model = S.refit_users(model, train, wd)
    assert torch.equal(model.U.data, before)
    assert (result.status == 0).all()
    gap = (at_model - result.objective).cpu().numpy()
    print(f"gap f(U_model) - f(U*): min {gap.min():.3e} max {gap.max():.3e}")
    assert (gap >= 0).all() and (gap > 0).any()
    ref = FM.solve(model.V.data.cpu().numpy(), rec, off, wd * N, before.cpu().numpy())
    for r, row in enumerate(ref):
        assert abs(float(result.objective[r]) - row.objective) <= F_TOL * max(1.0, row.objective)


def test_refit_solution_fed_back_converges_at_once(dev):
    """The fp32 solution of `refit_users`, fed back as U_init: every row converges, with at most 2 iterations — one
    Newton step that removes the fp32 rounding and one whose length is below xtol.  The decrease of that first step,
    about 4e-16 H u^2, is below the 2e-16 f that f64 resolves of f (logits around 0.2 here), which is why the Armijo
    test is taken on the decrease summed term by term (include/mfcd.h): decided on two rounded values of f, rows of
    these inputs took 3 and 4 iterations, on the device and in tests/foldin_model.py alike."""
    import structure as S
    from mfcd import engine, foldin
    torch.manual_seed(3)
    np.random.seed(3)
    n, m, d, wd = 40, FM.M_ITEMS, 2, 1e-5
    X = torch.randn(n, m).to(dev)
    train, _, _ = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    result, _ = S.refit_users(model, train, wd)
    rows = engine.dataset_records(train.dataset)
    u, i, j, z = (torch.from_numpy(rows[:, k].copy()).to(dev) for k in range(4))
    rec, off = foldin.group_by_user(u, i, j, z, n)
    again = foldin.fold_in_users(model.V.data, rec, off, wd * rows.shape[0], result.U)
    print("iterations from the fed-back solution:", again.iters.tolist())
    assert (again.status == 0).all() and int(again.iters.max()) <= 2
