"""GPU tests of the one-launch ratings fold-in (include/mfcd.h: mfcd_ratings_fold_in_users; mfcd/ratings_foldin.py;
structure.fold_in_users_ratings, refit_users_ratings_kernel, ratings_user_information) against the float64 model of
tests/ratings_foldin_model.py.

Inputs: ratings_foldin_model.Family — m = 600 items, one row per length of {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 515}
in a shuffled order (the closed forms, the 64-term run, the 256-entry tile, two tiles and more), widths d in {1, 2, 3,
16, 17, 33, 64} (the kernel's forms of 4, 16, 32 and 64 columns on either side).  The kernel re-gathers the item vectors
in every pass, so there is no resident / streamed split whose boundary would need a length of its own.
test_ratings_foldin_cpu.py shows that these inputs leave room for the certificate.

Tolerances: a returned row lies within gtol |u*|_inf + noise / l2 of the model's minimiser (strong convexity, modulus
l2; noise: the gradient's fp32 bound, ratings_hvp_model.user_noise), test_ratings_hvp.py's rule; objectives are held to
that file's RTOL = 2e-5, ATOL = 2e-6; the information matrix to pair_info_model.bounds with the tie weights.  The
references are computed once per (d, skip)."""
import numpy as np
import pytest
import torch

import pair_info_model as PI
import ratings_foldin_model as FM
import ratings_hvp_model as RH

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
L2, GTOL = FM.L2, FM.GTOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table(fam, dev):
    from mfcd import ratings
    return ratings.RatingsData(fam.users, fam.items, fam.values, fam.n, FM.M_ITEMS).to(dev)


def raw(dev, V, idx, x, row_off, skip, coef, U0=None, max_newton=20, want=("objective", "grad_ratio", "info")):
    """One call of the C entry on raw arrays → dict of numpy arrays; outputs not named in `want` are passed as NULL."""
    from mfcd import _lib
    L = _lib.load()
    n, (m, d) = len(row_off) - 1, V.shape
    Vd, idxd, xd = to(dev, V.astype(np.float32)), to(dev, np.asarray(idx, np.int32)), to(dev, np.asarray(x, np.float32))
    rod = to(dev, np.asarray(row_off, np.int64))
    U0d = None if U0 is None else to(dev, np.asarray(U0, np.float32))
    rows = torch.full((n, d), 7.0, dtype=torch.float32, device=dev)
    out = {"objective": torch.full((n, 2), 7.0, dtype=torch.float64, device=dev),
           "grad_ratio": torch.full((n,), 7.0, dtype=torch.float64, device=dev),
           "info": torch.full((n, d, d), 7.0, dtype=torch.float64, device=dev)}
    its = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
    work = torch.empty(L.mfcd_ratings_fold_in_workspace_bytes(n, d, len(idx)), dtype=torch.uint8, device=dev)
    ptrs = [_lib.ptr(out[k]) if k in want else None for k in ("objective", "grad_ratio")]
    _lib.check(L.mfcd_ratings_fold_in_users(
        _lib.ptr(Vd), m, d, _lib.ptr(idxd), _lib.ptr(xd), len(idx), _lib.ptr(rod), n, FM.SCALE, 1 if skip else 0,
        float(coef), L2, _lib.ptr(U0d), max_newton, GTOL, _lib.ptr(rows), ptrs[0], ptrs[1], _lib.ptr(its),
        _lib.ptr(out["info"]) if "info" in want else None, _lib.ptr(work), work.numel(), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in want}
    res.update(rows=rows.cpu().numpy(), iters=its[:, 0].cpu().numpy(), status=its[:, 1].cpu().numpy())
    return res


def raw_family(dev, fam, **kw):
    return raw(dev, fam.V, fam.items, fam.values, fam.row_off, fam.skip, fam.prob.c, **kw)


def model_objective(fam, U):
    return np.array([fam.prob.user_objective(np.asarray(U[r], np.float64), fam.V64, r, L2) for r in range(fam.n)])


def check_rows(fam, res, start, what):
    """`res`: a PopulationStepResult of the family's table from `start` (None: zeros)."""
    p = fam.paired
    rows32 = res.rows.cpu().numpy()
    rows = rows32.astype(np.float64)
    status, ratio, iters = res.status.cpu().numpy(), res.grad_ratio.cpu().numpy(), res.newton_iters.cpu().numpy()
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert res.rows.dtype == torch.float32 and rows.shape == (fam.n, fam.d)
    dist = np.linalg.norm(rows - fam.Uopt, axis=1)
    bound = GTOL * np.abs(fam.Uopt).max(axis=1) + fam.noise / L2
    print(f"{what} d={fam.d} skip={fam.skip}: lengths {fam.lengths.tolist()}, status {status.tolist()}, Newton "
          f"{iters.tolist()}, grad_ratio {np.round(ratio, 6).tolist()}, |u - u*| / bound "
          f"{np.round(dist[p] / bound[p], 3).tolist()}")
    assert (status[p] == 0).all() and (ratio[p] <= GTOL).all()
    assert (dist[p] <= bound[p]).all()                                            # strong convexity, modulus l2
    assert (iters <= 20).all() and (iters[p] >= 1).all() and (res.cg_iters.cpu().numpy() == 0).all()
    u0 = np.zeros((fam.n, fam.d)) if start is None else start.astype(np.float64)
    np.testing.assert_allclose(before[p], model_objective(fam, u0)[p], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(after[p], model_objective(fam, rows)[p], rtol=RTOL, atol=ATOL)
    assert (after <= before).all()
    lone = np.flatnonzero(~p)
    assert len(lone) == (3 if fam.skip else 2)
    assert rows32[lone].tobytes() == np.zeros((len(lone), fam.d), np.float32).tobytes()   # exactly +0
    assert (status[lone] == 0).all() and (iters[lone] == 0).all() and (after[lone] == 0.0).all()
    assert (ratio[lone] == 0.0).all()
    np.testing.assert_allclose(before[lone], 0.5 * L2 * (u0[lone] ** 2).sum(1), rtol=1e-12, atol=0)
    return rows


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("d", FM.DS)
def test_rows_reach_the_models_minimisers(dev, d, skip):
    from mfcd import ratings_foldin
    fam = FM.family(d, skip)
    data, Vd = table(fam, dev), to(dev, fam.V)
    fold = ratings_foldin.ratings_fold_in_users(None, Vd, data, FM.SCALE, L2, skip)
    check_rows(fam, fold, None, "fold-in")
    U0d = to(dev, fam.start)
    far = ratings_foldin.ratings_fold_in_users(U0d, Vd, data, FM.SCALE, L2, skip)          # exercises rejected trials
    check_rows(fam, far, fam.start, "far start")
    assert torch.equal(U0d, to(dev, fam.start)) and torch.equal(Vd, to(dev, fam.V))        # the inputs are not modified


def check_info(fam, rows, H, status):
    for r in range(fam.n):
        sl = fam.prob.rows[r]
        Hr = H[r]
        assert Hr.tobytes() == np.ascontiguousarray(Hr.T).tobytes()               # [p][q] and [q][p] bit-equal
        if not fam.paired[r]:
            assert Hr.tobytes() == np.zeros((fam.d, fam.d)).tobytes()             # +0
            continue
        B, x = fam.V64[fam.items[sl]], fam.values[sl]
        a = B @ rows[r].astype(np.float64)
        want = FM.info(fam.prob, fam.V64, r, rows[r])
        _, hb = PI.bounds(a, B, RH.tie_weights(x, fam.skip))
        err = np.abs(Hr - want)
        print(f"  info d={fam.d} skip={fam.skip} L={sl.stop - sl.start} status {status[r]}: max |H| {np.abs(want).max():.3e}, "
              f"max error / bound {(err / hb).max():.3f}")
        assert (err <= hb).all(), r


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("d", FM.DS)
def test_information_matrices(dev, d, skip):
    from mfcd import ratings_foldin
    fam = FM.family(d, skip)
    data, Vd = table(fam, dev), to(dev, fam.V)
    res, H = ratings_foldin.ratings_fold_in_users(None, Vd, data, FM.SCALE, L2, skip, info=True)
    assert H.dtype == torch.float64 and tuple(H.shape) == (fam.n, d, d)
    check_info(fam, res.rows.cpu().numpy(), H.cpu().numpy(), res.status.cpu().numpy())
    # max_newton = 0: the start row rounded, and the information there
    U0d = to(dev, fam.start)
    res0, H0 = ratings_foldin.ratings_fold_in_users(U0d, Vd, data, FM.SCALE, L2, skip, max_newton=0, info=True)
    rows0 = res0.rows.cpu().numpy()
    p = fam.paired
    assert rows0[p].tobytes() == fam.start[p].tobytes() and (rows0[~p] == 0.0).all()
    assert (res0.newton_iters.cpu().numpy() == 0).all() and (res0.status.cpu().numpy()[p] == 1).all()
    assert (res0.objective_after.cpu().numpy()[p] == res0.objective_before.cpu().numpy()[p]).all()
    check_info(fam, rows0, H0.cpu().numpy(), res0.status.cpu().numpy())
    info = ratings_foldin.ratings_user_information(U0d, Vd, data, FM.SCALE, skip)
    assert info.info.cpu().numpy().tobytes() == H0.cpu().numpy().tobytes()
    assert info.weight.cpu().numpy().tolist() == fam.prob.support.tolist() and (info.status.cpu().numpy() == 0).all()


@pytest.mark.parametrize("skip", [False, True])
def test_same_answers_as_the_lockstep_solver(dev, skip):
    """On ratings_hvp_model.step_inputs (d = 3) the new function passes what test_ratings_hvp.check_user_rows asserts of
    ratings_user_step."""
    from mfcd import ratings, ratings_foldin
    U0, V, users, items, values = RH.step_inputs(skip)
    data = ratings.RatingsData(users, items, values, RH.STEP_N, RH.STEP_M).to(dev)
    prob = RH.Problem(data.row_off.cpu().numpy(), data.item.cpu().numpy(), data.value.cpu().numpy(), 1.0, skip)
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(RH.STEP_D), V64, r, RH.STEP_L2)[0] for r in range(RH.STEP_N)])
    noise, paired = prob.user_noise(Uopt, V64), prob.support > 0
    for what, start in (("user step", to(dev, U0)), ("fold-in", None)):
        res = ratings_foldin.ratings_fold_in_users(start, to(dev, V), data, 1.0, RH.STEP_L2, skip)
        rows = res.rows.cpu().numpy().astype(np.float64)
        status, ratio = res.status.cpu().numpy(), res.grad_ratio.cpu().numpy()
        assert res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (RH.STEP_N, RH.STEP_D)
        dist = np.linalg.norm(rows - Uopt, axis=1)
        bound = RH.STEP_GTOL * np.abs(Uopt).max(axis=1) + noise / RH.STEP_L2
        print(f"{what} skip={skip}: status {status.tolist()}, Newton {res.newton_iters.tolist()}, grad_ratio "
              f"{np.round(ratio, 6).tolist()}, |u - u*| / bound {np.round(dist[paired] / bound[paired], 3).tolist()}")
        assert (status[paired] == 0).all() and (ratio[paired] <= RH.STEP_GTOL).all()
        assert (dist[paired] <= bound[paired]).all()
        f_model = np.array([prob.user_objective(rows[r], V64, r, RH.STEP_L2) for r in range(RH.STEP_N)])
        np.testing.assert_allclose(res.objective_after.cpu().numpy(), f_model, rtol=RTOL, atol=ATOL)
        lone = np.flatnonzero(~paired)
        assert len(lone) == (3 if skip else 2)
        assert res.rows.cpu().numpy()[lone].tobytes() == np.zeros((len(lone), RH.STEP_D), np.float32).tobytes()
        assert (status[lone] == 0).all() and (res.newton_iters.cpu().numpy()[lone] == 0).all()
        assert (res.cg_iters.cpu().numpy()[lone] == 0).all() and (res.objective_after.cpu().numpy()[lone] == 0.0).all()
        assert (res.objective_after.cpu().numpy() <= res.objective_before.cpu().numpy()).all()


def same(a, b, keys=("rows", "iters", "status", "objective", "grad_ratio", "info")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys if k in a and k in b)


@pytest.mark.parametrize("d,skip", [(2, True), (17, False), (64, True)])
def test_determinism_and_independence(dev, d, skip):
    fam = FM.family(d, skip)
    one = raw_family(dev, fam, U0=fam.start)
    assert same(one, raw_family(dev, fam, U0=fam.start))                          # two calls are bit-equal
    slices = fam.prob.rows

    def subset(order):
        idx = np.concatenate([fam.items[slices[r]] for r in order])
        x = np.concatenate([fam.values[slices[r]] for r in order])
        row_off = np.concatenate(([0], np.cumsum([fam.lengths[r] for r in order])))
        return raw(dev, fam.V, idx, x, row_off, skip, fam.prob.c, U0=fam.start[order])

    order = np.random.default_rng(5).permutation(fam.n)                           # a permutation of the users
    perm = subset(order)
    assert all(perm[k].tobytes() == one[k][order].tobytes() for k in perm)
    keep = np.arange(0, fam.n, 2)                                                 # other users removed, coef fixed
    part = subset(keep)
    assert all(part[k].tobytes() == one[k][keep].tobytes() for k in part)
    # the row does not depend on which outputs are asked for
    for want in ((), ("info",), ("objective",), ("grad_ratio",)):
        less = raw_family(dev, fam, U0=fam.start, want=want)
        assert same(one, less), want
    # a NULL start is a zero start
    assert same(raw_family(dev, fam), raw_family(dev, fam, U0=np.zeros((fam.n, d), np.float32)))


def test_refused_rows(dev):
    """Validation stops each of these before any address is formed from the bad value."""
    from mfcd import _lib
    d, skip = 3, False
    fam = FM.family(d, skip)
    good = raw_family(dev, fam, U0=fam.start)
    r = int(np.flatnonzero(fam.lengths == 65)[0])
    sl = fam.prob.rows[r]
    others = np.array([q for q in range(fam.n) if q != r])
    nan32 = np.float32("nan")

    def check(res, what):
        print(f"{what}: status {res['status'].tolist()}")
        assert res["status"][r] == 2 and res["iters"][r] == 0, what
        assert np.isnan(res["rows"][r]).all() and np.isnan(res["objective"][r]).all() and np.isnan(res["info"][r]).all()
        assert all(res[k][others].tobytes() == good[k][others].tobytes() for k in res), what   # the neighbours

    for bad_index in (FM.M_ITEMS, -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min):
        idx = fam.items.copy()
        idx[sl.start + 7] = bad_index
        check(raw(dev, fam.V, idx, fam.values, fam.row_off, skip, fam.prob.c, U0=fam.start), f"item {bad_index}")
    for bad_x in (nan32, np.float32("inf")):
        x = fam.values.copy()
        x[sl.start + 3] = bad_x
        check(raw(dev, fam.V, fam.items, x, fam.row_off, skip, fam.prob.c, U0=fam.start), f"rating {bad_x}")
    used = np.zeros(FM.M_ITEMS, np.int64)
    np.add.at(used, fam.items, 1)
    mine = [i for i in fam.items[sl] if used[i] == 1]                             # an item of this user alone
    for bad_v in (nan32, np.float32("-inf")):
        V = fam.V.copy()
        V[mine[0], d - 1] = bad_v
        check(raw(dev, V, fam.items, fam.values, fam.row_off, skip, fam.prob.c, U0=fam.start), f"V entry {bad_v}")
    U0 = fam.start.copy()
    U0[r, 1] = nan32
    check(raw(dev, fam.V, fam.items, fam.values, fam.row_off, skip, fam.prob.c, U0=U0), "NaN start row")

    # descending and out-of-range offsets: rows 0 and 2 are sound, row 1 is refused; nothing of it is read
    a, b = fam.prob.rows[int(np.flatnonzero(fam.lengths == 63)[0])], fam.prob.rows[int(np.flatnonzero(fam.lengths == 64)[0])]
    idx = np.concatenate((fam.items[a], fam.items[b]))
    x = np.concatenate((fam.values[a], fam.values[b]))
    sound = raw(dev, fam.V, idx, x, [0, 63, 63, 127], skip, fam.prob.c)
    assert sound["status"].tolist() == [0, 0, 0]
    for row_off in ([0, 63, 40, 127], [0, 63, 63, 128], [0, 63, 63, 1 << 40], [-5, 63, 63, 127]):
        res = raw(dev, fam.V, idx, x, row_off, skip, fam.prob.c)
        bad = [q for q in range(3) if not (0 <= row_off[q] <= row_off[q + 1] <= 127)]
        print(f"offsets {row_off}: status {res['status'].tolist()}")
        assert bad and all(res["status"][q] == 2 and np.isnan(res["rows"][q]).all() and res["iters"][q] == 0 for q in bad)
        for q in range(3):
            if q not in bad and (row_off[q], row_off[q + 1]) in ((0, 63), (63, 127)):
                src = 0 if row_off[q] == 0 else 2
                assert all(res[k][q].tobytes() == sound[k][src].tobytes() for k in res)

    # a row longer than the cap: status 3, nothing of it is read
    cap = _lib.load().mfcd_ratings_fold_in_max_len()
    rng = np.random.default_rng(11)
    Vbig = rng.standard_normal((cap + 1, d)).astype(np.float32)
    idx = np.concatenate((fam.items[a], np.arange(cap + 1)))
    x = np.concatenate((fam.values[a], rng.integers(1, 6, cap + 1).astype(np.float32)))
    Vbig[:FM.M_ITEMS] = fam.V
    res = raw(dev, Vbig, idx, x, [0, 63, 63 + cap + 1], skip, fam.prob.c)
    assert res["status"].tolist() == [0, 3] and res["iters"][1] == 0 and np.isnan(res["rows"][1]).all()
    assert np.isnan(res["objective"][1]).all() and np.isnan(res["info"][1]).all()
    assert all(res[k][0].tobytes() == sound[k][0].tobytes() for k in res)


def test_stopped_rows(dev):
    d = 17
    fam = FM.family(d, False)
    p = fam.paired
    res = raw_family(dev, fam, U0=fam.start, max_newton=1)                         # far from the minimiser: one step is not enough
    print(f"max_newton=1: status {res['status'].tolist()}, iterations {res['iters'].tolist()}")
    assert (res["status"][p] == 1).all() and (res["iters"][p] == 1).all()
    assert np.isfinite(res["rows"]).all() and (res["objective"][:, 1] <= res["objective"][:, 0]).all()
    # ratings of one value without skip-ties: pairs, the minimiser 0, and no certificate relative to |u|_inf that a
    # non-zero iterate could meet: the row must stop, finite, and not hang
    items = np.arange(5) * 7
    U0 = np.full((1, d), 0.5, np.float32)
    res = raw(dev, fam.V, items, np.full(5, 3.0, np.float32), [0, 5], False, 0.1, U0=U0)
    print(f"all-equal row: status {res['status'].tolist()}, iterations {res['iters'].tolist()}, row max "
          f"{np.abs(res['rows']).max():.3e}, grad_ratio {res['grad_ratio'].tolist()}")
    assert res["status"].tolist() == [1] and np.isfinite(res["rows"]).all() and 1 <= res["iters"][0] <= 20
    assert res["objective"][0, 1] <= res["objective"][0, 0] and np.abs(res["rows"]).max() < 0.5


def test_structure_functions(dev):
    import structure as S
    fam = FM.family(3, True)
    data = table(fam, dev)
    model = S.MatrixFactorization(fam.n, FM.M_ITEMS, 3).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, 0.3 * fam.start))
        model.V.copy_(to(dev, fam.V))
    U_before, V_before = model.U.detach().clone(), model.V.detach().clone()
    fold = S.fold_in_users_ratings(model, data, L2, skip_ties=True)
    check_rows(fam, fold, None, "structure fold-in")
    bare = S.fold_in_users_ratings(model.V.data, data, L2, skip_ties=True)
    assert torch.equal(bare.rows, fold.rows)
    result, gain = S.refit_users_ratings_kernel(model, data, FM.SCALE, L2, skip_ties=True)
    check_rows(fam, result, 0.3 * fam.start, "structure refit")
    assert bool((gain >= 0).all()) and torch.equal(gain, result.objective_before - result.objective_after)
    info = S.ratings_user_information(model, data, FM.SCALE, skip_ties=True)
    check_info(fam, (0.3 * fam.start).astype(np.float32), info.info.cpu().numpy(), info.status.cpu().numpy())
    assert info.weight.cpu().numpy().tolist() == fam.prob.support.tolist()
    assert torch.equal(model.U.detach(), U_before) and torch.equal(model.V.detach(), V_before)   # the model is not modified
    wide = torch.zeros((FM.M_ITEMS, 65), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="ratings_user_step"):
        S.fold_in_users_ratings(wide, data, L2)
