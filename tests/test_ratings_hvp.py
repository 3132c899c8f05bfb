"""GPU tests of the ragged pair Hessian-vector kernel and of what is built on it (include/mfcd.h: mfcd_pair_ragged_hvp;
mfcd/ratings.py: pair_ragged_hvp, ratings_hvp; mfcd/ratings_exact.py; structure.ratings_hvp, fit_users_ratings,
refit_users_ratings, refit_items_ratings, train_model_ratings_exact) against the float64 model of
tests/ratings_hvp_model.py.

Shapes: test_ratings.py's layout — with T = mfcd_pair_ragged_tile(), one call holds rows of lengths {0, 1, 2, 63, 64, 65,
T-1, T, T+1, 2T+3, 4T+1} in a shuffled order for each of nine kinds of (a, x) rows (test_pair_grad.py's `case_rows` and
integer ratings 1..5).  The direction y of a row is distinct values in [-2, 2], except for the rows of kind 2, whose y is
constant (q is exactly +0).

Tolerance, as test_pair_hvp.py states and counts it: on the mean term q_e / (L - 1), 2e-5 times the mean magnitude of
the terms (mean_l w s |y_e - y_l| from the model) plus 2e-6 max |y| of the row; deg_e / (L - 1) is held to 2e-5 mean_l
w s + 2e-6.  The per-pair arithmetic is pairs_common.h's pair_curvature, the function the dense kernel runs, and an
accumulator still adds at most 64 fp32 terms before it is widened, so that count carries over unchanged.  The references
are computed once per module."""
import functools

import numpy as np
import pytest
import torch

import pair_hvp_model as HM
import ratings_hvp_model as RH
import ratings_model as RM
from test_pair_grad import case_rows
from test_ratings import _plain_rows, _tile, build, case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
GTOL, L2 = RH.STEP_GTOL, RH.STEP_L2
CONST_KIND = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def kernel_case():
    """test_ratings.case(1.0) with a direction per row → (rows of (kind, L, a, x), y over all entries, row_off)."""
    rows = case(1.0)
    rng = np.random.default_rng(4100)
    ys = []
    for kind, L, _, _ in rows:
        ys.append(np.full(L, 0.3, np.float32) if kind == CONST_KIND else
                  (rng.permutation(L).astype(np.float64) / max(L, 1) * 4.0 - 2.0).astype(np.float32))
    row_off = np.concatenate(([0], np.cumsum([r[1] for r in rows])))
    return rows, np.concatenate(ys), row_off


@functools.lru_cache(maxsize=None)
def kernel_reference(skip):
    rows, y, row_off = kernel_case()
    a = np.concatenate([r[2] for r in rows])
    x = np.concatenate([r[3] for r in rows])
    return RH.hvp(a, y, x, row_off, skip)


def run_hvp(a, y, data, skip=False, deg=True):
    from mfcd import ratings
    out = ratings.pair_ragged_hvp(a, y, data, skip, deg)
    assert len(out) == (3 if deg else 2)
    assert all(t.dtype == torch.float32 and t.shape == a.shape for t in out[:-1])
    return tuple(t.cpu().numpy() for t in out)


def zeros_like_bytes(v):
    return np.zeros_like(v).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True])
def test_kernel_matches_the_f64_model(dev, skip):
    rows, y, row_off = kernel_case()
    data, a_dev, _, _ = build([(r[2], r[3]) for r in rows], dev)
    Q, D, status = run_hvp(a_dev, to(dev, y), data, skip)
    q, deg, mag = kernel_reference(skip)
    assert (status == 0).all() and np.isfinite(Q).all() and np.isfinite(D).all()
    worst_q = worst_d = 0.0
    for r, sl in enumerate(RM.rows_of(row_off)):
        kind, L = rows[r][0], rows[r][1]
        if L == 1:
            assert Q[sl].tobytes() == zeros_like_bytes(Q[sl]) and D[sl].tobytes() == zeros_like_bytes(D[sl])   # exactly +0
        if L < 2:
            continue
        ymax = np.abs(y[sl].astype(np.float64)).max()
        bound_q = RTOL * mag[sl] / (L - 1) + ATOL * ymax
        bound_d = RTOL * deg[sl] / (L - 1) + ATOL
        err_q = np.abs(Q[sl].astype(np.float64) - q[sl]) / (L - 1)
        err_d = np.abs(D[sl].astype(np.float64) - deg[sl]) / (L - 1)
        worst_q, worst_d = max(worst_q, (err_q / bound_q).max()), max(worst_d, (err_d / bound_d).max())
        assert (err_q <= bound_q).all(), (r, kind, L)
        assert (err_d <= bound_d).all(), (r, kind, L)
        assert abs(Q[sl].astype(np.float64).sum()) / (L - 1) <= bound_q.sum(), (r, kind, L)   # every pair enters twice
        if kind == CONST_KIND:
            assert Q[sl].tobytes() == zeros_like_bytes(Q[sl]), (r, L)                       # a constant direction: +0
        dead = deg[sl] == 0                                           # under skip-ties: no pair of the entry counts
        assert Q[sl][dead].tobytes() == zeros_like_bytes(Q[sl][dead]) and D[sl][dead].tobytes() == zeros_like_bytes(D[sl][dead])
    print(f"skip {skip}: q max error / bound {worst_q:.3f}, deg max error / bound {worst_d:.3f}")


@pytest.mark.parametrize("L", [64, 257, 1024 + 5])
def test_equal_rows_are_bit_equal_to_the_dense_kernel(dev, L):
    """The same 64-column runs from the row's start and the same arithmetic: the bits of pairs.pair_hvp_rows."""
    from mfcd import pairs
    A, X = case_rows(L)
    rng = np.random.default_rng(5200 + L)
    Y = np.stack([(rng.permutation(L).astype(np.float64) / L * 4.0 - 2.0).astype(np.float32) for _ in range(len(A))])
    data, a_dev, _, _ = build([(A[r], X[r]) for r in range(len(A))], dev)
    Q, D, status = run_hvp(a_dev, to(dev, Y.reshape(-1)), data)
    dq, dd = pairs.pair_hvp_rows(to(dev, A), to(dev, Y), True)
    assert (status == 0).all()
    assert Q.tobytes() == dq.cpu().numpy().tobytes()
    assert D.tobytes() == dd.cpu().numpy().tobytes()
    assert run_hvp(a_dev, to(dev, Y.reshape(-1)), data, deg=False)[0].tobytes() == Q.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism and edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_calls_deg_or_not_and_a_rows_place_are_bit_equal(dev):
    rows, y, row_off = kernel_case()
    pairs_ = [(r[2], r[3]) for r in rows]
    data, a_dev, _, _ = build(pairs_, dev)
    y_dev = to(dev, y)
    sls = RM.rows_of(row_off)
    for skip in (False, True):
        Q, D, _ = run_hvp(a_dev, y_dev, data, skip)
        again = run_hvp(a_dev, y_dev, data, skip)
        assert again[0].tobytes() == Q.tobytes() and again[1].tobytes() == D.tobytes()
        assert run_hvp(a_dev, y_dev, data, skip, deg=False)[0].tobytes() == Q.tobytes()
        perm = np.random.default_rng(3).permutation(len(rows))
        pdata, pa, _, _ = build([pairs_[i] for i in perm], dev)
        py = np.concatenate([y[sls[i]] for i in perm])
        PQ, PD, _ = run_hvp(pa, to(dev, py), pdata, skip)
        poff = pdata.row_off.cpu().numpy()
        for k, i in enumerate(perm):
            assert PQ[poff[k]:poff[k + 1]].tobytes() == Q[sls[i]].tobytes(), (k, i)
            assert PD[poff[k]:poff[k + 1]].tobytes() == D[sls[i]].tobytes(), (k, i)
        for i in [r for r, row in enumerate(rows) if row[0] == 8]:                     # the ratings rows, each alone
            one, oa, _, _ = build([pairs_[i]], dev)
            OQ, OD, _ = run_hvp(oa, to(dev, y[sls[i]]), one, skip)
            assert OQ.tobytes() == Q[sls[i]].tobytes() and OD.tobytes() == D[sls[i]].tobytes(), i


def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(dev):
    T = _tile()
    rows = _plain_rows([T + 37, 40, T + 37, 2 * T + 5, 70, 3, 90], 5)
    data, a_dev, a, x = build(rows, dev)
    off = data.row_off.cpu().numpy()
    y = np.random.default_rng(6).uniform(-2, 2, data.entries).astype(np.float32)
    clean = {skip: run_hvp(a_dev, to(dev, y), data, skip) for skip in (False, True)}
    assert all(np.isfinite(t).all() for out in clean.values() for t in out[:2])
    a, x, y = a.copy(), x.copy(), y.copy()
    a[off[0] + 3] = np.inf                     # first tile: the second tile's workgroup must see it
    a[off[2] + T + 30] = np.nan                # second tile: the first tile's workgroup must see it
    y[off[3] + 2 * T + 4] = -np.inf            # the last entry of a row
    y[off[4] + 1] = np.nan
    x[off[6] + 5] = np.nan                     # read under skip-ties only
    bad = build([(a[s], x[s]) for s in RM.rows_of(off)], dev)
    for skip in (False, True):
        Q, D, status = run_hvp(bad[1], to(dev, y), bad[0], skip)
        nan_rows = [0, 2, 3, 4] + ([6] if skip else [])
        assert (status == 0).all()
        for r in range(7):
            sl = slice(off[r], off[r + 1])
            if r in nan_rows:
                assert np.isnan(Q[sl]).all() and np.isnan(D[sl]).all(), (skip, r)
            else:
                assert Q[sl].tobytes() == clean[skip][0][sl].tobytes() and D[sl].tobytes() == clean[skip][1][sl].tobytes(), (skip, r)


def test_invalid_rows_get_status_2_and_nothing_of_them_is_written(dev):
    from mfcd import _lib
    rows = _plain_rows([300, 10, 20, 5], 8)
    data, a_dev, _, _ = build(rows, dev)
    off = data.row_off.cpu().numpy()                      # 0, 300, 310, 330, 335
    y_dev = to(dev, np.random.default_rng(2).uniform(-2, 2, data.entries).astype(np.float32))
    Q0, D0, st0 = run_hvp(a_dev, y_dev, data)
    assert (st0 == 0).all()
    broken_tiles = data.tile_off.cpu().numpy().copy()     # 0, 2, 3, 4, 5
    broken_tiles[2] = 2                                   # row 1 without a tile, row 2 with two
    for name, ro_edit, tile_off, bad_rows in (("decreasing", {2: 290}, None, [1]), ("past entries", {4: 336}, None, [3]),
                                              ("negative", {0: -1}, None, [0]), ("tile count", {2: 600}, None, [1, 2]),
                                              ("tile offsets", {}, broken_tiles, [1, 2])):
        ro = off.copy()
        for k, v in ro_edit.items():
            ro[k] = v
        ro_dev = to(dev, ro)
        to_dev = data.tile_off if tile_off is None else to(dev, tile_off)
        for flags in (0, 1):
            q, d = torch.full_like(a_dev, -123.0), torch.full_like(a_dev, -321.0)
            status = torch.zeros(4, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().mfcd_pair_ragged_hvp(a_dev.data_ptr(), data.value.data_ptr(), y_dev.data_ptr(),
                                                        data.entries, ro_dev.data_ptr(), 4, to_dev.data_ptr(), data.n_tiles,
                                                        flags, q.data_ptr(), d.data_ptr(), status.data_ptr(),
                                                        _lib.stream_ptr(dev)))
            q, d = q.cpu().numpy(), d.cpu().numpy()
            assert status.tolist() == [2 if r in bad_rows else 0 for r in range(4)], (name, flags)
            written = np.zeros(data.entries, dtype=bool)
            for r in range(4):
                if r not in bad_rows:
                    written[ro[r]:ro[r + 1]] = True
                    if flags == 0 and ro[r] == off[r] and ro[r + 1] == off[r + 1]:
                        sl = slice(off[r], off[r + 1])
                        assert q[sl].tobytes() == Q0[sl].tobytes() and d[sl].tobytes() == D0[sl].tobytes(), (name, r)
            assert (q[~written] == -123.0).all() and (d[~written] == -321.0).all(), (name, flags)
            assert not (q[written] == -123.0).any(), (name, flags)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ratings_hvp against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 16])
def test_ratings_hvp_matches_the_model(dev, d):
    """Q's bound carried through the gather-sums as test_pair_hvp.check_tables_hvp carries it through the GEMMs, with the
    users' lengths L in place of m: per entry (2e-5 + slack + L 2^-24) mag_e + 2e-6 (L - 1) ymax_row, plus for the exact
    product G's own (2e-5 + L 2^-24) |g_e| + 2e-6 (L - 1); slack = 2 d 2^-24 covers the rounding of y's own two dots.
    The fp32 store of the gather-sum adds 2^-23 of the entry."""
    import structure as S
    from mfcd import ratings
    n, m, s = 30, 50, 0.7
    rng = np.random.default_rng(17)
    keep = rng.random((n, m)) < 0.4
    users, items = np.nonzero(keep)
    values = rng.integers(1, 6, users.size).astype(np.float32)
    data = ratings.RatingsData(users, items, values, n, m).to(dev)
    torch.manual_seed(17 + d)
    model = S.MatrixFactorization(n, m, d).to(dev)
    g = torch.Generator().manual_seed(d)
    dU, dV = torch.randn(n, d, generator=g).to(dev), torch.randn(m, d, generator=g).to(dev)
    U, V, dUh, dVh = (t.detach().cpu().numpy().astype(np.float64) for t in (model.U, model.V, dU, dV))
    ro, item = data.row_off.cpu().numpy(), data.item.cpu().numpy().astype(np.int64)
    col = (data.col_off.cpu().numpy(), data.col_user.cpu().numpy().astype(np.int64), data.col_perm.cpu().numpy())
    Lm1 = np.repeat(np.maximum(data.lengths - 1, 0), data.lengths).astype(np.float64)
    Lr = np.repeat(data.lengths, data.lengths) * 2.0 ** -24
    for skip in (False, True):
        prob = RH.Problem(ro, item, values, s, skip)
        for gn in (False, True):
            got = S.ratings_hvp(model, data, dU, dV, s, skip, gn)
            HU, HV, (mag, y, sg) = prob.hvp(U, V, dUh, dVh, gn)
            ymax = np.concatenate([np.full(sl.stop - sl.start, np.abs(y[sl]).max() if sl.stop > sl.start else 0.0)
                                   for sl in RM.rows_of(ro)])
            eq = (RTOL + 2 * d * 2.0 ** -24 + Lr) * mag + ATOL * Lm1 * ymax
            eg = (RTOL + Lr) * np.abs(sg) + ATOL * Lm1
            bU = RM.gather_sum(np.abs(V), ro, item, eq)[0]
            bV = RM.gather_sum(np.abs(U), col[0], col[1], eq, col[2])[0]
            if not gn:
                bU = bU + RM.gather_sum(np.abs(dVh), ro, item, eg)[0]
                bV = bV + RM.gather_sum(np.abs(dUh), col[0], col[1], eg, col[2])[0]
            for name, t, want, bound in (("HU", got[0], HU, prob.c * bU), ("HV", got[1], HV, prob.c * bV)):
                assert t.dtype == torch.float32 and tuple(t.shape) == want.shape
                bound = bound + 2.0 ** -22 * np.abs(want)
                err = np.abs(t.cpu().numpy().astype(np.float64) - want)
                live = bound > 0
                print(f"d={d} skip={skip} gauss_newton={gn}: {name} max |entry| {np.abs(want).max():.3e}, max error / bound "
                      f"{(err[live] / bound[live]).max():.3f}")
                assert (err <= bound).all(), (skip, gn, name)
    with pytest.raises(ValueError):
        S.ratings_hvp(model, data, dU[:-1], dV)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the exact steps
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_problem(skip):
    """(users, items, values, U0, V, the model problem, the model's user minimisers, the gradient noise there)."""
    U0, V, users, items, values = RH.step_inputs(skip)
    order = np.lexsort((items, users))
    users, items, values = users[order], items[order], values[order]
    row_off = np.concatenate(([0], np.cumsum(np.bincount(users, minlength=RH.STEP_N))))
    prob = RH.Problem(row_off, items, values, 1.0, skip)
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(RH.STEP_D), V64, r, L2)[0] for r in range(RH.STEP_N)])
    return users, items, values, U0, V, prob, Uopt, prob.user_noise(Uopt, V64)


def step_data(skip, dev):
    from mfcd import ratings
    users, items, values = step_problem(skip)[:3]
    return ratings.RatingsData(users, items, values, RH.STEP_N, RH.STEP_M).to(dev)


def check_user_rows(res, skip, what):
    _, _, _, _, V, prob, Uopt, noise = step_problem(skip)
    paired = prob.support > 0
    rows = res.rows.cpu().numpy().astype(np.float64)
    status, ratio = res.status.cpu().numpy(), res.grad_ratio.cpu().numpy()
    assert res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (RH.STEP_N, RH.STEP_D)
    dist = np.linalg.norm(rows - Uopt, axis=1)
    bound = GTOL * np.abs(Uopt).max(axis=1) + noise / L2
    print(f"{what} skip={skip}: status {status.tolist()}, Newton {res.newton_iters.tolist()}, CG {res.cg_iters.tolist()}, "
          f"grad_ratio {np.round(ratio, 6).tolist()}, |u - u*| / bound {np.round(dist[paired] / bound[paired], 3).tolist()}")
    assert (status[paired] == 0).all() and (ratio[paired] <= GTOL).all()
    assert (dist[paired] <= bound[paired]).all()                                  # strong convexity, modulus l2
    V64 = V.astype(np.float64)
    f_model = np.array([prob.user_objective(rows[r], V64, r, L2) for r in range(RH.STEP_N)])
    np.testing.assert_allclose(res.objective_after.cpu().numpy(), f_model, rtol=RTOL, atol=ATOL)
    lone = np.flatnonzero(~paired)
    assert len(lone) == (3 if skip else 2)
    assert res.rows.cpu().numpy()[lone].tobytes() == np.zeros((len(lone), RH.STEP_D), np.float32).tobytes()   # exactly +0
    assert (status[lone] == 0).all() and (res.newton_iters.cpu().numpy()[lone] == 0).all()
    assert (res.cg_iters.cpu().numpy()[lone] == 0).all() and (res.objective_after.cpu().numpy()[lone] == 0.0).all()
    return rows


@pytest.mark.parametrize("skip", [False, True])
def test_user_step_and_fold_in_reach_the_models_minimisers(dev, skip):
    from mfcd import ratings, ratings_exact
    users, items, values, U0, V, prob, Uopt, _ = step_problem(skip)
    data, U0d, Vd = step_data(skip, dev), to(dev, U0), to(dev, V)
    res = ratings_exact.ratings_user_step(U0d, Vd, data, 1.0, L2, skip)
    check_user_rows(res, skip, "user step")
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all()
    f0 = np.array([prob.user_objective(U0[r].astype(np.float64), V.astype(np.float64), r, L2) for r in range(RH.STEP_N)])
    np.testing.assert_allclose(before, f0, rtol=RTOL, atol=ATOL)
    assert torch.equal(U0d, to(dev, U0)) and torch.equal(Vd, to(dev, V))            # the inputs are not modified
    fold = ratings_exact.ratings_user_step(None, Vd, data, 1.0, L2, skip)
    check_user_rows(fold, skip, "fold-in")
    # a user with a NaN rating: status 2, a NaN row; the others as in a call without that user (the same normaliser)
    bad_user = 0
    assert prob.support[bad_user] > 0
    vbad = values.copy()
    vbad[np.flatnonzero(users == bad_user)[1]] = np.nan
    bad = ratings_exact.ratings_user_step(U0d, Vd, ratings.RatingsData(users, items, vbad, RH.STEP_N, RH.STEP_M).to(dev),
                                          1.0, L2, skip, coef=prob.c)
    others = [r for r in range(RH.STEP_N) if r != bad_user]
    assert bad.status.tolist() == [2 if r == bad_user else 0 for r in range(RH.STEP_N)]
    assert bool(torch.isnan(bad.rows[bad_user]).all())
    rest = users != bad_user
    without = ratings_exact.ratings_user_step(U0d, Vd, ratings.RatingsData(users[rest], items[rest], values[rest], RH.STEP_N,
                                                                           RH.STEP_M).to(dev), 1.0, L2, skip, coef=prob.c)
    assert bad.rows[others].cpu().numpy().tobytes() == without.rows[others].cpu().numpy().tobytes()
    assert bad.newton_iters[others].tolist() == without.newton_iters[others].tolist()
    assert without.rows[bad_user].tolist() == [0.0] * RH.STEP_D and int(without.status[bad_user]) == 0
    with pytest.raises(ValueError):
        ratings_exact.ratings_user_step(U0d, Vd, data, 1.0, 0.0, skip)
    with pytest.raises(ValueError):
        ratings_exact.ratings_user_step(U0d, Vd[:-1], data, 1.0, L2, skip)
    lone = ratings.RatingsData([0, 1], [0, 1], [1.0, 2.0], RH.STEP_N, RH.STEP_M).to(dev)
    with pytest.raises(ValueError):
        ratings_exact.ratings_user_step(U0d, Vd, lone, 1.0, L2, skip)                 # no supporting pair


@pytest.mark.parametrize("skip", [False, True])
def test_item_step_descends_to_a_certified_point(dev, skip):
    from mfcd import ratings, ratings_exact
    users, items, values, U0, V, prob, _, _ = step_problem(skip)
    data, U0d, Vd = step_data(skip, dev), to(dev, U0), to(dev, V)
    res = ratings_exact.ratings_item_step(U0d, Vd, data, 1.0, L2, skip)
    rows = res.rows.cpu().numpy().astype(np.float64)
    U64 = U0.astype(np.float64)
    gnorm = np.linalg.norm(prob.item_grad(U64, rows, L2))
    print(f"skip={skip}: Newton {int(res.newton_iters)}, CG {int(res.cg_iters)}, |grad| {gnorm:.3e} against gtol l2 max|V| "
          f"{GTOL * L2 * np.abs(rows).max():.3e}, grad_ratio {float(res.grad_ratio):.2e}, F {float(res.objective_before):.6f} "
          f"-> {float(res.objective_after):.6f}")
    assert int(res.status) == 0 and res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (RH.STEP_M, RH.STEP_D)
    assert res.status.dim() == 0 and res.objective_after.dim() == 0
    assert float(res.objective_after) <= float(res.objective_before) and float(res.grad_ratio) <= GTOL
    np.testing.assert_allclose(float(res.objective_after), prob.item_objective(U64, rows, L2), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(res.objective_before), prob.item_objective(U64, V.astype(np.float64), L2), rtol=RTOL,
                               atol=ATOL)
    assert torch.equal(Vd, to(dev, V))
    vbad = values.copy()
    vbad[7] = np.nan
    bad = ratings_exact.ratings_item_step(U0d, Vd, ratings.RatingsData(users, items, vbad, RH.STEP_N, RH.STEP_M).to(dev), 1.0,
                                          L2, skip)
    assert int(bad.status) == 2 and torch.equal(bad.rows, Vd)


def test_alternating_fit_descends_and_records_the_models_objective(dev):
    from mfcd import ratings_exact
    skip = False
    _, _, _, U0, V, prob, _, _ = step_problem(skip)
    data = step_data(skip, dev)
    rng = np.random.default_rng(8)
    V0 = (0.3 * rng.standard_normal(V.shape)).astype(np.float32)
    tables = (to(dev, U0), to(dev, V0))
    seen = []
    for sweep in range(3):                                       # one sweep at a time
        res = ratings_exact.fit_ratings_exact(*tables, data, 1.0, L2, 1, skip)
        assert res.U is tables[0] and res.V is tables[1]
        if sweep == 0:
            start = prob.objective(U0.astype(np.float64), V0.astype(np.float64), L2)
            np.testing.assert_allclose(float(res.objective_start), start, rtol=RTOL, atol=ATOL)
            seen.append(float(res.objective_start))
        seen += res.history[0].tolist()
    U3, V3 = to(dev, U0), to(dev, V0)
    res = ratings_exact.fit_ratings_exact(U3, V3, data, 1.0, L2, 3, skip)
    flat = res.history.reshape(-1).tolist()
    print(f"F: start {seen[0]:.7f}, sub-steps {np.round(flat, 7).tolist()}")
    assert tuple(res.history.shape) == (3, 2) and not torch.equal(U3, to(dev, U0)) and not torch.equal(V3, to(dev, V0))
    assert all(b <= a for a, b in zip([float(res.objective_start)] + flat[:-1], flat))   # non-increasing
    np.testing.assert_allclose(flat, seen[1:], rtol=1e-9)        # three sweeps are three chained calls of one sweep
    np.testing.assert_allclose(U3.cpu().numpy(), tables[0].cpu().numpy(), rtol=1e-5, atol=1e-7)
    # every recorded value against the model, at the tables of that sub-step: replay with the steps
    U, Vt = to(dev, U0), to(dev, V0)
    for sweep in range(3):
        U = ratings_exact.ratings_user_step(U, Vt, data, 1.0, L2, skip).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(flat[2 * sweep], want, rtol=RTOL, atol=ATOL)
        Vt = ratings_exact.ratings_item_step(U, Vt, data, 1.0, L2, skip).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(flat[2 * sweep + 1], want, rtol=RTOL, atol=ATOL)
    assert tuple(res.user_status.shape) == (RH.STEP_N,) and res.item_status.dim() == 0


def test_a_fully_observed_table_agrees_with_the_dense_steps(dev):
    """Both rows are certified, so each lies within gtol |u|_inf of the one minimiser."""
    import structure as S
    from mfcd import population, ratings_exact
    Ustar, V, X = HM.solver_inputs(40)
    Xd, Vd = to(dev, X), to(dev, V)
    U0 = to(dev, (0.3 * np.random.default_rng(12).standard_normal(Ustar.shape)).astype(np.float32))
    data = S.observe_ratings(Xd, 1.0)
    got = ratings_exact.ratings_user_step(U0, Vd, data, 1.0, L2)
    want = population.population_user_step(U0, Vd, Xd, 1.0, L2)
    assert got.status.tolist() == [0] * 8 == want.status.tolist()
    diff = (got.rows.double() - want.rows.double()).norm(dim=1).cpu().numpy()
    room = 2 * GTOL * want.rows.abs().amax(1).cpu().numpy()
    print(f"|ragged - dense| / (2 gtol |u|_inf) {np.round(diff / room, 4).tolist()}")
    assert (diff <= room).all()
    np.testing.assert_allclose(got.objective_before.cpu().numpy(), want.objective_before.cpu().numpy(), rtol=RTOL)


def test_structure_entries_on_a_small_model(dev):
    import structure as S
    skip = False
    data = step_data(skip, dev)
    torch.manual_seed(3)
    model = S.MatrixFactorization(RH.STEP_N, RH.STEP_M, RH.STEP_D).to(dev)
    U0, V0 = model.U.detach().clone(), model.V.detach().clone()
    fold = S.fit_users_ratings(model, data, L2)
    bare = S.fit_users_ratings(model.V.data, data, L2)
    assert tuple(fold.rows.shape) == (RH.STEP_N, RH.STEP_D) and torch.equal(fold.rows, bare.rows)
    res_u, gain_u = S.refit_users_ratings(model, data, 1.0, L2)
    res_v, gain_v = S.refit_items_ratings(model, data, 1.0, L2)
    assert (gain_u >= 0).all() and float(gain_v) >= 0 and gain_v.dim() == 0 and tuple(gain_u.shape) == (RH.STEP_N,)
    assert tuple(res_v.rows.shape) == (RH.STEP_M, RH.STEP_D)
    assert torch.equal(model.U.detach(), U0) and torch.equal(model.V.detach(), V0)  # the refits leave the model alone
    hist = S.train_model_ratings_exact(model, data, 1.0, L2, sweeps=2)
    flat = [f for pair in hist for f in pair]
    assert len(hist) == 2 and all(len(pair) == 2 for pair in hist) and all(b <= a for a, b in zip(flat[:-1], flat[1:]))
    assert not torch.equal(model.U.detach(), U0) and not torch.equal(model.V.detach(), V0) and not model.training
