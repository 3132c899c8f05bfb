"""GPU tests of the one-launch implicit fold-in (include/mfcd.h: mfcd_implicit_fold_in_users; mfcd/implicit_foldin.py;
structure.fold_in_users_implicit, refit_users_implicit_kernel, implicit_user_information) against the float64 model of
tests/implicit_foldin_model.py.

Inputs: implicit_foldin_model.Family — m in {97, 600} at the widths d in {1, 2, 3, 16, 17, 33, 64} (the kernel's forms of
4, 16, 32 and 64 columns on either side) and m = 2 chunk + 37 (several stages of the column loop and a ragged last one)
at d in {3, 64}; one row per observed length (the closed forms, the 64-term run, the 256-positive tile, a stage's
boundary) in a shuffled order, odd rows with barred columns.  test_implicit_foldin_cpu.py shows that these inputs leave
room for the certificate.

Tolerances: a returned row lies within gtol |u*|_inf + noise / l2 of the model's minimiser (strong convexity, modulus
l2; noise: the gradient's fp32 bound, implicit_hvp_model.Problem.user_noise); objectives are held to RTOL = 2e-5,
ATOL = 2e-6 (test_ratings_foldin.py's rule); the information matrix to pair_info_model.bounds with the bipartite 0/1
weights (implicit_foldin_model.info_bound is that bound without the m x m x d arrays; the CPU test holds the two
equal).  The references are computed once per (m, d)."""
import math

import numpy as np
import pytest
import torch

import implicit_foldin_model as FM
import implicit_hvp_model as HM

pytestmark = pytest.mark.gpu

RTOL, ATOL = FM.RTOL, FM.ATOL
L2, GTOL = FM.L2, FM.GTOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def lists(dev, rows):
    off, items = HM.lists([np.asarray(x, dtype=np.int64) for x in rows])
    return to(dev, off), to(dev, items)


def table(dev, rows, m):
    from mfcd.ratings import RatingsData
    u = np.concatenate([np.full(len(x), k) for k, x in enumerate(rows)])
    return RatingsData(u, np.concatenate(rows), np.ones(u.size), len(rows), m).to(dev)


def raw(dev, V, pos, excl, coef, U0=None, max_newton=20, want=("objective", "grad_ratio", "info"), l2=L2, pos_off=None,
        excl_off=None, entries=None):
    """One call of the C entry on raw arrays → dict of numpy arrays; outputs not named in `want` are passed as NULL.
    pos / excl: lists of columns per row (excl None: NULL lists); pos_off / excl_off / entries override the offsets."""
    from mfcd import _lib
    L = _lib.load()
    n, (m, d) = len(pos), V.shape
    off, items = HM.lists([np.asarray(x) for x in pos])
    pod, pid = to(dev, np.asarray(off if pos_off is None else pos_off, np.int64)), to(dev, np.concatenate((items, [0])).astype(np.int32))
    eod = eid = None
    excl_entries = 0
    if excl is not None:
        eoff, eitems = HM.lists([np.asarray(x) for x in excl])
        excl_entries = len(eitems)
        eod = to(dev, np.asarray(eoff if excl_off is None else excl_off, np.int64))
        eid = to(dev, np.concatenate((eitems, [0])).astype(np.int32))
    Vd = to(dev, V.astype(np.float32))
    cd = None if coef is None else to(dev, np.broadcast_to(np.asarray(coef, np.float64), (n,)).copy())
    U0d = None if U0 is None else to(dev, np.asarray(U0, np.float32))
    rows = torch.full((n, d), 7.0, dtype=torch.float32, device=dev)
    out = {"objective": torch.full((n, 2), 7.0, dtype=torch.float64, device=dev),
           "grad_ratio": torch.full((n,), 7.0, dtype=torch.float64, device=dev),
           "info": torch.full((n, d, d), 7.0, dtype=torch.float64, device=dev)}
    its = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
    work = torch.empty(L.mfcd_implicit_fold_in_workspace_bytes(n, m, d), dtype=torch.uint8, device=dev)
    ptrs = [_lib.ptr(out[k]) if k in want else None for k in ("objective", "grad_ratio", "info")]
    _lib.check(L.mfcd_implicit_fold_in_users(
        _lib.ptr(Vd), m, d, _lib.ptr(pod), _lib.ptr(pid), len(items) if entries is None else entries, _lib.ptr(eod),
        _lib.ptr(eid), excl_entries, n, _lib.ptr(cd), l2, _lib.ptr(U0d), max_newton, GTOL, _lib.ptr(rows), ptrs[0], ptrs[1],
        _lib.ptr(its), ptrs[2], _lib.ptr(work), work.numel(), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in want}
    res.update(rows=rows.cpu().numpy(), iters=its[:, 0].cpu().numpy(), status=its[:, 1].cpu().numpy())
    return res


def raw_family(dev, fam, **kw):
    return raw(dev, fam.V, fam.pos, fam.excl, fam.prob.c.max(), **kw)


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
    print(f"{what} m={fam.m} d={fam.d}: lengths {fam.lengths.tolist()}, status {status.tolist()}, Newton "
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
    assert len(lone) == (3 if fam.m == 600 else 2 if fam.m == 97 else 1)
    assert rows32[lone].tobytes() == np.zeros((len(lone), fam.d), np.float32).tobytes()   # exactly +0
    assert (status[lone] == 0).all() and (iters[lone] == 0).all() and (after[lone] == 0.0).all()
    assert (ratio[lone] == 0.0).all()
    np.testing.assert_allclose(before[lone], 0.5 * L2 * (u0[lone] ** 2).sum(1), rtol=1e-12, atol=0)
    return rows


@pytest.mark.parametrize("m,d", FM.CASES)
def test_rows_reach_the_models_minimisers(dev, m, d):
    from mfcd import implicit_foldin
    fam = FM.family(m, d)
    data, excl, Vd = lists(dev, fam.pos), lists(dev, fam.excl), to(dev, fam.V)
    fold = implicit_foldin.implicit_fold_in_users(None, Vd, data, L2, excl)
    check_rows(fam, fold, None, "fold-in")
    U0d = to(dev, fam.start)
    far = implicit_foldin.implicit_fold_in_users(U0d, Vd, data, L2, excl)                  # a start away from zero
    check_rows(fam, far, fam.start, "far start")
    assert torch.equal(U0d, to(dev, fam.start)) and torch.equal(Vd, to(dev, fam.V))        # the inputs are not modified
    assert torch.equal(data[1], lists(dev, fam.pos)[1]) and torch.equal(excl[1], lists(dev, fam.excl)[1])


def check_info(fam, rows, H, status, bounded):
    for r in range(fam.n):
        Hr = H[r]
        assert Hr.tobytes() == np.ascontiguousarray(Hr.T).tobytes()               # [p][q] and [q][p] bit-equal
        if not fam.paired[r]:
            assert Hr.tobytes() == np.zeros((fam.d, fam.d)).tobytes()             # +0
            continue
        assert np.isfinite(Hr).all()
        if not bounded:
            continue
        P, N = fam.prob.classes[r]
        u = rows[r].astype(np.float64)
        want = FM.info(fam.prob, fam.V64, r, u)
        hb = FM.info_bound(fam.V64 @ u, fam.V64, P, N)
        err = np.abs(Hr - want)
        print(f"  info m={fam.m} d={fam.d} L={fam.lengths[r]} status {status[r]}: max |H| {np.abs(want).max():.3e}, "
              f"max error / bound {(err / hb).max():.3f}")
        assert (err <= hb).all(), r


@pytest.mark.parametrize("m,d", FM.CASES)
def test_information_matrices(dev, m, d):
    from mfcd import implicit_foldin
    fam = FM.family(m, d)
    data, excl, Vd = lists(dev, fam.pos), lists(dev, fam.excl), to(dev, fam.V)
    bounded = m in (97, 600)
    res, H = implicit_foldin.implicit_fold_in_users(None, Vd, data, L2, excl, info=True)
    assert H.dtype == torch.float64 and tuple(H.shape) == (fam.n, d, d)
    check_info(fam, res.rows.cpu().numpy(), H.cpu().numpy(), res.status.cpu().numpy(), bounded)
    # max_newton = 0: the start row rounded, and the information there
    U0d = to(dev, fam.start)
    res0, H0 = implicit_foldin.implicit_fold_in_users(U0d, Vd, data, L2, excl, max_newton=0, info=True)
    rows0 = res0.rows.cpu().numpy()
    p = fam.paired
    assert rows0[p].tobytes() == fam.start[p].tobytes() and (rows0[~p] == 0.0).all()
    assert (res0.newton_iters.cpu().numpy() == 0).all() and (res0.status.cpu().numpy()[p] == 1).all()
    assert (res0.status.cpu().numpy()[~p] == 0).all()
    assert (res0.objective_after.cpu().numpy()[p] == res0.objective_before.cpu().numpy()[p]).all()
    check_info(fam, rows0, H0.cpu().numpy(), res0.status.cpu().numpy(), bounded)
    info = implicit_foldin.implicit_user_information(U0d, Vd, data, excl)
    assert info.info.cpu().numpy().tobytes() == H0.cpu().numpy().tobytes()
    assert info.weight.cpu().numpy().tolist() == fam.pairs.tolist() and (info.status.cpu().numpy() == 0).all()


@pytest.mark.parametrize("m", [40, FM.CHUNK + 5])
def test_same_answers_as_the_lockstep_solver(dev, m):
    """On implicit_hvp_model.step_inputs the new function passes what test_implicit_hvp.py asserts of implicit_user_step,
    and its rows lie within the sum of the two bounds of implicit_user_step's rows."""
    from mfcd import _lib, implicit_exact, implicit_foldin
    assert _lib.load().mfcd_implicit_fold_in_chunk() == FM.CHUNK
    Ustar, V, pos = HM.step_inputs(m)
    data = lists(dev, pos)
    prob, Uopt, noise = HM.user_minimisers(m)
    paired = prob.paired
    U0, Vd = torch.zeros(8, 3, device=dev), to(dev, V)
    res = implicit_foldin.implicit_fold_in_users(U0, Vd, data, HM.L2)
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert res.rows.dtype == torch.float32 and res.status.tolist() == [0] * 8
    V64 = V.astype(np.float64)
    gnorm = np.array([np.linalg.norm(prob.user_grad(rows[r], V64, r, HM.L2)) for r in range(8)])
    bound = HM.GTOL * HM.L2 * np.abs(rows).max(axis=1) + noise
    dist = np.linalg.norm(rows - Uopt, axis=1)
    print(f"m={m}: Newton {res.newton_iters.tolist()}, |grad| / bound {np.round(gnorm[paired] / bound[paired], 3).tolist()}, "
          f"|u - u*| / (bound / l2) {np.round(dist[paired] / (bound[paired] / HM.L2), 3).tolist()}, grad_ratio "
          f"{np.round(res.grad_ratio.cpu().numpy(), 5).tolist()}")
    assert (gnorm <= bound).all()
    assert (dist <= bound / HM.L2).all()                         # strong convexity, modulus l2
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all() and (res.grad_ratio.cpu().numpy() <= HM.GTOL).all()
    f_model = np.array([prob.user_objective(rows[r], V64, r, HM.L2) for r in range(8)])
    np.testing.assert_allclose(after, f_model, rtol=RTOL, atol=ATOL)
    # the two users without a pair: exactly +0, no iteration
    assert res.rows[[1, 2]].cpu().numpy().tobytes() == np.zeros((2, 3), dtype=np.float32).tobytes()
    assert res.newton_iters[[1, 2]].tolist() == [0, 0] == res.cg_iters[[1, 2]].tolist() and (after[[1, 2]] == 0).all()
    assert (res.newton_iters.cpu().numpy()[paired] > 0).all()
    # started elsewhere, such a user still returns the zero row and reports what its start cost
    U1 = torch.full((8, 3), 0.25, device=dev)
    moved = implicit_foldin.implicit_fold_in_users(U1, Vd, data, HM.L2)
    assert moved.rows[[1, 2]].cpu().numpy().tobytes() == np.zeros((2, 3), dtype=np.float32).tobytes()
    np.testing.assert_allclose(moved.objective_before[[1, 2]].cpu().numpy(), 0.5 * HM.L2 * 3 * 0.25 ** 2, rtol=1e-12)
    assert moved.status.tolist() == [0] * 8
    np.testing.assert_allclose(moved.rows.cpu().numpy(), rows, rtol=0, atol=2 * (bound / HM.L2).max())
    # the fold-in: users who were not in training, from their lists alone, under the training table's normaliser
    c = float(prob.c[0])
    full = implicit_foldin.implicit_fold_in_users(None, Vd, data, HM.L2, coef=c)
    assert full.rows.cpu().numpy().tobytes() == res.rows.cpu().numpy().tobytes()         # the same problem as above
    some = [3, 5, 7, 1]
    fold = implicit_foldin.implicit_fold_in_users(None, Vd, lists(dev, [pos[u] for u in some]), HM.L2, coef=c)
    assert fold.rows.cpu().numpy().tobytes() == full.rows[some].cpu().numpy().tobytes()
    assert fold.status.tolist() == [0] * 4 and fold.newton_iters.tolist() == full.newton_iters[some].tolist()
    # a user with a NaN start row: status 2, a NaN row; its neighbours as without it
    Ubad = U0.clone()
    Ubad[3, 1] = float("nan")
    bad = implicit_foldin.implicit_fold_in_users(Ubad, Vd, data, HM.L2)
    others = [0, 1, 2, 4, 5, 6, 7]
    assert bad.status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and bool(torch.isnan(bad.rows[3]).all())
    assert bad.rows[others].cpu().numpy().tobytes() == res.rows[others].cpu().numpy().tobytes()
    assert bad.newton_iters[others].tolist() == res.newton_iters[others].tolist()
    assert torch.equal(bad.objective_after[others], res.objective_after[others])
    # against the lockstep solver: both lie within their bound of the same minimiser
    lock = implicit_exact.implicit_user_step(U0, Vd, data, HM.L2)
    lrows = lock.rows.cpu().numpy().astype(np.float64)
    lbound = HM.GTOL * HM.L2 * np.abs(lrows).max(axis=1) + noise
    apart = np.linalg.norm(rows - lrows, axis=1)
    print(f"m={m}: |kernel - lockstep| / (sum of the bounds) {np.round(apart[paired] / ((bound + lbound)[paired] / HM.L2), 3).tolist()}")
    assert (apart <= (bound + lbound) / HM.L2).all()


def test_short_row_under_a_tiny_normaliser(dev):
    """A user with 3 observed items under a whole table's 1 / pairs = 1e-7, from the far start: the risk part of f is
    tiny against the ridge part.  The row is certified.  A build without the pair-by-pair decrease
    (VALUES_ONLY_STOPPED's) certifies rows of this kind as well (measured on 16 rows of 3 to 200 observed items under
    coef = 1e-7, l2 = 3e-2: the same statuses and iteration counts): coef scales only the fp32 part of f, so f's
    rounding is far below the decrease here.  test_the_decrease_summed_pair_by_pair_decides holds the inputs on which
    that path decides."""
    d, m = 17, 600
    fam = FM.family(m, d)
    r = int(np.flatnonzero(fam.lengths == 3)[0])
    res = raw(dev, fam.V, [fam.pos[r]], [fam.excl[r]], 1e-7, U0=fam.start[[r]])
    print(f"short row: status {res['status'].tolist()}, Newton {res['iters'].tolist()}, grad_ratio {res['grad_ratio'].tolist()}, "
          f"objective {res['objective'].tolist()}")
    assert res["status"].tolist() == [0] and res["grad_ratio"][0] <= GTOL and 1 <= res["iters"][0] <= 20
    prob = HM.Problem(m, [fam.pos[r]], [fam.excl[r]], coef=1e-7)
    ustar = FM.minimiser(prob, fam.V64, 0, L2)
    bound = GTOL * np.abs(ustar).max() + FM.user_noise(prob, fam.V64, 0, ustar) / L2
    assert np.linalg.norm(res["rows"][0].astype(np.float64) - ustar) <= bound


# What a build of the kernel without the pair-by-pair decrease (csrc/implicit_foldin.hip compiled with
# -DMFCD_IF_VALUES_ONLY: `make exp NAME=values_only EXPFLAGS=-DMFCD_IF_VALUES_ONLY`, run with MFCD_LIB set to it) returned
# on the inputs of the next two tests, recorded on one MI355X: the rows it left at status 1, with their iteration counts.
# The shipped kernel certifies every one of them; under that build both tests fail.
VALUES_ONLY_STOPPED = {("decrease", 3, "zero"): {12: 17}, ("decrease", 3, "far"): {10: 20}, ("decrease", 16, "far"): {11: 19, 13: 20},
                       ("decrease", 64, "zero"): {14: 15}, ("unit coef", 3): {3: 20, 10: 20, 11: 20},
                       ("unit coef", 16): {1: 20, 3: 20, 6: 20, 11: 20}}


@pytest.mark.parametrize("d", [3, 16, 64])
def test_the_decrease_summed_pair_by_pair_decides(dev, d):
    """implicit_foldin_model.DecreaseFamily: f is dominated by its fp32 part, so the last Newton steps' decreases lie
    below the rounding of the two values of f and the Armijo test on the values alone halves the step until the row
    stops (VALUES_ONLY_STOPPED: measured, not estimated).  With the decrease summed pair by pair every row is certified
    from both starts.  The worst-case noise bound of these inputs does not promise that (it is up to 120 times the
    certificate's term); the kernel's arithmetic is deterministic, so what is asserted is what it does on exactly these
    inputs, and the distance bound holds for any certified row."""
    fam = FM.decrease_family(d)
    l2 = FM.DECREASE_L2
    for name, U0 in (("zero", None), ("far", fam.start)):
        res = raw(dev, fam.V, fam.pos, None, FM.DECREASE_COEF, U0=U0, l2=l2)
        dist = np.linalg.norm(res["rows"].astype(np.float64) - fam.Uopt, axis=1)
        bound = GTOL * np.abs(fam.Uopt).max(axis=1) + fam.noise / l2
        print(f"decrease d={d} {name}: status {res['status'].tolist()}, Newton {res['iters'].tolist()}, grad_ratio "
              f"{np.round(res['grad_ratio'], 6).tolist()}, the values-only build stopped {VALUES_ONLY_STOPPED.get(('decrease', d, name), {})}")
        assert (res["status"] == 0).all() and (res["grad_ratio"] <= GTOL).all() and (res["iters"] <= 20).all()
        assert (dist <= bound).all()
        assert (res["objective"][:, 1] <= res["objective"][:, 0]).all()


@pytest.mark.parametrize("d", [3, 16])
def test_rejected_trials_still_certify(dev, d):
    """The m = 600 family under coef = NULL (1) from the far start: the curvature at the start is far from the
    minimiser's, full Newton steps overshoot, and the model rejects up to 6 trials per row (test_implicit_foldin_cpu.py
    asserts it) — the halving, the kept direction and the doubling back all run.  Every paired row must still be
    certified within 20 iterations; the values-only build leaves 3 and 4 of them at the cap (VALUES_ONLY_STOPPED).
    Checked against the model: f at the returned row, and the model's gradient there within the certificate plus the
    gradient's fp32 bound."""
    fam = FM.family(600, d)
    prob = HM.Problem(600, fam.pos, fam.excl, coef=1.0)
    p = prob.paired
    res = raw(dev, fam.V, fam.pos, fam.excl, None, U0=fam.start)
    rows = res["rows"].astype(np.float64)
    print(f"unit coef d={d}: status {res['status'].tolist()}, Newton {res['iters'].tolist()}, the values-only build stopped "
          f"{VALUES_ONLY_STOPPED[('unit coef', d)]}")
    assert (res["status"] == 0).all() and (res["grad_ratio"] <= GTOL).all() and (res["iters"] <= 20).all()
    assert res["iters"][p].min() >= 2 and res["iters"][p].max() >= 10                 # more trials than Newton steps
    assert (res["objective"][:, 1] <= res["objective"][:, 0]).all()
    for r in np.flatnonzero(p):
        f_model = prob.user_objective(rows[r], fam.V64, r, L2)
        np.testing.assert_allclose(res["objective"][r, 1], f_model, rtol=RTOL, atol=ATOL)
        g = np.linalg.norm(prob.user_grad(rows[r], fam.V64, r, L2))
        assert g <= GTOL * L2 * np.abs(rows[r]).max() + FM.user_noise(prob, fam.V64, r, rows[r])


def same(a, b, keys=("rows", "iters", "status", "objective", "grad_ratio", "info")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys if k in a and k in b)


@pytest.mark.parametrize("d,m", [(2, 97), (17, 600), (64, 600)])
def test_determinism_and_independence(dev, d, m):
    fam = FM.family(m, d)
    c = fam.prob.c.max()
    one = raw_family(dev, fam, U0=fam.start)
    assert same(one, raw_family(dev, fam, U0=fam.start))                          # two calls are bit-equal

    def subset(order):
        return raw(dev, fam.V, [fam.pos[r] for r in order], [fam.excl[r] for r in order], c, U0=fam.start[order])

    order = np.random.default_rng(5).permutation(fam.n)                           # a permutation of the users
    perm = subset(order)
    assert all(perm[k].tobytes() == one[k][order].tobytes() for k in perm)
    keep = np.arange(0, fam.n, 2)                                                 # other users removed, coef fixed
    part = subset(keep)
    assert all(part[k].tobytes() == one[k][keep].tobytes() for k in part)
    # the row does not depend on which outputs are asked for
    for want in ((), ("info",), ("objective",), ("grad_ratio",), ("objective", "info"), ("grad_ratio", "info"),
                 ("objective", "grad_ratio")):
        less = raw_family(dev, fam, U0=fam.start, want=want)
        assert same(one, less), want
    # a NULL start is a zero start
    assert same(raw_family(dev, fam), raw_family(dev, fam, U0=np.zeros((fam.n, d), np.float32)))
    # NULL barred lists are empty barred lists
    assert same(raw(dev, fam.V, fam.pos, None, c, U0=fam.start),
                raw(dev, fam.V, fam.pos, [np.zeros(0, np.int64)] * fam.n, c, U0=fam.start))


def test_refused_rows(dev):
    """Validation stops each of these before any address is formed from the bad value."""
    from mfcd import _lib
    L = _lib.load()
    d, m = 3, 600
    fam = FM.family(m, d)
    c = fam.prob.c.max()
    good = raw_family(dev, fam, U0=fam.start)
    r = int(np.flatnonzero(fam.lengths == 64)[0])
    assert len(fam.excl[r]) == 5                                                  # an odd row: it has a barred list
    others = np.array([q for q in range(fam.n) if q != r])
    nan32 = np.float32("nan")

    def check(res, what, status=2):
        print(f"{what}: status {res['status'].tolist()}")
        assert res["status"][r] == status and res["iters"][r] == 0, what
        assert np.isnan(res["rows"][r]).all() and np.isnan(res["objective"][r]).all() and np.isnan(res["info"][r]).all()
        assert np.isnan(res["grad_ratio"][r])
        assert all(res[k][others].tobytes() == good[k][others].tobytes() for k in res), what   # the neighbours

    def with_row(pos_r=None, excl_r=None):
        pos, excl = list(fam.pos), list(fam.excl)
        if pos_r is not None:
            pos[r] = pos_r
        if excl_r is not None:
            excl[r] = excl_r
        return pos, excl

    for bad_item in (m, -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min):
        for which in (0, 1):
            row = np.array((fam.pos[r], fam.excl[r])[which], dtype=np.int64)
            row[3] = bad_item
            pos, excl = with_row(*((row, None) if which == 0 else (None, row)))
            check(raw(dev, fam.V, pos, excl, c, U0=fam.start), f"item {bad_item} in list {which}")
    for which in (0, 1):                                                          # not strictly ascending: a repeat, a swap
        for kind in ("repeat", "swap"):
            row = np.array((fam.pos[r], fam.excl[r])[which], dtype=np.int64)
            if kind == "repeat":
                row[2] = row[1]
            else:
                row[[1, 2]] = row[[2, 1]]
            pos, excl = with_row(*((row, None) if which == 0 else (None, row)))
            check(raw(dev, fam.V, pos, excl, c, U0=fam.start), f"{kind} in list {which}")
    P, N = fam.prob.classes[r]
    for col, bad_v in ((P[4], nan32), (N[7], np.float32("-inf")), (N[-1], np.float32("inf"))):   # a V row the user uses
        V = fam.V.copy()
        V[col, d - 1] = bad_v
        res = raw(dev, V, fam.pos, fam.excl, c, U0=fam.start)
        print(f"V[{col}] = {bad_v}: status {res['status'].tolist()}")
        assert res["status"][r] == 2 and np.isnan(res["rows"][r]).all() and np.isnan(res["info"][r]).all()
    V = fam.V.copy()                                                              # a barred column's row is not used
    V[fam.excl[r][0]] = nan32
    res = raw(dev, V, [fam.pos[r]], [fam.excl[r]], c, U0=fam.start[[r]])
    assert all(res[k][0].tobytes() == good[k][r].tobytes() for k in res)
    U0 = fam.start.copy()
    U0[r, 1] = nan32
    check(raw(dev, fam.V, fam.pos, fam.excl, c, U0=U0), "NaN start row")
    for bad_c in (0.0, -1e-6, float("nan"), float("inf")):
        cs = np.full(fam.n, c)
        cs[r] = bad_c
        check(raw(dev, fam.V, fam.pos, fam.excl, cs, U0=fam.start), f"coef {bad_c}")

    # descending and out-of-range offsets: rows 0 and 2 are sound, row 1 is refused; nothing of it is read
    a, b = fam.pos[int(np.flatnonzero(fam.lengths == 63)[0])], fam.pos[int(np.flatnonzero(fam.lengths == 64)[0])]
    three = [a, np.zeros(0, np.int64), b]
    sound = raw(dev, fam.V, three, None, c)
    assert sound["status"].tolist() == [0, 0, 0]
    for pos_off in ([0, 63, 40, 127], [0, 63, 63, 128], [0, 63, 63, 1 << 40], [-5, 63, 63, 127]):
        res = raw(dev, fam.V, three, None, c, pos_off=pos_off)
        bad = [q for q in range(3) if not (0 <= pos_off[q] <= pos_off[q + 1] <= 127)]
        print(f"offsets {pos_off}: status {res['status'].tolist()}")
        assert bad and all(res["status"][q] == 2 and np.isnan(res["rows"][q]).all() and res["iters"][q] == 0 for q in bad)
        for q in range(3):
            if q not in bad and (pos_off[q], pos_off[q + 1]) in ((0, 63), (63, 127)):
                src = 0 if pos_off[q] == 0 else 2
                assert all(res[k][q].tobytes() == sound[k][src].tobytes() for k in res)
    none = [np.zeros(0, np.int64)] * 3
    for excl_off in ([0, 0, -1, 0], [0, 2, 0, 0], [0, 0, 0, 1]):                  # the barred list's offsets likewise
        res = raw(dev, fam.V, three, none, c, excl_off=excl_off)
        bad = [q for q in range(3) if not (0 <= excl_off[q] <= excl_off[q + 1] <= 0)]
        print(f"barred offsets {excl_off}: status {res['status'].tolist()}")
        assert bad and all(res["status"][q] == 2 and np.isnan(res["rows"][q]).all() for q in bad)
        assert all(res["status"][q] == 0 for q in range(3) if q not in bad)

    # a row over the pairs cap: refused from its lengths, status 3; its neighbour is unaffected
    cap = L.mfcd_implicit_fold_in_max_pairs()
    half = math.isqrt(cap - 1) + 2                                                # > sqrt(cap)
    mb = 2 * half + 2
    rng = np.random.default_rng(11)
    Vbig = rng.standard_normal((mb, d)).astype(np.float32)
    Vbig[:m] = fam.V
    near = raw(dev, Vbig, [a], None, c)
    res = raw(dev, Vbig, [a, np.arange(0, mb, 2)], None, c)
    assert (mb // 2) * (mb - mb // 2) > cap
    assert res["status"].tolist() == [0, 3] and res["iters"][1] == 0 and np.isnan(res["rows"][1]).all()
    assert np.isnan(res["objective"][1]).all() and np.isnan(res["info"][1]).all() and np.isnan(res["grad_ratio"][1])
    assert all(res[k][0].tobytes() == near[k][0].tobytes() for k in res)
    # a row over the positives cap
    mp = L.mfcd_implicit_fold_in_max_pos()
    Vp = rng.standard_normal((mp + 2, d)).astype(np.float32)
    res = raw(dev, Vp, [np.arange(5), np.arange(mp + 1)], None, c)
    assert res["status"].tolist() == [0, 3] and np.isnan(res["rows"][1]).all() and res["iters"][1] == 0
    # ... one that is over it only before its barred columns are taken out is solved (101 positives, one negative) ...
    res = raw(dev, Vp, [np.arange(mp + 1)], [np.arange(mp - 100)], c)
    assert res["status"][0] in (0, 1) and res["iters"][0] >= 1 and np.isfinite(res["rows"]).all()
    # ... and where the lengths do not decide, the counts do: a barred column that is not observed
    res = raw(dev, Vp, [np.arange(5), np.arange(mp + 1)], [[], [mp + 1]], c)
    assert res["status"].tolist() == [0, 3] and np.isnan(res["rows"][1]).all() and res["iters"][1] == 0


def test_bad_calls_are_refused_before_the_device(dev):
    from mfcd import _lib, implicit_foldin
    import structure as S
    L = _lib.load()
    fam = FM.family(97, 3)
    Vd = to(dev, fam.V)
    off, items = lists(dev, fam.pos)
    rows = torch.empty((fam.n, 3), dtype=torch.float32, device=dev)
    its = torch.empty((fam.n, 2), dtype=torch.int32, device=dev)
    work = torch.empty(256, dtype=torch.uint8, device=dev)

    def call(V=Vd, d=3, l2=L2, max_newton=20, gtol=GTOL, out=rows, ws=work, ws_bytes=256):
        return L.mfcd_implicit_fold_in_users(_lib.ptr(V), 97, d, _lib.ptr(off), _lib.ptr(items), items.numel(), None, None, 0,
                                             fam.n, None, l2, None, max_newton, gtol, _lib.ptr(out), None, None,
                                             _lib.ptr(its), None, _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev))

    assert call() == 0
    assert call(d=65) == -1 and call(l2=0.0) == -1 and call(l2=float("nan")) == -1 and call(max_newton=1001) == -1
    assert call(gtol=-1.0) == -1 and call(out=Vd) == -1 and call(V=None) == -1 and call(ws=None) == -1
    assert call(ws_bytes=255) == -2
    wide = torch.zeros((97, 65), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="implicit_user_step"):
        implicit_foldin.implicit_fold_in_users(None, wide, (off, items), L2)
    with pytest.raises(ValueError, match="implicit_user_step"):
        S.fold_in_users_implicit(wide, table(dev, fam.pos, 97), L2)


def test_stopped_rows(dev):
    fam = FM.family(600, 17)
    p = fam.paired
    res = raw_family(dev, fam, U0=fam.start, max_newton=1)                         # far from the minimiser: one step is not enough
    print(f"max_newton=1: status {res['status'].tolist()}, iterations {res['iters'].tolist()}")
    assert (res["status"][p] == 1).all() and (res["iters"][p] == 1).all()
    assert (res["status"][~p] == 0).all() and (res["iters"][~p] == 0).all()
    assert np.isfinite(res["rows"]).all() and (res["objective"][:, 1] <= res["objective"][:, 0]).all()


def test_structure_functions(dev):
    import structure as S
    from mfcd import implicit_foldin
    m, d = 600, 3
    fam = FM.family(m, d)
    data, excl = table(dev, fam.pos, m), lists(dev, fam.excl)
    model = S.MatrixFactorization(fam.n, m, d).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, 0.3 * fam.start))
        model.V.copy_(to(dev, fam.V))
    U_before, V_before = model.U.detach().clone(), model.V.detach().clone()
    fold = S.fold_in_users_implicit(model, data, L2, exclude=excl)
    check_rows(fam, fold, None, "structure fold-in")
    module = implicit_foldin.implicit_fold_in_users(None, model.V.data, lists(dev, fam.pos), L2, excl)
    assert all(torch.equal(a, b) for a, b in zip(fold, module))                   # bit-equal to the module call
    assert torch.equal(S.fold_in_users_implicit(model.V.data, data, L2, exclude=excl).rows, fold.rows)
    result, gain = S.refit_users_implicit_kernel(model, data, L2, exclude=excl)
    check_rows(fam, result, (0.3 * fam.start).astype(np.float32), "structure refit")
    assert bool((gain >= 0).all()) and torch.equal(gain, result.objective_before - result.objective_after)
    info = S.implicit_user_information(model, data, exclude=excl)
    want = implicit_foldin.implicit_user_information(model.U.data, model.V.data, lists(dev, fam.pos), excl)
    assert all(torch.equal(a, b) for a, b in zip(info, want))
    check_info(fam, (0.3 * fam.start).astype(np.float32), info.info.cpu().numpy(), info.status.cpu().numpy(), True)
    assert info.weight.cpu().numpy().tolist() == fam.pairs.tolist()
    assert torch.equal(model.U.detach(), U_before) and torch.equal(model.V.detach(), V_before)   # the model is not modified
    # the folded-in rows are ready for recommend_items
    served = S.MatrixFactorization(fam.n, m, d).to(dev)
    with torch.no_grad():
        served.U.copy_(fold.rows)
        served.V.copy_(model.V)
    seen = np.stack([np.concatenate([np.full(len(x), k) for k, x in enumerate(fam.pos)]), np.concatenate(fam.pos)], 1)
    top = S.recommend_items(served, k=5, exclude=to(dev, seen.astype(np.int64)))
    assert tuple(top.shape) == (fam.n, 5)
