"""GPU tests of the Newton-CG form of the exact user step (include/mfcd.h: mfcd_fold_in_users_cg; mfcd/foldin.py:
fold_in_users with method="cg" / "auto"; structure.fit_users, refit_users at d > 64) against the Cholesky numpy model of
tests/foldin_model.py run with max_iter = 1000.

Inputs (foldin_cg_model.user_case): m = 97 items, V ~ N(0, 1 / d) in fp32, labels from a hidden u0 ~ N(0, 9 I) per row.
With C = mfcd_fold_in_cg_chunk(d) and R = mfcd_fold_in_cg_resident(d) a call's rows have the lengths
{0, 1, 3, 50, 1000} | {C - 1, C, C + 1, 2 C + 3} | {R - 1, R, R + 1}: the empty row, less than a chunk, the chunk edges,
the last resident row and the first streamed one.  tests/test_fold_in_cg_cpu.py checks on the same inputs that the
reference certifies every row.

Tolerances: |U_out - u*|_inf <= 2^-22 |u*|_inf.  The kernel gives status 0 only when |g|_2 <= l2 2^-26 |u|_inf, and f is
l2-strongly convex, so the f64 iterate is within 2^-26 |u|_inf of u*; the one fp32 rounding adds 2^-24; the reference
stops after a Newton step below 2^-30 |u|_inf.  The objective: within 1e-9 max(1, f(u*)), as for the Cholesky form."""
import functools

import numpy as np
import pytest
import torch

import foldin_cg_model as CG
import foldin_model as FM

pytestmark = pytest.mark.gpu

U_TOL = 2.0 ** -22
F_TOL = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def capacity(d):
    from mfcd import _lib
    L = _lib.load()
    return L.mfcd_fold_in_cg_chunk(d), L.mfcd_fold_in_cg_resident(d)


@functools.lru_cache(maxsize=None)
def case(d, labels, start):
    """The inputs of one ragged call; the same for both l2."""
    return CG.user_case(d, labels, start, *capacity(d))


@functools.lru_cache(maxsize=None)
def reference(d, l2, labels, start):
    V, rec, off, U0 = case(d, labels, start)
    return FM.solve(V, rec, off, l2, U0, max_iter=CG.MODEL_MAX_ITER)


def to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, V, rec, off, l2, U0=None, method="cg", max_iter=CG.DEVICE_MAX_ITER, **kw):
    """→ [U, objective, iters, status, cg_iters] as numpy arrays."""
    from mfcd import foldin
    out = foldin.fold_in_users(to(dev, V), to(dev, rec), to(dev, off), l2, to(dev, U0), max_iter, method=method, **kw)
    return [t.cpu().numpy() for t in out] + [None if out.cg_iters is None else out.cg_iters.cpu().numpy()]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("start", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("labels", FM.LABELS)
@pytest.mark.parametrize("l2", CG.L2S)
@pytest.mark.parametrize("d", CG.DS)
def test_parity_with_the_cholesky_model(dev, d, l2, labels, start):
    V, rec, off, U0 = case(d, labels, start)
    ref = reference(d, l2, labels, start)
    U, f, iters, status, cg = run(dev, V, rec, off, l2, U0)
    assert U.dtype == np.float32 and f.dtype == np.float64 and iters.dtype == np.int32 and status.dtype == np.int32
    assert cg.dtype == np.int32 and cg.shape == iters.shape
    worst_u = worst_f = 0.0
    for r, row in enumerate(ref):
        assert row.status == FM.CONVERGED, (r, "the host model did not converge on this input")
        scale = np.abs(row.u).max()
        err = np.abs(U[r].astype(np.float64) - row.u).max()
        ferr = abs(f[r] - row.objective)
        if scale > 0:
            worst_u = max(worst_u, err / (U_TOL * scale))
        worst_f = max(worst_f, ferr / (F_TOL * max(1.0, row.objective)))
        print(f"row {r}: n {off[r + 1] - off[r]} solves {iters[r]} cg {cg[r]} (model {row.iters} Newton) status {status[r]} "
              f"|dU| {err:.3e} of |u*| {scale:.3e}, |df| {ferr:.3e} of f {row.objective:.6e}")
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
        assert (iters[r] >= 1 and cg[r] >= iters[r]) if n > 0 else (iters[r] == 0 and cg[r] == 0 and f[r] == 0.0), r


@pytest.mark.parametrize("d", [16, 64])
def test_the_two_solvers_agree_where_both_apply(dev, d):
    """Each is within 2^-22 of the same minimiser: outputs within 2^-21, objectives within 2e-9 max(1, f)."""
    from mfcd import _lib
    V, rec, off, U0 = FM.make_case(d, "hard", FM.row_lengths(_lib.load().mfcd_fold_in_chunk()), 1000 * d + 1, True)
    for l2 in CG.L2S:
        a = run(dev, V, rec, off, l2, U0, method="cg")
        b = run(dev, V, rec, off, l2, U0, method="cholesky")
        auto = run(dev, V, rec, off, l2, U0, method="auto", max_iter=50)
        assert b[4] is None and auto[4] is None and same(auto[:4], run(dev, V, rec, off, l2, U0, method="cholesky", max_iter=50)[:4])
        assert (a[3] == 0).all() and (b[3] == 0).all()
        for r, row in enumerate(FM.solve(V, rec, off, l2, U0)):
            assert row.status == 0
            assert np.abs(a[0][r].astype(np.float64) - b[0][r]).max() <= 2.0 ** -21 * np.abs(row.u).max(), (l2, r)
            assert abs(a[1][r] - b[1][r]) <= 2e-9 * max(1.0, b[1][r]), (l2, r)


def test_two_calls_are_bit_equal_and_rows_permute(dev):
    d = 128
    V, rec, off, U0 = case(d, "hard", True)
    first = run(dev, V, rec, off, 1e-3, U0)
    assert same(first, run(dev, V, rec, off, 1e-3, U0))
    rows = len(off) - 1
    perm = np.random.default_rng(3).permutation(rows)
    blocks = [rec[off[r]:off[r + 1]] for r in perm]
    poff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    moved = run(dev, V, np.concatenate(blocks), poff, 1e-3, U0[perm])
    assert same([a[perm] for a in first], moved)


def test_many_short_rows_in_one_call_or_two(dev):
    """700 rows of 1 to 12 comparisons, d = 128: more workgroups than CUs; the same rows in two calls of 350."""
    rng = np.random.default_rng(11)
    lengths = rng.integers(1, 13, 700).tolist()
    V, rec, off, U0 = FM.make_case(128, "hard", lengths, seed=77, start=True)
    whole = run(dev, V, rec, off, 1.0, U0)
    assert (whole[3] == 0).all()
    cut = int(off[350])
    a = run(dev, V, rec[:cut], off[:351], 1.0, U0[:350])
    b = run(dev, V, rec[cut:], off[350:] - cut, 1.0, U0[350:])
    assert same(whole, [np.concatenate((x, y)) for x, y in zip(a, b)])
    model = FM.solve(V, rec[:int(off[20])], off[:21], 1.0, U0[:20])                  # and they are the model's rows
    for r, row in enumerate(model):
        assert row.status == 0 and np.abs(whole[0][r].astype(np.float64) - row.u).max() <= U_TOL * np.abs(row.u).max(), r


def test_invalid_rows_get_status_two_and_leave_the_others_alone(dev):
    """One bad row per rule among good rows, resident and streamed (R = 63 at d = 128).  Every bad index is small (m or
    -1), so that no faulting read could occur even if a check were missing."""
    d, l2 = 128, 1e-3
    rules = ["i=m", "j=-1", "z=nan", "z=1.5", "table inf", "start nan", "streamed i=m"]
    lengths = [5, 20, 0, 64, 9, 70, 31, 40, 12, 100, 7, 90]
    good = [0, 2, 3, 5, 10]
    bad_rows = [1, 4, 6, 7, 8, 9, 11]
    V, rec, off, U0 = FM.make_case(d, "hard", lengths, seed=5, start=True)
    V, rec, U0 = V.copy(), rec.copy(), U0.copy()
    own = FM.M_ITEMS - 1                                                 # an item that only the "table inf" row gathers
    blk = rec[:, 1:3]
    for c in (0, 1):
        hit = blk[:, c] == own
        blk[hit, c] = np.where(blk[hit, 1 - c] == 0, 1, 0)
    assert not (blk == own).any() and (blk[:, 0] != blk[:, 1]).all()
    clean = run(dev, V, rec, off, l2, U0)
    assert (clean[3] == 0).all()
    for rule, r in zip(rules, bad_rows):
        t = int(off[r]) + 2
        if rule in ("i=m", "streamed i=m"):
            rec[t, 1] = FM.M_ITEMS
        elif rule == "j=-1":
            rec[t, 2] = -1
        elif rule == "z=nan":
            rec[t, 3] = np.float32(np.nan).view(np.int32)
        elif rule == "z=1.5":
            rec[t, 3] = np.float32(1.5).view(np.int32)
        elif rule == "table inf":
            rec[t, 1] = own
            V[own, 3] = np.inf
        elif rule == "start nan":
            U0[r, d - 1] = np.nan
    out = U, f, iters, status, cg = run(dev, V, rec, off, l2, U0)
    for rule, r in zip(rules, bad_rows):
        assert status[r] == 2 and np.isnan(U[r]).all() and np.isnan(f[r]) and iters[r] == 0 and cg[r] == 0, rule
    assert same([a[good] for a in out], [a[good] for a in clean])
    blocks = [rec[off[r]:off[r + 1]] for r in good]
    goff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    alone = run(dev, V, np.concatenate(blocks), goff, l2, U0[good])
    assert same([a[good] for a in out], alone) and (alone[3] == 0).all()
    # descending offsets: the row whose end lies below its start is refused, its neighbours are not read past their ends
    doff = off.copy()
    doff[4] = doff[3] - 1                                                # row 3 descends; row 4 now starts one record early
    desc = run(dev, V, rec, doff, l2, U0)
    assert desc[3][3] == 2 and np.isnan(desc[0][3]).all() and desc[2][3] == 0
    assert same([a[[0, 2, 5, 10]] for a in desc], [a[[0, 2, 5, 10]] for a in clean])
    # a workspace with room for fewer records than a row ends at: the row is refused, nothing is written past the end
    from mfcd import _lib
    L = _lib.load()
    rows, cut = len(lengths), 6                                          # rows 0 .. 5 fit, the others do not
    Vt, rt, ot, U0t = to(dev, V), to(dev, rec), to(dev, off), to(dev, U0)
    room = 256 + 24 * int(off[cut])
    ws = torch.zeros(room + 24 * 64, dtype=torch.uint8, device=dev)
    Uo = torch.empty((rows, d), dtype=torch.float32, device=dev)
    obj = torch.empty(rows, dtype=torch.float64, device=dev)
    info = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    _lib.check(L.mfcd_fold_in_users_cg(Vt.data_ptr(), FM.M_ITEMS, d, rt.data_ptr(), ot.data_ptr(), rows, l2, U0t.data_ptr(),
                                       CG.DEVICE_MAX_ITER, 2.0 ** -26, Uo.data_ptr(), obj.data_ptr(), info.data_ptr(), None,
                                       ws.data_ptr(), room, _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert info[:cut, 1].cpu().numpy().tolist() == status[:cut].tolist() and (info[cut:, 1] == 2).all()
    assert bits(Uo[:cut].cpu().numpy()) == bits(U[:cut]) and not ws[room:].any()


def test_iteration_cap_stops_with_the_last_accepted_iterate(dev):
    d, l2 = 128, 1e-3
    V, rec, off, U0 = FM.make_case(d, "hard", [50], seed=21, start=True)
    z = rec[:, 3].copy().view(np.float32)
    U, f, iters, status, cg = run(dev, V, rec, off, l2, U0, max_iter=1)
    start_f = FM.objective(U0[0].astype(np.float64), FM.deltas(V, rec[:, 1], rec[:, 2]), z.astype(np.float64), l2)
    assert status[0] == 1 and iters[0] == 1 and cg[0] >= 1 and np.isfinite(U[0]).all() and f[0] < start_f
    # f at the returned fp32 row, evaluated here: the iterate lowers f (an inexact CG step is not pinned further: two
    # correct CG solves to eta = 1e-3 may differ by that much of the step)
    here = FM.objective(U[0].astype(np.float64), FM.deltas(V, rec[:, 1], rec[:, 2]), z.astype(np.float64), l2)
    assert here < start_f
    assert CG.solve_user_row(V, rec[:, 1], rec[:, 2], z, l2, U0[0], max_iter=1).status == FM.STOPPED


def test_a_solution_fed_back_is_certified_within_two_solves(dev):
    d = 128
    V, rec, off, U0 = case(d, "hard", True)
    for l2 in CG.L2S:
        first = run(dev, V, rec, off, l2, U0)
        again = run(dev, V, rec, off, l2, first[0])
        print(f"l2 {l2}: solves from the fed-back solution {again[2].tolist()}, cg {again[4].tolist()}")
        assert (again[3] == 0).all() and int(again[2].max()) <= 2


def test_public_path(dev):
    """structure.fit_users and refit_users at d = 128: they raised before the CG form existed."""
    import structure as S
    from mfcd import engine
    torch.manual_seed(3)
    np.random.seed(3)
    n, m, d, wd = 53, FM.M_ITEMS, 128, 1e-5
    X = torch.randn(n, m).to(dev)
    train, _, _ = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    rows = engine.dataset_records(train.dataset)
    N = rows.shape[0]
    public = S.fit_users(model, train, 0.5)
    assert tuple(public.U.shape) == (n, d) and (public.status == 0).all() and torch.isfinite(public.U).all()
    assert public.cg_iters is not None and int(public.cg_iters.max()) >= 1
    order = np.argsort(rows[:, 0], kind="stable")
    rec = engine.pack_records(rows[order], n, m)
    off = np.concatenate(([0], np.cumsum(np.bincount(rows[:, 0].astype(np.int64), minlength=n)))).astype(np.int64)
    ref = FM.solve(model.V.data.cpu().numpy(), rec, off, 0.5, max_iter=CG.MODEL_MAX_ITER)
    for r, row in enumerate(ref):
        assert row.status == 0
        assert np.abs(public.U[r].cpu().numpy().astype(np.float64) - row.u).max() <= U_TOL * np.abs(row.u).max(), r
    before = model.U.data.clone()
    result, at_model = S.refit_users(model, train, wd)
    assert torch.equal(model.U.data, before) and (result.status == 0).all() and torch.isfinite(result.U).all()
    gap = (at_model - result.objective).cpu().numpy()
    slack = F_TOL * np.maximum(1.0, at_model.cpu().numpy())
    print(f"gap f(U_model) - f(U*): min {gap.min():.3e} max {gap.max():.3e}; l2 = {wd * N:.3f}")
    assert (gap >= -slack).all() and (gap > 0).any()
