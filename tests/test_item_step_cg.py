"""GPU tests of the Newton-CG form of the exact item step and of the alternating fit at d > 64 (include/mfcd.h:
mfcd_item_step_cg; mfcd/foldin.py: fold_in_items, fold_in_items_cg; mfcd/alternating.py; structure.fit_items, refit_items,
refit_alternating) against the Cholesky numpy model of tests/itemstep_model.py run with max_iter = 1000.

Inputs (foldin_cg_model.item_case, the recipe of itemstep_model.make_case): n = 53 users, m = 97 items, U ~ N(0, 2 / d)
in fp32, a hidden item table ~ N(0, 9 I); row r solves item 5 + 7 r over a number of comparisons from
{0, 1, 3, 50, 1000} | {C - 1, C, C + 1, 2 C + 3} | {R - 1, R, R + 1} (C = mfcd_fold_in_cg_chunk(d), R =
mfcd_fold_in_cg_resident(d)); the solved rows start at 0 or at N(0, 100 I).  tests/test_fold_in_cg_cpu.py checks on the
same inputs that the reference certifies every row.

Tolerances: |V_out - model|_inf <= 2^-22 max(|v*|_inf, |v_old|_inf): status 0 means |g|_2 <= l2 2^-26 |v|_inf, so by
strong convexity the f64 iterate is within 2^-26 |v*|_inf of v*; then one fp32 rounding (2^-24) of the f64 combination
v_old + theta (v* - v_old).  The two objectives: within 1e-9 max(1, f).

Descent: F(V_new) <= F(V) - (1/2) sum_k (f_k(v_k) - f_k(v*_k)) + slack for every simultaneous half step, slack =
itemstep_model.rounding_slack; the bound needs convexity only, so it also holds for rows that stopped early."""
import functools

import numpy as np
import pytest
import torch

import foldin_cg_model as CG
import itemstep_model as IM

pytestmark = pytest.mark.gpu

V_TOL = 2.0 ** -22
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
    """The inputs of one ragged call; the same for both l2 and both theta."""
    return CG.item_case(d, labels, start, *capacity(d))


@functools.lru_cache(maxsize=None)
def reference(d, l2, labels, start):
    """The model's rows at theta = 1 (v* does not depend on theta)."""
    U, V, rec, off, items = case(d, labels, start)
    return IM.solve(U, V, rec, off, l2, items, max_iter=CG.MODEL_MAX_ITER)


def to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, U, V, rec, off, l2, items=None, theta=1.0, max_iter=CG.DEVICE_MAX_ITER, **kw):
    """→ [V_out, objective_start, objective, iters, status, cg_iters] as numpy arrays, by the CG form."""
    from mfcd import foldin
    out = foldin.fold_in_items_cg(to(dev, U), to(dev, V), to(dev, rec), to(dev, off), l2, to(dev, items), theta, max_iter, **kw)
    return [t.cpu().numpy() for t in out] + [out.cg_iters.cpu().numpy()]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("start", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("labels", IM.LABELS)
@pytest.mark.parametrize("l2", CG.L2S)
@pytest.mark.parametrize("d", CG.DS)
def test_parity_with_the_cholesky_model(dev, d, l2, labels, start, theta):
    U, V, rec, off, items = case(d, labels, start)
    ref = reference(d, l2, labels, start)
    Vo, f0, f, iters, status, cg = run(dev, U, V, rec, off, l2, items, theta)
    assert Vo.dtype == np.float32 and f0.dtype == np.float64 and f.dtype == np.float64
    assert iters.dtype == np.int32 and status.dtype == np.int32 and cg.dtype == np.int32 and Vo.shape == (len(items), d)
    worst_v = worst_f = 0.0
    checks = []
    for r, row in enumerate(ref):
        assert row.status == IM.CONVERGED, (r, "the host model did not converge on this input")
        v_old = V[items[r]].astype(np.float64)
        want = v_old + theta * (row.v_star - v_old)
        scale = max(np.abs(row.v_star).max(), np.abs(v_old).max())
        err = np.abs(Vo[r].astype(np.float64) - want).max()
        ferr0, ferr = abs(f0[r] - row.f_start), abs(f[r] - row.objective)
        if scale > 0:
            worst_v = max(worst_v, err / (V_TOL * scale))
        worst_f = max(worst_f, ferr0 / (F_TOL * max(1.0, row.f_start)), ferr / (F_TOL * max(1.0, row.objective)))
        checks.append((err, scale, ferr0, ferr))
        print(f"row {r}: n {off[r + 1] - off[r]} solves {iters[r]} cg {cg[r]} (model {row.iters} Newton) status {status[r]} "
              f"|dV| {err:.3e} of {scale:.3e}, |df0| {ferr0:.3e} of {row.f_start:.6e}, |df| {ferr:.3e} of {row.objective:.6e}")
    print(f"worst share of the bounds: V {worst_v:.3f}, objectives {worst_f:.3f}")
    assert (status == 0).all(), status
    for r, row in enumerate(ref):
        err, scale, ferr0, ferr = checks[r]
        n = off[r + 1] - off[r]
        v_old = V[items[r]].astype(np.float64)
        if scale == 0.0:                                    # the zero row: no comparisons and the start 0
            assert bits(Vo[r]) == bits(np.zeros(d, dtype=np.float32)), r
        assert err <= V_TOL * scale, r
        assert ferr0 <= F_TOL * max(1.0, row.f_start) and ferr <= F_TOL * max(1.0, row.objective), r
        if n > 0:
            assert iters[r] >= 1 and cg[r] >= iters[r] and f[r] <= f0[r], r
        else:                                               # the empty row, exactly: (1 - theta) v_old, {(l2 / 2) |v_old|^2, 0}
            assert bits(Vo[r]) == bits((v_old + theta * (0.0 - v_old)).astype(np.float32)), r
            assert iters[r] == 0 and cg[r] == 0 and f[r] == 0.0, r


@pytest.mark.parametrize("d", [16, 64])
def test_the_two_solvers_agree_where_both_apply(dev, d):
    """Each is within 2^-22 of the same point: outputs within 2^-21 of the scale, objectives within 2e-9 max(1, f)."""
    from mfcd import _lib, foldin
    T = _lib.load().mfcd_fold_in_chunk()
    U, V, rec, off, items = IM.make_case(d, "hard", IM.FM.row_lengths(T), 5000 + 1000 * d + 1, True)    # test_item_step.case
    for l2 in CG.L2S:
        a = run(dev, U, V, rec, off, l2, items, 0.5)
        res = foldin.fold_in_items(to(dev, U), to(dev, V), to(dev, rec), to(dev, off), l2, to(dev, items), 0.5,
                                   CG.DEVICE_MAX_ITER)
        assert res.cg_iters is None                         # d <= 64: the Cholesky form
        b = [t.cpu().numpy() for t in res]
        assert (a[4] == 0).all() and (b[4] == 0).all()
        for r, row in enumerate(IM.solve(U, V, rec, off, l2, items, max_iter=CG.MODEL_MAX_ITER)):
            assert row.status == 0
            scale = max(np.abs(row.v_star).max(), np.abs(V[items[r]]).max())
            assert np.abs(a[0][r].astype(np.float64) - b[0][r]).max() <= 2.0 ** -21 * scale, (l2, r)
            for k in (1, 2):
                assert abs(a[k][r] - b[k][r]) <= 2e-9 * max(1.0, b[k][r]), (l2, r, k)


def test_two_calls_are_bit_equal_rows_permute_and_twins_agree(dev):
    d = 128
    U, V, rec, off, items = case(d, "hard", True)
    first = run(dev, U, V, rec, off, 1e-3, items, 0.5)
    assert same(first, run(dev, U, V, rec, off, 1e-3, items, 0.5))
    rows = len(off) - 1
    perm = np.random.default_rng(3).permutation(rows)
    blocks = [rec[off[r]:off[r + 1]] for r in perm]
    poff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    moved = run(dev, U, V, np.concatenate(blocks), poff, 1e-3, items[perm], 0.5)
    assert same([a[perm] for a in first], moved)
    # two rows that name one item, each with its own copy of the records, agree bit for bit: a resident and a streamed one
    for r in (rows - 1, 3):
        blk = rec[off[r]:off[r + 1]]
        twice = run(dev, U, V, np.concatenate([blk, blk]), np.array([0, len(blk), 2 * len(blk)], dtype=np.int64), 1e-3,
                    items[[r, r]], 0.5)
        assert same([a[[r, r]] for a in first], twice)


def short_rows_case(d):
    """700 rows of 1 to 12 comparisons, row r solving item r % 97 from a start of N(0, 1)."""
    rng = np.random.default_rng(11)
    n, m, rows = IM.N_USERS, IM.M_ITEMS, 700
    lengths = rng.integers(1, 13, rows)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    N = int(off[-1])
    items = (np.arange(rows) % m).astype(np.int32)
    own = np.repeat(items, lengths)
    partner = (own + 1 + rng.integers(0, m - 1, N)) % m
    first = rng.random(N) < 0.5
    rec = np.empty((N, 4), dtype=np.int32)
    rec[:, 0] = rng.integers(0, n, N)
    rec[:, 1], rec[:, 2] = np.where(first, own, partner), np.where(first, partner, own)
    rec[:, 3] = (rng.random(N) < 0.5).astype(np.float32).view(np.int32)
    U = (rng.standard_normal((n, d)) * np.sqrt(2.0 / d)).astype(np.float32)
    V = rng.standard_normal((m, d)).astype(np.float32)
    return U, V, rec, off, items


def test_many_short_rows_in_one_call_or_two(dev):
    U, V, rec, off, items = short_rows_case(128)
    whole = run(dev, U, V, rec, off, 1.0, items, 0.5)
    assert (whole[4] == 0).all()
    cut = int(off[350])
    a = run(dev, U, V, rec[:cut], off[:351], 1.0, items[:350], 0.5)
    b = run(dev, U, V, rec[cut:], off[350:] - cut, 1.0, items[350:], 0.5)
    assert same(whole, [np.concatenate((x, y)) for x, y in zip(a, b)])
    model = IM.solve(U, V, rec[:int(off[20])], off[:21], 1.0, items[:20], 0.5)      # and they are the model's rows
    for r, row in enumerate(model):
        scale = max(np.abs(row.v_star).max(), np.abs(V[items[r]]).max())
        assert row.status == 0 and np.abs(whole[0][r].astype(np.float64) - row.v_out).max() <= V_TOL * scale, r


def test_invalid_rows_get_status_two_and_leave_the_others_alone(dev):
    """One bad row per rule, among good rows that stay bit-equal to a call without the bad ones.  Every bad index is
    small (m, n, -1 or a foreign item), so that no faulting read could occur even if a check were missing."""
    d, l2 = 128, 1e-3
    n, m = IM.N_USERS, IM.M_ITEMS
    rules = ["u=n", "u=-1", "i=m", "j=-1", "row_item=m", "row_item=-1", "foreign", "z=1.5", "z=nan", "U nan", "V partner inf",
             "V own nan"]
    good = [0, 3, 7, 11, 15, 17, 18]
    rows = len(rules) + len(good)
    bad_rows = [r for r in range(rows) if r not in good]
    rng = np.random.default_rng(5)
    lengths = rng.integers(5, 80, rows)                                   # resident and streamed rows (R = 63)
    lengths[3], lengths[7], lengths[8] = 0, 70, 75                        # an empty good row, a streamed good and bad one
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    N = int(off[-1])
    items = (3 + 4 * np.arange(rows)).astype(np.int32)                    # 3 .. 75, all different
    # users 0 .. 49, partners among the items >= 80; user 52, item 96 and the bad rows' own items are touched by nobody else
    own = np.repeat(items, lengths)
    partner = 80 + rng.integers(0, 16, N)
    first = rng.random(N) < 0.5
    rec = np.empty((N, 4), dtype=np.int32)
    rec[:, 0] = rng.integers(0, 50, N)
    rec[:, 1], rec[:, 2] = np.where(first, own, partner), np.where(first, partner, own)
    rec[:, 3] = (rng.random(N) < 0.5).astype(np.float32).view(np.int32)
    U = (rng.standard_normal((n, d)) * np.sqrt(2.0 / d)).astype(np.float32)
    V = rng.standard_normal((m, d)).astype(np.float32)
    clean = run(dev, U, V, rec, off, l2, items, 0.5)
    assert (clean[4] == 0).all()
    rec, U, V, items = rec.copy(), U.copy(), V.copy(), items.copy()
    for rule, r in zip(rules, bad_rows):
        t = int(off[r]) + 2
        slot = 1 if rec[t, 1] == items[r] else 2                          # where the row's own item sits
        if rule == "u=n":
            rec[t, 0] = n
        elif rule == "u=-1":
            rec[t, 0] = -1
        elif rule == "i=m":
            rec[t, 3 - slot] = m
        elif rule == "j=-1":
            rec[t, 3 - slot] = -1
        elif rule == "row_item=m":
            items[r] = m
        elif rule == "row_item=-1":
            items[r] = -1
        elif rule == "foreign":
            rec[t, slot] = 79                                            # a valid item, but not the row's
        elif rule == "z=1.5":
            rec[t, 3] = np.float32(1.5).view(np.int32)
        elif rule == "z=nan":
            rec[t, 3] = np.float32(np.nan).view(np.int32)
        elif rule == "U nan":
            rec[t, 0] = 52
            U[52, 3] = np.nan
        elif rule == "V partner inf":
            rec[t, 3 - slot] = 96
            V[96, 0] = np.inf
        elif rule == "V own nan":
            V[items[r], d - 1] = np.nan
    Vo, f0, f, iters, status, cg = out = run(dev, U, V, rec, off, l2, items, 0.5)
    for rule, r in zip(rules, bad_rows):
        assert status[r] == 2 and np.isnan(Vo[r]).all() and np.isnan(f0[r]) and np.isnan(f[r]) and iters[r] == 0 and cg[r] == 0, rule
    assert same([a[good] for a in out], [a[good] for a in clean])
    blocks = [rec[off[r]:off[r + 1]] for r in good]
    goff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    alone = run(dev, U, V, np.concatenate(blocks), goff, l2, items[good], 0.5)
    assert same([a[good] for a in out], alone)
    # descending offsets: the row whose end lies below its start is refused
    doff = off.copy()
    doff[12] = doff[11] - 1                                               # row 11's end lies below its start; row 12 is a bad row
    desc = run(dev, U, V, rec, doff, l2, items, 0.5)
    assert desc[4][11] == 2 and np.isnan(desc[0][11]).all() and desc[3][11] == 0 and desc[5][11] == 0
    rest = [0, 3, 7, 15, 17, 18]
    assert same([a[rest] for a in desc], [a[rest] for a in clean])
    # a workspace with room for fewer records than a row ends at: the row is refused, nothing is written past the end
    from mfcd import _lib
    L = _lib.load()
    t = lambda a: to(dev, a)                                             # noqa: E731
    Ut, Vt, rt, ot, it = t(U), t(V), t(rec), t(off), t(items)
    cut = 9                                                              # rows 0 .. 8 fit, the others do not
    room = 256 + 32 * int(off[cut])
    ws = torch.zeros(room + 32 * 64, dtype=torch.uint8, device=dev)
    Vout = torch.empty((rows, d), dtype=torch.float32, device=dev)
    obj = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    info = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    _lib.check(L.mfcd_item_step_cg(Ut.data_ptr(), n, Vt.data_ptr(), m, d, rt.data_ptr(), ot.data_ptr(), it.data_ptr(), rows,
                                   l2, 0.5, CG.DEVICE_MAX_ITER, 2.0 ** -26, Vout.data_ptr(), obj.data_ptr(), info.data_ptr(),
                                   None, ws.data_ptr(), room, _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert info[:cut, 1].cpu().numpy().tolist() == status[:cut].tolist() and (info[cut:, 1] == 2).all()
    assert bits(Vout[:cut].cpu().numpy()) == bits(Vo[:cut]) and not ws[room:].any()


def test_iteration_cap_stops_with_the_last_accepted_iterate(dev):
    d, l2, r = 128, 1e-3, 3
    U, V, rec, off, items = case(d, "hard", True)
    blk = rec[off[r]:off[r + 1]]
    z = blk[:, 3].copy().view(np.float32)
    one = CG.solve_item_row(U, V, int(items[r]), blk[:, 0], blk[:, 1], blk[:, 2], z, l2, max_iter=1)
    assert one.status == IM.STOPPED and one.iters == 1
    Vo, f0, f, iters, status, cg = run(dev, U, V, blk, np.array([0, len(blk)], dtype=np.int64), l2, items[r:r + 1], 0.5, max_iter=1)
    assert status[0] == 1 and iters[0] == 1 and cg[0] >= 1 and f[0] < f0[0]
    # f_k at v* = v_old + 2 (V_out - v_old), evaluated here: the iterate lowers f_k (an inexact CG step is not pinned
    # further: two correct CG solves to eta = 1e-3 may differ by that much of the step)
    v_old = V[items[r]].astype(np.float64)
    D, c = IM.staged(U, V, int(items[r]), blk[:, 0].astype(np.int64), blk[:, 1].astype(np.int64), blk[:, 2].astype(np.int64))
    here = IM.objective(v_old + 2.0 * (Vo[0].astype(np.float64) - v_old), D, c, z.astype(np.float64), l2)
    assert abs(IM.objective(v_old, D, c, z.astype(np.float64), l2) - f0[0]) <= F_TOL * max(1.0, f0[0])
    assert here < f0[0]


def test_a_solution_fed_back_is_certified_within_two_solves(dev):
    d = 128
    U, V, rec, off, items = case(d, "hard", True)
    for l2 in CG.L2S:
        first = run(dev, U, V, rec, off, l2, items, 1.0)
        V2 = V.copy()
        V2[items] = first[0]
        again = run(dev, U, V2, rec, off, l2, items, 1.0)
        print(f"l2 {l2}: solves from the fed-back solution {again[3].tolist()}, cg {again[5].tolist()}")
        assert (again[4] == 0).all() and int(again[3].max()) <= 2


@pytest.mark.parametrize("d", [128, 65])
def test_every_sub_step_descends_by_the_jensen_bound(dev, d):
    """itemstep_model.descent_case at width d, l2 = 1: fit_alternating's chain of 3 sweeps of one user step and two
    item half steps, composed by hand so that every sub-step can be checked."""
    from mfcd import alternating, foldin
    l2 = 1.0
    U0, V0, u, i, j, z = IM.descent_case(d=d)
    data = (u, i, j, z)
    U, V = to(dev, U0), to(dev, V0)
    by_user = foldin.group_by_user(*(to(dev, a) for a in data), U0.shape[0])
    by_item = foldin.group_by_item(*(to(dev, a) for a in data), V0.shape[0])
    F = IM.total_objective(U0, V0, *data, l2)
    F_start, worst = F, 0.0
    for sweep in range(3):
        step = foldin.fold_in_users(V, by_user[0], by_user[1], l2, U)
        assert step.cg_iters is not None and (step.status <= 1).all()
        U = step.U
        Un, Vn = U.cpu().numpy(), V.cpu().numpy()
        Fn = IM.total_objective(Un, Vn, *data, l2)
        slack = IM.rounding_slack(IM.total_gradients(Un, Vn, *data, l2)[0], Un, Fn)
        print(f"sweep {sweep} users: F {F:.9f} -> {Fn:.9f}, slack {slack:.3e}, statuses {step.status.unique().tolist()}")
        assert Fn <= F + slack
        F = Fn
        for k in range(2):
            step = foldin.fold_in_items(U, V, by_item[0], by_item[1], l2, None, 0.5)
            assert step.cg_iters is not None and (step.status <= 1).all()
            gain = float((step.objective_start - step.objective).sum())
            V = step.V
            Vn = V.cpu().numpy()
            Fn = IM.total_objective(Un, Vn, *data, l2)
            slack = IM.rounding_slack(IM.total_gradients(Un, Vn, *data, l2)[1], Vn, Fn)
            share = (Fn - (F - 0.5 * gain)) / slack
            worst = max(worst, share)
            print(f"sweep {sweep} items {k}: F {F:.9f} -> {Fn:.9f}, bound {F - 0.5 * gain:.9f}, gain {gain:.6e}, slack "
                  f"{slack:.3e}, (F_new - bound) / slack {share:.3f}, statuses {step.status.unique().tolist()}")
            assert gain >= 0.0 and Fn <= F - 0.5 * gain + slack
            F = Fn
    print(f"F {F_start:.6f} -> {F:.6f}; largest share of the slack {worst:.3f}")
    assert F < F_start
    # and the driver is this chain
    fit = alternating.fit_alternating(to(dev, U0), to(dev, V0), *(to(dev, a) for a in data), l2, sweeps=3, item_steps=2)
    assert bits(fit.U.cpu().numpy()) == bits(U.cpu().numpy()) and bits(fit.V.cpu().numpy()) == bits(V.cpu().numpy())
    assert abs(float(fit.history[-1, -1]) - F) <= 1e-12 * F


def test_public_path(dev):
    """A MatrixFactorization(53, 97, 128) through structure.fit_items (one appended item), refit_items and
    refit_alternating(sweeps=2): every one of these calls raised before the CG form existed."""
    import structure as S
    from mfcd import engine
    torch.manual_seed(3)
    np.random.seed(3)
    n, m, d, wd = IM.N_USERS, IM.M_ITEMS, 128, 1e-5
    X = torch.randn(n, m).to(dev)
    train, _, _ = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    before = (model.U.data.clone(), model.V.data.clone())
    rows = engine.dataset_records(train.dataset)
    N = rows.shape[0]
    u, i, j = (rows[:, k].astype(np.int64) for k in range(3))
    z = rows[:, 3].astype(np.float32)
    Un, Vn = (t.cpu().numpy() for t in before)
    # fit_items for one new item: a zero row appended to V, comparisons that pit it against trained items
    rng = np.random.default_rng(8)
    T = 40
    nu, old = rng.integers(0, n, T), rng.integers(0, m, T)
    first = rng.random(T) < 0.5
    ni, nj = np.where(first, m, old), np.where(first, old, m)
    nz = (rng.random(T) < 0.5).astype(np.float32)
    V_ext = torch.cat((model.V.data, torch.zeros(1, d, device=dev)))
    res = S.fit_items((model.U.data, V_ext), tuple(torch.from_numpy(a) for a in (nu, ni, nj, nz)), 0.5, [m])
    assert tuple(res.V.shape) == (1, d) and (res.status == 0).all() and torch.isfinite(res.V).all() and res.cg_iters is not None
    row = IM.solve_item(Un, V_ext.cpu().numpy(), m, nu, ni, nj, nz, 0.5, max_iter=CG.MODEL_MAX_ITER)
    assert row.status == 0
    assert np.abs(res.V[0].cpu().numpy().astype(np.float64) - row.v_out).max() <= V_TOL * np.abs(row.v_star).max()
    assert abs(float(res.objective[0]) - row.objective) <= F_TOL * max(1.0, row.objective)
    # refit_items: the gaps of the model's own tables at l2 = wd N
    result, gap = S.refit_items(model, train, wd)
    assert (result.status == 0).all() and torch.isfinite(result.V).all()
    g, f0 = gap.cpu().numpy(), result.objective_start.cpu().numpy()
    print(f"item gaps f_k(V_model) - f_k(v*): min {g.min():.3e} max {g.max():.3e} sum {g.sum():.3e}")
    assert (g >= -F_TOL * np.maximum(1.0, f0)).all() and (g > 0).any()
    # refit_alternating: finite tables, F fell
    alt, F_model = S.refit_alternating(model, train, wd, sweeps=2, item_steps=2)
    hist = np.concatenate(([float(F_model)], alt.history.cpu().numpy().reshape(-1)))
    print("F at the model and after every sub-step:", hist.tolist())
    assert torch.isfinite(alt.U).all() and torch.isfinite(alt.V).all()
    assert (alt.user_status == 0).all() and (alt.item_status == 0).all()
    assert abs(hist[0] - IM.total_objective(Un, Vn, u, i, j, z, wd * N)) <= 1e-12 * hist[0]
    slack = 0.0                                         # of one rounding of both tables, at the model and at the result
    for Ua, Va, Fa in ((Un, Vn, hist[0]), (alt.U.cpu().numpy(), alt.V.cpu().numpy(), hist[-1])):
        GU, GV = IM.total_gradients(Ua, Va, u, i, j, z, wd * N)
        slack += IM.rounding_slack(GU, Ua, Fa) + IM.rounding_slack(GV, Va, Fa)
    assert (np.diff(hist) <= slack).all() and hist[-1] < hist[0]
    assert bits(model.U.data.cpu().numpy()) == bits(Un) and bits(model.V.data.cpu().numpy()) == bits(Vn)
