"""GPU tests of the item step and the alternating fit (include/mfcd.h: mfcd_item_step; mfcd/foldin.py: fold_in_items;
mfcd/alternating.py; structure.fit_items, refit_items, refit_alternating) against the f64 numpy model of
tests/itemstep_model.py.

Inputs (itemstep_model.make_case): n = 53 users, m = 97 items, U ~ N(0, 2 / d) in fp32, a hidden item table ~ N(0, 9 I);
nine rows solve the items 5 + 7 r over 0, 1, 3, 50, 1000, T - 1, T, T + 1 and 2 T + 3 comparisons (T =
mfcd_fold_in_chunk()), the solved item in the i or the j slot by a fair coin, the partner among the 88 other items; the
solved rows start at 0 or at N(0, 100 I).

Tolerances: |V_out - model|_inf <= 2^-22 max(|v*|_inf, |v_old|_inf) — one fp32 rounding (2^-24 relative) of the f64
combination v_old + theta (v* - v_old), whose size either of the two can set, with a factor 4 of margin; both solvers
stop only after a Newton step below 2^-30 |v|_inf.  The two objectives: within 1e-9 max(1, f), as for the user step.

Descent: F(V_new) <= F(V) - (1/2) sum_k (f_k(v_k) - f_k(v*_k)) + slack for every simultaneous half step, F from an f64
numpy evaluation; slack = 2 x 2^-24 sum |dF/dV| |V| at V_new + 1e-12 |F|: the first-order effect of the one output
rounding with a factor 2, and the f64 evaluation of F."""
import functools

import numpy as np
import pytest
import torch

import itemstep_model as IM

pytestmark = pytest.mark.gpu

DS = (1, 2, 7, 16, 64)
L2S = (1e-3, 1.0)
V_TOL = 2.0 ** -22
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
    """The inputs of one ragged call; the same for both l2 and both theta."""
    seed = 5000 + 1000 * d + 10 * IM.LABELS.index(labels) + int(start)
    return IM.make_case(d, labels, IM.FM.row_lengths(chunk()), seed, start)


@functools.lru_cache(maxsize=None)
def reference(d, l2, labels, start):
    """The model's rows at theta = 1 (v* does not depend on theta; the tests form v_old + theta (v* - v_old) from it)."""
    U, V, rec, off, items = case(d, labels, start)
    return IM.solve(U, V, rec, off, l2, items)


def to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, U, V, rec, off, l2, items=None, theta=1.0, **kw):
    from mfcd import foldin
    out = foldin.fold_in_items(to(dev, U), to(dev, V), to(dev, rec), to(dev, off), l2, to(dev, items), theta, **kw)
    return [t.cpu().numpy() for t in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("start", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("labels", IM.LABELS)
@pytest.mark.parametrize("l2", L2S)
@pytest.mark.parametrize("d", DS)
def test_parity_with_the_host_model(dev, d, l2, labels, start, theta):
    U, V, rec, off, items = case(d, labels, start)
    ref = reference(d, l2, labels, start)
    Vo, f0, f, iters, status = run(dev, U, V, rec, off, l2, items, theta)
    assert Vo.dtype == np.float32 and f0.dtype == np.float64 and f.dtype == np.float64
    assert iters.dtype == np.int32 and status.dtype == np.int32 and Vo.shape == (9, d)
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
        print(f"row {r}: n {off[r + 1] - off[r]} iters {iters[r]} (model {row.iters}, {row.halvings} halvings) status "
              f"{status[r]} |dV| {err:.3e} of {scale:.3e}, |df0| {ferr0:.3e} of {row.f_start:.6e}, |df| {ferr:.3e} of "
              f"{row.objective:.6e}")
    print(f"worst share of the bounds: V {worst_v:.3f}, objectives {worst_f:.3f}")
    assert (status == 0).all(), status
    for r, row in enumerate(ref):
        err, scale, ferr0, ferr = checks[r]
        n = off[r + 1] - off[r]
        assert err <= V_TOL * scale, r
        assert ferr0 <= F_TOL * max(1.0, row.f_start) and ferr <= F_TOL * max(1.0, row.objective), r
        if n > 0:
            assert iters[r] >= 1 and f[r] <= f0[r], r
        else:                                               # the empty row, exactly: (1 - theta) v_old, {(l2 / 2) |v_old|^2, 0}
            v_old = V[items[r]].astype(np.float64)
            assert bits(Vo[r]) == bits((v_old + theta * (0.0 - v_old)).astype(np.float32)), r   # (1 - theta) v_old
            vv = 0.0
            for x in v_old:
                vv = vv + x * x                             # squares of fp32 values are exact in f64; the sum is ascending
            assert iters[r] == 0 and f[r] == 0.0 and abs(f0[r] - 0.5 * l2 * vv) <= 4 * np.finfo(np.float64).eps * f0[r], r


@pytest.mark.parametrize("d", [2, 64])
def test_two_calls_are_bit_equal_and_rows_permute(dev, d):
    U, V, rec, off, items = case(d, "hard", True)
    first = run(dev, U, V, rec, off, 1e-3, items, 0.5)
    assert same(first, run(dev, U, V, rec, off, 1e-3, items, 0.5))
    rows = len(off) - 1
    perm = np.random.default_rng(3).permutation(rows)
    blocks = [rec[off[r]:off[r + 1]] for r in perm]
    poff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    moved = run(dev, U, V, np.concatenate(blocks), poff, 1e-3, items[perm], 0.5)
    assert same([a[perm] for a in first], moved)
    # two rows that name one item, each with its own copy of the records, agree bit for bit
    r = 4
    twice = run(dev, U, V, np.concatenate([rec[off[r]:off[r + 1]]] * 2), np.array([0, 1000, 2000], dtype=np.int64), 1e-3,
                items[[r, r]], 0.5)
    assert same([a[[r, r]] for a in first], twice)


def short_rows_case():
    """700 rows of 1 to 12 comparisons at d = 16, row r solving item r % 97 from a start of N(0, 1)."""
    rng = np.random.default_rng(11)
    n, m, d, rows = IM.N_USERS, IM.M_ITEMS, 16, 700
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
    U, V, rec, off, items = short_rows_case()
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
    d, l2 = 7, 1e-3
    n, m = IM.N_USERS, IM.M_ITEMS
    rules = ["u=n", "u=-1", "i=m", "j=-1", "row_item=m", "row_item=-1", "foreign", "z=1.5", "z=nan", "U nan", "V partner inf",
             "V own nan"]
    good = [0, 3, 7, 11, 15, 17, 18]
    rows = len(rules) + len(good)
    bad_rows = [r for r in range(rows) if r not in good]
    rng = np.random.default_rng(5)
    lengths = rng.integers(5, 80, rows)
    lengths[3] = 0                                                        # an empty good row
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
    Vo, f0, f, iters, status = out = run(dev, U, V, rec, off, l2, items, 0.5)
    for rule, r in zip(rules, bad_rows):
        assert status[r] == 2 and np.isnan(Vo[r]).all() and np.isnan(f0[r]) and np.isnan(f[r]) and iters[r] == 0, rule
    model = IM.solve(U, V, rec, off, l2, items, 0.5)
    assert [row.status for row in model] == [0 if r in good else 2 for r in range(rows)]
    assert same([a[good] for a in out], [a[good] for a in clean])
    # and bit-equal to a call that holds the good rows only
    blocks = [rec[off[r]:off[r + 1]] for r in good]
    goff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int64)
    alone = run(dev, U, V, np.concatenate(blocks), goff, l2, items[good], 0.5)
    assert same([a[good] for a in out], alone)
    # a workspace with room for fewer records than a row ends at: the row is refused, nothing is written past the end
    from mfcd import _lib
    L = _lib.load()
    t = lambda a: to(dev, a)                                             # noqa: E731
    Ut, Vt, rt, ot, it = t(U), t(V), t(rec), t(off), t(items)
    cut = 9                                                              # rows 0 .. 8 fit, the others do not
    ws = torch.zeros(256 + 8 * int(off[cut]) + 8 * 64, dtype=torch.uint8, device=dev)
    Vout = torch.empty((rows, d), dtype=torch.float32, device=dev)
    obj = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    info = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    _lib.check(L.mfcd_item_step(Ut.data_ptr(), n, Vt.data_ptr(), m, d, rt.data_ptr(), ot.data_ptr(), it.data_ptr(), rows,
                                l2, 0.5, 50, 2.0 ** -30, Vout.data_ptr(), obj.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                256 + 8 * int(off[cut]), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert info[:cut, 1].cpu().numpy().tolist() == status[:cut].tolist() and (info[cut:, 1] == 2).all()
    assert bits(Vout[:cut].cpu().numpy()) == bits(Vo[:cut]) and not ws[256 + 8 * int(off[cut]):].any()


def test_iteration_cap_stops_with_the_last_accepted_iterate(dev):
    U, V, rec, off, items = case(7, "hard", True)
    r, l2 = 3, 1e-3
    blk = rec[off[r]:off[r + 1]]
    z = blk[:, 3].copy().view(np.float32)
    assert reference(7, l2, "hard", True)[r].iters > 1
    one = IM.solve_item(U, V, int(items[r]), blk[:, 0], blk[:, 1], blk[:, 2], z, l2, 0.5, max_iter=1)
    Vo, f0, f, iters, status = run(dev, U, V, blk, np.array([0, len(blk)], dtype=np.int64), l2, items[r:r + 1], 0.5, max_iter=1)
    assert status[0] == 1 and iters[0] == 1 and f[0] <= f0[0]
    scale = max(np.abs(one.v_star).max(), np.abs(V[items[r]]).max())
    assert np.abs(Vo[0].astype(np.float64) - one.v_out).max() <= V_TOL * scale


def test_every_sub_step_descends_by_the_jensen_bound(dev):
    """n = 40, m = 30, d = 3, N = 600, start 0.1 N(0, I), l2 = 0.5, three sweeps of one user step and two item steps."""
    from mfcd import foldin
    l2 = 0.5
    U0, V0, u, i, j, z = IM.descent_case()
    data = (u, i, j, z)
    U, V = to(dev, U0), to(dev, V0)
    by_user = foldin.group_by_user(*(to(dev, a) for a in data), U0.shape[0])
    by_item = foldin.group_by_item(*(to(dev, a) for a in data), V0.shape[0])
    F = IM.total_objective(U0, V0, *data, l2)
    F_start, worst = F, 0.0
    for sweep in range(3):
        step = foldin.fold_in_users(V, by_user[0], by_user[1], l2, U)
        assert (step.status == 0).all()
        U = step.U
        Un, Vn = U.cpu().numpy(), V.cpu().numpy()
        Fn = IM.total_objective(Un, Vn, *data, l2)
        slack = IM.rounding_slack(IM.total_gradients(Un, Vn, *data, l2)[0], Un, Fn)
        print(f"sweep {sweep} users: F {F:.9f} -> {Fn:.9f}, slack {slack:.3e}")
        assert Fn <= F + slack
        F = Fn
        for k in range(2):
            step = foldin.fold_in_items(U, V, by_item[0], by_item[1], l2, None, 0.5)
            assert (step.status == 0).all()
            gain = float((step.objective_start - step.objective).sum())
            V = step.V
            Vn = V.cpu().numpy()
            Fn = IM.total_objective(Un, Vn, *data, l2)
            slack = IM.rounding_slack(IM.total_gradients(Un, Vn, *data, l2)[1], Vn, Fn)
            share = (Fn - (F - 0.5 * gain)) / slack
            worst = max(worst, share)
            print(f"sweep {sweep} items {k}: F {F:.9f} -> {Fn:.9f}, bound {F - 0.5 * gain:.9f}, gain {gain:.6e}, slack "
                  f"{slack:.3e}, (F_new - bound) / slack {share:.3f}")
            assert gain >= 0.0 and Fn <= F - 0.5 * gain + slack
            F = Fn
    print(f"F {F_start:.6f} -> {F:.6f}; largest share of the slack {worst:.3f}")
    assert F < F_start


def test_driver_is_the_hand_composed_chain(dev):
    from mfcd import alternating, foldin
    l2 = 0.5
    U0, V0, u, i, j, z = IM.descent_case()
    U, V = to(dev, U0), to(dev, V0)
    data = tuple(to(dev, a) for a in (u, i, j, z))
    before = (U.clone(), V.clone())
    one = alternating.fit_alternating(U, V, *data, l2, sweeps=1, item_steps=2)
    by_user = foldin.group_by_user(*data, U0.shape[0])
    by_item = foldin.group_by_item(*data, V0.shape[0])
    a = foldin.fold_in_users(V, by_user[0], by_user[1], l2, U)
    b = foldin.fold_in_items(a.U, V, by_item[0], by_item[1], l2, None, 0.5)
    c = foldin.fold_in_items(a.U, b.V, by_item[0], by_item[1], l2, None, 0.5)
    assert torch.equal(one.U, a.U) and torch.equal(one.V, c.V) and bits(one.V.cpu().numpy()) == bits(c.V.cpu().numpy())
    assert torch.equal(one.user_status, a.status) and torch.equal(one.item_status, c.status)
    assert tuple(one.history.shape) == (1, 3) and one.history.dtype == torch.float64
    assert torch.equal(U, before[0]) and torch.equal(V, before[1])                  # the inputs are not modified
    three = alternating.fit_alternating(U, V, *data, l2, sweeps=3, item_steps=2)
    again = alternating.fit_alternating(U, V, *data, l2, sweeps=3, item_steps=2)
    for x, y in zip(three, again):
        assert bits(x.cpu().numpy()) == bits(y.cpu().numpy())
    assert bits(three.objective_start.cpu().numpy()) == bits(again.objective_start.cpu().numpy())
    chain, hist = one, [one.history]
    for _ in range(2):
        chain = alternating.fit_alternating(chain.U, chain.V, *data, l2, sweeps=1, item_steps=2)
        hist.append(chain.history)
    assert bits(three.U.cpu().numpy()) == bits(chain.U.cpu().numpy()) and bits(three.V.cpu().numpy()) == bits(chain.V.cpu().numpy())
    assert bits(three.history.cpu().numpy()) == bits(torch.cat(hist).cpu().numpy())
    assert tuple(three.history.shape) == (3, 3)
    last = foldin.total_objective(three.U, three.V, *data, l2)
    assert bits(three.history[-1, -1].cpu().numpy()) == bits(last.cpu().numpy())
    assert bits(three.objective_start.cpu().numpy()) == bits(foldin.total_objective(U, V, *data, l2).cpu().numpy())
    flat = torch.cat((three.objective_start.reshape(1), three.history.reshape(-1))).cpu().numpy()
    assert abs(flat[0] - IM.total_objective(U0, V0, u, i, j, z, l2)) <= 1e-12 * flat[0]
    assert (np.diff(flat) < 0).all(), flat                                            # far from the optimum: strict descent


def test_public_path(dev):
    import structure as S
    from mfcd import engine
    torch.manual_seed(3)
    np.random.seed(3)
    n, m, d = 40, IM.M_ITEMS, 2
    X = torch.randn(n, m).to(dev)
    train, _, _ = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    before = (model.U.data.clone(), model.V.data.clone())
    rows = engine.dataset_records(train.dataset)
    N = rows.shape[0]
    u, i, j = (rows[:, k].astype(np.int64) for k in range(3))
    z = rows[:, 3].astype(np.float32)
    Un, Vn = (t.cpu().numpy() for t in before)
    # fit_items for 3 new items: zero rows appended to V, comparisons that pit them against trained items
    rng = np.random.default_rng(8)
    new = np.array([m + 1, m, m + 2])
    T = 150
    nu, old = rng.integers(0, n, T), rng.integers(0, m, T)
    mine = new[rng.integers(0, 3, T)]
    first = rng.random(T) < 0.5
    ni, nj = np.where(first, mine, old), np.where(first, old, mine)
    nz = (rng.random(T) < 0.5).astype(np.float32)
    V_ext = torch.cat((model.V.data, torch.zeros(3, d, device=dev)))
    data = tuple(torch.from_numpy(a) for a in (nu, ni, nj, nz))
    res = S.fit_items((model.U.data, V_ext), data, 0.5, new.tolist())
    assert tuple(res.V.shape) == (3, d) and (res.status == 0).all()
    Vx = V_ext.cpu().numpy()
    for r, k in enumerate(new):
        at = np.flatnonzero((ni == k) | (nj == k))
        row = IM.solve_item(Un, Vx, int(k), nu[at], ni[at], nj[at], nz[at], 0.5)
        assert row.status == 0
        assert np.abs(res.V[r].cpu().numpy().astype(np.float64) - row.v_out).max() <= V_TOL * np.abs(row.v_star).max()
        assert abs(float(res.objective[r]) - row.objective) <= F_TOL * max(1.0, row.objective)
    whole = S.fit_items(model, train, 0.5)
    named = S.fit_items(model, train, 0.5, [9, 2, 40])
    assert tuple(whole.V.shape) == (m, d) and same([t.cpu().numpy() for t in named], [t[[9, 2, 40]].cpu().numpy() for t in whole])
    # refit_items: the gaps of the model's own tables at l2 = wd N
    wd = 1e-5
    result, gap = S.refit_items(model, train, wd)
    assert (result.status == 0).all()
    g, f0 = gap.cpu().numpy(), result.objective_start.cpu().numpy()
    print(f"item gaps f_k(V_model) - f_k(v*): min {g.min():.3e} max {g.max():.3e} sum {g.sum():.3e}")
    assert (g >= -1e-9 * np.maximum(1.0, f0)).all() and (g > 0).any()
    ref = IM.solve(Un, Vn, *IM.group_by_item(u, i, j, z, m), wd * N)
    for r, row in enumerate(ref):
        assert abs(float(result.objective[r]) - row.objective) <= F_TOL * max(1.0, row.objective)
    ures, at_model = S.refit_users(model, train, wd)
    user_gap_before = (at_model - ures.objective).cpu().numpy()
    # refit_alternating: the returned tables are closer to block optimality on both sides, and F fell
    alt, F_model = S.refit_alternating(model, train, wd, sweeps=4, item_steps=2)
    hist = np.concatenate(([float(F_model)], alt.history.cpu().numpy().reshape(-1)))
    print("F at the model and after every sub-step:", hist.tolist())
    assert abs(hist[0] - IM.total_objective(Un, Vn, u, i, j, z, wd * N)) <= 1e-12 * hist[0]
    assert hist[-1] < hist[0]                                   # (descent of every sub-step: the test above)
    fitted = S.MatrixFactorization(n, m, d).to(dev)
    with torch.no_grad():
        fitted.U.copy_(alt.U)
        fitted.V.copy_(alt.V)
    _, gap_after = S.refit_items(fitted, train, wd)
    ures, at_fitted = S.refit_users(fitted, train, wd)
    user_gap_after = (at_fitted - ures.objective).cpu().numpy()
    ga = gap_after.cpu().numpy()
    print(f"gaps before -> after: items sum {g.sum():.3e} -> {ga.sum():.3e}, max {g.max():.3e} -> {ga.max():.3e}; users sum "
          f"{user_gap_before.sum():.3e} -> {user_gap_after.sum():.3e}, max {user_gap_before.max():.3e} -> {user_gap_after.max():.3e}")
    assert ga.sum() < g.sum() and ga.max() < g.max()
    assert user_gap_after.sum() < user_gap_before.sum() and user_gap_after.max() < user_gap_before.max()
    assert bits(model.U.data.cpu().numpy()) == bits(Un) and bits(model.V.data.cpu().numpy()) == bits(Vn)
