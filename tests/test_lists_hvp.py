"""GPU tests of the second-order list machinery (include/mfcd.h: mfcd_list_pl_hvp; mfcd.lists.pl_hvp_rows, pl_hvp;
mfcd/lists_exact.py; structure.rankings_hvp, fit_users_rankings, refit_users_rankings, refit_items_rankings,
train_model_rankings_exact): the kernel against the numpy model (tests/list_pl_hvp_model.py) on the same fp32 inputs over
every length and depth at which it takes another path, the scores that break the naive form and four kinds of y; lists of
two against the ragged pair Hessian and depth-1 rows against torch's softmax; bit-equality, independence of a row's place,
of `deg` and of y; non-finite and invalid rows; the table-level product; the exact user step and fold-in against the
model's minimisers, the item step, the alternating fit and the structure entries.

Bounds.  q: |q - q_model| <= 2^-24 |q_model| + 8 (L + 128) 2^-53 scale_l, deg: the same with deg_model and psum_l — one
fp32 rounding (which below 2^-126 is not relative: half of the smallest subnormal, 2^-150, is granted beside it), and
the f64 accumulation along the row (about L roundings of a few operations each on the model's sequential path, the same
on the kernel's log-depth path plus at most 64 carry joins; the factor 8 is the operations per step).  The steps follow test_ratings_hvp.py: a certified row lies within gtol |u*|_inf + noise / l2 of the minimiser
(strong convexity, modulus l2; noise: the gradient's fp32 bound, list_pl_hvp_model.Problem.user_noise), objectives are
held to RTOL = 2e-5, ATOL = 2e-6."""
import functools

import numpy as np
import pytest
import torch

import list_pl_hvp_model as HM
import list_pl_model as LM
from test_lists import ATOL, KINDS, RTOL, _offsets, _scores, _tile

pytestmark = pytest.mark.gpu

YKINDS = ("normal", "ones", "onehot", "big")
U24, U53 = 2.0 ** -24, 2.0 ** -53
TINY = 2.0 ** -150        # the fp32 rounding of a value below 2^-126: half of the smallest subnormal instead of 2^-24 |x|
L2, GTOL = HM.STEP_L2, HM.STEP_GTOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _y(kind, L, rng):
    if kind == "ones":
        return np.ones(L, dtype=np.float32)
    if kind == "onehot":
        y = np.zeros(L, dtype=np.float32)
        if L:
            y[(2 * L) // 3] = 1.0
        return y
    if kind == "big":
        return (np.float32(3e30) * (1 - 2 * (np.arange(L) % 2))).astype(np.float32)
    return rng.standard_normal(L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case():
    """Every length with every depth that applies and every kind of scores; the kinds of y take turns over the depths and
    the kinds of scores, so that every kind of scores meets every kind of y at every length with four depths or more.
    One row of 70 001.  → (rows [(scores, y, depth, kind, ykind)], a, y, off, depth, model (q, deg, scale, psum))."""
    T = _tile()
    rng = np.random.default_rng(0)
    rows = []
    for L in (0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 64 * T + 1):
        for di, depth in enumerate(sorted({d for d in (0, 1, 2, L - 1, L, T, T + 1) if 0 <= d <= L})):
            for ki, kind in enumerate(KINDS):
                yk = YKINDS[(ki + di) % 4]
                rows.append((_scores(kind, L, rng), _y(yk, L, rng), depth, kind, yk))
    rows.append((_scores("normal", 70001, rng), _y("normal", 70001, rng), 70001, "normal", "normal"))
    a, y = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    off, _ = _offsets([r[0].size for r in rows], T)
    depth = np.array([r[2] for r in rows], dtype=np.int32)
    q, deg, scale, psum = HM.rows(a, y, off, depth)
    for r, (s, yy, d, kind, _) in enumerate(rows):
        if kind == "huge" and LM.stages_of(s.size, d) > 0:
            # the head holds 3e38: the model folds the payload's logarithm into a number of that size and loses it, in
            # this one entry.  The closed form: stage 0 picks entry 0 with probability 1 exactly, so ybar_0 = y_0 and the
            # entry's q is 0, its scale p (|y_0| + |y_0|)
            q[off[r]], scale[off[r]] = 0.0, 2.0 * abs(float(yy[0]))
    return rows, a, y, off, depth, (q, deg, scale, psum)


def run(dev, a, y, off, depth, deg=True, tile_off=None, n_tiles=None, entries=None, fill=None):
    """One call of the entry on host arrays → (q, deg or None, status) as numpy."""
    from mfcd import _lib
    L = _lib.load()
    off = np.asarray(off, dtype=np.int64)
    rows = off.size - 1
    if tile_off is None:
        tile_off = _offsets(np.diff(off), _tile())[1]
    n_tiles = int(tile_off[-1]) if n_tiles is None else n_tiles
    entries = int(np.asarray(a).size) if entries is None else entries
    a_d, y_d = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (a, y))
    off_d, tile_d = torch.from_numpy(off).to(dev), torch.from_numpy(np.asarray(tile_off, dtype=np.int64)).to(dev)
    depth_d = None if depth is None else torch.from_numpy(np.asarray(depth, dtype=np.int32)).to(dev)
    outs = []
    for want in (True, deg):
        t = None
        if want:
            t = torch.empty(max(entries, 1), dtype=torch.float32, device=dev)
            t.fill_(float("nan") if fill is None else fill)
        outs.append(t)
    status = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_list_pl_hvp_workspace_bytes(rows, n_tiles), dev)
    _lib.check(L.mfcd_list_pl_hvp(_lib.ptr(a_d), _lib.ptr(y_d), entries, _lib.ptr(off_d), _lib.ptr(depth_d), rows,
                                  _lib.ptr(tile_d), n_tiles, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(status),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    host = lambda t: None if t is None else t.cpu().numpy()[:entries]    # noqa: E731
    return host(outs[0]), host(outs[1]), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case_outputs():
    rows, a, y, off, depth, _ = case()
    return run(torch.device("cuda:0"), a, y, off, depth)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
def test_q_and_deg_match_the_model(dev):
    rows, a, y, off, depth, (mq, mdeg, scale, psum) = case()
    q, deg, status = case_outputs()
    assert (status == 0).all()
    worst = {}
    for r, (s, yy, d, kind, yk) in enumerate(rows):
        L, sl = s.size, slice(off[r], off[r + 1])
        if LM.stages_of(L, d) == 0:
            assert q[sl].tobytes() == np.zeros(L, np.float32).tobytes() == deg[sl].tobytes(), (kind, L, d)   # +0, not -0
            continue
        second = 8 * (L + 128) * U53
        eq, edeg = np.abs(q[sl] - mq[sl]), np.abs(deg[sl] - mdeg[sl])
        bq, bdeg = U24 * np.abs(mq[sl]) + TINY + second * scale[sl], U24 * mdeg[sl] + TINY + second * psum[sl]
        # the largest error in units of each term, printed before anything is asserted
        for name, err, first, size in (("q", eq, U24 * np.abs(mq[sl]), scale[sl]), ("deg", edeg, U24 * mdeg[sl], psum[sl])):
            big = first >= second * size
            w = worst.setdefault((name, kind), [0.0, 0.0])
            normal = big & (first >= U24 * 2.0 ** -126)    # fp32 normals: below them the rounding is not relative
            w[0] = max(w[0], float((err[normal] / first[normal]).max(initial=0.0)))
            live = (size > 0) & (size >= 1e-30 * size.max())    # what the first term and the subnormal floor do not cover
            left = np.maximum(err - first - TINY, 0.0)
            w[1] = max(w[1], float((left[live] / (U53 * size[live])).max(initial=0.0) / (L + 128)))
        assert (eq <= bq).all(), ("q", kind, yk, L, d, float((eq - bq).max()))
        assert (edeg <= bdeg).all() and (deg[sl] >= 0).all(), ("deg", kind, yk, L, d, float((edeg - bdeg).max()))
        if yk == "ones":
            assert (np.abs(q[sl]) <= second * scale[sl]).all(), (kind, L, d)                 # H 1 = 0
    print("largest error by kind, (in units of 2^-24 |model| where that term leads; what the first term leaves, in units "
          "of (L + 128) 2^-53 size, bound 8):", {f"{n} {k}": (round(v[0], 3), round(v[1], 3)) for (n, k), v in worst.items()})


def test_lists_of_two_are_the_ragged_pair_hessian(dev):
    """The Hessian of a pair's risk depends on neither the scale nor the values: sigmoid'(a_0 - a_1) [[1, -1], [-1, 1]]."""
    from mfcd import lists, ratings
    n = 300
    rng = np.random.default_rng(5)
    users, items = np.repeat(np.arange(n), 2), np.tile([0, 1], n)
    a, y = to(dev, (3.0 * rng.standard_normal(2 * n)).astype(np.float32)), to(dev, rng.standard_normal(2 * n).astype(np.float32))
    data = ratings.RatingsData(users, items, rng.integers(1, 6, 2 * n).astype(np.float64), n, 2).to(dev)
    want_q, want_deg, _ = ratings.pair_ragged_hvp(a, y, data, False, True)
    for depth in (1, 2):
        R = lists.RankedLists(users, items, items, n, 2, depth).to(dev)
        q, deg, status = lists.pl_hvp_rows(a, y, R, True)
        assert (status == 0).all() and R.stages == n
        np.testing.assert_allclose(q.cpu().numpy(), want_q.cpu().numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(deg.cpu().numpy(), want_deg.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_depth_one_rows_are_the_softmax(dev):
    T = _tile()
    rng = np.random.default_rng(6)
    lens = [2, 5, 64, 65, T, T + 1, 3 * T + 5, 5000]
    off, _ = _offsets(lens, T)
    a = (2.0 * rng.standard_normal(off[-1])).astype(np.float32)
    y = rng.standard_normal(off[-1]).astype(np.float32)
    q, deg, status = run(dev, a, y, off, [1] * len(lens))
    assert (status == 0).all()
    for r, L in enumerate(lens):
        sl = slice(off[r], off[r + 1])
        at, yt = torch.from_numpy(a[sl]).double(), torch.from_numpy(y[sl]).double()
        p = torch.softmax(at, 0)
        want = (p * (yt - (p * yt).sum())).numpy()
        size = (p * (yt.abs() + (p * yt.abs()).sum())).numpy()
        second = 8 * (L + 128) * U53
        assert (np.abs(q[sl] - want) <= U24 * np.abs(want) + TINY + second * size).all(), L
        assert (np.abs(deg[sl] - (p * (1 - p)).numpy()) <= U24 * (p * (1 - p)).numpy() + TINY + second * p.numpy()).all(), L


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism and independence
# ---------------------------------------------------------------------------------------------------------------------
def test_calls_are_bit_equal_and_q_deg_and_rows_are_independent(dev):
    rows, a, y, off, depth, _ = case()
    q, deg, _ = case_outputs()
    again = run(dev, a, y, off, depth)
    assert again[0].tobytes() == q.tobytes() and again[1].tobytes() == deg.tobytes()
    alone = run(dev, a, y, off, depth, deg=False)
    assert alone[1] is None and alone[0].tobytes() == q.tobytes() and (alone[2] == 0).all()    # q does not depend on deg
    other = run(dev, a, np.random.default_rng(3).standard_normal(a.size).astype(np.float32), off, depth)
    assert other[1].tobytes() == deg.tobytes() and other[0].tobytes() != q.tobytes()           # deg does not depend on y
    # a sample of the rows, permuted and embedded between other rows
    rng = np.random.default_rng(1)
    long_rows = [r for r in range(len(rows)) if rows[r][0].size >= 64 * _tile() and rows[r][2] >= 2][:2]
    pick = list(rng.permutation([r for r in range(len(rows)) if rows[r][0].size < 64 * _tile()])[:150]) + long_rows
    pick = [int(r) for r in rng.permutation(pick)]
    filler = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(0, 600, len(pick) + 1)]
    pa, py, lens, deps, where = [], [], [], [], {}
    for k, r in enumerate(pick + [None]):
        pa.append(filler[k])
        py.append(filler[k][::-1].copy())
        lens.append(filler[k].size)
        deps.append(filler[k].size // 2)
        if r is not None:
            where[r] = len(lens)
            pa.append(rows[r][0])
            py.append(rows[r][1])
            lens.append(rows[r][0].size)
            deps.append(rows[r][2])
    off2, _ = _offsets(lens, _tile())
    q2, deg2, status2 = run(dev, np.concatenate(pa), np.concatenate(py), off2, deps)
    assert (status2 == 0).all() and len(long_rows) == 2
    for r, k in where.items():
        assert q2[off2[k]:off2[k + 1]].tobytes() == q[off[r]:off[r + 1]].tobytes(), rows[r][2:]
        assert deg2[off2[k]:off2[k + 1]].tobytes() == deg[off[r]:off[r + 1]].tobytes(), rows[r][2:]
    # depth = NULL is every row fully ranked
    full = [r for r in range(len(rows)) if rows[r][2] == rows[r][0].size and rows[r][0].size < 1000]
    offf, _ = _offsets([rows[r][0].size for r in full], _tile())
    qf, degf, _ = run(dev, np.concatenate([rows[r][0] for r in full]), np.concatenate([rows[r][1] for r in full]), offf, None)
    for k, r in enumerate(full):
        assert qf[offf[k]:offf[k + 1]].tobytes() == q[off[r]:off[r + 1]].tobytes()
        assert degf[offf[k]:offf[k + 1]].tobytes() == deg[off[r]:off[r + 1]].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. bad rows
# ---------------------------------------------------------------------------------------------------------------------
LENS = [300, 10, 600, 5, 20]                      # offsets 0, 300, 310, 910, 915, 935; tiles 2, 1, 3, 1, 1


def _plain():
    rng = np.random.default_rng(8)
    a, y = (rng.standard_normal(sum(LENS)).astype(np.float32) for _ in range(2))
    off, tile_off = _offsets(LENS, _tile())
    return a, y, off, tile_off, np.array([300, 4, 599, 5, 0], dtype=np.int32)


def test_a_non_finite_row_gets_nan_and_its_neighbours_are_untouched(dev):
    a, y, off, tile_off, depth = _plain()
    q0, deg0, st0 = run(dev, a, y, off, depth)
    assert (st0 == 0).all() and np.isfinite(q0).all() and np.isfinite(deg0).all()
    for which, value, rows_hit, at in (("a", np.nan, [2], [off[2] + 599]), ("a", np.inf, [1], [off[1]]),
                                       ("a", -np.inf, [0, 3], [5, off[3] + 2]), ("y", np.nan, [2], [off[2] + 300]),
                                       ("y", np.nan, [0], [299]), ("y", np.inf, [1, 4], [off[1] + 9, off[4] + 7])):
        b, z = a.copy(), y.copy()
        (b if which == "a" else z)[at] = value
        for want_deg in (True, False):
            q, deg, status = run(dev, b, z, off, depth, deg=want_deg)
            assert (status == 0).all()
            for r in range(5):
                sl = slice(off[r], off[r + 1])
                if r in rows_hit:
                    assert np.isnan(q[sl]).all() and (deg is None or np.isnan(deg[sl]).all()), (which, value, r)
                else:
                    assert q[sl].tobytes() == q0[sl].tobytes(), (which, value, r)
                    assert deg is None or deg[sl].tobytes() == deg0[sl].tobytes(), (which, value, r)


def test_invalid_rows_get_status_2_and_nothing_of_them_is_written(dev):
    """Offsets that decrease or run past `entries`, a depth outside [0, L], a wrong tile count: the bad values are only
    compared, so nothing outside the buffers is read; the row is marked and the other rows keep their bytes."""
    a, y, off, tile_off, depth = _plain()
    q0, deg0, _ = run(dev, a, y, off, depth)
    cases = (("decreasing", {2: 290}, {}, {}, [1]), ("past entries", {5: 936}, {}, {}, [4]),
             ("negative", {0: -1}, {}, {}, [0]), ("tile count", {2: 700}, {}, {}, [1, 2]),
             ("depth < 0", {}, {1: -1}, {}, [1]), ("depth > L", {}, {3: 6}, {}, [3]),
             ("depth > L, long", {}, {2: 601}, {}, [2]), ("tile offsets", {}, {}, {3: 7}, [2, 3]),
             ("tiles past n_tiles", {}, {}, {5: 9}, [4]))
    for name, edit_off, edit_depth, edit_tiles, bad_rows in cases:
        ro, dp, tl = off.copy(), depth.copy(), tile_off.copy()
        for k, v in edit_off.items():
            ro[k] = v
        for k, v in edit_depth.items():
            dp[k] = v
        for k, v in edit_tiles.items():
            tl[k] = v
        q, deg, status = run(dev, a, y, ro, dp, tile_off=tl, n_tiles=int(tile_off[-1]), fill=-123.0)
        assert status.tolist() == [2 if r in bad_rows else 0 for r in range(5)], name
        owners = np.zeros(a.size, dtype=np.int64)         # "decreasing" makes row 2 start inside row 0: two writers there
        for r in range(5):
            if r not in bad_rows:
                owners[ro[r]:ro[r + 1]] += 1
        for r in range(5):
            if r not in bad_rows and ro[r] == off[r] and ro[r + 1] == off[r + 1]:
                mine = np.arange(off[r], off[r + 1])[owners[off[r]:off[r + 1]] == 1]
                assert q[mine].tobytes() == q0[mine].tobytes() and deg[mine].tobytes() == deg0[mine].tobytes(), (name, r)
        assert (q[owners == 0] == -123.0).all() and (deg[owners == 0] == -123.0).all(), name   # the sentinels survive


# ---------------------------------------------------------------------------------------------------------------------
# 4. the table-level product
# ---------------------------------------------------------------------------------------------------------------------
def _ragged_lists(n, m, low, high, seed):
    from mfcd.lists import RankedLists
    rng = np.random.default_rng(seed)
    users, items, positions, depth = [], [], [], []
    for u in range(n):
        L = int(rng.integers(low, high + 1))
        users += [u] * L
        items += rng.choice(m, L, replace=False).tolist()
        positions += list(range(L))
        depth.append(int(rng.integers(0, L + 1)) if u % 2 else L)
    return RankedLists(users, items, positions, n, m, depth)


@pytest.mark.parametrize("d", [1, 3, 16])
def test_pl_hvp_matches_the_models_table_product(dev, d):
    """The model is given the device's own fp32 scores a and dA, so what is compared is the kernels' q and g and the
    gather-sums.  Per entry the kernels differ from the model by eq = 2^-24 |q| + 8 (L + 128) 2^-53 scale (this file's
    bound) and eg = RTOL |g| + ATOL (test_lists.py's); a gather-sum of k fp32 products adds at most (k + 2) 2^-24 of the
    sum of their sizes, the two sums' addition and the product with c three more roundings of the result."""
    import structure as S
    from mfcd import lists as ML
    n, m = 12, 40
    host = _ragged_lists(n, m, 0, 40, 9)
    R = host.to(dev)
    rng = np.random.default_rng(20 + d)
    U, V, dU, dV = (rng.standard_normal(s).astype(np.float32) * f for s, f in (((n, d), 0.7), ((m, d), 0.7), ((n, d), 1.0),
                                                                                ((m, d), 1.0)))
    Ud, Vd, dUd, dVd = (to(dev, t) for t in (U, V, dU, dV))
    model = S.MatrixFactorization(n, m, d).to(dev)
    with torch.no_grad():
        model.U.copy_(Ud)
        model.V.copy_(Vd)
    a = ML.list_scores(Ud, Vd, R)[0]
    dA = ML.list_scores(dUd, Vd, R)[0] + ML.list_scores(Ud, dVd, R)[0]
    off, item, user = host.row_off.numpy(), host.item.numpy().astype(np.int64), host.user.numpy().astype(np.int64)
    prob = HM.Problem(off, item, host.depth.numpy())
    assert prob.c == 1.0 / host.stages
    lens = np.diff(off)[user]
    per_item = np.bincount(item, minlength=m)
    for gn in (False, True):
        got = S.rankings_hvp(model, R, dUd, dVd, gauss_newton=gn)
        assert torch.equal(got[0], ML.pl_hvp(Ud, Vd, dUd, dVd, R, gn)[0])
        HU, HV, (q, scale, g) = prob.hvp(U, V, dU, dV, gn, a=a.cpu().numpy(), y=dA.cpu().numpy())
        eq = U24 * np.abs(q) + 8 * (lens + 128) * U53 * scale
        eg = RTOL * np.abs(g) + ATOL
        for name, t, want, idx, tab, dtab, k in (("HU", got[0], HU, user, V[item], dV[item], np.diff(off)[:, None]),
                                                 ("HV", got[1], HV, item, U[user], dU[user], per_item[:, None])):
            bound, size = np.zeros_like(want), np.zeros_like(want)
            np.add.at(bound, idx, eq[:, None] * np.abs(tab))
            np.add.at(size, idx, np.abs(q)[:, None] * np.abs(tab))
            if not gn:
                np.add.at(bound, idx, eg[:, None] * np.abs(dtab))
                np.add.at(size, idx, np.abs(g)[:, None] * np.abs(dtab))
            bound = prob.c * (bound + (k + 2) * U24 * size) + 3 * U24 * np.abs(want)
            assert t.dtype == torch.float32 and tuple(t.shape) == want.shape
            err = np.abs(t.cpu().numpy().astype(np.float64) - want)
            live = bound > 0
            print(f"d={d} gauss_newton={gn}: {name} max |entry| {np.abs(want).max():.3e}, max error / bound "
                  f"{(err[live] / bound[live]).max():.3f}")
            assert (err <= bound).all(), (gn, name)
    # a loose second witness: the central difference of pl_risk's own autograd gradients, h = 2^-6; fp32 gradients at
    # 2e-5 relative over 2 h give 1e-3 of their size, the truncation h^2 times the third derivative: 5 % of the largest entry
    h = 2.0 ** -6

    def grads(sign):
        Ut, Vt = (Ud + sign * h * dUd).requires_grad_(), (Vd + sign * h * dVd).requires_grad_()
        ML.pl_risk(Ut, Vt, R).backward()
        return Ut.grad.double(), Vt.grad.double()

    (pU, pV), (mU, mV) = grads(1.0), grads(-1.0)
    HU, HV = ML.pl_hvp(Ud, Vd, dUd, dVd, R)
    for fd, H in (((pU - mU) / (2 * h), HU.double()), ((pV - mV) / (2 * h), HV.double())):
        assert float((fd - H).abs().max()) <= 0.05 * float(H.abs().max())
    with pytest.raises(ValueError):
        S.rankings_hvp(model, R, dUd[:-1], dVd)


def test_rankings_hvp_is_symmetric(dev):
    import structure as S
    n, m, d = 12, 40, 4
    R = _ragged_lists(n, m, 0, 40, 10).to(dev)
    torch.manual_seed(4)
    model = S.MatrixFactorization(n, m, d).to(dev)
    g = torch.Generator().manual_seed(5)
    xU, xV, yU, yV = (torch.randn(s, generator=g).to(dev) for s in ((n, d), (m, d), (n, d), (m, d)))
    for gn in (False, True):
        HxU, HxV = S.rankings_hvp(model, R, xU, xV, gn)
        HyU, HyV = S.rankings_hvp(model, R, yU, yV, gn)
        left = float((yU.double() * HxU.double()).sum() + (yV.double() * HxV.double()).sum())
        right = float((xU.double() * HyU.double()).sum() + (xV.double() * HyV.double()).sum())
        size = float((yU.abs().double() * HxU.abs().double()).sum() + (yV.abs().double() * HxV.abs().double()).sum())
        assert abs(left - right) <= RTOL * size, (gn, left, right)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the exact steps
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_problem():
    """(the lists on the host, U0, V, the model problem, the model's user minimisers, the gradient noise there)."""
    from mfcd import lists
    U0, V, users, items, positions, depth = HM.step_inputs()
    R = lists.RankedLists(users, items, positions, HM.STEP_N, HM.STEP_M, depth)
    prob = HM.Problem(R.row_off.numpy(), R.item.numpy(), R.depth.numpy())
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(HM.STEP_D), V64, r, L2)[0] for r in range(HM.STEP_N)])
    return R, U0, V, prob, Uopt, prob.user_noise(Uopt, V64)


def check_user_rows(res, what):
    _, _, V, prob, Uopt, noise = step_problem()
    staged = prob.stages > 0
    rows = res.rows.cpu().numpy().astype(np.float64)
    status, ratio = res.status.cpu().numpy(), res.grad_ratio.cpu().numpy()
    assert res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (HM.STEP_N, HM.STEP_D)
    dist = np.linalg.norm(rows - Uopt, axis=1)
    bound = GTOL * np.abs(Uopt).max(axis=1) + noise / L2
    print(f"{what}: status {status.tolist()}, Newton {res.newton_iters.tolist()}, CG {res.cg_iters.tolist()}, "
          f"grad_ratio {np.round(ratio, 6).tolist()}, |u - u*| / bound {np.round(dist[staged] / bound[staged], 3).tolist()}")
    assert (status[staged] == 0).all() and (ratio[staged] <= GTOL).all()
    assert (dist[staged] <= bound[staged]).all()                                  # strong convexity, modulus l2
    V64 = V.astype(np.float64)
    f_model = np.array([prob.user_objective(rows[r], V64, r, L2) for r in range(HM.STEP_N)])
    np.testing.assert_allclose(res.objective_after.cpu().numpy(), f_model, rtol=RTOL, atol=ATOL)
    lone = np.flatnonzero(~staged)
    assert len(lone) == 4
    assert res.rows.cpu().numpy()[lone].tobytes() == np.zeros((len(lone), HM.STEP_D), np.float32).tobytes()   # exactly +0
    assert (status[lone] == 0).all() and (res.newton_iters.cpu().numpy()[lone] == 0).all()
    assert (res.cg_iters.cpu().numpy()[lone] == 0).all() and (res.objective_after.cpu().numpy()[lone] == 0.0).all()
    return rows


def test_user_step_and_fold_in_reach_the_models_minimisers(dev):
    from mfcd import lists, lists_exact
    host, U0, V, prob, Uopt, _ = step_problem()
    R, U0d, Vd = host.to(dev), to(dev, U0), to(dev, V)
    res = lists_exact.lists_user_step(U0d, Vd, R, L2)
    check_user_rows(res, "user step")
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all()
    f0 = np.array([prob.user_objective(U0[r].astype(np.float64), V.astype(np.float64), r, L2) for r in range(HM.STEP_N)])
    np.testing.assert_allclose(before, f0, rtol=RTOL, atol=ATOL)
    assert torch.equal(U0d, to(dev, U0)) and torch.equal(Vd, to(dev, V))            # the inputs are not modified
    fold = lists_exact.lists_user_step(None, Vd, R, L2)
    check_user_rows(fold, "fold-in")
    # a user whose list names a NaN-scoring item: status 2, a NaN row; the others as in a call without that user
    bad_user = 4
    assert prob.stages[bad_user] > 0 and HM.SPARE_ITEM not in host.item.tolist()
    users, items, positions = host.user.numpy().astype(np.int64), host.item.numpy().astype(np.int64), host.position.numpy()
    poisoned = items.copy()
    poisoned[np.flatnonzero(users == bad_user)[1]] = HM.SPARE_ITEM
    Vbad = Vd.clone()
    Vbad[HM.SPARE_ITEM] = float("nan")
    depth = host.depth.numpy()
    bad = lists_exact.lists_user_step(U0d, Vbad, lists.RankedLists(users, poisoned, positions, HM.STEP_N, HM.STEP_M,
                                                                   depth).to(dev), L2, coef=prob.c)
    others = [r for r in range(HM.STEP_N) if r != bad_user]
    assert bad.status.tolist() == [2 if r == bad_user else 0 for r in range(HM.STEP_N)]
    assert bool(torch.isnan(bad.rows[bad_user]).all())
    rest = users != bad_user
    d_rest = depth.copy()
    d_rest[bad_user] = 0
    without = lists_exact.lists_user_step(U0d, Vbad, lists.RankedLists(users[rest], items[rest], positions[rest], HM.STEP_N,
                                                                       HM.STEP_M, d_rest).to(dev), L2, coef=prob.c)
    assert bad.rows[others].cpu().numpy().tobytes() == without.rows[others].cpu().numpy().tobytes()
    assert bad.newton_iters[others].tolist() == without.newton_iters[others].tolist()
    assert without.rows[bad_user].tolist() == [0.0] * HM.STEP_D and int(without.status[bad_user]) == 0
    with pytest.raises(ValueError):
        lists_exact.lists_user_step(U0d, Vd, R, 0.0)
    with pytest.raises(ValueError):
        lists_exact.lists_user_step(U0d, Vd[:-1], R, L2)
    lone = lists.RankedLists([0, 1, 1], [0, 1, 2], [0, 0, 1], HM.STEP_N, HM.STEP_M, depth=[1, 0] + [0] * (HM.STEP_N - 2)).to(dev)
    for coef in (None, 0.5):
        with pytest.raises(ValueError):
            lists_exact.lists_user_step(U0d, Vd, lone, L2, coef=coef)                # no stage


def test_item_step_descends_to_a_certified_point(dev):
    from mfcd import lists_exact
    host, U0, V, prob, _, _ = step_problem()
    R, U0d, Vd = host.to(dev), to(dev, U0), to(dev, V)
    res = lists_exact.lists_item_step(U0d, Vd, R, L2)
    rows = res.rows.cpu().numpy().astype(np.float64)
    U64 = U0.astype(np.float64)
    gnorm = np.linalg.norm(prob.grads(U64, rows)[1] + L2 * rows)
    print(f"Newton {int(res.newton_iters)}, CG {int(res.cg_iters)}, |grad| {gnorm:.3e} against gtol l2 max|V| "
          f"{GTOL * L2 * np.abs(rows).max():.3e}, grad_ratio {float(res.grad_ratio):.2e}, F {float(res.objective_before):.6f} "
          f"-> {float(res.objective_after):.6f}")
    assert int(res.status) == 0 and res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (HM.STEP_M, HM.STEP_D)
    assert res.status.dim() == 0 and res.objective_after.dim() == 0
    assert float(res.objective_after) <= float(res.objective_before) and float(res.grad_ratio) <= GTOL
    np.testing.assert_allclose(float(res.objective_after), prob.item_objective(U64, rows, L2), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(res.objective_before), prob.item_objective(U64, V.astype(np.float64), L2), rtol=RTOL,
                               atol=ATOL)
    assert torch.equal(Vd, to(dev, V))
    Ubad = U0d.clone()
    Ubad[3, 1] = float("nan")
    bad = lists_exact.lists_item_step(Ubad, Vd, R, L2)
    assert int(bad.status) == 2 and torch.equal(bad.rows, Vd)


def test_alternating_fit_descends_and_records_the_models_objective(dev):
    from mfcd import lists_exact
    host, U0, V, prob, _, _ = step_problem()
    R = host.to(dev)
    rng = np.random.default_rng(8)
    V0 = (0.3 * rng.standard_normal(V.shape)).astype(np.float32)
    tables = (to(dev, U0), to(dev, V0))
    seen = []
    for sweep in range(3):                                       # one sweep at a time
        res = lists_exact.fit_lists_exact(*tables, R, L2, 1)
        assert res.U is tables[0] and res.V is tables[1]
        if sweep == 0:
            start = prob.objective(U0.astype(np.float64), V0.astype(np.float64), L2)
            np.testing.assert_allclose(float(res.objective_start), start, rtol=RTOL, atol=ATOL)
            seen.append(float(res.objective_start))
        seen += res.history[0].tolist()
    U3, V3 = to(dev, U0), to(dev, V0)
    res = lists_exact.fit_lists_exact(U3, V3, R, L2, 3)
    flat = res.history.reshape(-1).tolist()
    print(f"F: start {seen[0]:.7f}, sub-steps {np.round(flat, 7).tolist()}")
    assert tuple(res.history.shape) == (3, 2) and not torch.equal(U3, to(dev, U0)) and not torch.equal(V3, to(dev, V0))
    assert all(b <= a for a, b in zip([float(res.objective_start)] + flat[:-1], flat))   # non-increasing
    np.testing.assert_allclose(flat, seen[1:], rtol=1e-9)        # three sweeps are three chained calls of one sweep
    # every recorded value against the model, at the tables of that sub-step: replay with the steps
    U, Vt = to(dev, U0), to(dev, V0)
    for sweep in range(3):
        U = lists_exact.lists_user_step(U, Vt, R, L2).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(flat[2 * sweep], want, rtol=RTOL, atol=ATOL)
        Vt = lists_exact.lists_item_step(U, Vt, R, L2).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(flat[2 * sweep + 1], want, rtol=RTOL, atol=ATOL)
    assert tuple(res.user_status.shape) == (HM.STEP_N,) and res.item_status.dim() == 0


def test_structure_entries_on_a_small_model(dev):
    import structure as S
    n, m, d, wd = 40, 30, 3, 0.05
    g = torch.Generator().manual_seed(21)
    X = (torch.randn(n + 8, 2, generator=g).double() @ torch.randn(m, 2, generator=g).double().t()).float().to(dev)
    train = S.observe_rankings(X[:n], 10, s=2.0, seed=0)
    fresh = S.observe_rankings(X[n:], 8, depth=4, s=2.0, seed=1)                    # users who were not in training
    torch.manual_seed(3)
    model = S.MatrixFactorization(n, m, d).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=wd)
    S.train_model_rankings(model, train, opt, dev, num_steps=20, log_every=0)
    U0, V0 = model.U.detach().clone(), model.V.detach().clone()
    res_u, gain_u = S.refit_users_rankings(model, train, wd)
    res_v, gain_v = S.refit_items_rankings(model, train, wd)
    assert (gain_u >= 0).all() and float(gain_v) >= 0 and gain_v.dim() == 0 and tuple(gain_u.shape) == (n,)
    assert tuple(res_u.rows.shape) == (n, d) and tuple(res_v.rows.shape) == (m, d)
    assert torch.equal(model.U.detach(), U0) and torch.equal(model.V.detach(), V0)  # the refits leave the model alone
    fold = S.fit_users_rankings(model, fresh, wd, coef=1.0 / train.stages)
    bare = S.fit_users_rankings(model.V.data, fresh, wd, coef=1.0 / train.stages)
    assert tuple(fold.rows.shape) == (8, d) and torch.equal(fold.rows, bare.rows) and (fold.status != 2).all()
    guest = S.MatrixFactorization(8, m, d).to(dev)
    with torch.no_grad():
        guest.U.copy_(fold.rows)
        guest.V.copy_(model.V)
    top = S.recommend_items(guest, k=5)
    assert tuple(top.shape) == (8, 5) and int(top.min()) >= 0 and int(top.max()) < m
    hist = S.train_model_rankings_exact(model, train, wd, sweeps=2)
    flat = [f for pair in hist for f in pair]
    assert len(hist) == 2 and all(len(pair) == 2 for pair in hist) and all(b <= a for a, b in zip(flat[:-1], flat[1:]))
    assert not torch.equal(model.U.detach(), U0) and not torch.equal(model.V.detach(), V0) and not model.training
