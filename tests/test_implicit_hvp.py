"""GPU tests of the implicit-feedback Hessian-vector kernel and of what is built on it (include/mfcd.h:
mfcd_implicit_hvp_rows; mfcd/implicit.py: implicit_hvp_rows, implicit_hvp; mfcd/implicit_exact.py;
structure.implicit_hvp, fit_users_implicit, refit_users_implicit, refit_items_implicit, train_model_implicit_exact)
against the float64 model of tests/implicit_hvp_model.py.

Shapes: those of tests/test_implicit.py, whose lists and score rows are used as they are — m in {1, 2, 63, 64, 65, C-1, C,
C+1, 2C+3} with C = implicit.CHUNK, per m one row for every L in {0, 1, 2, 63, 64, 65, T-1, T, T+1, m-1, m} clipped to m
and the row of scores in {-60, 0, 60}, in the variants none / barred / overlap.  Directions: the four kinds of
tests/test_pair_hvp.py, one per row in turn — distinct values in [-2, 2], three levels, a constant row (q is exactly +0)
and integers in [-3, 3] times 2^-130 (denormals).

Tolerance: the project's fp32 pair tolerance of tests/test_pair_hvp.py, whose derivation carries over because the per-pair
arithmetic (the difference, one v_exp_f32, one reciprocal, e h h, the difference of y, one FMA) and the fp32 runs of at
most 64 terms are the same.  It is stated on the mean term — q_c divided by the number k_c of pairs the column takes part
in, neg for an observed column and pos for an unobserved one — as 2e-5 times the model's mean magnitude mean w |y_i - y_j|
plus 2e-6 max |y| of the row; for deg, 2e-5 mean w + 2e-6.  The references are computed once per module and shared."""
import functools

import numpy as np
import pytest
import torch

import implicit_hvp_model as HM
import rank_entries_model as RM
from test_implicit import VARIANTS, _CT, _dev_lists, _device_scores, _lists, _Ls, _ms, _scores

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
GTOL, L2 = HM.GTOL, HM.L2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def direction(kind, m, rng):
    if kind == 0:
        return (rng.permutation(m).astype(np.float64) / m * 4.0 - 2.0).astype(np.float32)
    if kind == 1:
        return rng.choice(np.array([-1.0, 0.0, 0.5], dtype=np.float32), m)
    if kind == 2:
        return np.full(m, 0.3, dtype=np.float32)
    return (rng.integers(-3, 4, m).astype(np.float64) * 2.0 ** -130).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _dirs(m):
    """One direction row per score row of `_scores(m)` → (Y fp32 [rows, m], kinds); the extreme row gets distinct values."""
    rng = np.random.default_rng(4000 + m)
    rows = len(_Ls(m)) + 1
    kinds = [(r + m) % 4 for r in range(rows - 1)] + [0]
    return np.stack([direction(k, m, rng) for k in kinds]), np.array(kinds)


@functools.lru_cache(maxsize=None)
def _want(m, variant):
    """(q, deg, mag, k) of the dense case (m, variant), computed once; k: the pairs every column takes part in."""
    pos, excl = _lists(m, variant)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    q, deg, mag = HM.hvp_rows(_scores(m), _dirs(m)[0], po, pi, None if variant == "none" else eo, ei)
    k = np.stack([HM.partners(m, p, e if variant != "none" else ()) for p, e in zip(pos, excl)])
    return q, deg, mag, k


def check(Q, D, want, Y, tag, coef=None):
    """Device outputs against the model's on the mean term, the row sums, and the exact zeros."""
    q, deg, mag, k = want
    c = np.ones((len(q), 1)) if coef is None else np.asarray(coef, dtype=np.float64)[:, None]
    ymax = np.abs(Y.astype(np.float64)).max(axis=1, keepdims=True)
    bound_q = RTOL * mag / k + ATOL * c * ymax
    bound_d = RTOL * deg / k + ATOL * c
    err_q = np.abs(Q.astype(np.float64) - q) / k
    err_d = np.abs(D.astype(np.float64) - deg) / k
    live = bound_q > 0
    print(f"{tag}: q max error / bound {(err_q[live] / bound_q[live]).max() if live.any() else 0.0:.3f}, "
          f"deg max error / bound {(err_d / bound_d).max():.3f}, largest mean term {np.abs(q / k).max():.3e}")
    assert np.isfinite(Q).all() and np.isfinite(D).all(), tag
    assert (err_q <= bound_q).all(), tag
    assert (err_d <= bound_d).all(), tag
    # every pair enters twice with opposite signs: a row of q sums to 0 within the sum of its entries' bounds
    assert (np.abs(Q.astype(np.float64).sum(axis=1)) <= (bound_q * k).sum(axis=1)).all(), tag
    dead = deg == 0                                    # barred columns, rows without a pair: exactly +0
    assert Q[dead].tobytes() == np.zeros_like(Q[dead]).tobytes() and D[dead].tobytes() == np.zeros_like(D[dead]).tobytes(), tag


def run(dev, X, Y, P, E, deg=True, **kw):
    from mfcd import implicit
    q, dg, status = implicit.implicit_hvp_rows(X, Y, P, E, deg=deg, **kw)
    assert q.dtype == torch.float32 and status.dtype == torch.int32 and (dg is None) == (not deg)
    return q.cpu().numpy(), None if dg is None else dg.cpu().numpy(), status.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", _ms())
def test_dense_rows_match_the_f64_model(dev, m, variant):
    Y, kinds = _dirs(m)
    X = to(dev, _scores(m))
    P, E = _dev_lists(m, variant, dev)
    Q, D, status = run(dev, X, to(dev, Y), P, E)
    assert (status == 0).all() and Q.shape == (len(kinds), m)
    want = _want(m, variant)
    check(Q, D, want, Y, f"dense m={m} {variant}")
    const = kinds == 2
    assert Q[const].tobytes() == np.zeros_like(Q[const]).tobytes()             # a constant direction: exactly +0
    pos, excl = _lists(m, variant)
    for r, (p, e) in enumerate(zip(pos, excl)):                                # rows with pos neg = 0: exactly +0
        Pu, Nu = HM.IM.classes(m, p, e if variant != "none" else ())
        if Pu.size * Nu.size == 0:
            assert Q[r].tobytes() == np.zeros(m, dtype=np.float32).tobytes() == D[r].tobytes(), r
    tiny = kinds == 3
    if tiny.any():
        assert (np.abs(Q[tiny]) <= want[3][tiny] * 0.25 * 6.0 * 2.0 ** -130).all()     # k terms of at most w |dy|
        assert (Q[tiny] != 0).any() or not (want[0][tiny] != 0).any()          # denormal directions are not flushed
    assert run(dev, X, to(dev, Y), P, E, deg=False)[0].tobytes() == Q.tobytes()       # deg = NULL: the same q


@pytest.mark.parametrize("d", [1, 33])
@pytest.mark.parametrize("m", _ms())
def test_factor_mode_with_exact_scores_matches_the_f64_model(dev, m, d):
    """Factors on the grid of halves: every product and every partial sum is exact in fp32, so the device's scores and
    directions are the model's whatever the order of the MFMA sums."""
    rng = np.random.default_rng(37 * m + d)
    variant = VARIANTS[(m + d) % 3]
    rows = len(_Ls(m)) + 1
    n = rows + 3
    hi = 3 if d == 1 else 1
    A, Ay = ((rng.integers(-2, 3, (n, d)) * 0.5).astype(np.float32) for _ in range(2))
    B, By = ((rng.integers(-2 * hi, 2 * hi + 1, (m, d)) * 0.5).astype(np.float32) for _ in range(2))
    ids = rng.permutation(n)[:rows]
    S = A.astype(np.float64) @ B.astype(np.float64).T
    Y = Ay.astype(np.float64) @ By.astype(np.float64).T
    assert (S.astype(np.float32) == S).all() and (Y.astype(np.float32) == Y).all()
    pos, excl = _lists(m, variant)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    bar = variant != "none"
    q, deg, mag = HM.hvp_rows(S, Y, po, pi, eo if bar else None, ei, row_ids=ids)
    k = np.stack([HM.partners(m, p, e if bar else ()) for p, e in zip(pos, excl)])
    P, E = _dev_lists(m, variant, dev)
    Q, D, status = run(dev, (to(dev, A), to(dev, B)), (to(dev, Ay), to(dev, By)), P, E, rows=ids)
    assert (status == 0).all()
    check(Q, D, (q, deg, mag, k), Y[ids].astype(np.float32), f"factored m={m} d={d} {variant}")
    # the user step's and the item step's forms: one table passed twice
    Qu = run(dev, (to(dev, A), to(dev, B)), (to(dev, Ay), to(dev, B)), P, E, rows=ids)[0]
    qu, _, magu = HM.hvp_rows(S, Ay.astype(np.float64) @ B.astype(np.float64).T, po, pi, eo if bar else None, ei, row_ids=ids)
    assert (np.abs(Qu - qu) / k <= RTOL * magu / k + ATOL * np.abs(Ay.astype(np.float64) @ B.T).max()).all()


@pytest.mark.parametrize("m,d", [(65, 33), (2049, 2), (4099, 33)])
def test_dense_mode_and_factor_mode_agree_on_random_factors(dev, m, d):
    """Random fp32 factors.  The factor mode is held to the model on the device's own scores and directions (what
    mfcd_rank_entries reports for every column: the same score kernel), at the tolerance above.  The dense mode gets a
    library GEMM's products, which differ from those by the GEMM's rounding: the two results are compared with each other
    at the same tolerance, on the model's magnitudes."""
    assert m in _ms()
    rng = np.random.default_rng(5 * m + d)
    rows = len(_Ls(m)) + 1
    n = rows + 2
    A, Ay = (to(dev, (rng.standard_normal((n, d)) * (1.5 / np.sqrt(d))).astype(np.float32)) for _ in range(2))
    B, By = (to(dev, rng.standard_normal((m, d)).astype(np.float32)) for _ in range(2))
    ids = rng.permutation(n)[:rows]
    S, Y = _device_scores(A, B, ids, m, dev), _device_scores(Ay, By, ids, m, dev)
    pos, excl = _lists(m, "overlap")
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(excl)
    q, deg, mag = HM.hvp_rows(S, Y, po, pi, eo, ei)
    k = np.stack([HM.partners(m, p, e) for p, e in zip(pos, excl)])
    P, E = _dev_lists(m, "overlap", dev)
    Qf, Df, st = run(dev, (A, B), (Ay, By), P, E, rows=ids)
    assert (st == 0).all()
    check(Qf, Df, (q, deg, mag, k), Y, f"factor mode on the device's scores m={m} d={d}")
    Qd, Dd, _ = run(dev, A @ B.t(), Ay @ By.t(), P, E, rows=ids)
    ymax = np.abs(Y.astype(np.float64)).max(axis=1, keepdims=True)
    err_q, err_d = np.abs(Qf.astype(np.float64) - Qd) / k, np.abs(Df.astype(np.float64) - Dd) / k
    bound_q, bound_d = RTOL * mag / k + ATOL * ymax, RTOL * deg / k + ATOL
    print(f"m={m} d={d}: dense against factor mode, q max error / bound {(err_q / bound_q).max():.3f}, deg "
          f"{(err_d / bound_d).max():.3f}; bit-equal: {Qf.tobytes() == Qd.tobytes()}")
    assert (err_q <= bound_q).all() and (err_d <= bound_d).all()


def test_factor_mode_across_a_slab_boundary(dev):
    """500 rows of m = 70 001 at d = 2: 479 rows of 70 016 floats fit 128 MiB and a slab takes whole blocks of 128 rows
    of them, 384, so rows 384 .. 499 go through the entry's second block of rows — other slab rows, the row ids from the
    384th on, the non-finite counts of a block indexed from its first row.  Rows on both sides of the boundary, a
    non-finite row in either block among them, equal a call on those rows alone (one block, other positions) to the bits,
    with and without deg, and the model.  Factors on the grid of halves: the scores and directions are exact."""
    from mfcd import _lib
    rng = np.random.default_rng(6)
    n, m, d = 500, 70001, 2
    ws = _lib.load().mfcd_implicit_hvp_rows_workspace_bytes(n, m, d)
    slab_rows = ws // (2 * 70016 * 4)
    assert slab_rows == 384
    A, Ay = ((rng.integers(-2, 3, (n, d)) * 0.5).astype(np.float32) for _ in range(2))
    B, By = ((rng.integers(-3, 4, (m, d)) * 0.5).astype(np.float32) for _ in range(2))
    order = rng.permutation(n)                                  # the requested rows: any order
    bad = [10, 450]
    A[order[10], 0], Ay[order[450], 1] = np.inf, np.nan         # a non-finite score row, a non-finite direction row
    pos = [np.sort(rng.choice(m, 3, replace=False)) for _ in range(n)]
    exc = [np.sort(rng.choice(m, 50, replace=False)) for _ in range(n)]
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(exc)
    X, Yf = (to(dev, A), to(dev, B)), (to(dev, Ay), to(dev, By))
    Q, D, status = run(dev, X, Yf, (to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)), rows=order)
    assert (status == 0).all()
    finite = np.isfinite(Q).all(axis=1) & np.isfinite(D).all(axis=1)
    assert np.flatnonzero(~finite).tolist() == bad and np.isnan(Q[bad]).all() and np.isnan(D[bad]).all()
    Q0 = run(dev, X, Yf, (to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)), rows=order, deg=False)[0]
    assert Q0.tobytes() == Q.tobytes()
    at = list(range(slab_rows - 4, slab_rows + 4)) + [0, n - 1] + bad
    (pa, pia), (ea, eia) = RM.csr([pos[r] for r in at]), RM.csr([exc[r] for r in at])
    lists = ((to(dev, pa), to(dev, pia)), (to(dev, ea), to(dev, eia)))
    alone = run(dev, X, Yf, *lists, rows=order[at])
    assert alone[0].tobytes() == Q[at].tobytes() and alone[1].tobytes() == D[at].tobytes()
    assert run(dev, X, Yf, *lists, rows=order[at], deg=False)[0].tobytes() == Q[at].tobytes()
    good = at[:-2]
    S = A.astype(np.float64)[order[good]] @ B.astype(np.float64).T
    Y = Ay.astype(np.float64)[order[good]] @ By.astype(np.float64).T
    (pg, pig), (eg, eig) = RM.csr([pos[r] for r in good]), RM.csr([exc[r] for r in good])
    q, deg, mag = HM.hvp_rows(S, Y, pg, pig, eg, eig)
    k = np.stack([HM.partners(m, pos[r], exc[r]) for r in good])
    check(Q[good], D[good], (q, deg, mag, k), Y.astype(np.float32), "rows on both sides of the slab boundary")


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism and independence
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_calls_are_bit_equal_and_rows_do_not_depend_on_their_neighbours(dev):
    C, _ = _CT()
    m = 2 * C + 3
    rng = np.random.default_rng(8)
    d, n = 5, len(_lists(m, "overlap")[0])
    A, B, Ay, By = (to(dev, rng.standard_normal(s).astype(np.float32)) for s in ((n, d), (m, d), (n, d), (m, d)))
    X, Y = (A @ B.t()).contiguous(), (Ay @ By.t()).contiguous()
    P, E = _dev_lists(m, "overlap", dev)
    for Mx, My in (((A, B), (Ay, By)), (X, Y)):
        one = run(dev, Mx, My, P, E)
        assert _same(one, run(dev, Mx, My, P, E))                              # two calls
        assert run(dev, Mx, My, P, E, deg=False)[0].tobytes() == one[0].tobytes()
        order = np.concatenate((rng.permutation(n), [2, 2, n - 1]))            # another order, with repeats
        Pp, Ep = _dev_lists(m, "overlap", dev, sel=order)
        moved = run(dev, Mx, My, Pp, Ep, rows=order)
        assert _same(moved, tuple(t[order] for t in one))
        for keep in (np.array([n - 2, 3]), np.array([5])):                     # alone
            Pk, Ek = _dev_lists(m, "overlap", dev, sel=keep)
            assert _same(run(dev, Mx, My, Pk, Ek, rows=keep), tuple(t[keep] for t in one))
    # the factor mode in calls of five rows, each with a slab of its own, against one call
    parts = []
    for r0 in range(0, n, 5):
        sel = np.arange(r0, min(n, r0 + 5))
        Pk, Ek = _dev_lists(m, "overlap", dev, sel=sel)
        parts.append(run(dev, (A, B), (Ay, By), Pk, Ek, rows=sel))
    whole = run(dev, (A, B), (Ay, By), P, E)
    assert _same(tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), whole)
    # strided dense views
    wideX, wideY = torch.full((n, m + 5), 7.0, device=dev), torch.full((n, m + 9), -7.0, device=dev)
    wideX[:, 2:2 + m], wideY[:, 6:6 + m] = X, Y
    vx, vy = wideX[:, 2:2 + m], wideY[:, 6:6 + m]
    assert vx.stride(0) == m + 5 and not vx.is_contiguous()
    assert _same(run(dev, vx, vy, P, E), run(dev, X, Y, P, E))
    # ldq, ldd > m through the C entry: the same bits, and the padding columns are left alone
    from mfcd import _lib
    L = _lib.load()
    ldq, ldd = m + 7, m + 3
    wideQ, wideD = torch.full((n, ldq), -123.0, device=dev), torch.full((n, ldd), -321.0, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(L.mfcd_implicit_hvp_rows_workspace_bytes(n, m, 0), dtype=torch.uint8, device=dev)
    _lib.check(L.mfcd_implicit_hvp_rows(vx.data_ptr(), vx.stride(0), vy.data_ptr(), vy.stride(0), None, None, None, None, 0,
                                        None, n, n, m, P[0].data_ptr(), P[1].data_ptr(), P[1].numel(), E[0].data_ptr(),
                                        E[1].data_ptr(), E[1].numel(), None, wideQ.data_ptr(), ldq, wideD.data_ptr(), ldd,
                                        status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    ref = run(dev, X, Y, P, E)
    hq, hd = wideQ.cpu().numpy(), wideD.cpu().numpy()
    assert np.ascontiguousarray(hq[:, :m]).tobytes() == ref[0].tobytes() and (hq[:, m:] == -123.0).all()
    assert np.ascontiguousarray(hd[:, :m]).tobytes() == ref[1].tobytes() and (hd[:, m:] == -321.0).all()


def test_coefficients_scale_the_rows(dev):
    C, _ = _CT()
    m = C + 1
    rng = np.random.default_rng(3)
    S, (Y, _) = _scores(m), _dirs(m)
    n = S.shape[0]
    ids = np.concatenate((rng.permutation(n), [2, 2, n - 1, 0]))
    coef = rng.uniform(0.5, 2.0, ids.size).astype(np.float32)
    pos, excl = _lists(m, "overlap")
    (po, pi), (eo, ei) = RM.csr([pos[k] for k in ids]), RM.csr([excl[k] for k in ids])
    q, deg, mag = HM.hvp_rows(S, Y, po, pi, eo, ei, row_ids=ids, coef=coef)
    k = np.stack([HM.partners(m, pos[u], excl[u]) for u in ids])
    P, E = _dev_lists(m, "overlap", dev, sel=ids)
    Q, D, _ = run(dev, to(dev, S), to(dev, Y), P, E, rows=ids, coef=to(dev, coef))
    check(Q, D, (q, deg, mag, k), Y[ids], "rows + coef", coef=coef)
    # a zero is +0 whatever the coefficient's sign: a constant direction, rows without a pair, barred columns
    flat = np.full_like(Y, 0.3)
    Qn, Dn, _ = run(dev, to(dev, S), to(dev, flat), P, E, rows=ids, coef=to(dev, -coef))
    assert Qn.tobytes() == np.zeros_like(Qn).tobytes() and Dn[deg == 0].tobytes() == np.zeros_like(Dn[deg == 0]).tobytes()
    assert (Dn <= 0).all() and (Dn < 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. invalid input
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_rows_get_status_2_and_nothing_else_changes(dev):
    m, n = 70, 6
    rng = np.random.default_rng(12)
    X, Y = (to(dev, rng.uniform(-3, 3, (n, m)).astype(np.float32)) for _ in range(2))
    pos = [np.sort(rng.choice(m, 7, replace=False)) for _ in range(8)]
    exc = [np.sort(rng.choice(m, 5, replace=False)) for _ in range(8)]
    pos[1][3] = m                                       # an item >= m
    pos[2][[2, 3]] = pos[2][[3, 2]]                     # not ascending
    exc[4][[0, 1]] = exc[4][[1, 0]]                     # a barred list that is not ascending
    exc[5][4] = -1                                      # a negative barred item
    pos[6][1] = pos[6][0]                               # a repeat: not strictly ascending
    ids = np.array([0, 1, 2, n + 3, 4, 5, 1, -1])       # rows 3 and 7: a row id outside [0, n)
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(exc)
    Q, D, status = run(dev, X, Y, (to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)), rows=ids)
    assert status.tolist() == [0, 2, 2, 2, 2, 2, 2, 2]
    assert np.isnan(Q[1:]).all() and np.isnan(D[1:]).all() and np.isfinite(Q[0]).all() and np.isfinite(D[0]).all()
    alone = run(dev, X, Y, (to(dev, po[:2]), to(dev, pi[:7])), (to(dev, eo[:2]), to(dev, ei[:5])), rows=ids[:1])
    assert _same(tuple(t[:1] for t in (Q, D, status)), alone)
    # without deg, and in factor mode: the same statuses and fills
    Q2, _, st2 = run(dev, X, Y, (to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)), rows=ids, deg=False)
    assert st2.tolist() == status.tolist() and np.isnan(Q2[1:]).all() and Q2[0].tobytes() == Q[0].tobytes()
    A, B = to(dev, rng.standard_normal((n, 3)).astype(np.float32)), to(dev, rng.standard_normal((m, 3)).astype(np.float32))
    Qf, Df, stf = run(dev, (A, B), (B.new_ones(n, 3), B), (to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)), rows=ids)
    assert stf.tolist() == status.tolist() and np.isnan(Qf[1:]).all() and np.isnan(Df[1:]).all() and np.isfinite(Qf[0]).all()


def test_non_finite_scores_and_directions_give_nan_rows(dev):
    m, n = 2 * _CT()[0] + 3, 8
    rng = np.random.default_rng(13)
    S, Y = (rng.uniform(-3, 3, (n, m)).astype(np.float32) for _ in range(2))
    pos = [np.sort(rng.choice(m, 40, replace=False)) for _ in range(n)]
    exc = [np.sort(rng.choice(m, 30, replace=False)) for _ in range(n)]
    free = [np.setdiff1d(np.arange(m), np.union1d(p, e)) for p, e in zip(pos, exc)]
    (po, pi), (eo, ei) = RM.csr(pos), RM.csr(exc)
    lists = ((to(dev, po), to(dev, pi)), (to(dev, eo), to(dev, ei)))
    clean = run(dev, to(dev, S), to(dev, Y), *lists)
    assert all(np.isfinite(t).all() for t in clean)
    S[0, free[0][-1]] = np.nan                          # at a negative of the last chunk
    S[1, np.setdiff1d(pos[1], exc[1])[0]] = np.inf      # at a positive: w = 0 would swallow it
    S[2, free[2][5]] = -np.inf
    Y[3, free[3][-2]] = np.inf                          # the direction, at a negative
    Y[4, np.setdiff1d(pos[4], exc[4])[-1]] = np.nan     # the direction, at a positive
    S[5, exc[5]] = np.nan                               # only at barred columns: an ordinary row
    Y[5, exc[5][::2]] = np.inf
    Y[6, exc[6]] = np.nan
    bad = [0, 1, 2, 3, 4]
    for deg in (True, False):
        got = run(dev, to(dev, S), to(dev, Y), *lists, deg=deg)
        assert got[2].tolist() == [0] * n
        for t, c in zip(got[:2 if deg else 1], clean):
            assert np.isnan(t[bad]).all()
            assert t[[5, 6, 7]].tobytes() == c[[5, 6, 7]].tobytes()            # the neighbours, and what is barred is ignored


# ---------------------------------------------------------------------------------------------------------------------
# 4. implicit_hvp against the model
# ---------------------------------------------------------------------------------------------------------------------
def _table(m, n, rng):
    pos = [np.sort(rng.choice(m, int(rng.integers(1, m // 2)), replace=False)) for _ in range(n)]
    pos[1], pos[2] = np.zeros(0, dtype=np.int64), np.arange(m)
    exc = [np.sort(rng.choice(m, int(rng.integers(0, m // 4)), replace=False)) for _ in range(n)]
    return pos, exc


def _data(lists, n, m, dev):
    from mfcd.ratings import RatingsData
    u = np.concatenate([np.full(len(x), k) for k, x in enumerate(lists)])
    return RatingsData(u, np.concatenate(lists), np.ones(u.size), n, m).to(dev)


def tables_bound(prob, U, V, dU, dV, gauss_newton):
    """The elementwise bounds (bU, bV) on the device's (HU, HV).  The kernel runs on the two parts of the direction, Y1 =
    dU V^T and Y2 = U dV^T, so q's bound is the sum of theirs: per user and column (2e-5 + slack) mag_c + 2e-6 c_u k_c
    max |y|, carried through the f64 GEMMs with |V| (mirror: |U|).  The exact form adds the gradient's own bound times
    |dV| (|dU|): (2e-5 + slack) |g_c| + 2e-6 c_u k_c.  slack: the device's fp32 scores and directions lie within
    (d + 1) 2^-24 sum_k |u_k v_k| of the model's f64 ones, which moves a weight, relatively, and a sigmoid by at most
    twice that, and a direction's difference by twice its own rounding (that goes with max |y|)."""
    n, m, d = U.shape[0], V.shape[0], U.shape[1]
    eps = (d + 1) * 2.0 ** -24
    A = U @ V.T
    parts = (dU @ V.T, U @ dV.T)
    absY = (np.abs(dU) @ np.abs(V).T, np.abs(U) @ np.abs(dV).T)
    slack = 2 * eps * (np.abs(U) @ np.abs(V).T).max()
    K = np.stack([HM.partners(m, p, e) * (np.diag(HM.laplacian(A[u], p, e)) > 0) for u, (p, e) in enumerate(zip(prob.pos, prob.excl))])
    cK = prob.c[:, None] * K
    bq = np.zeros((n, m))
    for Y, aY in zip(parts, absY):
        rows = [HM.hvp_row(A[u], Y[u], prob.pos[u], prob.excl[u], prob.c[u]) for u in range(n)]
        mag, deg = np.stack([r[2] for r in rows]), np.stack([r[1] for r in rows])
        ymax = np.abs(Y).max(1, keepdims=True)
        bq += (RTOL + slack) * mag + ATOL * cK * ymax + 2 * eps * aY.max(1, keepdims=True) * deg + 2.0 ** -24 * mag
    bU, bV = bq @ np.abs(V), bq.T @ np.abs(U)
    if not gauss_newton:
        G = prob.score_grads(U, V)
        bg = (RTOL + slack + 2.0 ** -24) * np.abs(G) + ATOL * cK
        bU, bV = bU + bg @ np.abs(dV), bV + bg.T @ np.abs(dU)
    return bU, bV


@pytest.mark.parametrize("normalize", ["pairs", "user"])
def test_implicit_hvp_matches_the_model_and_is_symmetric(dev, normalize):
    import structure as S
    from mfcd import _lib, implicit
    n, m, d = 12, 40, 3
    rng = np.random.default_rng(41)
    pos, exc = _table(m, n, rng)
    data, excl = _data(pos, n, m, dev), _data(exc, n, m, dev)
    prob = HM.Problem(m, pos, exc, normalize)
    torch.manual_seed(41)
    model = S.MatrixFactorization(n, m, d).to(dev)
    U, V = (t.detach().cpu().numpy().astype(np.float64) for t in (model.U, model.V))
    dU, dV, eU, eV = (rng.standard_normal(s).astype(np.float32) for s in ((n, d), (m, d), (n, d), (m, d)))
    for gn in (False, True):
        got = {}
        for name, (a, b) in (("d", (dU, dV)), ("e", (eU, eV))):
            HU, HV = S.implicit_hvp(model, data, to(dev, a), to(dev, b), excl, normalize, gauss_newton=gn)
            assert HU.dtype == torch.float64 and tuple(HU.shape) == (n, d) and tuple(HV.shape) == (m, d)
            wU, wV, _ = prob.hvp(U, V, a.astype(np.float64), b.astype(np.float64), gn)
            bU, bV = tables_bound(prob, U, V, a.astype(np.float64), b.astype(np.float64), gn)
            for what, g, w, bound in (("HU", HU, wU, bU), ("HV", HV, wV, bV)):
                err = np.abs(g.cpu().numpy() - w)
                live = bound > 0
                print(f"{normalize} gauss_newton={gn} {name}: {what} max |entry| {np.abs(w).max():.3e}, max error / bound "
                      f"{(err[live] / bound[live]).max():.3f}")
                assert (err <= bound).all(), (what, gn)
            got[name] = (HU.cpu().numpy(), HV.cpu().numpy(), bU, bV)
            assert (got[name][0][[1, 2]] == 0).all()                           # users without a pair
        # <e, H d> = <d, H e> within the bounds of the two products
        lhs = (eU * got["d"][0]).sum() + (eV * got["d"][1]).sum()
        rhs = (dU * got["e"][0]).sum() + (dV * got["e"][1]).sum()
        room = (np.abs(eU) * got["d"][2]).sum() + (np.abs(eV) * got["d"][3]).sum() + \
            (np.abs(dU) * got["e"][2]).sum() + (np.abs(dV) * got["e"][3]).sum()
        print(f"{normalize} gauss_newton={gn}: <e, H d> {lhs:.6e}, <d, H e> {rhs:.6e}, room {room:.2e}")
        assert abs(lhs - rhs) <= room
    # row blocks: three blocks against one, to the bound (the GEMMs' shapes differ)
    one = implicit.implicit_hvp(model.U.data, model.V.data, to(dev, dU), to(dev, dV), data, excl, normalize)
    three = implicit.implicit_hvp(model.U.data, model.V.data, to(dev, dU), to(dev, dV), data, excl, normalize, row_block=5)
    bU, bV = tables_bound(prob, U, V, dU.astype(np.float64), dV.astype(np.float64), False)
    assert ((one[0] - three[0]).abs().cpu().numpy() <= 2 * bU).all() and ((one[1] - three[1]).abs().cpu().numpy() <= 2 * bV).all()
    bf = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        S.implicit_hvp(bf, data, to(dev, dU), to(dev, dV))
    with pytest.raises(ValueError):
        S.implicit_hvp(model, data, to(dev, dU)[:-1], to(dev, dV))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the exact steps
# ---------------------------------------------------------------------------------------------------------------------
def _step_data(m, dev, users=None):
    Ustar, V, pos = HM.step_inputs(m)
    if users is not None:
        pos = [pos[u] for u in users]
    off, items = HM.lists(pos)
    return Ustar, V, (to(dev, off), to(dev, items))


@pytest.mark.parametrize("m", [40, 2048 + 5])
def test_user_step_reaches_the_models_minimiser(dev, m):
    from mfcd import implicit, implicit_exact
    assert m in (40, implicit.CHUNK + 5)
    Ustar, V, data = _step_data(m, dev)
    prob, Uopt, noise = HM.user_minimisers(m)
    paired = prob.paired
    U0, Vd = torch.zeros(8, 3, device=dev), to(dev, V)
    res = implicit_exact.implicit_user_step(U0, Vd, data, L2)
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert res.rows.dtype == torch.float32 and res.status.tolist() == [0] * 8
    V64 = V.astype(np.float64)
    gnorm = np.array([np.linalg.norm(prob.user_grad(rows[r], V64, r, L2)) for r in range(8)])
    # the noise is evaluated at the model's minimiser; the CPU test holds it below the certificate's own term
    bound = GTOL * L2 * np.abs(rows).max(axis=1) + noise
    dist = np.linalg.norm(rows - Uopt, axis=1)
    print(f"m={m}: Newton {res.newton_iters.tolist()}, CG {res.cg_iters.tolist()}, |grad| / bound "
          f"{np.round(gnorm[paired] / bound[paired], 3).tolist()}, |u - u*| / (bound / l2) "
          f"{np.round(dist[paired] / (bound[paired] / L2), 3).tolist()}, grad_ratio "
          f"{np.round(res.grad_ratio.cpu().numpy(), 5).tolist()}")
    assert (gnorm <= bound).all()
    assert (dist <= bound / L2).all()                            # strong convexity, modulus l2
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all() and (res.grad_ratio.cpu().numpy() <= GTOL).all()
    f_model = np.array([prob.user_objective(rows[r], V64, r, L2) for r in range(8)])
    np.testing.assert_allclose(after, f_model, rtol=RTOL, atol=ATOL)
    # the two users without a pair: exactly +0, no iteration
    assert res.rows[[1, 2]].cpu().numpy().tobytes() == np.zeros((2, 3), dtype=np.float32).tobytes()
    assert res.newton_iters[[1, 2]].tolist() == [0, 0] == res.cg_iters[[1, 2]].tolist() and (after[[1, 2]] == 0).all()
    assert (res.newton_iters.cpu().numpy()[paired] > 0).all()
    # started elsewhere, such a user still returns the zero row and reports what its start cost
    U1 = torch.full((8, 3), 0.25, device=dev)
    moved = implicit_exact.implicit_user_step(U1, Vd, data, L2)
    assert moved.rows[[1, 2]].cpu().numpy().tobytes() == np.zeros((2, 3), dtype=np.float32).tobytes()
    np.testing.assert_allclose(moved.objective_before[[1, 2]].cpu().numpy(), 0.5 * L2 * 3 * 0.25 ** 2, rtol=1e-12)
    assert moved.status.tolist() == [0] * 8
    np.testing.assert_allclose(moved.rows.cpu().numpy(), rows, rtol=0, atol=2 * (bound / L2).max())
    # the fold-in: users who were not in training, from their lists alone, under the training table's normaliser
    c = float(prob.c[0])
    full = implicit_exact.implicit_user_step(None, Vd, data, L2, coef=c)
    assert full.rows.cpu().numpy().tobytes() == res.rows.cpu().numpy().tobytes()         # the same problem as above
    some = [3, 5, 7, 1]
    fold = implicit_exact.implicit_user_step(None, Vd, _step_data(m, dev, some)[2], L2, coef=c)
    assert fold.rows.cpu().numpy().tobytes() == full.rows[some].cpu().numpy().tobytes()
    assert fold.status.tolist() == [0] * 4 and fold.newton_iters.tolist() == full.newton_iters[some].tolist()
    import structure as S
    again = S.fit_users_implicit(Vd, _data(HM.step_inputs(m)[2], 8, m, dev), L2, coef=c)
    assert torch.equal(again.rows, full.rows)
    # a user with a NaN score: status 2, a NaN row; its neighbours as without it
    Ubad = U0.clone()
    Ubad[3, 1] = float("nan")
    bad = implicit_exact.implicit_user_step(Ubad, Vd, data, L2)
    others = [0, 1, 2, 4, 5, 6, 7]
    assert bad.status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and bool(torch.isnan(bad.rows[3]).all())
    assert bad.rows[others].cpu().numpy().tobytes() == res.rows[others].cpu().numpy().tobytes()
    assert bad.newton_iters[others].tolist() == res.newton_iters[others].tolist()
    assert torch.equal(bad.objective_after[others], res.objective_after[others])


def test_item_step_reaches_the_models_minimiser(dev):
    from mfcd import implicit_exact
    m = 40
    Ustar, V, data = _step_data(m, dev)
    prob, Vopt, noise = HM.item_minimiser(m)
    res = implicit_exact.implicit_item_step(to(dev, Ustar), torch.zeros(m, 3, device=dev), data, L2)
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert int(res.status) == 0 and res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (m, 3)
    U64 = Ustar.astype(np.float64)
    gnorm = np.linalg.norm(prob.item_grad(U64, rows, L2))
    bound = GTOL * L2 * np.abs(rows).max() + noise
    dist = np.linalg.norm(rows - Vopt)
    print(f"m={m}: Newton {int(res.newton_iters)}, CG {int(res.cg_iters)}, |grad| {gnorm:.3e}, bound {bound:.3e} "
          f"(noise {noise:.3e}), |V - V*| {dist:.3e} against {bound / L2:.3e}, grad_ratio {float(res.grad_ratio):.2e}")
    assert gnorm <= bound and dist <= bound / L2
    assert float(res.objective_after) <= float(res.objective_before) and float(res.grad_ratio) <= GTOL
    np.testing.assert_allclose(float(res.objective_after), prob.item_objective(U64, rows, L2), rtol=RTOL, atol=ATOL)
    Ubad = to(dev, Ustar)
    Ubad[4, 0] = float("inf")
    V0 = to(dev, V)
    bad = implicit_exact.implicit_item_step(Ubad, V0, data, L2)
    assert int(bad.status) == 2 and torch.equal(bad.rows, V0)


def test_alternating_fit_descends_and_records_the_models_objective(dev):
    import structure as S
    from mfcd import _lib, implicit_exact
    m = 40
    Ustar, V, data = _step_data(m, dev)
    _, _, pos = HM.step_inputs(m)
    prob = HM.Problem(m, pos)
    rng = np.random.default_rng(8)
    U0 = (0.3 * rng.standard_normal((8, 3))).astype(np.float32)
    V0 = (0.3 * rng.standard_normal((m, 3))).astype(np.float32)
    seen, tables = [], (to(dev, U0), to(dev, V0))
    for sweep in range(3):                                       # one sweep at a time: the tables of every sub-step
        U_before = tables[0].clone()
        res = implicit_exact.fit_implicit_exact(*tables, data, L2, 1)
        assert res.U is tables[0] and res.V is tables[1]
        Un, Vn = (t.cpu().numpy().astype(np.float64) for t in tables)
        if sweep == 0:
            start = prob.objective(U0.astype(np.float64), V0.astype(np.float64), L2)
            np.testing.assert_allclose(float(res.objective_start), start, rtol=RTOL, atol=ATOL)
            seen.append(float(res.objective_start))
        # after the user step: the new U with the V the sweep started from
        seen += res.history[0].tolist()
        np.testing.assert_allclose(res.history[0, 1].item(), prob.objective(Un, Vn, L2), rtol=RTOL, atol=ATOL)
        assert not torch.equal(U_before, tables[0])
        assert (tables[0][[1, 2]] == 0).all()                    # the users without a pair
    rated = _data(pos, 8, m, dev)
    model = S.MatrixFactorization(8, m, 3).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, U0))
        model.V.copy_(to(dev, V0))
    hist = S.train_model_implicit_exact(model, rated, L2, sweeps=3)
    flat = [f for pair in hist for f in pair]
    print(f"F: start {seen[0]:.7f}, sub-steps {np.round(flat, 7).tolist()}")
    assert len(hist) == 3 and all(len(pair) == 2 for pair in hist)
    assert all(b <= a for a, b in zip([seen[0]] + flat[:-1], flat))             # non-increasing
    assert flat == seen[1:]                                      # k sweeps are k chained calls of one sweep: the same calls
    assert torch.equal(model.U.data, tables[0]) and torch.equal(model.V.data, tables[1])
    # the user-step value of every sweep against the model, at the tables of that sub-step: replay with the steps
    U, Vt = to(dev, U0), to(dev, V0)
    for sweep in range(3):
        U = implicit_exact.implicit_user_step(U, Vt, data, L2).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(hist[sweep][0], want, rtol=RTOL, atol=ATOL)
        Vt = implicit_exact.implicit_item_step(U, Vt, data, L2).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(hist[sweep][1], want, rtol=RTOL, atol=ATOL)
    # what a trained table had left: the gains of the two refits are the steps' decreases
    result, gain = S.refit_users_implicit(model, rated, L2)
    assert tuple(gain.shape) == (8,) and bool((gain >= 0).all()) and result.status.tolist() == [0] * 8
    result, gain = S.refit_items_implicit(model, rated, L2)
    assert gain.dim() == 0 and float(gain) >= 0 and int(result.status) == 0
    bf = S.MatrixFactorization(8, m, 3, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        S.train_model_implicit_exact(bf, rated, L2, sweeps=1)
