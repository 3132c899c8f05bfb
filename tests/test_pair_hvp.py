"""GPU tests of the pair Hessian-vector kernels and of what is built on them (include/mfcd.h: mfcd_pair_hvp_rows,
mfcd_pair_law_hvp_rows; mfcd/pairs.py: pair_hvp_rows, pair_law_hvp_rows, population_hvp; mfcd/population.py;
structure.train_model_population_exact) against the float64 model of tests/pair_hvp_model.py.

Shapes: test_pair_grad.py's, m in {1, 2, 63, 64, 65, T-1, T, T+1, 2T+3} with T = pairs.TILE.  Score rows: the eight kinds
of its `case_rows`, each met by two of four kinds of direction rows: distinct values in [-2, 2], three levels (heavy
ties), a constant row (Q is exactly +0) and denormals.  The denormal directions are integers in [-3, 3] times 2^-130:
Q is an fp32 output, whose spacing below 2^-126 is 2^-149 whatever the value, so only a denormal row near the top of the
denormal range can be held to a relative bound; here a term is about 2^-132 = 2^17 spacings.

Tolerance, on the mean term q_i / (m - 1): 2e-5 times the mean magnitude of the terms, mean_j w_ij s_ij |y_i - y_j| from
the model, plus 2e-6 max |y| of the row: the project's fp32 pair tolerance, applied to the sum of magnitudes because the
sum itself can cancel.  deg_i / (m - 1) is held to 2e-5 mean_j w_ij s_ij + 2e-6 (deg is the sum of magnitudes for
differences of size 1).  A worst-case count of the kernel's roundings lies inside it.  Per term, relative to its
magnitude: the score difference (half an ulp) and its product with log2(e) (half an ulp of an argument below 8.7 for
differences below 6) move log s by at most 4 * 2^-24 and 3 * 2^-24; the hardware exp and the two uses of the reciprocal
one ulp each, 1 + e half an ulp twice, the two products of e h h, the difference of y, the weight's product and the fma
half an ulp each: under 13 * 2^-24 = 8e-7 in all (for the row of scores in {-60, 0, 60} the argument is 87 or 173 and
its rounding 2^-18: 3e-6, and s underflows below 2^-126, which the 2e-6 max |y| covers).  The fp32 runs of 64 terms add
at most 32 * 2^-24 = 1.9e-6 of the sum of magnitudes, the f64 sums and the store 2^-24.  Together under 3e-6 (6e-6 for
the wide row) of the mean magnitude, against 2e-5.  The references are computed once per module and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pair_hvp_model as HM
import pair_law_model as LM
from test_pair_grad import _distinct, _levels, case_rows
from test_pair_law import grid, law_parts, make_law, spec_of

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
GTOL, L2 = 1e-3, 3e-2


def _tile():
    from mfcd import pairs
    return pairs.TILE


def _ms():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


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
        return _levels(m, rng, (-1.0, 0.0, 0.5))
    if kind == 2:
        return np.full(m, 0.3, dtype=np.float32)
    return (rng.integers(-3, 4, m).astype(np.float64) * 2.0 ** -130).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hvp_rows(m):
    """(A, X, Y, kinds) float32 [16, m]: score kind a = r % 8 of case_rows, direction kind (a + a // 4 + 2 (r // 8)) % 4."""
    A8, X8 = case_rows(m)
    rng = np.random.default_rng(3000 + m)
    kinds = [(r % 8 + (r % 8) // 4 + 2 * (r // 8)) % 4 for r in range(16)]
    Y = np.stack([direction(k, m, rng) for k in kinds])
    assert set(kinds) == {0, 1, 2, 3} and (np.abs(Y[np.array(kinds) == 3]) < 2.0 ** -126).all()
    return np.tile(A8, (2, 1)), np.tile(X8, (2, 1)), Y, kinds


def row_weights(X, spec, r):
    if spec is None:
        return None
    lab = spec.get("labels")
    return LM.weights(X[r], spec.get("alpha"), spec.get("beta"), spec.get("margin"),
                      None if lab is None else lab[r] if np.ndim(lab) == 2 else lab)


def reference(A, X, Y, spec=None):
    """(q, deg, mag) [rows, m] of the model."""
    out = [HM.pair_hvp(A[r], Y[r], row_weights(X, spec, r), None if spec is None else X[r]) for r in range(len(A))]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


@functools.lru_cache(maxsize=None)
def plain_reference(m):
    A, X, Y, _ = hvp_rows(m)
    return reference(A, X, Y)


def run(dev, A, Y, X=None, law=None, deg=True):
    from mfcd import pairs
    if law is None:
        out = pairs.pair_hvp_rows(to(dev, A), to(dev, Y), deg)
    else:
        out = pairs.pair_law_hvp_rows(to(dev, A), to(dev, X), to(dev, Y), law, deg)
    out = out if deg else (out,)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == A.shape for t in out)
    return tuple(t.cpu().numpy() for t in out)


def check(got, want, Y, m, what):
    (Q, D), (q, deg, mag) = got, want
    if m == 1:
        assert Q.tobytes() == np.zeros_like(Q).tobytes() and D.tobytes() == np.zeros_like(D).tobytes(), what   # exactly +0
        return
    ymax = np.abs(Y.astype(np.float64)).max(axis=1, keepdims=True)
    bound_q = RTOL * mag / (m - 1) + ATOL * ymax
    bound_d = RTOL * deg / (m - 1) + ATOL
    err_q = np.abs(Q.astype(np.float64) - q) / (m - 1)
    err_d = np.abs(D.astype(np.float64) - deg) / (m - 1)
    live = bound_q > 0
    print(f"{what}: q max error / bound {(err_q[live] / bound_q[live]).max() if live.any() else 0.0:.3f}, "
          f"deg max error / bound {(err_d / bound_d).max():.3f}, largest mean term {np.abs(q).max() / (m - 1):.3e}")
    assert (err_q <= bound_q).all(), what
    assert (err_d <= bound_d).all(), what
    # every pair enters twice with opposite signs: a row of Q sums to 0 within the bound on its entries
    assert (np.abs(Q.astype(np.float64).sum(axis=1)) / (m - 1) <= bound_q.sum(axis=1)).all(), what
    dead = deg == 0                                                # no pair of the column has weight: exactly +0
    assert Q[dead].tobytes() == np.zeros_like(Q[dead]).tobytes() and D[dead].tobytes() == np.zeros_like(D[dead]).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", _ms())
def test_kernel_matches_the_f64_model(dev, m):
    A, X, Y, kinds = hvp_rows(m)
    Q, D = run(dev, A, Y)
    assert np.isfinite(Q).all() and np.isfinite(D).all()
    check((Q, D), plain_reference(m), Y, m, f"m={m}")
    const = np.array(kinds) == 2
    assert Q[const].tobytes() == np.zeros_like(Q[const]).tobytes()             # a constant direction: exactly +0
    if m > 1:
        tiny = np.array(kinds) == 3
        assert (np.abs(Q[tiny]) <= (m - 1) * 0.25 * 6.0 * 2.0 ** -130).all()         # m - 1 terms of at most s |dy|
        assert (Q[tiny] != 0).any() or not (plain_reference(m)[0][tiny] != 0).any()   # denormal directions are not flushed


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism and edge cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [65, 2 * 1024 + 3])
def test_two_calls_rows_alone_strided_views_and_deg_or_not_are_bit_equal(dev, m):
    from mfcd import _lib, pairs
    assert m in _ms()
    A, X, Y, _ = hvp_rows(m)
    rows = A.shape[0]
    Q, D = run(dev, A, Y)
    again = run(dev, A, Y)
    assert again[0].tobytes() == Q.tobytes() and again[1].tobytes() == D.tobytes()
    assert run(dev, A, Y, deg=False)[0].tobytes() == Q.tobytes()               # deg = NULL: the same Q
    for r in range(rows):                                                      # a row does not depend on its neighbours
        one = run(dev, A[r:r + 1], Y[r:r + 1])
        assert one[0].tobytes() == Q[r:r + 1].tobytes() and one[1].tobytes() == D[r:r + 1].tobytes(), r
    wideA = torch.full((rows, m + 5), 7.0, device=dev)
    wideY = torch.full((rows, m + 9), -7.0, device=dev)
    wideA[:, 2:2 + m], wideY[:, 6:6 + m] = to(dev, A), to(dev, Y)
    va, vy = wideA[:, 2:2 + m], wideY[:, 6:6 + m]
    assert va.stride(0) == m + 5 and not va.is_contiguous()
    sq, sd = pairs.pair_hvp_rows(va, vy, True)
    assert sq.cpu().numpy().tobytes() == Q.tobytes() and sd.cpu().numpy().tobytes() == D.tobytes()
    # ldq, ldd > m through the C entry: the same bits, and the padding columns are left alone
    ldq, ldd = m + 7, m + 3
    wideQ, wideD = torch.full((rows, ldq), -123.0, device=dev), torch.full((rows, ldd), -321.0, device=dev)
    _lib.check(_lib.load().mfcd_pair_hvp_rows(va.data_ptr(), va.stride(0), vy.data_ptr(), vy.stride(0), rows, m,
                                              wideQ.data_ptr(), ldq, wideD.data_ptr(), ldd, _lib.stream_ptr(dev)))
    hq, hd = wideQ.cpu().numpy(), wideD.cpu().numpy()
    assert np.ascontiguousarray(hq[:, :m]).tobytes() == Q.tobytes() and (hq[:, m:] == -123.0).all()
    assert np.ascontiguousarray(hd[:, :m]).tobytes() == D.tobytes() and (hd[:, m:] == -321.0).all()
    empty = pairs.pair_hvp_rows(to(dev, A)[:0], to(dev, Y)[:0], True)
    assert all(tuple(t.shape) == (0, m) and t.dtype == torch.float32 for t in empty)
    with pytest.raises(Exception):
        pairs.pair_hvp_rows(to(dev, A), to(dev, Y)[:, :-1])


def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(dev):
    T = _tile()
    m = T + 37
    rng = np.random.default_rng(5)
    A = np.stack([_distinct(m, rng) for _ in range(8)])
    Y = np.stack([_distinct(m, rng) for _ in range(8)])
    X = np.stack([_levels(m, rng, (-1.0, 0.5, 2.0, 3.0)) for _ in range(8)])
    law = make_law(dev, dict(labels=rng.integers(0, 3, m)))                    # no margin: x is read for finiteness only
    clean, clean_law = run(dev, A, Y), run(dev, A, Y, X, law)
    assert all(np.isfinite(t).all() for t in clean + clean_law)
    A[1, 3] = np.inf                                           # first tile: the second tile's workgroup must see it
    A[3, T + 30] = np.nan                                      # second tile: the first tile's workgroup must see it
    Y[4, 2] = -np.inf
    Y[5, m - 1] = np.nan                                       # the last column
    for got, base in ((run(dev, A, Y), clean), (run(dev, A, Y, X, law), clean_law)):
        for t, c in zip(got, base):
            assert np.isnan(t[[1, 3, 4, 5]]).all()
            assert t[[0, 2, 6, 7]].tobytes() == c[[0, 2, 6, 7]].tobytes()
    X[6, 5] = np.nan
    X[7, T + 1] = np.inf
    got = run(dev, A, Y, X, law)
    for t, c in zip(got, clean_law):
        assert np.isnan(t[[1, 3, 4, 5, 6, 7]]).all() and t[[0, 2]].tobytes() == c[[0, 2]].tobytes()
    q, deg, mag = reference(A[[0, 2]], X[[0, 2]], Y[[0, 2]], spec_of(law))
    check((got[0][[0, 2]], got[1][[0, 2]]), (q, deg, mag), Y[[0, 2]], m, "neighbours of bad rows")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the law twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [65, 1024 + 1, 2 * 1024 + 3])
@pytest.mark.parametrize("kind", ["weights", "margin_half", "shared_labels", "row_labels", "all"])
def test_law_kernel_matches_the_f64_model(dev, kind, m):
    assert m in _ms()
    A, X, Y, _ = hvp_rows(m)
    kw, on_grid = law_parts(kind, m, 16)
    kw = dict(kw)
    X = grid(X) if on_grid else X.copy()
    if "alpha" in kw:                                           # a column whose every weight is 0
        kw["alpha"], kw["beta"] = kw["alpha"].copy(), kw["beta"].copy()
        kw["alpha"][5] = kw["beta"][5] = 0.0
    elif "margin" in kw:
        X[:, 5] = 50.0                                          # farther than the margin from every other x
    law = make_law(dev, kw, slice(0, 16))
    spec = spec_of(law)
    Q, D = run(dev, A, Y, X, law)
    assert np.isfinite(Q).all() and np.isfinite(D).all()
    want = reference(A, X, Y, spec)
    if "alpha" in kw or "margin" in kw:
        assert (want[1][:, 5] == 0).all() and (want[1] > 0).any()
    check((Q, D), want, Y, m, f"{kind} m={m}")
    assert run(dev, A, Y, X, law, deg=False)[0].tobytes() == Q.tobytes()
    assert run(dev, A, Y, X, law)[0].tobytes() == Q.tobytes()


@pytest.mark.parametrize("m", [65, 1024 + 1])
def test_a_law_of_ones_is_the_plain_entry(dev, m):
    from mfcd import pairs
    A, X, Y, _ = hvp_rows(m)
    plain = run(dev, A, Y)
    from mfcd import _lib
    Ad, Xd, Yd = to(dev, A), to(dev, X), to(dev, Y)
    alpha, beta = torch.ones(m, device=dev), torch.full((m,), 0.5, device=dev)  # w = 1/2 + 1/2 (PairLaw would rescale beta)
    c = _lib.PairLawC()
    c.alpha, c.beta = alpha.data_ptr(), beta.data_ptr()
    Qd, Dd = torch.empty_like(Ad), torch.empty_like(Ad)
    _lib.check(_lib.load().mfcd_pair_law_hvp_rows(Ad.data_ptr(), m, Xd.data_ptr(), m, Yd.data_ptr(), m, A.shape[0], m,
                                                  ctypes.byref(c), Qd.data_ptr(), m, Dd.data_ptr(), m, _lib.stream_ptr(dev)))
    ones = (Qd.cpu().numpy(), Dd.cpu().numpy())
    check(ones, plain_reference(m), Y, m, f"law of ones m={m}")
    err = np.abs(ones[0].astype(np.float64) - plain[0]) / (m - 1)
    assert (err <= 2 * (RTOL * plain_reference(m)[2] / (m - 1) + ATOL * np.abs(Y).max(axis=1, keepdims=True))).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. population_hvp against the model
# ---------------------------------------------------------------------------------------------------------------------
def check_tables_hvp(got, prob, U, V, dU, dV, gauss_newton, what, slack=0.0):
    """(HU, HV) against the model's, elementwise.  Q's bound carried through the products as test_pair_grad.check_tables
    carries G's: per user row, with mag the sums of magnitudes of L Y and ymax the row's largest |y|,
      c [(2e-5 + m 2^-24) (mag @ |V|) + 2e-6 (m - 1) ymax sum_i |V_i|]
    plus, for the exact product, G's own term  c [(2e-5 + m 2^-24) (|G| @ |dV|) + 2e-6 (m - 1) sum_i |dV_i|];  the mirror
    image for V (inner dimension k, the rows of U and dU of the chosen users).  `slack` (relative to the sums of
    magnitudes) covers the rounding of Y's own two GEMMs and, under a law, of the fp32 weights in 1 / W."""
    U, V, dU, dV = (np.asarray(t, dtype=np.float64) for t in (U, V, dU, dV))
    HU, HV, (mag, ymax, G) = prob.hvp(U, V, dU, dV, gauss_newton)
    m, k, c, ids = prob.m, len(prob.ids), prob.c, prob.ids
    r1, r2 = RTOL + slack + m * 2.0 ** -24, RTOL + slack + k * 2.0 ** -24
    rowsU = r1 * (mag @ np.abs(V)) + ATOL * (m - 1) * ymax[:, None] * np.abs(V).sum(0)
    bV = r2 * (mag.T @ np.abs(U[ids])) + ATOL * (m - 1) * (ymax[:, None] * np.abs(U[ids])).sum(0)
    if not gauss_newton:
        rowsU = rowsU + r1 * (np.abs(G) @ np.abs(dV)) + ATOL * (m - 1) * np.abs(dV).sum(0)
        bV = bV + r2 * (np.abs(G).T @ np.abs(dU[ids])) + ATOL * (m - 1) * np.abs(dU[ids]).sum(0)
    bU = np.zeros_like(U)
    np.add.at(bU, ids, c * rowsU)
    for name, g, want, bound in (("HU", got[0], HU, bU), ("HV", got[1], HV, c * bV)):
        assert g.dtype == torch.float32 and tuple(g.shape) == want.shape
        err = np.abs(g.cpu().numpy().astype(np.float64) - want)
        live = bound > 0
        print(f"{what}: {name} max |entry| {np.abs(want).max():.3e}, max error / bound {(err[live] / bound[live]).max():.3f}")
        assert (err <= bound).all(), (what, name)


@pytest.mark.parametrize("shape", ["n12_m40_d3", "n5_mT5_d2"])
def test_population_hvp_matches_the_model(dev, shape):
    import generation_data as gd
    import structure as S
    from mfcd import pairs
    n, m, d = (12, 40, 3) if shape == "n12_m40_d3" else (5, _tile() + 5, 2)
    g = torch.Generator().manual_seed(41)
    F = gd.FactoredMatrix(torch.randn(n, 2, generator=g), torch.randn(m, 2, generator=g))
    Xd = F.dense(dev)
    Xh = Xd.cpu().numpy()
    torch.manual_seed(41)
    model = S.MatrixFactorization(n, m, d).to(dev)
    dU, dV = torch.randn(n, d, generator=g).to(dev), torch.randn(m, d, generator=g).to(dev)
    host = [t.detach().cpu().numpy() for t in (model.U, model.V, dU, dV)]
    s = 0.7
    users = [n - 1, 0, 2, n - 1, 1]
    y_slack = 2 * d * 2.0 ** -24                                # Y = dU V^T + U dV^T: 2 d products per entry
    for what, X, kw in (("dense", Xd, {}), ("factored", F, {}), ("ragged blocks", Xd, {"row_block": 5}),
                        ("users with a repeat", Xd, {"users": users, "row_block": 2})):
        prob = HM.Problem(Xh, s, None, kw.get("users"))
        for gn in (False, True):
            got = S.population_hvp(model, X, dU, dV, s, gauss_newton=gn, **kw)
            check_tables_hvp(got, prob, *host, gn, f"{shape} {what} gauss_newton={gn}", y_slack)
    rng = np.random.default_rng(9)
    law = pairs.PairLaw(alpha=rng.uniform(0.2, 1.0, m), beta=rng.uniform(0.2, 1.0, m), labels=rng.integers(0, 3, (n, m)),
                        users=[0, 2, n - 1], device=dev)
    prob = HM.Problem(Xh, s, spec_of(law))
    for gn in (False, True):
        got = S.population_hvp(model, Xd, dU, dV, s, law, row_block=2, gauss_newton=gn)
        check_tables_hvp(got, prob, *host, gn, f"{shape} law gauss_newton={gn}", y_slack + 4 * 2.0 ** -24)
    assert got[0].cpu().numpy()[[1, 3]].tobytes() == np.zeros((2, d), dtype=np.float32).tobytes()   # users outside the law
    trivial = S.population_hvp(model, Xd, dU, dV, s, pairs.PairLaw(device=dev))
    base = S.population_hvp(model, Xd, dU, dV, s)
    assert all(torch.equal(a, b) for a, b in zip(trivial, base))               # a trivial law takes the plain path
    bf = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    from mfcd import _lib
    with pytest.raises(_lib.MfcdError):
        S.population_hvp(bf, Xd, dU, dV, s)
    with pytest.raises(ValueError):
        S.population_hvp(model, Xd, dU[:-1], dV, s)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the exact steps
# ---------------------------------------------------------------------------------------------------------------------
def _step_law(m, dev):
    from mfcd import pairs
    rng = np.random.default_rng(77)
    return pairs.PairLaw(alpha=rng.uniform(0.3, 1.0, m), beta=rng.uniform(0.3, 1.0, m), labels=rng.integers(0, 4, m),
                         device=dev)


@functools.lru_cache(maxsize=None)
def user_minimisers(m, with_law):
    """The model's minimiser of every user's row and the worst-case gradient noise there."""
    Ustar, V, X = HM.solver_inputs(m)
    spec = spec_of(_step_law(m, "cpu")) if with_law else None
    prob = HM.Problem(X, 1.0, spec)
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(3), V64, r, L2)[0] for r in range(8)])
    return prob, Uopt, prob.user_noise(Uopt, V64)


@pytest.mark.parametrize("with_law", [False, True], ids=["plain", "law"])
@pytest.mark.parametrize("m", [40, 1029])
def test_user_step_reaches_the_models_minimiser(dev, m, with_law):
    from mfcd import population
    Ustar, V, X = HM.solver_inputs(m)
    prob, Uopt, noise = user_minimisers(m, with_law)
    law = _step_law(m, dev) if with_law else None
    U0, Vd, Xd = torch.zeros(8, 3, device=dev), to(dev, V), to(dev, X)
    res = population.population_user_step(U0, Vd, Xd, 1.0, L2, law)
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert res.rows.dtype == torch.float32 and res.status.tolist() == [0] * 8
    V64 = V.astype(np.float64)
    gnorm = np.array([np.linalg.norm(prob.user_grad(rows[r], V64, r, L2)) for r in range(8)])
    # the noise is evaluated at the model's minimiser; the score gradients at the returned row differ from those by far
    # less than the room of 4 the CPU test establishes
    bound = GTOL * L2 * np.abs(rows).max(axis=1) + noise
    dist = np.linalg.norm(rows - Uopt, axis=1)
    print(f"m={m} law={with_law}: Newton {res.newton_iters.tolist()}, CG {res.cg_iters.tolist()}, "
          f"|grad| / bound {np.round(gnorm / bound, 3).tolist()}, |u - u*| / (bound / l2) "
          f"{np.round(dist / (bound / L2), 3).tolist()}, grad_ratio {np.round(res.grad_ratio.cpu().numpy(), 5).tolist()}")
    assert (gnorm <= bound).all()
    assert (dist <= bound / L2).all()                            # strong convexity, modulus l2
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all() and (res.grad_ratio.cpu().numpy() <= GTOL).all()
    f_model = np.array([prob.user_objective(rows[r], V64, r, L2) for r in range(8)])
    np.testing.assert_allclose(after, f_model, rtol=RTOL, atol=ATOL)
    # a user with a NaN truth row: status 2, a NaN row; its neighbours as without it
    Xbad = Xd.clone()
    Xbad[3, m // 2] = float("nan")
    bad = population.population_user_step(U0, Vd, Xbad, 1.0, L2, law)
    others = [0, 1, 2, 4, 5, 6, 7]
    assert bad.status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and bool(torch.isnan(bad.rows[3]).all())
    if not with_law:
        base = res                                               # the clean run: the plain normaliser counts the users named
        pick = others
    else:                                                        # under a law the user leaves 1 / sum W: the run without it
        base = population.population_user_step(U0, Vd, Xd, 1.0, L2, law, users=others)
        pick = list(range(7))
    # Bit-equal wherever 1 / sum W and the score GEMMs are: a sum of seven addends instead of eight may round its last f64
    # bit differently and a GEMM of seven rows may take another kernel, so the law's run is held to 4 fp32 ulps of the
    # rows instead and to 1e-6 of the objective (an fp32 ulp of a score moves the risk by about 1e-7); the plain run to the
    # bits.  grad_ratio is a residual at the gradient's noise level: both runs are held to the certificate, not to each other.
    got, want = bad.rows[others].cpu().numpy(), base.rows[pick].cpu().numpy()
    if with_law:
        print(f"m={m}: neighbours under the law bit-equal to the run without the user: {got.tobytes() == want.tobytes()}")
        np.testing.assert_array_max_ulp(got, want, maxulp=4)
    else:
        assert got.tobytes() == want.tobytes()
    assert bad.newton_iters[others].tolist() == base.newton_iters[pick].tolist()
    np.testing.assert_allclose(bad.objective_after[others].cpu().numpy(), base.objective_after[pick].cpu().numpy(),
                               rtol=1e-6 if with_law else 0, atol=0)
    assert (bad.grad_ratio[others].cpu().numpy() <= GTOL).all() and (base.grad_ratio[pick].cpu().numpy() <= GTOL).all()
    assert base.status[pick].tolist() == [0] * 7


@functools.lru_cache(maxsize=None)
def item_minimiser(m):
    Ustar, V, X = HM.solver_inputs(m)
    prob = HM.Problem(X, 1.0)
    U64 = Ustar.astype(np.float64)
    Vopt = prob.solve_items(U64, np.zeros((m, 3)), L2)[0]
    return prob, Vopt, prob.item_noise(U64, Vopt)


@pytest.mark.parametrize("m", [40, 1029])
def test_item_step_reaches_the_models_minimiser(dev, m):
    from mfcd import population
    Ustar, V, X = HM.solver_inputs(m)
    prob, Vopt, noise = item_minimiser(m)
    res = population.population_item_step(to(dev, Ustar), torch.zeros(m, 3, device=dev), to(dev, X), 1.0, L2)
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert int(res.status) == 0 and res.rows.dtype == torch.float32 and tuple(res.rows.shape) == (m, 3)
    gnorm = np.linalg.norm(prob.item_grad(Ustar.astype(np.float64), rows, L2))
    bound = GTOL * L2 * np.abs(rows).max() + noise
    dist = np.linalg.norm(rows - Vopt)
    print(f"m={m}: Newton {int(res.newton_iters)}, CG {int(res.cg_iters)}, |grad| {gnorm:.3e}, bound {bound:.3e} "
          f"(noise {noise:.3e}), |V - V*| {dist:.3e} against {bound / L2:.3e}, grad_ratio {float(res.grad_ratio):.2e}")
    assert gnorm <= bound and dist <= bound / L2
    assert float(res.objective_after) <= float(res.objective_before) and float(res.grad_ratio) <= GTOL
    Xbad = to(dev, X)
    Xbad[2, 1] = float("inf")
    V0 = to(dev, V)
    bad = population.population_item_step(to(dev, Ustar), V0, Xbad, 1.0, L2)
    assert int(bad.status) == 2 and torch.equal(bad.rows, V0)


def test_alternating_fit_descends_and_records_the_models_objective(dev):
    import structure as S
    from mfcd import _lib, population
    Ustar, V, X = HM.solver_inputs(40)
    rng = np.random.default_rng(8)
    U0 = (0.3 * rng.standard_normal((8, 3))).astype(np.float32)
    V0 = (0.3 * rng.standard_normal((40, 3))).astype(np.float32)
    prob = HM.Problem(X, 1.0)
    Xd = to(dev, X)
    seen, tables = [], (to(dev, U0), to(dev, V0))
    for sweep in range(3):                                       # one sweep at a time: the tables of every sub-step
        U_before = tables[0].clone()
        res = population.fit_population_exact(*tables, Xd, 1.0, L2, 1)
        assert res.U is tables[0] and res.V is tables[1]
        Un, Vn = (t.cpu().numpy().astype(np.float64) for t in tables)
        if sweep == 0:
            start = prob.objective(U0.astype(np.float64), V0.astype(np.float64), L2)
            np.testing.assert_allclose(float(res.objective_start), start, rtol=RTOL, atol=ATOL)
            seen.append(float(res.objective_start))
        seen += res.history[0].tolist()
        np.testing.assert_allclose(res.history[0, 1].item(), prob.objective(Un, Vn, L2), rtol=RTOL, atol=ATOL)
        assert not torch.equal(U_before, tables[0])
    model = S.MatrixFactorization(8, 40, 3).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, U0))
        model.V.copy_(to(dev, V0))
    hist = S.train_model_population_exact(model, Xd, 1.0, L2, sweeps=3)
    flat = [f for pair in hist for f in pair]
    print(f"F: start {seen[0]:.7f}, sub-steps {np.round(flat, 7).tolist()}")
    assert len(hist) == 3 and all(len(pair) == 2 for pair in hist)
    assert all(b <= a for a, b in zip([seen[0]] + flat[:-1], flat))             # non-increasing
    np.testing.assert_allclose(flat, seen[1:], rtol=1e-9)        # k sweeps are k chained calls of one sweep
    for mine, chained in ((model.U.data, tables[0]), (model.V.data, tables[1])):  # the model's own parameters moved
        np.testing.assert_allclose(mine.cpu().numpy(), chained.cpu().numpy(), rtol=1e-5, atol=1e-7)
    assert not np.array_equal(model.U.detach().cpu().numpy(), U0)
    Uf, Vf = (t.cpu().numpy().astype(np.float64) for t in tables)
    np.testing.assert_allclose(flat[-1], prob.objective(Uf, Vf, L2), rtol=RTOL, atol=ATOL)
    # the user-step value of every sweep against the model, at the tables of that sub-step: replay with the steps
    U, Vt = to(dev, U0), to(dev, V0)
    for sweep in range(3):
        step = population.population_user_step(U, Vt, Xd, 1.0, L2)
        U = step.rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(hist[sweep][0], want, rtol=RTOL, atol=ATOL)
        Vt = population.population_item_step(U, Vt, Xd, 1.0, L2).rows
        want = prob.objective(U.cpu().numpy().astype(np.float64), Vt.cpu().numpy().astype(np.float64), L2)
        np.testing.assert_allclose(hist[sweep][1], want, rtol=RTOL, atol=ATOL)
    bf = S.MatrixFactorization(8, 40, 3, dtype=torch.bfloat16).to(dev)
    with pytest.raises(_lib.MfcdError):
        S.train_model_population_exact(bf, Xd, 1.0, L2, sweeps=1)
    with pytest.raises(_lib.MfcdError):
        population.population_user_step(bf.U.data, bf.V.data, Xd, 1.0, L2)
