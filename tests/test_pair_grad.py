"""GPU tests of the pair-gradient kernel and of the population fit built on it (include/mfcd.h: mfcd_pair_grad_rows;
mfcd/pairs.py: pair_grad_rows, population_risk, fit_population; structure.population_risk, train_model_population)
against the float64 model of tests/pair_grad_model.py.

Shapes: with T = pairs.TILE columns per workgroup tile, m in {1, 2, 63, 64, 65, T-1, T, T+1, 2T+3} reaches the empty sum,
a single pair, the wave boundary, a partly filled / exactly full tile, a second tile of one column (tile 1 must visit
tile 0) and three tiles with a short last one (pad columns must stay silent for every tile I).  Values lie in [-3, 3],
except one row of a in {-60, 0, 60} (differences of 120: exp underflows, nothing may overflow), at scale 1 only.

Tolerance of the gradient, on the mean term g_i / (m - 1): rtol 2e-5, atol 2e-6, the project's fp32-loss tolerance
(tests/test_pairs.py).  A worst-case count of the kernel's roundings lies inside it: per term about 10 * 2^-24 absolute
(argument roundings times max |v| sigmoid'(v) = 0.224, one ulp each of exp and reciprocal, two adds, one multiply, the
subtraction), and up to 33 * 2^-24 relative from fp32 runs of 64 terms: 6e-7 + 2e-6 |mean term|.  The reference of
every shape is computed once per module and shared."""
import functools

import numpy as np
import pytest
import torch

import pair_grad_model as GM

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.25, 4.0)
RTOL, ATOL = 2e-5, 2e-6


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


def _levels(m, rng, values):
    return np.asarray(values, dtype=np.float32)[rng.integers(0, len(values), m)]


def _distinct(m, rng):
    return (rng.permutation(m).astype(np.float64) / m * 6.0 - 3.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_rows(m):
    """(A, X) float32 [8, m]; the LAST row is the large-spread one, used at scale 1 only."""
    rng = np.random.default_rng(2000 + m)
    three = (-1.5, 0.0, 2.25)
    zeros = (-0.0, 0.0, 0.0, -0.0, 1.0, -2.0)
    tiny = np.float32(1e-42)                                   # denormal values whose differences are denormal too
    rows = [
        (_distinct(m, rng), _distinct(m, rng)),                # no ties
        (_levels(m, rng, three), _distinct(m, rng)),           # heavy ties in a
        (_distinct(m, rng), _levels(m, rng, three)),           # heavy ties in x
        (_levels(m, rng, three), _levels(m, rng, three)),      # heavy ties in both
        (np.full(m, 0.75, dtype=np.float32), _distinct(m, rng)),                  # constant row
        (_levels(m, rng, zeros), _levels(m, rng, zeros)),      # -0.0 equals +0.0
        (rng.integers(-3, 4, m).astype(np.float32) * tiny, rng.integers(-2, 3, m).astype(np.float32) * tiny),
        (_levels(m, rng, (-60.0, 0.0, 60.0)), _distinct(m, rng)),                 # large spread
    ]
    A, X = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert np.abs(A[:-1]).max() <= 3 and np.abs(X).max() <= 3
    return A, X


def rows_for(m, scale):
    A, X = case_rows(m)
    return (A, X) if scale == 1.0 else (A[:-1], X[:-1])


@functools.lru_cache(maxsize=None)
def ref_grad(m, scale):
    A, X = rows_for(m, scale)
    return np.stack([GM.pair_grad(a, x, scale) for a, x in zip(A, X)])


def run(dev, A, X, scale=1.0):
    from mfcd import pairs
    G = pairs.pair_grad_rows(torch.from_numpy(np.ascontiguousarray(A)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(X)).to(dev), scale)
    assert G.dtype == torch.float32 and tuple(G.shape) == A.shape
    return G.cpu().numpy()


def check_grad(got, want, m, what):
    if m == 1:
        assert got.tobytes() == np.zeros_like(got).tobytes(), what            # an empty sum: exactly +0
        return
    g, w = got.astype(np.float64) / (m - 1), want / (m - 1)
    err = np.abs(g - w)
    print(f"{what}: max |mean term| {np.abs(w).max():.4f}, max abs error {err.max():.3e}, "
          f"max error / bound {(err / (ATOL + RTOL * np.abs(w))).max():.3f}, "
          f"max error of g_i in units of (m - 1) 2^-24: {(err * 2.0 ** 24).max():.3f}")
    np.testing.assert_allclose(g, w, rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", _ms())
def test_gradient_matches_the_f64_model(dev, m, scale):
    A, X = rows_for(m, scale)
    got = run(dev, A, X, scale)
    check_grad(got, ref_grad(m, scale), m, f"m={m} scale={scale}")
    assert np.isfinite(got).all()
    # every pair enters twice with opposite signs: a row's gradient sums to 0 within the bound on its entries
    if m > 1:
        assert (np.abs(got.astype(np.float64).sum(1)) / (m - 1) <= m * (ATOL + RTOL)).all()


@pytest.mark.parametrize("m", [65, _ms()[-1]])
def test_two_calls_rows_alone_and_strided_views_are_bit_equal(dev, m):
    from mfcd import _lib, pairs
    A, X = case_rows(m)
    rows = A.shape[0]
    base = run(dev, A, X, 4.0)
    assert run(dev, A, X, 4.0).tobytes() == base.tobytes()
    for r in range(rows):                                      # a row does not depend on its neighbours
        assert run(dev, A[r:r + 1], X[r:r + 1], 4.0).tobytes() == base[r:r + 1].tobytes(), r
    Ad, Xd = torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)
    wideA = torch.full((rows, m + 5), 7.0, device=dev)
    wideX = torch.full((rows, m + 9), -7.0, device=dev)
    wideA[:, 2:2 + m], wideX[:, 6:6 + m] = Ad, Xd
    va, vx = wideA[:, 2:2 + m], wideX[:, 6:6 + m]
    assert va.stride(0) == m + 5 and not va.is_contiguous()
    assert pairs.pair_grad_rows(va, vx, 4.0).cpu().numpy().tobytes() == base.tobytes()
    # ldg > m through the C entry: the same bits, and the padding columns of G are left alone
    ldg = m + 7
    wideG = torch.full((rows, ldg), -123.0, device=dev)
    _lib.check(_lib.load().mfcd_pair_grad_rows(va.data_ptr(), va.stride(0), vx.data_ptr(), vx.stride(0), rows, m, 4.0,
                                               wideG.data_ptr(), ldg, _lib.stream_ptr(dev)))
    host = wideG.cpu().numpy()
    assert np.ascontiguousarray(host[:, :m]).tobytes() == base.tobytes()
    assert (host[:, m:] == -123.0).all()
    empty = pairs.pair_grad_rows(Ad[:0], Xd[:0])
    assert tuple(empty.shape) == (0, m) and empty.dtype == torch.float32
    with pytest.raises(Exception):
        pairs.pair_grad_rows(Ad, Xd[:, :-1])


def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(dev):
    T = _tile()
    m = T + 37
    rng = np.random.default_rng(5)
    A = np.stack([_distinct(m, rng) for _ in range(6)])
    X = np.stack([_levels(m, rng, (-1.0, 0.5, 2.0, 3.0)) for _ in range(6)])
    clean = run(dev, A, X, 1.0)
    assert np.isfinite(clean).all()
    A[1, 3] = np.inf                                           # first tile: the second tile's workgroup must see it
    A[3, T + 30] = np.nan                                      # second tile: the first tile's workgroup must see it
    X[4, 2] = -np.inf
    X[5, m - 1] = np.nan                                       # the last column
    got = run(dev, A, X, 1.0)
    assert np.isnan(got[[1, 3, 4, 5]]).all()
    assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    check_grad(got[[0, 2]], np.stack([GM.pair_grad(A[r], X[r], 1.0) for r in (0, 2)]), m, "neighbours of bad rows")


# ---------------------------------------------------------------------------------------------------------------------
# population_risk: value and table gradients
# ---------------------------------------------------------------------------------------------------------------------
def _problem(n, m, d, seed, dev):
    import generation_data as gd
    import structure as S
    g = torch.Generator().manual_seed(seed)
    F = gd.FactoredMatrix(torch.randn(n, 2, generator=g), torch.randn(m, 2, generator=g))
    torch.manual_seed(seed)
    model = S.MatrixFactorization(n, m, d).to(dev)
    return S, model, F, F.dense(dev)


def check_tables(model, Xh, s, users, what):
    """model.U.grad / model.V.grad against the f64 model's, elementwise.  G's bound carried through the product, plus
    the GEMM's own worst-case rounding (one 2^-24 per term of the inner dimension): for U, with k users in the mean,
      (2e-5 + m 2^-24) (|G64| @ |V|) / (k n0) + 2e-6 (m - 1) sum_i |V_i| / (k n0),
    and the mirror image for V (inner dimension k, |G64|^T @ |U[users]|, sum over the chosen users of |U_u|)."""
    U, V = model.U.detach().cpu().numpy().astype(np.float64), model.V.detach().cpu().numpy().astype(np.float64)
    n, m = U.shape[0], V.shape[0]
    ids = np.arange(n) if users is None else np.asarray(users)
    k, n0 = len(ids), m * (m - 1) // 2
    dU, dV, G = GM.population_grad(U, V, Xh, s, users)
    per_row = ((RTOL + m * 2.0 ** -24) * (np.abs(G) @ np.abs(V)) + ATOL * (m - 1) * np.abs(V).sum(0)) / (k * n0)
    boundU = np.zeros_like(U)
    np.add.at(boundU, ids, per_row)
    boundV = ((RTOL + k * 2.0 ** -24) * (np.abs(G).T @ np.abs(U[ids])) + ATOL * (m - 1) * np.abs(U[ids]).sum(0)) / (k * n0)
    for name, got, want, bound in (("U", model.U.grad, dU, boundU), ("V", model.V.grad, dV, boundV)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        live = bound > 0
        print(f"{what}: d{name} max |grad| {np.abs(want).max():.3e}, max abs error {err.max():.3e}, "
              f"max error / bound {(err[live] / bound[live]).max():.3f}")
        assert (err <= bound).all(), (what, name)


@pytest.mark.parametrize("shape", ["n5_m65_d3", "n3_mT1_d2"])
def test_population_risk_value_and_gradients(dev, shape):
    n, m, d = (5, 65, 3) if shape == "n5_m65_d3" else (3, _tile() + 1, 2)
    S, model, F, Xd = _problem(n, m, d, 21, dev)
    Xh = Xd.cpu().numpy().astype(np.float64)
    U, V = model.U.detach().cpu().numpy(), model.V.detach().cpu().numpy()
    s = 0.7
    variants = [("all users", {}, None), ("row_block=2", {"row_block": 2}, None)]
    if n == 5:
        variants.append(("users=[4, 0, 4]", {"users": [4, 0, 4], "row_block": 2}, [4, 0, 4]))
    for what, kw, users in variants:
        model.zero_grad()
        risk = S.population_risk(model, Xd, s, **kw)
        assert risk.dim() == 0 and risk.is_cuda and risk.dtype == torch.float32 and risk.requires_grad
        want = GM.population_risk(U, V, Xh, s, users)
        print(f"{shape} {what}: risk {float(risk.detach()):.6f}, model {want:.6f}")
        np.testing.assert_allclose(float(risk.detach()), want, rtol=RTOL, atol=ATOL, err_msg=what)
        risk.backward()
        check_tables(model, Xh, s, users, f"{shape} {what}")
    # a factored X against the dense X of the same factors: the same tolerance, not the same bits (the GEMM differs)
    model.zero_grad()
    risk = S.population_risk(model, F, s)
    np.testing.assert_allclose(float(risk.detach()), GM.population_risk(U, V, Xh, s), rtol=RTOL, atol=ATOL)
    risk.backward()
    check_tables(model, Xh, s, None, f"{shape} factored X")
    with pytest.raises(IndexError):
        S.population_risk(model, Xd, s, users=[n])
    with pytest.raises(ValueError):
        S.population_risk(model, Xd[:, :-1], s)
    one = S.MatrixFactorization(n, 1, d).to(dev)
    with pytest.raises(ValueError):
        S.population_risk(one, Xd[:, :1], s)


# ---------------------------------------------------------------------------------------------------------------------
# train_model_population
# ---------------------------------------------------------------------------------------------------------------------
FIT = dict(n=12, m=40, d=2, s=1.0, lr=0.05, steps=400, log_every=100)


def row_centred_error(S, model, Xd, s, dev):
    """The row-centred reconstruction error, from structure.compute_reconstruction_error.  That function centres
    U V^T over the USERS (dim 0, as the reference does), and the pair risk leaves every user's row free up to a
    constant: so it is given the transposed problem — item table as users, user table as items, (X - row mean)^T as
    the truth — where its centring over dim 0 removes each user's row mean.  ||(P - rowmean P) - s (X - rowmean X)||_F /
    ||s (X - rowmean X)||_F: the denominator is no larger than ||s X||_F, so the value is no smaller."""
    n, m, d = model.U.shape[0], model.V.shape[0], model.U.shape[1]
    swapped = S.MatrixFactorization(m, n, d).to(dev)
    with torch.no_grad():
        swapped.U.copy_(model.V)
        swapped.V.copy_(model.U)
    Xc = (Xd - Xd.mean(dim=1, keepdim=True)).t().contiguous()
    return S.compute_reconstruction_error(swapped, Xc, s)


@pytest.fixture(scope="module")
def fit_setup(dev):
    """X from generate_X under a fixed seed, the model's start, and the f64 model's run from the same start."""
    import structure as S
    np.random.seed(0)
    torch.manual_seed(0)
    X = S.generate_X(FIT["n"], FIT["m"], FIT["d"], "cpu")
    model = S.MatrixFactorization(FIT["n"], FIT["m"], FIT["d"])
    U0, V0 = model.U.detach().numpy().copy(), model.V.detach().numpy().copy()
    Xh = X.numpy().astype(np.float64)
    Uf, Vf, at, risks = GM.fit(U0, V0, Xh, FIT["s"], FIT["steps"], FIT["lr"], log_every=FIT["log_every"])
    bayes = GM.bayes_risk(Xh, FIT["s"])
    Xc = Xh - Xh.mean(1, keepdims=True)
    P = Uf @ Vf.T
    rec = np.linalg.norm((P - P.mean(1, keepdims=True)) - FIT["s"] * Xc) / np.linalg.norm(FIT["s"] * Xc)
    print(f"f64 model: risks {np.round(risks, 7).tolist()}, bayes {bayes:.7f}, gap {risks[-1] - bayes:.2e}, "
          f"row-centred reconstruction error {rec:.2e}")
    # a bad seed fails here, as a bad seed
    assert risks[-1] - bayes <= 1e-4 and rec <= 0.02 and at == [0, 100, 200, 300, 400]
    return S, X.to(dev), U0, V0, at, risks, bayes


def _model_at(S, U0, V0, dev):
    model = S.MatrixFactorization(*U0.shape[:1], V0.shape[0], U0.shape[1])
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(U0))
        model.V.copy_(torch.from_numpy(V0))
    return model.to(dev)


def test_fused_fit_reaches_the_bayes_risk_and_the_truth(fit_setup, dev):
    S, Xd, U0, V0, at, ref_risks, bayes = fit_setup
    model = _model_at(S, U0, V0, dev)
    opt = torch.optim.Adam(model.parameters(), lr=FIT["lr"])
    assert model.training
    steps, risks = S.train_model_population(model, Xd, FIT["s"], opt, dev, num_steps=FIT["steps"],
                                            log_every=FIT["log_every"])
    assert not model.training
    assert steps == at and len(risks) == len(at) and all(isinstance(r, float) for r in risks)
    res = S.compute_pairwise_metrics(model, Xd, s=FIT["s"])
    gap = -res["expected_log_likelihood"] - -res["bayes_log_likelihood"]
    rec = row_centred_error(S, model, Xd, FIT["s"], dev)
    print(f"fused fit: logged risks {np.round(risks, 7).tolist()} (model {np.round(ref_risks, 7).tolist()}), "
          f"risk - bayes {gap:.3e}, row-centred reconstruction error {rec:.3e}, "
          f"compute_reconstruction_error as is {S.compute_reconstruction_error(model, Xd, FIT['s']):.3f}")
    assert gap <= 1e-4 and rec <= 0.02
    np.testing.assert_allclose(risks[0], ref_risks[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(-res["bayes_log_likelihood"], bayes, rtol=RTOL, atol=ATOL)
    for a, b in zip(risks[:-1], risks[1:]):
        if a > bayes + 1e-3:
            assert b <= a, risks
    assert float(opt.state[model.U]["step"]) == FIT["steps"] == float(opt.state[model.V]["step"])


def test_fused_first_step_with_weight_decay_is_the_models_adam_step(fit_setup, dev):
    S, Xd, U0, V0, _, ref_risks, _ = fit_setup
    model = _model_at(S, U0, V0, dev)
    opt = torch.optim.Adam(model.parameters(), lr=FIT["lr"], weight_decay=1e-2)
    steps, risks = S.train_model_population(model, Xd, FIT["s"], opt, dev, num_steps=1, log_every=1)
    assert steps == [0, 1] and float(opt.state[model.U]["step"]) == 1
    Xh = Xd.cpu().numpy().astype(np.float64)
    Uf, Vf, _, want = GM.fit(U0, V0, Xh, FIT["s"], 1, FIT["lr"], weight_decay=1e-2, log_every=1)
    np.testing.assert_allclose(risks, want, rtol=RTOL, atol=ATOL)
    # the first step is -+lr per element wherever |grad| is far above eps: compare those elements only
    dU, dV, _ = GM.population_grad(U0, V0, Xh, FIT["s"])
    for name, got, ref, g in (("U", model.U, Uf, dU + 1e-2 * U0), ("V", model.V, Vf, dV + 1e-2 * V0)):
        live = np.abs(g) > 1e-6
        assert live.sum() >= live.size // 2, name
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)[live]
        print(f"first step, {name}: {live.sum()} of {live.size} elements compared, max abs error {err.max():.2e}")
        assert err.max() <= 1e-6, name


def test_generic_path_is_plain_backward_and_manual_updates(dev):
    S, model, F, Xd = _problem(5, 65, 3, 33, dev)
    twin = _model_at(S, model.U.detach().cpu().numpy(), model.V.detach().cpu().numpy(), dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    steps, risks = S.train_model_population(model, Xd, 0.7, opt, dev, num_steps=3, log_every=1)
    assert steps == [0, 1, 2, 3] and not model.training
    seen = []
    for _ in range(3):
        twin.zero_grad()
        risk = S.population_risk(twin, Xd, 0.7)
        seen.append(float(risk.detach()))
        risk.backward()
        with torch.no_grad():
            twin.U -= 0.1 * twin.U.grad
            twin.V -= 0.1 * twin.V.grad
    with torch.no_grad():
        seen.append(float(S.population_risk(twin, Xd, 0.7)))
    np.testing.assert_allclose(model.U.detach().cpu().numpy(), twin.U.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(model.V.detach().cpu().numpy(), twin.V.detach().cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(risks, seen, rtol=1e-5, atol=0)
    assert risks[3] < risks[0]


def test_fit_population_refuses_bf16_tables(dev):
    import structure as S
    from mfcd import _lib, pairs
    model = S.MatrixFactorization(4, 9, 2, dtype=torch.bfloat16).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    X = torch.randn(4, 9, device=dev)
    with pytest.raises(_lib.MfcdError):
        pairs.fit_population((model, opt), X, 1.0, 2)
    with pytest.raises(_lib.MfcdError):
        S.population_risk(model, X)


def test_population_risk_block_loop_at_a_ragged_last_block_and_a_repeated_user(dev):
    """n = 70, m = 130, d = 8 with row_block = 32 (blocks of 32, 32 and 6 or 8 rows) and = 70, every user and users with a
    repeat, dense and factored X: value and table gradients against the f64 model, under the bounds of the test above;
    the values at the two row blocks against each other under the same RTOL / ATOL (the score GEMMs may round
    differently, so not bits)."""
    n, m, d, s = 70, 130, 8, 0.7
    S, model, F, Xd = _problem(n, m, d, 23, dev)
    Xh = Xd.cpu().numpy().astype(np.float64)
    U, V = model.U.detach().cpu().numpy(), model.V.detach().cpu().numpy()
    users = list(range(n - 1, -1, -1)) + [3, 3]
    for sel in (None, users):
        want = GM.population_risk(U, V, Xh, s, sel)
        for X, kind in ((Xd, "dense"), (F, "factored")):
            risks = {}
            for rb in (32, 70):
                what = f"{kind} X, row_block={rb}, {'every user' if sel is None else 'users with a repeat'}"
                model.zero_grad()
                risk = S.population_risk(model, X, s, users=sel, row_block=rb)
                risks[rb] = float(risk.detach())
                np.testing.assert_allclose(risks[rb], want, rtol=RTOL, atol=ATOL, err_msg=what)
                risk.backward()
                check_tables(model, Xh, s, sel, what)
            np.testing.assert_allclose(risks[32], risks[70], rtol=RTOL, atol=ATOL, err_msg=kind)
