"""GPU tests of the joint Newton fit of the sampled BTL objective (mfcd/newton.py: fit_newton; structure.refit_newton)
against the numpy model of tests/newton_model.py (fit, gradient), on the four fit cases of that module: draws from
np.random.default_rng(1) — A ~ N(0, I), B ~ N(0, I / d), uniform (u, i, j), labels uniform < sigmoid(3 A[u] . (B[i] - B[j])),
then the start U, V ~ N(0, 1 / d) rounded to fp32.  tests/test_triplet_hess_cpu.py checks that the model certifies the
same cases.

Bounds.  Status 0 means |grad F|_inf <= 2^-26 l2 max|.|_inf at the f64 iterate; the one rounding of the output to fp32
moves every entry by at most 2^-24 max|.|_inf and so the gradient by at most |H|_inf 2^-24 max|.|_inf, |H|_inf bounded by
the largest absolute row sum of the Hessian (newton_model.hessian_inf_norm_bound).  The model's gradient at the returned
tables is held to the larger of 2^-22 l2 max|.|_inf and that rounding term.  The final F: within 1e-10 relative of the
model's (perturbed starts of the model end at the same F to 1e-15)."""
import functools

import numpy as np
import pytest
import torch

import newton_model as NM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def model_fit(case):
    n, m, d, N, l2 = case
    return NM.fit(*NM.make_fit_case(n, m, d, N), l2, max_iter=100)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).tobytes()


@pytest.mark.parametrize("case", NM.FIT_CASES, ids=lambda c: "n%d-m%d-d%d-N%d-l2_%g" % c)
def test_fit_certifies_and_agrees_with_the_model(dev, case):
    from mfcd import newton
    n, m, d, N, l2 = case
    U0, V0, u, i, j, z = NM.make_fit_case(n, m, d, N)
    Ut, Vt = torch.from_numpy(U0).to(dev), torch.from_numpy(V0).to(dev)
    data = tuple(torch.from_numpy(a).to(dev) for a in (u, i, j, z))
    res = newton.fit_newton(Ut, Vt, *data, l2, max_iter=100)
    hist = res.history.cpu().numpy()
    print(f"status {res.status}, outer iterations {len(hist)}, Hessian products {res.products}, F {hist[-1]!r}, "
          f"|g|_inf {res.grad_inf[-1].item():.3e}, CG iterations {res.cg_iters.tolist()}")
    assert res.status == 0 and len(hist) <= 100
    assert res.U.dtype == torch.float32 and res.V.dtype == torch.float32 and tuple(res.U.shape) == (n, d) and tuple(res.V.shape) == (m, d)
    assert res.history.dtype == torch.float64 and res.grad_inf.dtype == torch.float64 and len(res.grad_inf) == len(hist)
    assert len(res.cg_iters) == len(hist) - 1 and res.products == int(res.cg_iters.sum()) + len(res.cg_iters)
    assert (np.diff(hist) <= 0).all(), np.diff(hist).max()
    assert torch.equal(Ut.cpu(), torch.from_numpy(U0)) and torch.equal(Vt.cpu(), torch.from_numpy(V0))    # inputs untouched
    # the model's gradient at the returned tables, widened to f64
    U, V = res.U.cpu().numpy().astype(np.float64), res.V.cpu().numpy().astype(np.float64)
    _, gU, gV, _, _ = NM.gradient(U, V, u, i, j, z, l2)
    ginf, xmax = max(np.abs(gU).max(), np.abs(gV).max()), max(np.abs(U).max(), np.abs(V).max())
    certificate = 2.0 ** -22 * l2 * xmax
    rounding = NM.hessian_inf_norm_bound(U, V, u, i, j, z, l2) * 2.0 ** -24 * xmax
    print(f"|g|_inf at the fp32 tables {ginf:.3e}; certificate bound {certificate:.3e}, rounding term {rounding:.3e}")
    assert ginf <= max(certificate, rounding)
    ref = model_fit(case)
    assert ref.status == 0
    print(f"model: outer iterations {len(ref.history)}, products {ref.products}, F {ref.history[-1]!r}")
    assert abs(hist[-1] - ref.history[-1]) <= 1e-10 * abs(ref.history[-1])
    again = newton.fit_newton(Ut, Vt, *data, l2, max_iter=100)
    assert again.status == res.status and again.products == res.products
    for a, b in zip(res[:5], again[:5]):
        assert bits(a) == bits(b)


def test_fit_stops_and_refuses(dev):
    from mfcd import _lib, newton
    n, m, d, N, l2 = NM.FIT_CASES[0]
    U0, V0, u, i, j, z = NM.make_fit_case(n, m, d, N)
    Ut, Vt = torch.from_numpy(U0).to(dev), torch.from_numpy(V0).to(dev)
    data = [torch.from_numpy(a).to(dev) for a in (u, i, j, z)]
    short = newton.fit_newton(Ut, Vt, *data, l2, max_iter=3)
    assert short.status == 1 and len(short.history) == 3 and len(short.cg_iters) == 3 and (np.diff(short.history.cpu().numpy()) < 0).all()
    assert short.products == int(short.cg_iters.sum()) + 3
    z_bad = data[3].clone()
    z_bad[5] = 1.5
    nan = newton.fit_newton(Ut, Vt, data[0], data[1], data[2], z_bad, l2)
    assert nan.status == 1 and len(nan.history) == 1 and torch.isnan(nan.history[0])
    with pytest.raises(ValueError):
        newton.fit_newton(Ut, Vt, *data, 0.0)
    with pytest.raises(_lib.MfcdError):
        newton.fit_newton(torch.zeros(4, 257, device=dev), torch.zeros(3, 257, device=dev), *(t[:0] for t in data), 1.0)


def test_refit_newton_on_a_trained_model(dev):
    """structure.refit_newton on a model of the smallest benchmark size (n = m = 256, d = 8, 1310 training comparisons,
    weight decay 1e-5) after three epochs of Adam: F does not rise from the model's tables, ten sweeps of
    refit_alternating end no lower than the Newton fit, and the model is not changed."""
    import structure as S
    torch.manual_seed(5)
    np.random.seed(5)
    n = m = 256
    d, wd = 8, 1e-5
    X = torch.randn(n, m).to(dev)
    train, val, _ = S.split_dataset_from_triplets(X, 1638, scale=1.0, K=1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=wd)
    S.train_model(model, train, val, opt, dev, num_epochs=3)
    before = (model.U.data.clone(), model.V.data.clone())
    res, F_model = S.refit_newton(model, train, wd)
    hist = res.history.cpu().numpy()
    alt, F_alt0 = S.refit_alternating(model, train, wd)
    F_alt = float(alt.history[-1, -1])
    print(f"F at the model {float(F_model)!r}; Newton: status {res.status}, {len(hist)} outer iterations, {res.products} "
          f"products, F {hist[-1]!r}, |g|_inf {res.grad_inf[0].item():.3e} -> {res.grad_inf[-1].item():.3e}; alternating "
          f"(10 sweeps): F {F_alt!r}")
    assert bits(F_model) == bits(res.history[0]) and abs(float(F_model) - float(F_alt0)) <= 1e-12 * float(F_alt0)
    assert float(F_model) - hist[-1] >= 0 and (np.diff(hist) <= 0).all()
    assert F_alt >= hist[-1] - 1e-9 * abs(hist[-1])
    assert torch.equal(model.U.data, before[0]) and torch.equal(model.V.data, before[1])
