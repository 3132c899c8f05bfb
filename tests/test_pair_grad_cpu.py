"""CPU-only checks of the pair-gradient entry and what is built on it (include/mfcd.h: mfcd_pair_grad_rows;
mfcd/pairs.py: pair_grad_rows, population_risk, fit_population; structure.population_risk, train_model_population):
the entry is declared and bound, bad arguments are refused before the device is touched, there is no CPU fallback, and
the CPU model the GPU tests compare with (tests/pair_grad_model.py) is the derivative of tests/pairs_model.py's risk."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_grad_model as GM
from conftest import ROOT


def test_pair_grad_entry_is_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert "mfcd_pair_grad_rows" in _lib.SIGNATURES and re.search(r"\bmfcd_pair_grad_rows\(", header)
    assert len(_lib.SIGNATURES["mfcd_pair_grad_rows"][1]) == 10
    decl = re.search(r"int mfcd_pair_grad_rows\(([^)]*)\)", header).group(1)
    assert len(decl.split(",")) == 10
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    assert _lib.load().mfcd_abi_version() == 4


def test_pair_grad_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    P, Q, R = 4096, 8192, 12288                 # non-null addresses that are never dereferenced: every call is refused

    def call(rows=2, m=8, scale=1.0, A=P, X=Q, G=R, lda=8, ldx=8, ldg=8):
        return L.mfcd_pair_grad_rows(A, lda, X, ldx, rows, m, scale, G, ldg, None)

    assert call(m=0) == -1 and call(m=1048577, lda=1 << 21, ldx=1 << 21, ldg=1 << 21) == -1
    assert call(rows=-1) == -1
    assert call(A=None) == -1 and call(X=None) == -1 and call(G=None) == -1
    assert call(lda=7) == -1 and call(ldx=7) == -1 and call(ldg=7) == -1
    assert call(scale=float("inf")) == -1 and call(scale=float("nan")) == -1 and call(scale=1e300) == -1
    assert call(G=P) == -1 and call(G=Q) == -1                 # G == A, G == X
    assert call(rows=0) == 0                    # nothing to do, nothing launched
    assert call(rows=0, G=P) == -1              # and a bad call stays bad with no rows


def test_pair_grad_has_no_cpu_fallback():
    import generation_data as gd
    import structure as S
    from mfcd import _lib, pairs
    A, X = torch.randn(3, 9), torch.randn(3, 9)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_grad_rows(A, X)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_grad_rows(A.double(), X.double())
    model = S.MatrixFactorization(3, 9, 2)
    with pytest.raises(_lib.MfcdError):
        pairs.population_risk(model.U, model.V, X)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    with pytest.raises(_lib.MfcdError):
        pairs.fit_population((model, opt), X, 1.0, 2)
    for truth in (X, gd.FactoredMatrix(torch.randn(3, 2), torch.randn(9, 2))):
        with pytest.raises(RuntimeError):
            S.population_risk(model, truth)
        with pytest.raises(RuntimeError):
            S.train_model_population(model, truth, 1.0, opt, "cpu", num_steps=2)


def test_pair_grad_public_signatures():
    import structure as S
    from mfcd import pairs
    p = inspect.signature(pairs.pair_grad_rows).parameters
    assert list(p) == ["A", "X", "scale"] and p["scale"].default == 1.0
    p = inspect.signature(pairs.population_risk).parameters
    assert list(p) == ["U", "V", "X", "s", "users", "row_block"]
    assert p["s"].default == 1.0 and p["users"].default is None and p["row_block"].default == 2048
    p = inspect.signature(pairs.fit_population).parameters
    assert list(p)[1:] == ["X", "s", "steps", "log_every", "row_block"] and len(p) == 6
    assert p["log_every"].default == 0 and p["row_block"].default == 2048
    p = inspect.signature(S.population_risk).parameters
    assert list(p) == ["model", "X", "s", "users", "row_block"]
    assert p["s"].default == 1.0 and p["users"].default is None and p["row_block"].default == 2048
    p = inspect.signature(S.train_model_population).parameters
    assert list(p) == ["model", "X", "s", "optimizer", "device", "num_steps", "log_every", "row_block"]
    assert p["num_steps"].default == 1000 and p["log_every"].default == 100 and p["row_block"].default == 2048
    for fn in (S.population_risk, S.train_model_population):
        assert fn.__doc__.startswith("Extension (not in the reference)")
    assert not any("population" in k for k in S._RESULT_KEYS)                   # not part of the result dict


@pytest.mark.parametrize("scale", [0.7, 1.0, 4.0])
def test_model_gradient_is_the_derivative_of_the_models_risk(scale):
    """Central differences of pairs_model's risk in f64, h = 1e-6: the truncation error is h^2 / 6 times the third
    derivative (|sigmoid''| <= 0.1, m - 1 terms: ~1e-12) and the rounding error of the difference is about
    risk * 2^-52 / h ~ 1e-7 at m = 37, which is what is seen; 1e-6 leaves a factor of several."""
    m, h = 37, 1e-6
    rng = np.random.default_rng(37)
    a, x = rng.uniform(-3, 3, m), rng.uniform(-3, 3, m)
    g = GM.pair_grad(a, x, scale)
    fd = np.empty(m)
    for i in range(m):
        e = np.zeros(m)
        e[i] = h
        fd[i] = (GM.row_risk(a + e, x, scale) - GM.row_risk(a - e, x, scale)) / (2 * h)
    print(f"scale {scale}: max |g - central difference| = {np.abs(g - fd).max():.2e}")
    assert np.abs(g - fd).max() <= 1e-6
    assert abs(g.sum()) <= 1e-12 * m * m                # every pair enters twice with opposite signs
    assert np.abs(GM.pair_grad(scale * x, x, scale)).max() <= 1e-12 * m      # the ideal scores are stationary
    assert np.isnan(GM.pair_grad([1.0, np.inf, 0.0], [0.0, 1.0, 2.0], scale)).all()
    assert GM.pair_grad([1.5], [0.5], scale).tolist() == [0.0]


def test_model_table_gradients_and_adam_step():
    rng = np.random.default_rng(3)
    n, m, d, s = 4, 9, 2, 0.7
    U, V, X = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(n, m))
    for users in (None, [3, 0, 3]):
        dU, dV, G = GM.population_grad(U, V, X, s, users)
        assert np.abs(G.sum(axis=1)).max() <= 1e-13 * m * m
        h = 1e-6
        for T, dT in ((U, dU), (V, dV)):
            for idx in [(0, 0), (T.shape[0] - 1, 1)]:
                P, Mi = T.copy(), T.copy()
                P[idx] += h
                Mi[idx] -= h
                args = ((P, V), (Mi, V)) if T is U else ((U, P), (U, Mi))
                fd = (GM.population_risk(*args[0], X, s, users) - GM.population_risk(*args[1], X, s, users)) / (2 * h)
                assert abs(fd - dT[idx]) <= 1e-8, (users, idx, fd, dT[idx])
    # Adam against torch's own (CPU, float64): coupled weight decay, bias correction, eps outside the root
    tU, tV = torch.tensor(U, requires_grad=True), torch.tensor(V, requires_grad=True)
    topt = torch.optim.Adam([tU, tV], lr=0.05, weight_decay=1e-2)
    mine = GM.Adam([U, V], 0.05, weight_decay=1e-2)
    for _ in range(3):
        gU, gV = rng.normal(size=U.shape), rng.normal(size=V.shape)
        tU.grad, tV.grad = torch.tensor(gU), torch.tensor(gV)
        topt.step()
        mine.step([gU, gV])
    np.testing.assert_allclose(mine.p[0], tU.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(mine.p[1], tV.detach().numpy(), rtol=1e-12, atol=1e-14)
