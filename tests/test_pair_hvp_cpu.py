"""CPU-only checks of the pair Hessian-vector entries and what is built on them (include/mfcd.h: mfcd_pair_hvp_rows,
mfcd_pair_law_hvp_rows; mfcd/pairs.py: pair_hvp_rows, pair_law_hvp_rows, population_hvp; mfcd/population.py; the
structure.py names): the entries are declared and bound under the unchanged ABI version, every MFCD_EINVAL rule holds
before the device is touched, there is no CPU fallback, the CPU model the GPU tests compare with
(tests/pair_hvp_model.py) is the second derivative of the models of the risk, and the step tests' inputs leave room
between the certificate and the gradient's fp32 noise."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_grad_model as GM
import pair_hvp_model as HM
import pair_law_model as LM
from conftest import ROOT


def test_hvp_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_pair_hvp_rows", 11), ("mfcd_pair_law_hvp_rows", 14)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs, name
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header)) - {"mfcd_sample"}
    assert declared == set(_lib.SIGNATURES)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()                              # binds every symbol: both are exported
    assert L.mfcd_abi_version() == 4
    assert L.mfcd_pair_hvp_rows and L.mfcd_pair_law_hvp_rows


def test_hvp_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    A_, X_, Y_, Q_, D_, P = 4096, 8192, 12288, 16384, 20480, 24576   # non-null addresses that are never dereferenced

    def law(alpha=None, beta=None, labels=None, stride=0, use_margin=0, margin=0.0):
        c = _lib.PairLawC()
        c.alpha, c.beta, c.labels, c.label_stride, c.use_margin, c.margin = alpha, beta, labels, stride, use_margin, margin
        return c

    def plain(rows=2, m=8, A=A_, Y=Y_, Q=Q_, deg=D_, lda=8, ldy=8, ldq=8, ldd=8, **_):
        return L.mfcd_pair_hvp_rows(A, lda, Y, ldy, rows, m, Q, ldq, deg, ldd, None)

    ok = law()

    def under(rows=2, m=8, A=A_, X=X_, Y=Y_, Q=Q_, deg=D_, lda=8, ldx=8, ldy=8, ldq=8, ldd=8, c=ok):
        return L.mfcd_pair_law_hvp_rows(A, lda, X, ldx, Y, ldy, rows, m, None if c is None else ctypes.byref(c), Q, ldq, deg,
                                        ldd, None)

    for call in (plain, under):
        big = 1 << 21
        assert call(m=0) == -1 and call(m=1048577, lda=big, ldx=big, ldy=big, ldq=big, ldd=big) == -1
        assert call(rows=-1) == -1
        assert call(A=None) == -1 and call(Y=None) == -1 and call(Q=None) == -1
        assert call(lda=7) == -1 and call(ldy=7) == -1 and call(ldq=7) == -1 and call(ldd=7) == -1
        assert call(Q=A_) == -1 and call(Q=Y_) == -1 and call(Q=D_) == -1          # Q aliases A, Y, deg
        assert call(deg=A_) == -1 and call(deg=Y_) == -1
        assert call(rows=0) == 0 and call(rows=0, deg=None) == 0                      # nothing to do, nothing launched
        assert call(rows=0, deg=None, ldd=0) == 0                                     # ldd is not read without deg
        assert call(rows=0, Q=A_) == -1                                               # a bad call stays bad with no rows
    assert under(X=None) == -1 and under(ldx=7) == -1 and under(Q=X_) == -1 and under(deg=X_) == -1
    assert under(c=None) == -1
    assert under(c=law(alpha=P)) == -1 and under(c=law(beta=P)) == -1
    assert under(c=law(use_margin=1, margin=-1e-30)) == -1 and under(c=law(use_margin=1, margin=float("nan"))) == -1
    assert under(c=law(labels=P, stride=7)) == -1 and under(c=law(labels=P, stride=-8)) == -1
    assert under(c=law(alpha=P), rows=0) == -1
    assert under(c=law(alpha=P, beta=P, labels=P, stride=8, use_margin=1, margin=float("inf")), rows=0) == 0
    assert under(c=law(labels=P, stride=0, margin=-1.0), rows=0) == 0                 # the margin is not in use


def test_hvp_has_no_cpu_fallback_and_public_signatures():
    import structure as S
    from mfcd import _lib, pairs, population
    A = torch.randn(3, 9)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_hvp_rows(A, A)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_law_hvp_rows(A, A, A, pairs.PairLaw(margin=1.0))
    model = S.MatrixFactorization(3, 9, 2)
    U, V = model.U.data, model.V.data
    with pytest.raises(_lib.MfcdError):
        pairs.population_hvp(U, V, A, U, V)
    for fn in (population.population_user_step, population.population_item_step):
        with pytest.raises(_lib.MfcdError):
            fn(U, V, A, 1.0, 0.1)
    with pytest.raises(_lib.MfcdError):
        population.fit_population_exact(U, V, A, 1.0, 0.1, 1)
    for call in (lambda: S.population_hvp(model, A, U, V), lambda: S.refit_users_population(model, A, 1.0, 0.1),
                 lambda: S.refit_items_population(model, A, 1.0, 0.1),
                 lambda: S.train_model_population_exact(model, A, 1.0, 0.1, sweeps=1)):
        with pytest.raises(RuntimeError):
            call()
    p = inspect.signature(pairs.pair_hvp_rows).parameters
    assert list(p) == ["A", "Y", "deg"] and p["deg"].default is False
    p = inspect.signature(pairs.pair_law_hvp_rows).parameters
    assert list(p) == ["A", "X", "Y", "law", "deg"] and p["deg"].default is False
    p = inspect.signature(pairs.population_hvp).parameters
    assert list(p) == ["U", "V", "X", "dU", "dV", "s", "law", "users", "row_block", "gauss_newton"]
    assert p["s"].default == 1.0 and p["row_block"].default == 2048 and p["gauss_newton"].default is False
    p = inspect.signature(population.population_user_step).parameters
    assert list(p)[:10] == ["U", "V", "X", "s", "l2", "law", "users", "gtol", "max_newton", "row_block"]
    assert p["gtol"].default == 1e-3 and p["max_newton"].default == 20 and p["row_block"].default == 2048
    p = inspect.signature(population.population_item_step).parameters
    assert list(p)[:9] == ["U", "V", "X", "s", "l2", "law", "gtol", "max_newton", "row_block"]
    assert p["gtol"].default == 1e-3 and p["max_newton"].default == 20
    assert list(inspect.signature(population.fit_population_exact).parameters)[:7] == ["U", "V", "X", "s", "l2", "sweeps", "law"]
    for fn, first in ((S.population_hvp, ["model", "X", "dU", "dV", "s", "law"]),
                      (S.refit_users_population, ["model", "X", "s", "weight_decay", "law", "users"]),
                      (S.refit_items_population, ["model", "X", "s", "weight_decay", "law"]),
                      (S.train_model_population_exact, ["model", "X", "s", "weight_decay", "sweeps", "law"])):
        assert list(inspect.signature(fn).parameters)[:len(first)] == first
        assert fn.__doc__.startswith("Extension (not in the reference)")
    assert inspect.signature(S.train_model_population_exact).parameters["sweeps"].default == 10
    assert not any("population" in k for k in S._RESULT_KEYS)                   # not part of the result dict


def _spec(m, rng):
    return {"alpha": rng.uniform(0.1, 1.0, m).astype(np.float32), "beta": rng.uniform(0.1, 1.0, m).astype(np.float32),
            "labels": rng.integers(0, 3, m), "margin": 2.5}


def test_model_row_product_is_the_derivative_of_the_models_gradient():
    """Central differences of the gradient models in f64, h = 1e-5: truncation h^2 / 6 |sigmoid'''| (m - 1) |y| ~ 1e-10,
    rounding |g| 2^-52 / h ~ 1e-10."""
    m, h, s = 23, 1e-5, 0.7
    rng = np.random.default_rng(11)
    a, x, y = rng.uniform(-3, 3, m), rng.uniform(-3, 3, m).astype(np.float32), rng.uniform(-2, 2, m)
    spec = _spec(m, rng)
    w = LM.weights(x, spec["alpha"], spec["beta"], spec["margin"], spec["labels"])
    assert 0 < (w > 0).sum() < m * (m - 1)
    for name, wt, grad in (("plain", None, lambda v: GM.pair_grad(v, x, s)), ("law", w, lambda v: LM.law_grad(v, x, s, w))):
        q, deg, mag = HM.pair_hvp(a, y, wt)
        fd = (grad(a + h * y) - grad(a - h * y)) / (2 * h)
        print(f"{name}: max |q - central difference| = {np.abs(q - fd).max():.2e}")
        assert np.abs(q - fd).max() <= 1e-8
        L = HM.laplacian(a, wt)
        np.testing.assert_allclose(L @ y, q, rtol=0, atol=1e-13 * m)
        np.testing.assert_allclose(np.diag(L), deg, rtol=1e-14)
        assert np.abs(L - L.T).max() == 0 and abs(q.sum()) <= 1e-13 * m and (mag >= np.abs(q) - 1e-15).all()
        assert np.linalg.eigvalsh(L).min() >= -1e-13                           # a weighted graph Laplacian
    assert HM.pair_hvp(a, np.full(m, 0.3))[0].tolist() == [0.0] * m           # a constant direction
    assert HM.pair_hvp([1.5], [2.0])[0].tolist() == [0.0] and HM.pair_hvp([1.5], [2.0])[1].tolist() == [0.0]
    assert all(np.isnan(t).all() for t in HM.pair_hvp([1.0, np.inf, 0.0], [0.0, 1.0, 2.0]))
    assert all(np.isnan(t).all() for t in HM.pair_hvp([1.0, 0.5, 0.0], [0.0, np.nan, 2.0]))
    assert all(np.isnan(t).all() for t in HM.pair_hvp([1.0, 0.5, 0.0], [0.0, 1.0, 2.0], None, [0.0, -np.inf, 1.0]))


@pytest.mark.parametrize("kind", ["plain", "users with a repeat", "law"])
def test_model_table_product_is_the_derivative_of_the_table_gradients_and_symmetric(kind):
    """The table-level product against a central difference of pair_grad_model.population_grad (plain) / of
    pair_law_model.population's gradient (law) along the direction, h = 1e-5, and <P, H Q> = <Q, H P>."""
    rng = np.random.default_rng(5)
    n, m, d, s, h = 4, 9, 2, 0.7, 1e-5
    U, V = rng.normal(size=(n, d)), rng.normal(size=(m, d))
    X = rng.normal(size=(n, m)).astype(np.float32)
    users = [3, 0, 3] if kind == "users with a repeat" else None
    spec = None
    if kind == "law":
        spec = dict(_spec(m, rng), labels=rng.integers(0, 3, (n, m)), users=[0, 2, 3])
        grad = lambda U_, V_: LM.population(U_, V_, X, s, spec)[1:3]  # noqa: E731
    else:
        grad = lambda U_, V_: GM.population_grad(U_, V_, X, s, users)[:2]  # noqa: E731
    prob = HM.Problem(X, s, spec, users)
    np.testing.assert_allclose(prob.grads(U, V)[0], grad(U, V)[0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(prob.grads(U, V)[1], grad(U, V)[1], rtol=1e-12, atol=1e-15)
    dirs = [(rng.normal(size=U.shape), rng.normal(size=V.shape)) for _ in range(2)]
    prods = []
    for dU, dV in dirs:
        HU, HV, _ = prob.hvp(U, V, dU, dV)
        gp, gm = grad(U + h * dU, V + h * dV), grad(U - h * dU, V - h * dV)
        for name, got, fd in (("U", HU, (gp[0] - gm[0]) / (2 * h)), ("V", HV, (gp[1] - gm[1]) / (2 * h))):
            print(f"{kind}: H{name} max |product - central difference| = {np.abs(got - fd).max():.2e}")
            assert np.abs(got - fd).max() <= 1e-8
        prods.append((HU, HV))
        GU, GV, _ = prob.hvp(U, V, dU, dV, gauss_newton=True)
        assert (dU * GU).sum() + (dV * GV).sum() >= 0.0                        # Gauss-Newton: positive semidefinite
    (P1, P2), (Q1, Q2) = dirs
    left = (P1 * prods[1][0]).sum() + (P2 * prods[1][1]).sum()
    right = (Q1 * prods[0][0]).sum() + (Q2 * prods[0][1]).sum()
    assert abs(left - right) <= 1e-13 * max(1.0, abs(left))
    # F and its block gradients: central differences of the objective
    l2 = 0.05
    gU, gV, _ = prob.grads(U, V, l2)
    for T, g, idx in ((U, gU, (3, 1)), (V, gV, (m - 1, 0))):
        Tp, Tm = T.copy(), T.copy()
        Tp[idx] += 1e-6
        Tm[idx] -= 1e-6
        pair = ((Tp, V), (Tm, V)) if T is U else ((U, Tp), (U, Tm))
        fd = (prob.objective(*pair[0], l2) - prob.objective(*pair[1], l2)) / 2e-6
        assert abs(fd - g[idx]) <= 1e-8, (kind, idx)


@pytest.mark.parametrize("m", [40, 1029])
def test_solver_inputs_leave_room_between_the_certificate_and_the_gradient_noise(m):
    """At the model's minimiser of every user's row, gtol l2 |u*|_inf over the worst-case gradient noise
    c sum_i (2e-5 |g_i| + 2e-6 (m - 1)) |V_i|_2 is at least 4, and the model's Newton takes at most 5 iterations from
    U = 0."""
    gtol, l2 = 1e-3, 3e-2
    Ustar, V, X = HM.solver_inputs(m)
    prob = HM.Problem(X, 1.0)
    V64 = V.astype(np.float64)
    sol = [prob.solve_user(np.zeros(3), V64, r, l2) for r in range(8)]
    Uopt = np.stack([u for u, _ in sol])
    iters = max(it for _, it in sol)
    room = gtol * l2 * np.abs(Uopt).max(axis=1) / prob.user_noise(Uopt, V64)
    print(f"m={m}: room {room.min():.2f} (per user {np.round(room, 1).tolist()}), Newton iterations {iters}")
    assert room.min() >= 4.0 and iters <= 5
    assert max(np.linalg.norm(prob.user_grad(Uopt[r], V64, r, l2)) for r in range(8)) <= 1e-13
