"""CPU-only checks of the ragged Hessian-vector entry and what is built on it (include/mfcd.h: mfcd_pair_ragged_hvp;
mfcd/ratings.py: pair_ragged_hvp, ratings_hvp; mfcd/ratings_exact.py; structure.ratings_hvp, fit_users_ratings,
refit_users_ratings, refit_items_ratings, train_model_ratings_exact): the entry is declared and bound, bad arguments are
refused before the device is touched, there is no CPU fallback, and the CPU model the GPU tests compare with
(tests/ratings_hvp_model.py) is consistent with itself and with tests/ratings_model.py."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ratings_hvp_model as RH
import ratings_model as RM
from conftest import ROOT
from test_ratings_cpu import _small_data


def test_the_entry_is_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    name = "mfcd_pair_ragged_hvp"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 13
    decl = re.search(r"\b%s\(([^)]*)\);" % name, header).group(1)
    assert len(decl.split(",")) == 13
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, name)


A, X, Y, R, S, Q, D, W = 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768   # non-null, never dereferenced


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()

    def hvp(a=A, x=X, y=Y, entries=8, row_off=R, rows=2, tile_off=S, n_tiles=2, flags=0, q=Q, deg=D, status=W):
        return L.mfcd_pair_ragged_hvp(a, x, y, entries, row_off, rows, tile_off, n_tiles, flags, q, deg, status, None)

    assert hvp(rows=-1) == -1 and hvp(entries=-1) == -1 and hvp(n_tiles=-1) == -1
    assert hvp(row_off=None) == -1 and hvp(tile_off=None) == -1 and hvp(status=None) == -1
    assert hvp(a=None) == -1 and hvp(y=None) == -1 and hvp(q=None) == -1
    assert hvp(x=None, flags=1) == -1 and hvp(x=None, flags=1, rows=0) == -1          # x is required under the skip flag
    assert hvp(flags=2) == -1 and hvp(flags=-1) == -1 and hvp(flags=3) == -1
    for flags in (0, 1):
        assert hvp(q=A, flags=flags) == -1 and hvp(q=Y, flags=flags) == -1 and hvp(q=X, flags=flags) == -1
        assert hvp(deg=A, flags=flags) == -1 and hvp(deg=Y, flags=flags) == -1 and hvp(deg=X, flags=flags) == -1
        assert hvp(deg=Q, flags=flags) == -1
    assert hvp(n_tiles=(1 << 40) + 1) == -1 and hvp(n_tiles=(1 << 40) + 1, rows=0) == -1
    assert hvp(rows=0) == 0 and hvp(rows=0, deg=None) == 0 and hvp(rows=0, x=None) == 0    # nothing launched
    assert hvp(rows=0, flags=1) == 0 and hvp(rows=0, flags=2) == -1                   # a bad call stays bad with no rows
    assert hvp(rows=0, entries=0, a=None, y=None, q=None, deg=None, x=None) == 0
    assert hvp(rows=0, entries=0, a=None, y=None, q=None, deg=None, x=None, flags=1) == 0   # an empty table has no x


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, ratings, ratings_exact
    data = _small_data()
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    a = torch.randn(data.entries)
    for call in (lambda: ratings.pair_ragged_hvp(a, a.clone(), data), lambda: ratings.pair_ragged_hvp(a, a.clone(), data, True, True),
                 lambda: ratings.pair_ragged_hvp(a.double(), a, data), lambda: ratings.ratings_hvp(U, V, U, V, data),
                 lambda: ratings_exact.ratings_user_step(U, V, data, 1.0, 0.1),
                 lambda: ratings_exact.ratings_user_step(None, V, data, 1.0, 0.1),
                 lambda: ratings_exact.ratings_item_step(U, V, data, 1.0, 0.1),
                 lambda: ratings_exact.fit_ratings_exact(U, V, data, 1.0, 0.1, 1),
                 lambda: ratings_exact.ratings_user_step(U.double(), V.double(), data, 1.0, 0.1)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = St.MatrixFactorization(4, 5, 2)
    for call in (lambda: St.ratings_hvp(model, data, U, V), lambda: St.fit_users_ratings(model, data, 0.1),
                 lambda: St.fit_users_ratings(V, data, 0.1), lambda: St.refit_users_ratings(model, data, 1.0, 0.1),
                 lambda: St.refit_items_ratings(model, data, 1.0, 0.1),
                 lambda: St.train_model_ratings_exact(model, data, 1.0, 0.1, sweeps=1)):
        with pytest.raises(RuntimeError):
            call()


def test_public_signatures_and_docstrings():
    import structure as St
    from mfcd import population, ratings, ratings_exact

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(ratings.pair_ragged_hvp) == ["a", "y", "data", "skip_ties", "deg"]
    assert defaults(ratings.pair_ragged_hvp) == {"skip_ties": False, "deg": False}
    assert names(ratings.ratings_hvp) == ["U", "V", "dU", "dV", "data", "s", "skip_ties", "gauss_newton"]
    assert defaults(ratings.ratings_hvp) == {"s": 1.0, "skip_ties": False, "gauss_newton": False}
    assert names(ratings_exact.ratings_user_step) == ["U", "V", "data", "s", "l2", "skip_ties", "coef", "gtol", "max_newton",
                                                      "max_cg"]
    assert defaults(ratings_exact.ratings_user_step) == {"skip_ties": False, "coef": None, "gtol": 1e-3, "max_newton": 20,
                                                         "max_cg": None}
    assert names(ratings_exact.ratings_item_step) == names(ratings_exact.ratings_user_step)
    assert defaults(ratings_exact.ratings_item_step) == {"skip_ties": False, "coef": None, "gtol": 1e-3, "max_newton": 20,
                                                         "max_cg": 25}
    assert names(ratings_exact.fit_ratings_exact) == ["U", "V", "data", "s", "l2", "sweeps", "skip_ties", "gtol", "max_newton"]
    assert defaults(ratings_exact.fit_ratings_exact) == {"skip_ties": False, "gtol": 1e-3, "max_newton": 20}
    assert ratings_exact.PopulationStepResult is population.PopulationStepResult
    assert ratings_exact._newton is population._newton                                  # the solver is reused, not copied
    assert names(St.ratings_hvp) == ["model", "data", "dU", "dV", "s", "skip_ties", "gauss_newton"]
    assert defaults(St.ratings_hvp) == {"s": 1.0, "skip_ties": False, "gauss_newton": False}
    assert names(St.fit_users_ratings) == ["V_or_model", "data", "weight_decay", "s", "skip_ties", "coef"]
    assert defaults(St.fit_users_ratings) == {"s": 1.0, "skip_ties": False, "coef": None}
    assert names(St.refit_users_ratings) == ["model", "data", "s", "weight_decay", "skip_ties"]
    assert names(St.refit_items_ratings) == ["model", "data", "s", "weight_decay", "skip_ties"]
    assert names(St.train_model_ratings_exact) == ["model", "data", "s", "weight_decay", "sweeps", "skip_ties"]
    assert defaults(St.train_model_ratings_exact) == {"sweeps": 10, "skip_ties": False}
    for fn in (St.ratings_hvp, St.fit_users_ratings, St.refit_users_ratings, St.refit_items_ratings,
               St.train_model_ratings_exact):
        assert fn.__doc__.startswith("Extension (not in the reference)")
        assert " ".join(fn.__doc__.split()).endswith("Not part of the result dict / .pkl layout.")
    assert not any("rating" in k for k in St._RESULT_KEYS)


def test_per_user_supports_on_the_host():
    from mfcd import ratings
    data = ratings.RatingsData([0, 0, 0, 1, 3, 3, 4, 4, 4], [0, 1, 2, 0, 1, 2, 0, 1, 2],
                               [1.0, 1.0, 2.0, 5.0, 3.0, 3.0, 0.0, -0.0, 0.0], 5, 3)
    assert data.user_support(False).tolist() == [3, 0, 0, 1, 3] and data.user_support(True).tolist() == [2, 0, 0, 0, 0]
    assert data.user_support(False).sum() == data.support(False) and data.user_support(True).sum() == data.support(True)
    empty = ratings.RatingsData([], [], [], 3, 4)
    assert empty.user_support(True).tolist() == [0, 0, 0]
    rng = np.random.default_rng(3)
    keep = rng.random((20, 30)) < 0.4
    users, items = np.nonzero(keep)
    data = ratings.RatingsData(users, items, rng.integers(1, 4, users.size), 20, 30)
    x, ro = data.value.numpy(), data.row_off.numpy()
    for skip in (False, True):
        assert data.user_support(skip).tolist() == [RM.row_support(x[sl], skip) for sl in RM.rows_of(ro)]


@pytest.mark.parametrize("skip", [False, True])
def test_model_hvp_is_the_derivative_of_the_models_gradient(skip):
    """Central differences of ratings_model.row_grad in f64, h = 1e-6, bound 1e-6, as test_ratings_cpu.py argues it for
    the gradient (truncation ~1e-12, rounding of the difference ~1e-10 per entry, times |y| <= 2 over 37 entries)."""
    m, h, scale = 37, 1e-6, 0.7
    rng = np.random.default_rng(43)
    a, x, y = rng.uniform(-3, 3, m), rng.integers(1, 6, m).astype(np.float64), rng.uniform(-2, 2, m)
    q, deg, mag = RH.row_hvp(a, y, x, skip)
    fd = (RM.row_grad(a + h * y, x, scale, skip) - RM.row_grad(a - h * y, x, scale, skip)) / (2 * h)
    print(f"skip {skip}: max |q - central difference| = {np.abs(q - fd).max():.2e}")
    assert np.abs(q - fd).max() <= 1e-6
    assert abs(q.sum()) <= 1e-12 * m * m
    assert (mag >= np.abs(q) - 1e-12).all() and (deg > 0).all()
    const = RH.row_hvp(a, np.full(m, 0.3), x, skip)
    assert (const[0] == 0.0).all() and (const[2] == 0.0).all()
    # deg is the diagonal of the Laplacian written out over the pairs that count
    w = (x[:, None] != x[None, :]) if skip else np.ones((m, m), bool)
    Sm = RH.HM.dsigmoid(a[:, None] - a[None, :]) * w
    np.fill_diagonal(Sm, 0.0)
    Lap = np.diag(Sm.sum(1)) - Sm
    np.testing.assert_allclose(deg, np.diag(Lap), rtol=1e-14)
    np.testing.assert_allclose(q, Lap @ y, rtol=1e-12, atol=1e-14)
    # x is read under skip-ties only
    xbad = x.copy()
    xbad[3] = np.nan
    assert np.isnan(RH.row_hvp(a, y, xbad, True)[0]).all()
    assert RH.row_hvp(a, y, xbad, False)[0].tolist() == RH.row_hvp(a, y, x, False)[0].tolist()
    ybad = y.copy()
    ybad[0] = np.inf
    assert np.isnan(RH.row_hvp(a, ybad, x, skip)[1]).all()
    one = RH.row_hvp([1.5], [0.5], [2.0], skip)
    assert one[0].tolist() == [0.0] and one[1].tolist() == [0.0]


def test_model_table_product_is_the_derivative_of_the_models_table_gradients():
    rng = np.random.default_rng(6)
    data = _small_data()
    row_off, item, value = data.row_off.numpy(), data.item.numpy().astype(np.int64), data.value.numpy()
    U, V = rng.normal(size=(4, 2)), rng.normal(size=(5, 2))
    dU, dV = rng.normal(size=(4, 2)), rng.normal(size=(5, 2))
    h = 1e-6
    for skip in (False, True):
        prob = RH.Problem(row_off, item, value, 0.7, skip)
        assert prob.c == 1.0 / data.support(skip)
        HU, HV, _ = prob.hvp(U, V, dU, dV)
        pU, pV, _ = RM.ratings_grad(U + h * dU, V + h * dV, row_off, item, value, 0.7, skip)
        mU, mV, _ = RM.ratings_grad(U - h * dU, V - h * dV, row_off, item, value, 0.7, skip)
        assert np.abs((pU - mU) / (2 * h) - HU).max() <= 1e-8 and np.abs((pV - mV) / (2 * h) - HV).max() <= 1e-8
        GU, GV, _ = prob.hvp(U, V, dU, dV, gauss_newton=True)
        assert (dU * GU).sum() + (dV * GV).sum() >= 0.0                     # the Gauss-Newton part is positive semidefinite
        # the model's objective and block gradients against ratings_model's
        np.testing.assert_allclose(prob.risk(U, V), RM.ratings_risk(U, V, row_off, item, value, 0.7, skip), rtol=1e-13)
        gU, gV = prob.grads(U, V)
        rU, rV, _ = RM.ratings_grad(U, V, row_off, item, value, 0.7, skip)
        np.testing.assert_allclose(gU, rU, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(gV, rV, rtol=1e-12, atol=1e-15)


@functools.lru_cache(maxsize=None)
def step_problem(skip):
    from mfcd import ratings
    U0, V, users, items, values = RH.step_inputs(skip)
    data = ratings.RatingsData(users, items, values, RH.STEP_N, RH.STEP_M)
    prob = RH.Problem(data.row_off.numpy(), data.item.numpy(), data.value.numpy(), 1.0, skip)
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(RH.STEP_D), V64, r, RH.STEP_L2)[0] for r in range(RH.STEP_N)])
    return data, prob, Uopt, prob.user_noise(Uopt, V64)


@pytest.mark.parametrize("skip", [False, True])
def test_step_inputs_leave_room_for_the_certificate(skip):
    """At the model's minimisers of the GPU step test's inputs, the gradient's fp32 noise bound stays below half of
    gtol l2 |u*|_inf for every user with a pair: "every such row is certified" is a condition the inputs meet."""
    data, prob, Uopt, noise = step_problem(skip)
    assert data.lengths[RH.EMPTY_USER] == 0 and data.lengths[RH.SINGLE_USER] == 1
    if skip:
        assert data.user_support(False)[RH.LEVEL_USER] >= 1 and data.user_support(True)[RH.LEVEL_USER] == 0
    paired = prob.support > 0
    assert paired.tolist() == (data.user_support(skip) > 0).tolist()
    assert (~paired).sum() == (3 if skip else 2)
    assert (Uopt[~paired] == 0.0).all()
    room = 0.5 * RH.STEP_GTOL * RH.STEP_L2 * np.abs(Uopt).max(axis=1)
    print(f"skip {skip}: noise / (gtol l2 |u*|_inf) {np.round(noise[paired] / (2 * room[paired]), 3).tolist()}")
    assert (noise[paired] <= room[paired]).all()
    # the model's solves are minimisers: the block gradient vanishes, and the item solve descends F
    V64 = RH.step_inputs()[1].astype(np.float64)
    for r in range(RH.STEP_N):
        assert np.linalg.norm(prob.user_grad(Uopt[r], V64, r, RH.STEP_L2)) <= 1e-11
    U0 = RH.step_inputs()[0].astype(np.float64)
    Vopt, _ = prob.solve_items(U0, V64, RH.STEP_L2)
    assert np.linalg.norm(prob.item_grad(U0, Vopt, RH.STEP_L2)) <= 1e-11
    assert prob.item_objective(U0, Vopt, RH.STEP_L2) <= prob.item_objective(U0, V64, RH.STEP_L2)
    h, E = 1e-6, np.zeros_like(V64)
    E[3, 1] = 1.0
    fd = (prob.item_objective(U0, V64 + h * E, RH.STEP_L2) - prob.item_objective(U0, V64 - h * E, RH.STEP_L2)) / (2 * h)
    assert abs(fd - prob.item_grad(U0, V64, RH.STEP_L2)[3, 1]) <= 1e-8
