"""CPU-only checks of the second-order list machinery (include/mfcd.h: mfcd_list_pl_hvp; mfcd.lists.pl_hvp_rows, pl_hvp;
mfcd/lists_exact.py; structure.rankings_hvp, fit_users_rankings, refit_users_rankings, refit_items_rankings,
train_model_rankings_exact): the entry is declared and bound, bad arguments are refused before the device is touched,
there is no CPU fallback; the numpy model the GPU tests compare with (tests/list_pl_hvp_model.py) is the dense Hessian
of the definitions, annihilates constants, is the central difference of list_pl_model's gradient and reduces to the
softmax and to the BTL pair; the model's table-level product is the derivative of the model's table gradients; the exact
steps' inputs leave room for the certificate."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import list_pl_hvp_model as HM
import list_pl_model as LM
from conftest import ROOT
from test_lists import _scores

NAME = "mfcd_list_pl_hvp"
KINDS = ("normal", "equal", "down200", "down3000", "up200", "up3000", "peak")
U53 = 2.0 ** -53


def test_the_entry_is_declared_and_bound():
    from mfcd import _lib, lists
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 14
    assert len(re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1).split(",")) == 14
    assert len(_lib.SIGNATURES[NAME + "_workspace_bytes"][1]) == 2
    assert len(re.search(r"\b%s_workspace_bytes\(([^)]*)\);" % NAME, header).group(1).split(",")) == 2
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, NAME) and hasattr(L, NAME + "_workspace_bytes")
    csrc = os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc")
    src = open(os.path.join(csrc, "list_pl_hvp.hip")).read()
    assert "__global__" in src and "atomicAdd" not in src and '#include "list_common.h"' in src
    assert "list_pl_hvp.hip" in open(os.path.join(csrc, "Makefile")).read()
    # one definition of the join, in the header the two kernels share
    common = open(os.path.join(csrc, "list_common.h")).read()
    assert len(re.findall(r"\blse_join\(const E x, const E y\)\s*\{", common)) == 1
    for name in ("list_pl.hip", "list_pl_hvp.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "list_common.h"' in text and not re.search(r"\blse_join\([^)]*\)\s*\{", text)
    assert "mfcd_list_pl_hvp(" in inspect.getsource(lists.pl_hvp_rows)


def test_the_workspace_is_136_bytes_a_tile_and_4_a_row():
    from mfcd import _lib
    ws = _lib.load().mfcd_list_pl_hvp_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256    # noqa: E731
    assert ws(0, 0) == 512 and ws(1, 1) == 512
    assert ws(1000, 5000) == up(5000 * 136) + up(4000)
    assert ws(3, 1 << 40) == up((1 << 40) * 136) + 256
    assert ws(-1, 4) == 0 and ws(4, -1) == 0 and ws(4, (1 << 40) + 1) == 0
    sizes = [ws(r, t) for r, t in ((1, 1), (10, 1), (10, 100), (5000, 100), (5000, 70000), (1 << 20, 1 << 22))]
    assert sizes == sorted(sizes) and ws(1 << 20, 1 << 22) > ws(5000, 70000)


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
A, Y, OFF, DEPTH, TOFF, Q, DEG, ST, WS = (k << 20 for k in range(1, 10))


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    need = L.mfcd_list_pl_hvp_workspace_bytes(4, 6)

    def call(a=A, y=Y, entries=100, row_off=OFF, depth=DEPTH, rows=4, tile_off=TOFF, n_tiles=6, q=Q, deg=DEG, status=ST,
             workspace=WS, workspace_bytes=need):
        return L.mfcd_list_pl_hvp(a, y, entries, row_off, depth, rows, tile_off, n_tiles, q, deg, status, workspace,
                                  workspace_bytes, None)

    assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(n_tiles=-1) == -1
    assert call(n_tiles=(1 << 40) + 1, workspace_bytes=1 << 62) == -1
    assert call(row_off=None) == -1 and call(tile_off=None) == -1 and call(status=None) == -1
    assert call(a=None) == -1 and call(y=None) == -1 and call(q=None) == -1
    for deg in (DEG, None):
        assert call(q=A, deg=deg) == -1 and call(q=Y, deg=deg) == -1
    assert call(deg=Q) == -1 and call(deg=A) == -1 and call(deg=Y) == -1
    assert call(q=A, rows=0) == -1 and call(deg=Q, rows=0) == -1                 # a bad call stays bad with no rows
    assert call(workspace=None) == -1
    assert call(workspace_bytes=need - 1) == -2 and call(workspace_bytes=0) == -2
    # nothing to launch
    assert call(rows=0) == 0 and call(rows=0, deg=None) == 0 and call(rows=0, depth=None) == 0
    assert call(rows=0, entries=0, a=None, y=None, q=None, deg=None, workspace=None, workspace_bytes=0) == 0


def _example():
    from mfcd import lists
    return lists.RankedLists([2, 0, 2, 2, 0, 3], [1, 4, 5, 7, 3, 2], [20, 9, 10, 30, 2, 0], 4, 8)


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, lists, lists_exact
    R = _example()
    U, V = torch.randn(4, 2), torch.randn(8, 2)
    a = torch.randn(6)
    for call in (lambda: lists.pl_hvp_rows(a, a.clone(), R), lambda: lists.pl_hvp_rows(a, a.clone(), R, True),
                 lambda: lists.pl_hvp_rows(a.double(), a, R), lambda: lists.pl_hvp(U, V, U, V, R),
                 lambda: lists_exact.lists_user_step(U, V, R, 0.1), lambda: lists_exact.lists_user_step(None, V, R, 0.1),
                 lambda: lists_exact.lists_item_step(U, V, R, 0.1), lambda: lists_exact.lists_item_step(None, V, R, 0.1),
                 lambda: lists_exact.fit_lists_exact(U, V, R, 0.1, 1),
                 lambda: lists_exact.lists_user_step(U.double(), V.double(), R, 0.1)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = St.MatrixFactorization(4, 8, 2)
    for call in (lambda: St.rankings_hvp(model, R, U, V), lambda: St.fit_users_rankings(model, R, 0.1),
                 lambda: St.fit_users_rankings(V, R, 0.1), lambda: St.refit_users_rankings(model, R, 0.1),
                 lambda: St.refit_items_rankings(model, R, 0.1),
                 lambda: St.train_model_rankings_exact(model, R, 0.1, sweeps=1)):
        with pytest.raises(RuntimeError):
            call()
    assert "logcumsumexp" not in inspect.getsource(lists) + inspect.getsource(lists_exact)


def test_public_signatures_and_docstrings():
    import structure as St
    from mfcd import lists, lists_exact, population, ratings_exact

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(lists.pl_hvp_rows) == ["a", "y", "lists", "deg"] and defaults(lists.pl_hvp_rows) == {"deg": False}
    assert names(lists.pl_hvp) == ["U", "V", "dU", "dV", "lists", "gauss_newton"]
    assert defaults(lists.pl_hvp) == {"gauss_newton": False}
    assert names(lists_exact.lists_user_step) == ["U", "V", "lists", "l2", "coef", "gtol", "max_newton", "max_cg"]
    assert defaults(lists_exact.lists_user_step) == {"coef": None, "gtol": 1e-3, "max_newton": 20, "max_cg": None}
    assert names(lists_exact.lists_item_step) == names(lists_exact.lists_user_step)
    assert defaults(lists_exact.lists_item_step) == {"coef": None, "gtol": 1e-3, "max_newton": 20, "max_cg": 25}
    assert names(lists_exact.fit_lists_exact) == ["U", "V", "lists", "l2", "sweeps", "gtol", "max_newton"]
    assert defaults(lists_exact.fit_lists_exact) == {"gtol": 1e-3, "max_newton": 20}
    assert lists_exact.PopulationStepResult is population.PopulationStepResult
    assert lists_exact._newton is population._newton                                    # the solver is reused, not copied
    assert issubclass(lists_exact._UserProblem, ratings_exact._UserProblem)             # and so are the problem classes
    assert issubclass(lists_exact._ItemProblem, ratings_exact._ItemProblem)
    assert names(St.rankings_hvp) == ["model", "lists", "dU", "dV", "gauss_newton"]
    assert defaults(St.rankings_hvp) == {"gauss_newton": False}
    assert names(St.fit_users_rankings) == ["V_or_model", "lists", "weight_decay", "coef"]
    assert defaults(St.fit_users_rankings) == {"coef": None}
    assert names(St.refit_users_rankings) == ["model", "lists", "weight_decay"] == names(St.refit_items_rankings)
    assert names(St.train_model_rankings_exact) == ["model", "lists", "weight_decay", "sweeps"]
    assert defaults(St.train_model_rankings_exact) == {"sweeps": 10}
    for fn in (St.rankings_hvp, St.fit_users_rankings, St.refit_users_rankings, St.refit_items_rankings,
               St.train_model_rankings_exact):
        assert fn.__doc__.startswith("Extension (not in the reference)")
        assert " ".join(fn.__doc__.split()).endswith("Not part of the result dict / .pkl layout.")
    assert not any("ranking" in k and "exact" in k for k in St._RESULT_KEYS)


# ---------------------------------------------------------------------------------------------------------------------
# the model against the definitions
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    for L in (2, 3, 5, 64, 65, 300):
        for depth in sorted({d for d in (1, 2, L - 1, L) if 1 <= d <= L}):
            for kind in KINDS:
                yield L, depth, kind


def test_the_model_is_the_dense_hessian_and_annihilates_constants():
    """The bound is the GPU tests' second term, 8 (L + 128) 2^-53 of scale_l (of psum_l for the diagonal): the model's
    own sequential accumulate, about L roundings of a few operations each."""
    rng = np.random.default_rng(0)
    worst = {}
    for L, depth, kind in _cases():
        a = _scores(kind, L, rng)
        y = rng.uniform(-2.0, 2.0, L)
        q, deg, scale, psum = HM.row(a, y, depth)
        H = HM.dense(a, depth)
        unit = 8 * (L + 128) * U53
        err = np.abs(q - H @ y)
        assert (err <= unit * scale + 1e-300).all(), (L, depth, kind, float((err / np.maximum(scale, 1e-300)).max() / U53))
        assert (np.abs(deg - np.diag(H)) <= unit * psum + 1e-300).all() and (deg >= 0).all(), (L, depth, kind)
        # the sizes the bounds are stated in, from the dense form
        P = np.zeros((LM.stages_of(L, depth), L))
        for k in range(P.shape[0]):
            e = np.exp(a[k:].astype(np.float64) - a[k:].max())
            P[k, k:] = e / e.sum()
        np.testing.assert_allclose(psum, P.sum(0), rtol=unit, atol=1e-300)
        np.testing.assert_allclose(scale, (P * (np.abs(y)[None, :] + (P @ np.abs(y))[:, None])).sum(0), rtol=2 * unit,
                                   atol=1e-300)
        ones, _, ones_scale, _ = HM.row(a, np.ones(L), depth)
        assert (np.abs(ones) <= unit * ones_scale).all(), (L, depth, kind)                 # H 1 = 0
        assert abs(q.sum()) <= unit * scale.sum(), (L, depth, kind)                         # 1^T H = 0
        live = scale >= 1e-30 * scale.max()               # below that an entry's error is its underflow, not a rounding
        worst[kind] = max(worst.get(kind, 0.0), float((err[live] / scale[live]).max() / U53))
    print("largest |model - dense H y| in units of 2^-53 scale, by kind:", {k: round(v, 1) for k, v in worst.items()})


def test_the_model_is_the_derivative_of_the_list_gradient():
    """Central differences of list_pl_model.row's g along y, h = 1e-5.  Bound: the gradient's own rounding, which forms
    a + N at the size of the scores (16 ulp(max |a|) psum each side, over 2 h), and the truncation h^2 / 6 |D^3 g y^3|
    <= 2 h^2 psum |y|_inf^3."""
    rng = np.random.default_rng(1)
    h = 1e-5
    for L, depth, kind in _cases():
        a = _scores(kind, L, rng).astype(np.float64)
        y = rng.uniform(-2.0, 2.0, L)
        q, _, _, psum = HM.row(a, y, depth)
        fd = (LM.row(a + h * y, depth)[3] - LM.row(a - h * y, depth)[3]) / (2 * h)
        tol = 16 * 2.0 ** -52 * max(np.abs(a).max(), 1.0) * psum.max() / h + 2 * h * h * psum.max() * 8.0
        assert np.abs(q - fd).max() <= tol, (L, depth, kind, float(np.abs(q - fd).max()), tol)


def test_depth_one_is_the_softmax_and_a_list_of_two_the_btl_pair():
    rng = np.random.default_rng(2)
    for L in (2, 5, 64, 300):
        a, y = rng.standard_normal(L) * 2.0, rng.standard_normal(L)
        p = np.exp(a - a.max())
        p /= p.sum()
        q, deg, _, psum = HM.row(a, y, 1)
        np.testing.assert_allclose(q, p * (y - p @ y), rtol=0, atol=1e-14)
        np.testing.assert_allclose(deg, p * (1 - p), rtol=1e-12, atol=1e-16)
        np.testing.assert_allclose(psum, p, rtol=1e-13)
    for depth in (1, 2):
        a = np.array([0.3, -1.1])
        s = 1.0 / (1.0 + np.exp(-1.4))
        np.testing.assert_allclose(HM.dense(a, depth), s * (1 - s) * np.array([[1.0, -1.0], [-1.0, 1.0]]), rtol=1e-14)
        q, deg, _, _ = HM.row(a, [2.0, -1.0], depth)
        np.testing.assert_allclose(q, s * (1 - s) * 3.0 * np.array([1.0, -1.0]), rtol=1e-13)
        np.testing.assert_allclose(deg, [s * (1 - s)] * 2, rtol=1e-13)
    # no stage, and non-finite rows
    assert all(not v.any() for v in HM.row([1.0, 2.0, 3.0], [1.0, 1.0, 2.0], 0)) and HM.row([2.0], [1.0])[0].tolist() == [0.0]
    assert np.isnan(HM.row([1.0, np.inf], [0.0, 0.0])[0]).all() and np.isnan(HM.row([1.0, 2.0], [np.nan, 0.0])[1]).all()


@pytest.mark.parametrize("d", [1, 3])
def test_model_table_product_is_the_derivative_of_the_models_table_gradients(d):
    rng = np.random.default_rng(6 + d)
    n, m = 5, 9
    lens, depth = [4, 0, 9, 2, 6], [4, 0, 3, 1, 5]
    item = np.concatenate([rng.choice(m, L, replace=False) for L in lens])
    row_off = np.concatenate(([0], np.cumsum(lens)))
    user = np.repeat(np.arange(n), lens)
    prob = HM.Problem(row_off, item, depth)
    assert prob.c == 1.0 / (3 + 0 + 3 + 1 + 5)
    U, V, dU, dV = (rng.normal(size=s) for s in ((n, d), (m, d), (n, d), (m, d)))
    h = 1e-6
    HU, HV, _ = prob.hvp(U, V, dU, dV)
    _, pU, pV = LM.risk(U + h * dU, V + h * dV, user, item, row_off, depth)
    _, mU, mV = LM.risk(U - h * dU, V - h * dV, user, item, row_off, depth)
    assert np.abs((pU - mU) / (2 * h) - HU).max() <= 1e-8 and np.abs((pV - mV) / (2 * h) - HV).max() <= 1e-8
    GU, GV, _ = prob.hvp(U, V, dU, dV, gauss_newton=True)
    assert (dU * GU).sum() + (dV * GV).sum() >= 0.0                       # the Gauss-Newton part is positive semidefinite
    # Gauss-Newton is the product with the table gradient's g terms taken out
    g = prob.score_grads(prob.scores(U, V))
    gU, gV = prob.tables(g, dU, dV)
    np.testing.assert_allclose(HU - GU, prob.c * gU, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(HV - GV, prob.c * gV, rtol=1e-12, atol=1e-15)
    risk, rU, rV = LM.risk(U, V, user, item, row_off, depth)
    np.testing.assert_allclose(prob.risk(U, V), risk, rtol=1e-13)
    mine = prob.grads(U, V)
    np.testing.assert_allclose(mine[0], rU, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mine[1], rV, rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------
# the exact steps' inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_problem():
    from mfcd import lists
    U0, V, users, items, positions, depth = HM.step_inputs()
    R = lists.RankedLists(users, items, positions, HM.STEP_N, HM.STEP_M, depth)
    prob = HM.Problem(R.row_off.numpy(), R.item.numpy(), R.depth.numpy())
    V64 = V.astype(np.float64)
    Uopt = np.stack([prob.solve_user(np.zeros(HM.STEP_D), V64, r, HM.STEP_L2)[0] for r in range(HM.STEP_N)])
    return R, prob, Uopt, prob.user_noise(Uopt, V64)


def test_step_inputs_leave_room_for_the_certificate():
    """At the model's minimisers of the GPU step test's inputs, the gradient's fp32 noise bound stays below half of
    gtol l2 |u*|_inf for every user with a stage: "every such row is certified" is a condition the inputs meet."""
    R, prob, Uopt, noise = step_problem()
    assert sorted(set(R.lengths.tolist())) == list(range(15)) and R.n == 24 and R.m == 30
    assert (R.user_depth == 0).sum() >= 3 and HM.SPARE_ITEM not in R.item.tolist()
    staged = prob.stages > 0
    assert staged.tolist() == (R.user_stages > 0).tolist() and R.stages == prob.stages.sum()
    assert (~staged).sum() == 4 and (R.lengths[~staged] >= 2).sum() == 2        # empty, single, and two of depth 0
    assert (Uopt[~staged] == 0.0).all()
    room = 0.5 * HM.STEP_GTOL * HM.STEP_L2 * np.abs(Uopt).max(axis=1)
    print(f"noise / (gtol l2 |u*|_inf) {np.round(noise[staged] / (2 * room[staged]), 3).tolist()}")
    assert (noise[staged] <= room[staged]).all()
    V64 = HM.step_inputs()[1].astype(np.float64)
    for r in range(HM.STEP_N):
        assert np.linalg.norm(prob.user_grad(Uopt[r], V64, r, HM.STEP_L2)) <= 1e-12
        # a minimiser: no nearby point is lower
        f = prob.user_objective(Uopt[r], V64, r, HM.STEP_L2)
        for e in np.eye(HM.STEP_D):
            assert prob.user_objective(Uopt[r] + 1e-4 * e, V64, r, HM.STEP_L2) >= f
            assert prob.user_objective(Uopt[r] - 1e-4 * e, V64, r, HM.STEP_L2) >= f
