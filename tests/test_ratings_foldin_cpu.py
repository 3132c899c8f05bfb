"""CPU-only checks of the one-launch ratings fold-in (include/mfcd.h: mfcd_ratings_fold_in_users; mfcd/ratings_foldin.py;
structure.fold_in_users_ratings, refit_users_ratings_kernel, ratings_user_information): the entry is declared and bound,
bad arguments are refused before the device is touched, there is no CPU fallback, the CPU model the GPU tests compare
with (tests/ratings_foldin_model.py) reaches the plain Newton minimisers and differentiates the gradient, and the GPU
tests' inputs leave room for the certificate."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ratings_foldin_model as FM
from conftest import ROOT
from test_ratings_cpu import _small_data

NAME = "mfcd_ratings_fold_in_users"


def test_the_entry_is_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 23
    decl = re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1)
    assert len(decl.split(",")) == 23
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, NAME)
    assert L.mfcd_ratings_fold_in_max_d() == 64 and L.mfcd_ratings_fold_in_max_len() >= 515
    assert L.mfcd_ratings_fold_in_workspace_bytes(10, 64, 1000) >= 256
    # bounded independently of the table's size
    assert L.mfcd_ratings_fold_in_workspace_bytes(1 << 30, 64, 1 << 40) == L.mfcd_ratings_fold_in_workspace_bytes(1, 64, 1)
    assert L.mfcd_ratings_fold_in_workspace_bytes(1, 65, 1) == 0 and L.mfcd_ratings_fold_in_workspace_bytes(1, 0, 1) == 0
    assert L.mfcd_ratings_fold_in_workspace_bytes(-1, 4, 1) == 0 and L.mfcd_ratings_fold_in_workspace_bytes(1, 4, -1) == 0


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
V, IDX, X, RO, U0, OUT, OBJ, RAT, IST, INFO, WS = (k << 20 for k in range(1, 12))


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()

    def fold(V=V, m=50, d=8, idx=IDX, x=X, entries=100, row_off=RO, rows=4, scale=1.0, flags=0, coef=0.01, l2=0.1,
             U_init=U0, max_newton=20, gtol=1e-3, U_out=OUT, objective=OBJ, grad_ratio=RAT, iters_status=IST, info=INFO,
             workspace=WS, workspace_bytes=256):
        return L.mfcd_ratings_fold_in_users(V, m, d, idx, x, entries, row_off, rows, scale, flags, coef, l2, U_init,
                                            max_newton, gtol, U_out, objective, grad_ratio, iters_status, info, workspace,
                                            workspace_bytes, None)

    nan, inf = float("nan"), float("inf")
    assert fold(d=0) == -1 and fold(d=65) == -1 and fold(d=-1) == -1 and fold(m=0) == -1
    assert fold(rows=-1) == -1 and fold(entries=-1) == -1
    assert fold(flags=2) == -1 and fold(flags=-1) == -1 and fold(flags=3) == -1
    assert fold(scale=nan) == -1 and fold(scale=inf) == -1 and fold(scale=1e39) == -1     # not finite as a float
    for bad in (0.0, -1.0, nan, inf):
        assert fold(coef=bad) == -1 and fold(l2=bad) == -1
    assert fold(gtol=nan) == -1 and fold(gtol=inf) == -1 and fold(gtol=-1e-9) == -1
    assert fold(max_newton=-1) == -1 and fold(max_newton=1001) == -1
    assert fold(V=None) == -1 and fold(row_off=None) == -1 and fold(U_out=None) == -1 and fold(iters_status=None) == -1
    assert fold(idx=None) == -1 and fold(x=None) == -1 and fold(workspace=None) == -1
    for inp in (V, IDX, X, RO, U0):                                                     # an output on an input
        assert fold(U_out=inp) == -1 and fold(info=inp) == -1
    assert fold(info=OUT) == -1 and fold(U_out=INFO) == -1
    assert fold(U_out=V + 64) == -1 and fold(info=X + 8) == -1 and fold(U_out=U0 + 4) == -1   # partial overlaps
    assert fold(info=OUT + 16) == -1 and fold(U_out=INFO + 4 * 64 * 8 - 8) == -1
    assert fold(workspace_bytes=255) == -2 and fold(workspace_bytes=0) == -2
    # a bad call stays bad with no rows, a good one succeeds with nothing launched
    assert fold(rows=0, d=65) == -1 and fold(rows=0, flags=2) == -1 and fold(rows=0, l2=0.0) == -1
    assert fold(rows=0, max_newton=1001) == -1 and fold(rows=0, U_out=V) == -1 and fold(rows=0, info=OUT) == -1
    assert fold(rows=0) == 0 and fold(rows=0, flags=1) == 0 and fold(rows=0, max_newton=0) == 0
    assert fold(rows=0, workspace=None, workspace_bytes=0) == 0
    assert fold(rows=0, U_init=None, objective=None, grad_ratio=None, info=None) == 0
    assert fold(rows=0, entries=0, idx=None, x=None) == 0


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, ratings_foldin
    data = _small_data()
    U, Vt = torch.randn(4, 2), torch.randn(5, 2)
    for call in (lambda: ratings_foldin.ratings_fold_in_users(U, Vt, data, 1.0, 0.1),
                 lambda: ratings_foldin.ratings_fold_in_users(None, Vt, data, 1.0, 0.1),
                 lambda: ratings_foldin.ratings_fold_in_users(None, Vt, data, 1.0, 0.1, info=True),
                 lambda: ratings_foldin.ratings_fold_in_users(U.double(), Vt.double(), data, 1.0, 0.1),
                 lambda: ratings_foldin.ratings_user_information(U, Vt, data),
                 lambda: ratings_foldin.ratings_user_information(None, Vt, data)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = St.MatrixFactorization(4, 5, 2)
    for call in (lambda: St.fold_in_users_ratings(model, data, 0.1), lambda: St.fold_in_users_ratings(Vt, data, 0.1),
                 lambda: St.refit_users_ratings_kernel(model, data, 1.0, 0.1),
                 lambda: St.ratings_user_information(model, data)):
        with pytest.raises(RuntimeError):
            call()
    src = inspect.getsource(ratings_foldin)
    assert "ratings_user_step(" not in src and "_newton(" not in src          # the kernel, not the lockstep solver


def test_public_signatures_and_docstrings():
    import structure as St
    from mfcd import pairs, population, ratings_exact, ratings_foldin

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(ratings_foldin.ratings_fold_in_users) == ["U", "V", "data", "s", "l2", "skip_ties", "coef", "gtol",
                                                           "max_newton", "info"]
    assert defaults(ratings_foldin.ratings_fold_in_users) == {"skip_ties": False, "coef": None, "gtol": 1e-3,
                                                              "max_newton": 20, "info": False}
    assert names(ratings_foldin.ratings_user_information) == ["U", "V", "data", "s", "skip_ties"]
    assert defaults(ratings_foldin.ratings_user_information) == {"s": 1.0, "skip_ties": False}
    assert ratings_foldin._setup is ratings_exact._setup                             # the checks are reused, not copied
    assert ratings_foldin.PopulationStepResult is population.PopulationStepResult
    assert ratings_foldin.UserInformation is pairs.UserInformation
    assert names(St.fold_in_users_ratings) == names(St.fit_users_ratings)
    assert defaults(St.fold_in_users_ratings) == defaults(St.fit_users_ratings)
    assert names(St.refit_users_ratings_kernel) == names(St.refit_users_ratings)
    assert defaults(St.refit_users_ratings_kernel) == defaults(St.refit_users_ratings)
    assert names(St.ratings_user_information) == ["model", "data", "s", "skip_ties"]
    assert defaults(St.ratings_user_information) == {"s": 1.0, "skip_ties": False}
    for fn in (St.fold_in_users_ratings, St.refit_users_ratings_kernel, St.ratings_user_information):
        assert fn.__doc__.startswith("Extension (not in the reference)")
        assert " ".join(fn.__doc__.split()).endswith("Not part of the result dict / .pkl layout.")
    assert not any("rating" in k for k in St._RESULT_KEYS)


@pytest.mark.parametrize("skip", [False, True])
def test_the_models_fixed_algorithm_reaches_the_plain_newton_minimisers(skip):
    """In f64 the certificate |g| <= gtol l2 |u|_inf bounds the distance to the minimiser by |g| / l2 <= gtol |u|_inf
    (strong convexity, modulus l2), and solve_user's own minimiser lies within 1e-11 / l2 of it: with gtol = 1e-6 the
    fixed algorithm has to land within 2e-6 |u*|_inf.  (A much smaller gtol asks the Armijo test for decreases below the
    last bit of f: the rule then halves the step until it stops, which is the rule's behaviour and not the model's.)"""
    fam = FM.family(3, skip)
    prob, V = fam.prob, fam.V64
    for r in range(fam.n):
        for u0 in (np.zeros(3), fam.start[r].astype(np.float64)):
            u, it, status, f0, f, ratio = FM.fold_in(prob, V, r, u0, FM.L2, gtol=1e-6, max_newton=50)
            assert status == 0 and it <= 50 and f <= f0
            if fam.paired[r]:
                assert ratio <= 1e-6 and it >= 1
                assert np.linalg.norm(u - fam.Uopt[r]) <= 2e-6 * np.abs(fam.Uopt[r]).max()
                assert f == prob.user_objective(u, V, r, FM.L2) and f0 == prob.user_objective(u0, V, r, FM.L2)
            else:                                                               # the closed form
                assert it == 0 and f == 0.0 and ratio == 0.0 and f0 == 0.5 * FM.L2 * float(u0 @ u0)
                assert u.tobytes() == np.zeros(3).tobytes()
    # the iteration cap and max_newton = 0
    r = int(np.flatnonzero(fam.lengths == 65)[0])
    far = fam.start[r].astype(np.float64)
    u, it, status, f0, f, _ = FM.fold_in(prob, V, r, far, FM.L2, max_newton=1)
    assert (it, status) == (1, 1) and f <= f0
    u, it, status, f0, f, _ = FM.fold_in(prob, V, r, far, FM.L2, max_newton=0)
    assert (it, status) == (0, 1) and f == f0 and (u == far).all()


@pytest.mark.parametrize("skip", [False, True])
def test_the_models_info_is_the_derivative_of_the_models_gradient(skip):
    """Central differences of user_grad in f64, h = 1e-6, as test_ratings_hvp_cpu.py argues its bound: truncation
    ~h^2 = 1e-12 and rounding of the difference ~1e-16 / h = 1e-10 relative to the gradient's terms, so 1e-6 relative to
    the largest entry of c H + l2 I holds with four orders to spare."""
    fam = FM.family(3, skip)
    prob, V, h = fam.prob, fam.V64, 1e-6
    for r in np.flatnonzero(fam.paired):
        u = fam.start[r].astype(np.float64) * 0.3
        H = prob.c * FM.info(prob, V, r, u) + FM.L2 * np.eye(3)
        fd = np.stack([(prob.user_grad(u + h * e, V, r, FM.L2) - prob.user_grad(u - h * e, V, r, FM.L2)) / (2 * h)
                       for e in np.eye(3)])
        assert np.abs(fd - H).max() <= 1e-6 * np.abs(H).max()
        assert (H == H.T).all() or np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    lone = int(np.flatnonzero(fam.lengths == 1)[0])
    assert (FM.info(prob, V, lone, np.ones(3)) == 0.0).all()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("d", FM.DS)
def test_gpu_inputs_leave_room_for_the_certificate(d, skip):
    """At the model's minimisers of the GPU tests' inputs the gradient's fp32 noise bound stays below half of
    gtol l2 |u*|_inf for every row with a supporting pair: "every supported row is certified" is a property of the
    inputs.  The fixed algorithm reaches them from both starts within the iteration cap."""
    fam = FM.family(d, skip)
    assert sorted(fam.lengths.tolist()) == sorted(FM.LS + ([5] if skip else []))
    assert fam.lengths.tolist() != sorted(fam.lengths.tolist())                   # shuffled
    assert (~fam.paired).sum() == (3 if skip else 2) and (fam.Uopt[~fam.paired] == 0.0).all()
    room = 0.5 * FM.GTOL * FM.L2 * np.abs(fam.Uopt).max(axis=1)
    p = fam.paired
    print(f"d={d} skip={skip}: noise / (gtol l2 |u*|_inf) {np.round(fam.noise[p] / (2 * room[p]), 3).tolist()}")
    assert (fam.noise[p] <= room[p]).all()
    for r in range(fam.n):
        assert np.linalg.norm(fam.prob.user_grad(fam.Uopt[r], fam.V64, r, FM.L2)) <= 1e-11
    if d in (2, 17):                                                              # the model's own iteration counts
        its = [[FM.fold_in(fam.prob, fam.V64, r, u0[r], FM.L2)[1:3] for r in np.flatnonzero(p)]
               for u0 in (np.zeros((fam.n, d)), fam.start.astype(np.float64))]
        print(f"d={d} skip={skip}: model iterations from 0 {[a for a, _ in its[0]]}, from the far start {[a for a, _ in its[1]]}")
        assert all(s == 0 and 1 <= a <= 20 for part in its for a, s in part)
