"""CPU-only checks of the multi-column pair Laplacian entry and what is built on it (include/mfcd.h:
mfcd_pair_hvp_multi_rows; mfcd/pairs.py: pair_hvp_multi_rows, pair_info_rows, user_information; the direct user step of
mfcd/population.py; the structure.py names): the entry is declared and bound under the unchanged ABI version, every
MFCD_EINVAL rule holds before the device is touched, there is no CPU fallback, the new public signatures and defaults are
what the documents say, and the CPU model the GPU tests compare with (tests/pair_info_model.py) is the matrix the
Laplacian induces: B^T L B, the derivative of the model's user gradient, symmetric positive semidefinite and blind to a
constant row added to B."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_hvp_model as HM
import pair_info_model as IM
import pair_law_model as LM
from conftest import ROOT


def test_multi_entry_is_declared_and_bound():
    from mfcd import _lib, pairs
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs, res in (("mfcd_pair_hvp_multi_rows", 20, "int"), ("mfcd_pair_hvp_multi_workspace_bytes", 3, "size_t")):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\b%s %s\(([^)]*)\)" % (res, name), header).group(1)
        assert len(decl.split(",")) == nargs, name
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header)) - {"mfcd_sample"}
    assert declared == set(_lib.SIGNATURES)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and L.mfcd_pair_hvp_multi_rows
    W = L.mfcd_pair_hvp_multi_workspace_bytes
    assert W(0, 8, 3) > 0 and W(5, 8, 3) % 256 == 0 and W(5, 8, 3) >= 5 * 2080
    assert W(-1, 8, 3) == 0 and W(5, 0, 3) == 0 and W(5, 1048577, 3) == 0 and W(5, 8, 0) == 0 and W(5, 8, 257) == 0
    assert W(10 ** 6, 8, 256) == W(4096, 8, 256)                  # long inputs go through in blocks of rows
    assert pairs.INFO_TILE == 128 and pairs.INFO_MAX_D == 256


def test_multi_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    A_, X_, B_, I_, Z_, D_, W_, P = (4096 * q for q in range(1, 9))   # non-null addresses that are never dereferenced

    def law(alpha=None, beta=None, labels=None, stride=0, use_margin=0, margin=0.0):
        c = _lib.PairLawC()
        c.alpha, c.beta, c.labels, c.label_stride, c.use_margin, c.margin = alpha, beta, labels, stride, use_margin, margin
        return c

    def call(rows=2, k=8, d=3, mB=8, A=A_, X=X_, B=B_, index=None, stride=0, Z=Z_, deg=D_, lda=8, ldx=8, ldb=3, ldz=3, ldd=8,
             c=None, ws=W_, nbytes=1 << 20):
        return L.mfcd_pair_hvp_multi_rows(A, lda, X, ldx, B, ldb, mB, d, index, stride, rows, k,
                                          None if c is None else ctypes.byref(c), Z, ldz, deg, ldd, ws, nbytes, None)

    big = 1 << 21
    assert call(rows=0) == 0 and call(rows=0, deg=None, ldd=0) == 0 and call(rows=0, X=None, ldx=0) == 0
    assert call(rows=0, ws=None, nbytes=0) == 0                                     # nothing to do, nothing launched
    assert call(rows=0, c=law()) == 0 and call(rows=0, index=I_, mB=5) == 0 and call(rows=0, index=I_, stride=8, mB=99) == 0
    assert call(rows=-1) == -1 and call(k=0, mB=0) == -1 and call(k=1048577, mB=1048577, lda=big, ldx=big, ldd=big) == -1
    assert call(d=0, ldb=0, ldz=0) == -1 and call(d=257, ldb=257, ldz=257) == -1
    assert call(rows=0, d=256, ldb=256, ldz=256) == 0
    assert call(A=None) == -1 and call(B=None) == -1 and call(Z=None) == -1
    assert call(lda=7) == -1 and call(ldx=7) == -1 and call(ldb=2) == -1 and call(ldz=2) == -1 and call(ldd=7) == -1
    assert call(mB=9) == -1 and call(mB=7) == -1                                    # no index: k must equal mB
    assert call(index=I_, mB=0) == -1
    for bad in (1, 7, -8):                                                          # an index stride in (0, k), or negative
        assert call(index=I_, stride=bad) == -1
    for other in (A_, X_, B_, D_, I_):                                              # Z aliases an input or deg
        assert call(Z=other, index=I_) == -1
    for other in (A_, X_, B_, I_):
        assert call(deg=other, index=I_) == -1
    assert call(rows=0, Z=A_) == -1                                                 # a bad call stays bad with no rows
    assert call(ws=None) == -1 and call(nbytes=100) == -2                           # MFCD_EWORKSPACE
    assert call(c=law(alpha=P)) == -1 and call(c=law(beta=P)) == -1
    assert call(c=law(use_margin=1, margin=-1e-30)) == -1 and call(c=law(use_margin=1, margin=float("nan"))) == -1
    assert call(c=law(labels=P, stride=7)) == -1 and call(c=law(labels=P, stride=-8)) == -1
    assert call(c=law(use_margin=1, margin=0.5), X=None) == -1                      # a margin needs X
    assert call(rows=0, c=law(use_margin=1, margin=0.5)) == 0 and call(rows=0, c=law(margin=-1.0), X=None) == 0
    assert call(rows=0, c=law(alpha=P, beta=P, labels=P, stride=8, use_margin=1, margin=float("inf"))) == 0


def test_no_cpu_fallback_and_public_signatures():
    import structure as S
    from mfcd import _lib, pairs, population
    A, B = torch.randn(3, 9), torch.randn(9, 2)
    for call in (lambda: pairs.pair_hvp_multi_rows(A, B), lambda: pairs.pair_info_rows(A, B),
                 lambda: pairs.pair_hvp_multi_rows(A, B, A, pairs.PairLaw(margin=1.0), None, True)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = S.MatrixFactorization(3, 9, 2)
    U, V = model.U.data, model.V.data
    with pytest.raises(_lib.MfcdError):
        pairs.user_information(U, V, A)
    with pytest.raises(_lib.MfcdError):
        population.population_user_step(U, V, A, 1.0, 0.1, solver="direct")
    for call in (lambda: S.user_information(model, A), lambda: S.strategy_information(model, A, 1.0, 100),
                 lambda: S.refit_users_population(model, A, 1.0, 0.1, solver="direct")):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        pairs.user_information(U, V, A, at="elsewhere")
    for fn in (lambda: population.population_user_step(U, V, A, 1.0, 0.1, solver="lu"),
               lambda: population.fit_population_exact(U, V, A, 1.0, 0.1, 1, user_solver="lu"),
               lambda: population.fit_population_exact(torch.zeros(3, 257), torch.zeros(9, 257), A, 1.0, 0.1, 1,
                                                       user_solver="direct")):
        with pytest.raises(ValueError):
            fn()
    p = inspect.signature(pairs.pair_hvp_multi_rows).parameters
    assert list(p) == ["A", "B", "X", "law", "index", "deg"] and p["deg"].default is False
    assert all(p[k].default is None for k in ("X", "law", "index"))
    p = inspect.signature(pairs.pair_info_rows).parameters
    assert list(p) == ["A", "B", "X", "law", "index"]
    p = inspect.signature(pairs.user_information).parameters
    assert list(p) == ["U", "V", "X", "s", "law", "users", "at", "row_block"]
    assert p["s"].default == 1.0 and p["at"].default == "model" and p["row_block"].default == 2048
    assert pairs.UserInformation._fields == ("info", "weight", "status")
    p = inspect.signature(population.population_user_step).parameters
    assert list(p)[-2:] == ["max_cg", "solver"] and p["solver"].default == "cg" and p["max_cg"].default is None
    p = inspect.signature(population.fit_population_exact).parameters
    assert list(p)[-1] == "user_solver" and p["user_solver"].default == "cg"
    assert inspect.signature(S.refit_users_population).parameters["solver"].default == "cg"
    assert inspect.signature(S.train_model_population_exact).parameters["user_solver"].default == "cg"
    p = inspect.signature(S.user_information).parameters
    assert list(p) == ["model", "X", "s", "law", "users", "at"] and p["at"].default == "model" and p["s"].default == 1.0
    p = inspect.signature(S.strategy_information).parameters
    assert list(p) == ["model_or_V", "X", "s", "num_triplets", "strategies", "users"]
    assert p["strategies"].default == ("random", "margin", "popularity", "variance", "top_k", "proximity", "cluster")
    for fn in (S.user_information, S.strategy_information):
        assert fn.__doc__.startswith("Extension (not in the reference)")
    assert not any("information" in k for k in S._RESULT_KEYS)                  # not part of the result dict


def _spec(m, rng):
    return {"alpha": rng.uniform(0.1, 1.0, m).astype(np.float32), "beta": rng.uniform(0.1, 1.0, m).astype(np.float32),
            "labels": rng.integers(0, 3, m), "margin": 2.5}


def test_model_matrix_is_the_laplacian_between_the_tables_and_the_derivative_of_the_user_gradient():
    """H = B^T L B to f64 rounding; H is the central difference (h = 1e-5: truncation and rounding about 1e-10 each, as
    in test_pair_hvp_cpu.py) of pair_hvp_model's user gradient without the ridge; symmetric, positive semidefinite, and
    unchanged to rounding when a constant row is added to B."""
    m, d, s, h = 23, 3, 0.7, 1e-5
    rng = np.random.default_rng(13)
    V = rng.normal(size=(m, d))
    X = rng.uniform(-3, 3, (2, m)).astype(np.float32)
    spec = _spec(m, rng)
    for name, sp in (("plain", None), ("law", spec)):
        prob = HM.Problem(X, s, sp)
        for r in range(2):
            u = rng.normal(size=d)
            a, w = V @ u, (None if sp is None else prob.w[r])
            z, deg, H = IM.info_row(a, V, w)
            L = HM.laplacian(a, w)
            np.testing.assert_allclose(H, V.T @ L @ V, rtol=0, atol=1e-12 * m)
            np.testing.assert_allclose(z, L @ V, rtol=0, atol=1e-13 * m)
            np.testing.assert_allclose(deg, np.diag(L), rtol=1e-14)
            np.testing.assert_allclose(H, V.T @ z, rtol=0, atol=1e-12 * m)
            fd = np.stack([(prob.user_grad(u + h * e, V, r, 0.0) - prob.user_grad(u - h * e, V, r, 0.0)) / (2 * h)
                           for e in np.eye(d)], axis=1)
            print(f"{name} row {r}: max |c H - central difference| = {np.abs(prob.c * H - fd).max():.2e}")
            assert np.abs(prob.c * H - fd).max() <= 1e-8 * prob.c * m * m
            assert np.abs(H - H.T).max() <= 1e-13 * m and np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-12 * m
            z2, deg2, H2 = IM.info_row(a, V + np.array([1000.0, -7.0, 0.25]), w)
            np.testing.assert_allclose(H2, H, rtol=0, atol=1e-9 * m)
            np.testing.assert_allclose(z2, z, rtol=0, atol=1e-10 * m)
            zb, Hb = IM.bounds(a, V, w)
            zb2, Hb2 = IM.bounds(a, V + np.array([1000.0, -7.0, 0.25]), w)  # the bound is centred: it does not see an offset
            np.testing.assert_allclose(zb2, zb, rtol=1e-9)
            np.testing.assert_allclose(Hb2, Hb, rtol=1e-9)
            assert (zb >= 0).all() and np.abs(Hb - Hb.T).max() <= 1e-18 and (np.diag(Hb) > 0).all()
    z, deg, H = IM.info_row([1.5], [[2.0, -1.0]])
    assert z.tolist() == [[0.0, 0.0]] and deg.tolist() == [0.0] and H.tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert all(np.isnan(t).all() for t in IM.info_row([1.0, np.inf], [[0.0], [1.0]]))
    assert all(np.isnan(t).all() for t in IM.info_row([1.0, 0.5], [[0.0], [np.nan]]))
    assert all(np.isnan(t).all() for t in IM.info_row([1.0, 0.5], [[0.0], [1.0]], None, [0.0, -np.inf]))


def test_model_user_rows_follow_the_laws_columns():
    rng = np.random.default_rng(3)
    n, m, d, s = 4, 9, 2, 0.7
    U, V = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(m, d)).astype(np.float32)
    X = rng.normal(size=(n, m)).astype(np.float32)
    cols = np.stack([rng.permutation(m)[:5] for _ in range(n)])
    spec = dict(alpha=None, beta=None, labels=None, margin=None, columns=cols, users=np.array([0, 2]))
    rows = IM.user_rows(U, V, X, s, spec)
    assert len(rows) == 2
    for (a, B, w, x, W), u in zip(rows, (0, 2)):
        np.testing.assert_array_equal(B, V[cols[u]].astype(np.float64))
        np.testing.assert_allclose(a, U[u].astype(np.float64) @ V[cols[u]].astype(np.float64).T)
        assert W == 10.0 and w.shape == (5, 5) and x.tolist() == X[u][cols[u]].astype(np.float64).tolist()
    truth = IM.user_rows(U, V, X, s, None, [3], at="truth")[0]
    assert truth[0].tolist() == (X[3] * np.float32(s)).astype(np.float64).tolist() and truth[4] == 36.0
