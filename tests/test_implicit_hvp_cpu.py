"""CPU-only checks of the implicit-feedback Hessian-vector kernel and of what is built on it (include/mfcd.h:
mfcd_implicit_hvp_rows; mfcd/implicit.py: implicit_hvp_rows, implicit_hvp; mfcd/implicit_exact.py; structure.implicit_hvp,
fit_users_implicit, refit_users_implicit, refit_items_implicit, train_model_implicit_exact): the numpy model the GPU
tests compare with (tests/implicit_hvp_model.py) is the Laplacian it claims to be, its table product is the central
difference of the f64 model's gradient and is symmetric, the step tests' inputs leave the certificate room above the
kernels' noise, the entry is declared and bound and refuses bad arguments before the device, and nothing has a CPU
form."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import implicit_hvp_model as HM
import implicit_model as IM
from mfcd import implicit_exact          # every test of this file is about what that module solves: none runs without it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mfcd_implicit_hvp_rows"
MAX_D = 1024


def _small(seed=5, n=12, m=40, d=3):
    rng = np.random.default_rng(seed)
    pos = [np.sort(rng.choice(m, int(rng.integers(1, m // 2)), replace=False)) for _ in range(n)]
    pos[1], pos[2] = np.zeros(0, dtype=np.int64), np.arange(m)
    exc = [np.sort(rng.choice(m, int(rng.integers(0, m // 4)), replace=False)) for _ in range(n)]
    U, V = 0.6 * rng.standard_normal((n, d)), rng.standard_normal((m, d))
    return pos, exc, U, V, rng.standard_normal((n, d)), rng.standard_normal((m, d))


def test_the_models_row_product_is_its_dense_laplacian():
    rng = np.random.default_rng(0)
    m = 37
    a, y = rng.uniform(-3, 3, m), rng.uniform(-2, 2, m)
    pos, excl = np.sort(rng.choice(m, 9, replace=False)), np.sort(rng.choice(m, 8, replace=False))
    q, deg, mag = HM.hvp_row(a, y, pos, excl, coef=0.7)
    L = 0.7 * HM.laplacian(a, pos, excl)
    np.testing.assert_allclose(q, L @ y, rtol=0, atol=1e-13)
    np.testing.assert_allclose(deg, np.diag(L), rtol=0, atol=1e-14)
    assert np.allclose(L, L.T) and np.abs(L.sum(1)).max() < 1e-13 and np.linalg.eigvalsh(L).min() > -1e-12
    assert (q[excl] == 0).all() and (deg[excl] == 0).all() and abs(q.sum()) < 1e-13 and (mag >= np.abs(q) - 1e-15).all()
    assert (HM.hvp_row(a, np.full(m, 0.3), pos, excl)[0] == 0).all()           # a constant direction
    for empty in (np.zeros(0, dtype=np.int64), np.arange(m)):                  # no positive, no negative
        assert all((t == 0).all() for t in HM.hvp_row(a, y, empty))
    # the Laplacian is the derivative of the model's score gradient
    P, N = IM.classes(m, pos, excl)
    h = 1e-6
    for c in (int(P[0]), int(N[0])):
        e = np.zeros(m)
        e[c] = h
        prob = HM.Problem(m, [pos], [excl], coef=0.7)
        fd = (prob.c[0] * prob.row_grad(a + e, 0) - prob.c[0] * prob.row_grad(a - e, 0)) / (2 * h)
        np.testing.assert_allclose(fd, L[:, c], rtol=0, atol=1e-8)


@pytest.mark.parametrize("normalize", ["pairs", "user"])
def test_the_models_table_product_is_symmetric_and_the_central_difference_of_its_gradient(normalize):
    pos, exc, U, V, dU, dV = _small()
    prob = HM.Problem(V.shape[0], pos, exc, normalize)
    HU, HV, _ = prob.hvp(U, V, dU, dV)
    h = 1e-5
    gp, gm = prob.grads(U + h * dU, V + h * dV), prob.grads(U - h * dU, V - h * dV)
    np.testing.assert_allclose(HU, (gp[0] - gm[0]) / (2 * h), rtol=0, atol=1e-9)
    np.testing.assert_allclose(HV, (gp[1] - gm[1]) / (2 * h), rtol=0, atol=1e-9)
    rng = np.random.default_rng(1)
    eU, eV = rng.standard_normal(U.shape), rng.standard_normal(V.shape)
    for gn in (False, True):
        a = prob.hvp(U, V, dU, dV, gn)
        b = prob.hvp(U, V, eU, eV, gn)
        lhs, rhs = (eU * a[0]).sum() + (eV * a[1]).sum(), (dU * b[0]).sum() + (dV * b[1]).sum()
        assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))
        if gn:
            assert (dU * a[0]).sum() + (dV * a[1]).sum() >= 0.0                # the Gauss-Newton form is semi-definite
    # the model's gradient is the one tests/implicit_model.py holds for the same risk
    (po, pi), (eo, ei) = HM.lists(pos), HM.lists(exc)
    _, G = IM.risk_f64(U, V, po, pi, eo, ei, normalize)
    np.testing.assert_allclose(prob.score_grads(U, V), G, rtol=0, atol=1e-15)
    assert (HU[[1, 2]] == 0).all()                                             # users without a pair


@pytest.mark.parametrize("m", [40, 2048 + 5])
def test_the_step_inputs_leave_the_certificate_room_above_the_noise(m):
    """The GPU tests allow |grad f| <= gtol l2 |u|_inf + noise.  With noise below the certificate's own term a run that
    stops early (|grad f| of the order of the start's, about 0.08) cannot pass."""
    from mfcd import implicit
    assert m in (40, implicit.CHUNK + 5)
    prob, Uopt, noise = HM.user_minimisers(m)
    Ustar, V, pos = HM.step_inputs(m)
    assert prob.paired.tolist() == [True, False, False] + [True] * 5 and len(pos[1]) == 0 and len(pos[2]) == m
    cert = HM.GTOL * HM.L2 * np.abs(Uopt).max(axis=1)
    print(f"m={m}: noise / certificate {np.round(noise[prob.paired] / cert[prob.paired], 3).tolist()}")
    assert (noise[prob.paired] < cert[prob.paired]).all() and (Uopt[~prob.paired] == 0).all()
    V64 = V.astype(np.float64)
    for r in np.flatnonzero(prob.paired):
        assert np.linalg.norm(prob.user_grad(Uopt[r], V64, r, HM.L2)) < 1e-12
        assert np.linalg.norm(prob.user_grad(np.zeros(3), V64, r, HM.L2)) > 100 * (cert[r] + noise[r])


def test_the_item_minimiser_is_stationary():
    prob, Vopt, noise = HM.item_minimiser(40)
    Ustar, V, pos = HM.step_inputs(40)
    U64 = Ustar.astype(np.float64)
    assert np.linalg.norm(prob.item_grad(U64, Vopt, HM.L2)) < 1e-12
    cert = HM.GTOL * HM.L2 * np.abs(Vopt).max()
    start = np.linalg.norm(prob.item_grad(U64, np.zeros_like(Vopt), HM.L2))
    print(f"item block: noise {noise:.3e}, certificate {cert:.3e}, |grad| at the start {start:.3e}")
    assert start > 100 * (cert + noise)


def test_the_entries_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 28
    assert len(re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1).split(",")) == 28
    assert len(_lib.SIGNATURES[NAME + "_workspace_bytes"][1]) == 3
    assert len(re.search(r"\b%s_workspace_bytes\(([^)]*)\);" % NAME, header).group(1).split(",")) == 3
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, NAME) and hasattr(L, NAME + "_workspace_bytes")
    csrc = os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc")
    src = open(os.path.join(csrc, "implicit_hvp.hip")).read()
    assert "topk_scores_kernel" in src and "__global__" in src and "pair_curvature" in src and "atomicAdd" not in src
    # one prepare kernel, one marking, one argument struct: in the shared header only
    shared = open(os.path.join(csrc, "implicit_common.h")).read()
    grad = open(os.path.join(csrc, "implicit.hip")).read()
    for what in ("void implicit_prepare_kernel(", "void implicit_mark(", "implicit_lower(const", "struct ImplicitArgs {",
                 "bool implicit_overlap("):
        assert what in shared and what not in src and what not in grad, what


def test_the_workspace_is_bounded():
    from mfcd import _lib
    L = _lib.load()
    ws = L.mfcd_implicit_hvp_rows_workspace_bytes
    slab = L.mfcd_rank_entries_workspace_bytes(4, 50, 8, 0)
    assert ws(4, 50, 0) == 256                                         # dense: one int32 per (row, chunk)
    assert ws(4, 50, 8) == 2 * slab + 256                              # two slabs of mfcd_rank_entries
    assert ws(1000, 5000, 0) == (1000 * 3 * 4 + 255) // 256 * 256
    assert ws(1 << 30, 1000, 64) == ws(1 << 20, 1000, 64) <= 2 * (128 << 20) + (4 << 20)
    assert ws(1 << 30, 4194304, 0) <= 4 << 20
    assert ws(1, 10, MAX_D + 1) == 0 and ws(1, 10, -1) == 0 and ws(1, 0, 4) == 0 and ws(1, 4194305, 4) == 0
    assert ws(-1, 10, 4) == 0


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
XD, YD, A, B, AY, BY, IDS, PO, PI, EO, EI, COEF, Q, DEG, ST, WS = (k << 20 for k in range(1, 17))


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    need = L.mfcd_implicit_hvp_rows_workspace_bytes(4, 50, 8)
    need_dense = L.mfcd_implicit_hvp_rows_workspace_bytes(4, 50, 0)

    def call(X=None, ldx=0, Y=None, ldy=0, A=A, B=B, Ay=AY, By=BY, d=8, row_ids=IDS, rows=4, n=30, m=50, pos_off=PO,
             pos_items=PI, entries=100, excl_off=EO, excl_items=EI, excl_entries=60, coef=COEF, q=Q, ldq=50, deg=DEG,
             ldd=50, status=ST, workspace=WS, workspace_bytes=need):
        return L.mfcd_implicit_hvp_rows(X, ldx, Y, ldy, A, B, Ay, By, d, row_ids, rows, n, m, pos_off, pos_items, entries,
                                        excl_off, excl_items, excl_entries, coef, q, ldq, deg, ldd, status, workspace,
                                        workspace_bytes, None)

    def dense(**kw):
        args = dict(X=XD, ldx=50, Y=YD, ldy=50, A=None, B=None, Ay=None, By=None, d=0, workspace_bytes=need_dense)
        args.update(kw)
        return call(**args)

    assert call(rows=0, entries=0) == 0 and dense(rows=0, entries=0) == 0      # nothing to launch
    assert call(d=0) == -1 and call(d=MAX_D + 1) == -1 and call(m=0) == -1 and call(m=4194305) == -1 and call(n=0) == -1
    assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(excl_entries=-1) == -1
    assert dense(ldx=49) == -1 and dense(ldy=49) == -1 and call(ldq=49) == -1 and call(ldd=49) == -1
    assert call(deg=None, ldd=0, rows=0, entries=0) == 0                       # ldd is not read without deg
    # both dense or both by factors
    assert call(A=None) == -1 and call(B=None) == -1 and call(Ay=None) == -1 and call(By=None) == -1
    assert dense(Y=None) == -1 and dense(A=A) == -1 and dense(By=BY) == -1 and call(Y=YD, ldy=50) == -1
    assert call(pos_off=None) == -1 and call(pos_items=None) == -1 and call(q=None) == -1 and call(status=None) == -1
    assert call(excl_off=None) == -1 and call(excl_items=None) == -1           # both or neither
    for inp in (A, B, AY, BY, IDS, PO, PI, EO, EI, COEF):
        for out in ("q", "deg", "status", "workspace"):
            assert call(**{out: inp}) == -1
    for inp in (XD, YD):
        assert dense(q=inp) == -1 and dense(deg=inp) == -1
    assert call(deg=Q + 4 * 199) == -1 and call(status=Q) == -1
    assert call(B=A, By=AY, rows=0, entries=0) == 0 and call(Ay=A, By=B, rows=0, entries=0) == 0   # inputs may alias
    assert call(workspace_bytes=need - 1) == -2 and call(workspace=None) == -2 and call(workspace=WS + 4) == -3
    assert call(q=Q + 2) == -3 and call(Ay=AY + 1) == -3 and call(pos_off=PO + 4) == -3


def test_there_is_no_cpu_fallback_and_arguments_are_checked():
    import structure as St
    from mfcd import _lib, implicit, implicit_exact
    from mfcd.ratings import RatingsData
    data = RatingsData([0, 0, 1, 3], [1, 2, 0, 4], [1.0, 2.0, 3.0, 4.0], 4, 5)
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    model = St.MatrixFactorization(4, 5, 2)
    for call in (lambda: implicit.implicit_hvp_rows(U @ V.t(), U @ V.t(), data),
                 lambda: implicit.implicit_hvp_rows((U, V), (U, V), data, deg=True),
                 lambda: implicit.implicit_hvp(U, V, U, V, data),
                 lambda: implicit_exact.implicit_user_step(U, V, data, 0.1),
                 lambda: implicit_exact.implicit_user_step(None, V, data, 0.1, coef=0.5),
                 lambda: implicit_exact.implicit_item_step(U, V, data, 0.1),
                 lambda: implicit_exact.implicit_item_step(None, V, data, 0.1),
                 lambda: implicit_exact.fit_implicit_exact(U, V, data, 0.1, 1)):
        with pytest.raises(_lib.MfcdError):
            call()
    for call in (lambda: St.implicit_hvp(model, data, U, V), lambda: St.fit_users_implicit(model, data, 0.1),
                 lambda: St.refit_users_implicit(model, data, 0.1), lambda: St.refit_items_implicit(model, data, 0.1),
                 lambda: St.train_model_implicit_exact(model, data, 0.1, sweeps=1)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(TypeError):
        St.fit_users_implicit("V", data, 0.1)
    # the kernels, not a torch form
    assert "mfcd_implicit_hvp_rows(" in inspect.getsource(implicit._launch_hvp)
    for fn in (implicit._Plan.hvp_sweep, implicit_exact._Problem.score_hvp):
        src = inspect.getsource(fn)
        assert "_launch_hvp(" in src and "exp(" not in src and "sigmoid" not in src


def test_mixed_inputs_l2_and_shapes_raise_value_errors_before_the_device():
    """What can be refused without a device is refused with ValueError, whatever the tensors' device."""
    from mfcd import implicit, implicit_exact
    from mfcd.ratings import RatingsData
    data = RatingsData([0, 0, 1, 3], [1, 2, 0, 4], [1.0, 2.0, 3.0, 4.0], 4, 5)
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    X = U @ V.t()
    with pytest.raises(ValueError):
        implicit.implicit_hvp_rows(X, (U, V), data)                            # mixed dense and factor inputs
    with pytest.raises(ValueError):
        implicit.implicit_hvp_rows((U, V), X, data)
    with pytest.raises(ValueError):
        implicit.implicit_hvp_rows((U, V), (U[:, :1], V[:, :1]), data)         # two widths
    with pytest.raises(ValueError):
        implicit.implicit_hvp_rows(X, X[:, :-1], data)
    with pytest.raises(ValueError):
        implicit.implicit_hvp(U, V, U[:-1], V, data)
    for l2 in (0.0, -1.0):
        for call in (lambda: implicit_exact.implicit_user_step(U, V, data, l2),
                     lambda: implicit_exact.implicit_item_step(U, V, data, l2),
                     lambda: implicit_exact.fit_implicit_exact(U, V, data, l2, 1)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        implicit_exact.implicit_user_step(U[:-1], V, data, 0.1)
    with pytest.raises(ValueError):
        implicit_exact.implicit_item_step(U, V[:, :1], data, 0.1)
    with pytest.raises(ValueError):
        implicit_exact.fit_implicit_exact(U, V, data, 0.1, -1)
    sig = lambda f: list(inspect.signature(f).parameters)                      # noqa: E731
    assert sig(implicit_exact.implicit_user_step) == ["U", "V", "data", "l2", "exclude", "normalize", "coef", "gtol",
                                                      "max_newton", "max_cg", "row_block"]
    assert inspect.signature(implicit_exact.implicit_item_step).parameters["max_cg"].default == 25
    import structure as St
    for fn in (St.implicit_hvp, St.fit_users_implicit, St.refit_users_implicit, St.refit_items_implicit,
               St.train_model_implicit_exact):
        assert "Not part of the result dict" in " ".join(fn.__doc__.split())
