"""CPU-only checks of the implicit-feedback risk (include/mfcd.h: mfcd_implicit_rows; mfcd/implicit.py;
structure.implicit_risk, train_model_implicit, compute_implicit_metrics): the numpy model the GPU tests compare with
(tests/implicit_model.py) has the gradient torch autograd finds for the f64 risk, its `inverted` is the sum of (rank - pos)
that `ranking.metrics_from_ranks` forms from the ranks of tests/rank_entries_model.py and its AUC that function's
`auc_per_user`; the entries are declared and bound, bad arguments are refused before the device is touched, there is no
CPU fallback, and `min_value` builds the expected positives."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import implicit_model as IM
import rank_entries_model as RM
from conftest import ROOT

NAME = "mfcd_implicit_rows"
MAX_D = 1024


def _lists(rng, n, m, with_excl, overlap):
    pos, excl = [], []
    for u in range(n):
        L = int(rng.integers(0, m + 1)) if u else 0
        p = np.sort(rng.choice(m, L, replace=False))
        pool = np.arange(m) if overlap else np.setdiff1d(np.arange(m), p)
        k = int(rng.integers(0, pool.size + 1)) if with_excl else 0
        pos.append(p)
        excl.append(np.sort(rng.choice(pool, min(k, m // 2), replace=False)))
    return pos, excl


@pytest.mark.parametrize("normalize", ["pairs", "user"])
def test_the_models_gradient_is_autograd_of_the_f64_risk(normalize):
    rng = np.random.default_rng(5)
    n, m, d = 7, 19, 3
    pos, excl = _lists(rng, n, m, True, True)
    (p_off, p_items), (e_off, e_items) = RM.csr(pos), RM.csr(excl)
    U = torch.tensor(rng.standard_normal((n, d)), dtype=torch.float64, requires_grad=True)
    V = torch.tensor(rng.standard_normal((m, d)), dtype=torch.float64, requires_grad=True)
    A = U @ V.t()
    terms, pairs = [], []
    for u in range(n):
        P, N = IM.classes(m, pos[u], excl[u])
        v = A[u][torch.from_numpy(N)][None, :] - A[u][torch.from_numpy(P)][:, None]
        terms.append(torch.nn.functional.softplus(v).sum())
        pairs.append(P.size * N.size)
    R, pn = torch.stack(terms), torch.tensor(pairs, dtype=torch.float64)
    has = pn > 0
    loss = R.sum() / pn.sum() if normalize == "pairs" else (R[has] / pn[has]).mean()
    loss.backward()
    Ud, Vd = U.detach().numpy(), V.detach().numpy()
    want, G = IM.risk_f64(Ud, Vd, p_off, p_items, e_off, e_items, normalize)
    assert abs(want - float(loss.detach())) < 1e-12
    np.testing.assert_allclose(G @ Vd, U.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(G.T @ Ud, V.grad.numpy(), rtol=0, atol=1e-12)
    # the row form the GPU tests use (fp32 scores) is the same function of the scores
    S = (Ud @ Vd.T).astype(np.float32)
    counts, sums, g = IM.rows(S, p_off, p_items, e_off, e_items)
    _, G32 = IM.risk_f64(np.eye(n), S.astype(np.float64).T, p_off, p_items, e_off, e_items, normalize)
    np.testing.assert_allclose(g * IM.coefficients(counts, normalize)[:, None], G32, rtol=0, atol=1e-12)


@pytest.mark.parametrize("with_excl,overlap", [(False, False), (True, False), (True, True)])
def test_inverted_is_the_rank_sum_and_the_auc_is_the_ranking_auc(with_excl, overlap):
    from mfcd import implicit, ranking
    rng = np.random.default_rng(11 + 2 * with_excl + overlap)
    n, m = 9, 23
    S = rng.integers(-2, 3, (n, m)).astype(np.float32)                 # full of ties
    S[1, 3], S[2, 5], S[2, 6] = -0.0, np.inf, np.nan                   # the key order's corners
    pos, excl = _lists(rng, n, m, with_excl, overlap)
    (p_off, p_items), (e_off, e_items) = RM.csr(pos), RM.csr(excl)
    counts, sums, _ = IM.rows(S, p_off, p_items, e_off if with_excl else None, e_items)
    rank, _, adm = RM.rank_entries(S, p_off, p_items, e_off if with_excl else None, e_items)
    for u in range(n):
        rk = np.sort(rank[p_off[u]:p_off[u + 1]])
        rk = rk[rk >= 0]                                              # a barred positive is no target
        assert counts[u, 0] == rk.size and counts[u, 1] == adm[u] - rk.size
        assert counts[u, 2] == int((rk - np.arange(rk.size)).sum())   # sum of (rank - pos), pos = the targets before
    if overlap:
        assert any(np.intersect1d(pos[u], excl[u]).size for u in range(n))
    want = ranking.metrics_from_ranks(p_off, rank, adm, np.zeros(n, dtype=np.int32))
    got = implicit.metrics_from_counts(counts, np.nan_to_num(sums), np.zeros(n, dtype=np.int32))
    np.testing.assert_allclose(got["auc_per_user"], want["auc_per_user"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(np.isnan(got["auc_per_user"]), np.isnan(want["auc_per_user"]))
    assert abs(got["auc"] - want["auc"]) < 1e-12


def test_a_hand_case():
    #        col   0    1    2    3    4    5
    a = np.array([2.0, 1.0, 1.0, 0.0, 3.0, 1.0], dtype=np.float32)
    counts, s, g = IM.row(a, [1, 3], [4])                              # P = {1, 3}, E = {4}, N = {0, 2, 5}
    # positive 1 (score 1): 0 precedes (2 > 1); 2 and 5 tie and have larger numbers: after.  positive 3 (score 0): all three
    assert counts.tolist() == [2, 3, 1 + 3, 2]
    sp = lambda v: np.log1p(np.exp(v))    # noqa: E731
    assert abs(s - (sp(1.0) + 2 * sp(0.0) + sp(2.0) + 2 * sp(1.0))) < 1e-14
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))    # noqa: E731
    np.testing.assert_allclose(g, [sg(1.0) + sg(2.0), -(sg(1.0) + 2 * sg(0.0)), sg(0.0) + sg(1.0),
                                   -(sg(2.0) + 2 * sg(1.0)), 0.0, sg(0.0) + sg(1.0)], rtol=0, atol=1e-14)
    counts, s, g = IM.row(a, [1, 4], [4], coef=0.5)                    # a barred positive is barred
    assert counts.tolist() == [1, 4, 1, 2] and g[4] == 0.0
    m = __import__("mfcd.implicit", fromlist=["x"]).metrics_from_counts(counts[None], [s], [0], tied_before=[0])
    assert m["auc"] == 1 - 1 / 4 and m["auc_midrank"] == 1 - (1 + 0.5 * 2) / 4 and m["log_likelihood"] == -s / 4


def test_the_entries_are_declared_and_bound():
    from mfcd import _lib, implicit
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 24
    assert len(re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1).split(",")) == 24
    assert len(_lib.SIGNATURES[NAME + "_workspace_bytes"][1]) == 3
    assert len(re.search(r"\b%s_workspace_bytes\(([^)]*)\);" % NAME, header).group(1).split(",")) == 3
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, NAME) and hasattr(L, NAME + "_workspace_bytes")
    assert L.mfcd_implicit_chunk() == implicit.CHUNK and L.mfcd_implicit_tile() == implicit.TILE
    src = open(os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd", "csrc", "implicit.hip")).read()
    assert "topk_scores_kernel" in src and "__global__" in src


def test_the_workspace_is_bounded():
    from mfcd import _lib
    L = _lib.load()
    ws = L.mfcd_implicit_rows_workspace_bytes
    part = 40
    assert ws(4, 50, 0) == 256                                         # dense: 4 rows x 1 chunk of partials
    assert ws(4, 50, 8) == 128 * 64 * 4 + 256                          # the slab of mfcd_rank_entries, then the partials
    assert ws(4, 50, 8) == L.mfcd_rank_entries_workspace_bytes(4, 50, 8, 0) + 256
    assert ws(1000, 5000, 0) == (1000 * 3 * part + 255) // 256 * 256
    assert ws(1 << 30, 1000, 64) == ws(1 << 20, 1000, 64) <= (128 << 20) + (40 << 20)
    assert ws(1 << 30, 4194304, 0) <= 40 << 20
    assert ws(1, 10, MAX_D + 1) == 0 and ws(1, 10, -1) == 0 and ws(1, 0, 4) == 0 and ws(1, 4194305, 4) == 0
    assert ws(-1, 10, 4) == 0


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
XD, A, B, IDS, PO, PI, EO, EI, COEF, CNT, SUMS, G, ST, WS = (k << 20 for k in range(1, 15))


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    need = L.mfcd_implicit_rows_workspace_bytes(4, 50, 8)

    def call(X=None, ldx=0, A=A, B=B, d=8, row_ids=IDS, rows=4, n=30, m=50, pos_off=PO, pos_items=PI, entries=100,
             excl_off=EO, excl_items=EI, excl_entries=60, coef=COEF, counts=CNT, sums=SUMS, g=G, ldg=50, status=ST,
             workspace=WS, workspace_bytes=need):
        return L.mfcd_implicit_rows(X, ldx, A, B, d, row_ids, rows, n, m, pos_off, pos_items, entries, excl_off, excl_items,
                                    excl_entries, coef, counts, sums, g, ldg, status, workspace, workspace_bytes, None)

    assert call(d=0) == -1 and call(d=MAX_D + 1) == -1 and call(m=0) == -1 and call(m=4194305) == -1 and call(n=0) == -1
    assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(excl_entries=-1) == -1
    assert call(X=XD, ldx=49) == -1 and call(ldg=49) == -1
    assert call(A=None) == -1 and call(B=None) == -1 and call(pos_off=None) == -1 and call(pos_items=None) == -1
    assert call(counts=None) == -1 and call(status=None) == -1
    assert call(excl_off=None) == -1 and call(excl_items=None) == -1   # both or neither
    assert call(sums=None) == -1                                       # the prepare pass alone returns no gradient
    for inp in (A, B, IDS, PO, PI, EO, EI, COEF):
        for out in ("counts", "sums", "g", "status", "workspace"):
            assert call(**{out: inp}) == -1
    assert call(sums=CNT + 64) == -1 and call(status=G + 4 * 199) == -1
    assert call(workspace_bytes=need - 1) == -2 and call(workspace=None) == -2 and call(workspace=WS + 4) == -3
    assert call(g=G + 2) == -3 and call(sums=SUMS + 4) == -3 and call(pos_off=PO + 4) == -3
    # nothing to launch
    assert call(rows=0, entries=0) == 0 and call(rows=0, m=0) == -1
    assert call(rows=0, entries=0, sums=None, g=None, A=None, B=None, d=0, workspace=None, workspace_bytes=0) == 0


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, implicit
    from mfcd.ratings import RatingsData
    data = RatingsData([0, 0, 1, 3], [1, 2, 0, 4], [1.0, 2.0, 3.0, 4.0], 4, 5)
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    model = St.MatrixFactorization(4, 5, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    for call in (lambda: implicit.implicit_rows(U @ V.t(), data),
                 lambda: implicit.implicit_rows((U, V), data, grad=True),
                 lambda: implicit.implicit_rows((U, V), (data.row_off, data.item), exclude=data, prepare_only=True),
                 lambda: implicit.implicit_risk(U, V, data),
                 lambda: implicit.implicit_risk(U, V, data, data, "user"),
                 lambda: implicit.implicit_metrics(U, V, data),
                 lambda: implicit.implicit_metrics(U @ V.t(), None, data, data),
                 lambda: implicit.fit_implicit((model, opt), data, 2)):
        with pytest.raises(_lib.MfcdError):
            call()
    for call in (lambda: St.implicit_risk(model, data), lambda: St.compute_implicit_metrics(model, data),
                 lambda: St.train_model_implicit(model, data, opt, "cpu", num_steps=1)):
        with pytest.raises(RuntimeError):
            call()
    assert "mfcd_implicit_rows(" in inspect.getsource(implicit._launch)
    sweep = inspect.getsource(implicit._Plan.sweep)
    assert "_launch(" in sweep and "exp(" not in sweep and "log" not in sweep       # the kernel, not a torch form


def test_normalize_is_one_of_two():
    import structure as St
    from mfcd import implicit
    from mfcd.ratings import RatingsData
    data = RatingsData([0, 1], [1, 0], [1.0, 2.0], 2, 3)
    U, V = torch.randn(2, 2), torch.randn(3, 2)
    model = St.MatrixFactorization(2, 3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    for bad in ("mean", "users", None, "PAIRS"):
        with pytest.raises(ValueError):
            implicit.implicit_risk(U, V, data, normalize=bad)
        with pytest.raises(ValueError):
            implicit.fit_implicit((model, opt), data, 1, normalize=bad)


def test_min_value_builds_the_expected_positives():
    import structure as St
    from mfcd.ratings import RatingsData
    users = [0, 0, 0, 1, 3, 3]
    items = [4, 1, 2, 0, 3, 1]
    values = [5.0, 2.0, 4.0, 3.0, 4.0, 1.0]
    data = RatingsData(users, items, values, 4, 5)
    off, it = St.implicit_positives(data)
    assert off.tolist() == [0, 3, 4, 4, 6] and it.tolist() == [1, 2, 4, 0, 1, 3]
    off, it = St.implicit_positives(data, min_value=4.0)
    assert off.dtype == torch.int64 and it.dtype == torch.int32
    assert off.tolist() == [0, 2, 2, 2, 3] and it.tolist() == [2, 4, 3]     # ascending per user; 4.0 itself is kept
    off, it = St.implicit_positives(data, min_value=9.0)
    assert off.tolist() == [0, 0, 0, 0, 0] and it.numel() == 0


def test_public_signatures_and_docstrings():
    import structure as St
    from mfcd import implicit

    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(implicit.implicit_rows)[:6] == [("X", E), ("positives", E), ("exclude", None), ("rows", None), ("grad", False),
                                               ("coef", None)]
    assert sig(implicit.implicit_risk)[:5] == [("U", E), ("V", E), ("data", E), ("exclude", None), ("normalize", "pairs")]
    assert sig(implicit.implicit_metrics) == [("U_or_X", E), ("V", E), ("data", E), ("exclude", None)]
    assert sig(implicit.fit_implicit)[:6] == [("binding", E), ("data", E), ("steps", E), ("log_every", 0), ("exclude", None),
                                              ("normalize", "pairs")]
    assert sig(St.train_model_implicit) == [("model", E), ("data", E), ("optimizer", E), ("device", E), ("num_steps", 1000),
                                            ("log_every", 100), ("exclude", None), ("normalize", "pairs"), ("min_value", None)]
    assert sig(St.compute_implicit_metrics) == [("model", E), ("data", E), ("exclude", None), ("min_value", None)]
    for fn in (St.implicit_risk, St.train_model_implicit, St.compute_implicit_metrics, St.implicit_positives):
        assert "Extension (not in the reference)" in fn.__doc__ and "Not part of the result dict / .pkl" in fn.__doc__
