"""CPU-only checks of the all-pairs statistics (include/mfcd.h: mfcd_pair_stats_rows; mfcd/pairs.py;
structure.compute_pairwise_metrics): the entries are declared and bound, bad arguments are refused before the device is
touched, there is no CPU fallback, and the CPU model the GPU tests compare with (tests/pairs_model.py) agrees with
scipy.stats.kendalltau and with the direct form of the risk."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import pairs_model as M
from conftest import ROOT


def test_pair_entry_points_are_declared_and_bound():
    from mfcd import _lib, pairs
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name in ("mfcd_pair_stats_workspace_bytes", "mfcd_pair_stats_rows"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
    assert len(_lib.SIGNATURES["mfcd_pair_stats_rows"][1]) == 13
    decl = re.search(r"int mfcd_pair_stats_rows\(([^)]*)\)", header).group(1)
    assert len(decl.split(",")) == 13
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_pair_stats_workspace_bytes(4096, 4096) > 0
    assert L.mfcd_pair_stats_workspace_bytes(256, 20000) > 0
    assert L.mfcd_pair_stats_workspace_bytes(0, 10) > 0
    for rows, m in ((4, 0), (4, 1048577), (-1, 10)):
        assert L.mfcd_pair_stats_workspace_bytes(rows, m) == 0, (rows, m)
    # the tile width the GPU tests build their shapes from is the library's: one partial per (row, tile)
    one = L.mfcd_pair_stats_workspace_bytes(16, 1)
    assert L.mfcd_pair_stats_workspace_bytes(16, pairs.TILE) == one
    assert L.mfcd_pair_stats_workspace_bytes(16, pairs.TILE + 1) == 2 * one
    assert L.mfcd_pair_stats_workspace_bytes(1 << 30, 1 << 20) <= 80 << 20      # long inputs go through in row blocks


def test_pair_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    P = 4096                                    # a non-null address that is never dereferenced: every call is refused

    def call(rows=2, m=8, scale=1.0, what=3, counts=P, sums=P, A=P, X=P, lda=8, ldx=8, ws=P, ws_bytes=1 << 20):
        return L.mfcd_pair_stats_rows(A, lda, X, ldx, rows, m, scale, what, counts, sums, ws, ws_bytes, None)

    assert call(what=0) == -1 and call(what=4) == -1
    assert call(m=0) == -1 and call(m=1048577, lda=1 << 21, ldx=1 << 21) == -1
    assert call(what=1, counts=None) == -1 and call(what=3, counts=None) == -1
    assert call(what=2, sums=None) == -1 and call(what=3, sums=None) == -1
    assert call(scale=float("inf")) == -1 and call(scale=float("nan")) == -1 and call(scale=1e300) == -1
    assert call(rows=-1) == -1 and call(A=None) == -1 and call(X=None) == -1 and call(lda=7) == -1 and call(ldx=7) == -1
    assert call(ws=None) == -1
    assert call(ws_bytes=16) == -2
    assert call(rows=0) == 0                    # nothing to do, nothing launched
    assert L.mfcd_error_string(-1).decode().startswith("mfcd:")


def test_pairs_have_no_cpu_fallback():
    import generation_data as gd
    import structure as S
    from mfcd import _lib, pairs
    A, X = torch.randn(3, 9), torch.randn(3, 9)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_stats_rows(A, X)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_stats_rows(A.double(), X.double())
    with pytest.raises(ValueError):
        pairs.pair_stats_rows(A, X, what="neither")
    model = S.MatrixFactorization(3, 9, 2)
    with pytest.raises(RuntimeError):
        S.compute_pairwise_metrics(model, X)
    with pytest.raises(RuntimeError):
        S.compute_pairwise_metrics(model, gd.FactoredMatrix(torch.randn(3, 2), torch.randn(9, 2)))


def test_pair_public_signatures():
    import structure as S
    from mfcd import pairs
    p = inspect.signature(pairs.pair_stats_rows).parameters
    assert list(p) == ["A", "X", "scale", "what"] and p["scale"].default == 1.0 and p["what"].default == "both"
    assert list(inspect.signature(pairs.pairwise_from_counts).parameters) == ["counts", "sums", "m"]
    p = inspect.signature(S.compute_pairwise_metrics).parameters
    assert list(p) == ["model", "X", "s", "users", "row_block"]
    assert p["s"].default == 1.0 and p["users"].default is None and p["row_block"].default == 2048
    assert S.compute_pairwise_metrics.__doc__.startswith("Extension (not in the reference)")
    assert "kendall_tau" not in S._RESULT_KEYS                                  # not part of the result dict


def test_pairwise_from_counts_on_the_host():
    from mfcd import pairs
    m = 5                                        # n0 = 10
    counts = np.array([[7, 3, 0, 0], [4, 1, 2, 4], [0, 0, 10, 0], [0, 0, 0, 10], [-1, -1, -1, -1]])
    sums = np.array([[5.0, 4.0, 6.0, 7.0]] * 4 + [[np.nan] * 4])
    out = pairs.pairwise_from_counts(torch.from_numpy(counts), torch.from_numpy(sums), m)
    np.testing.assert_allclose(out["kendall_tau"][:2], [0.4, 3 / math.sqrt(8 * 6)], rtol=1e-15)
    assert np.isnan(out["kendall_tau"][2:]).all()
    np.testing.assert_allclose(out["pairwise_accuracy"][:3], [0.7, 4 / 6, 0.0], rtol=1e-15)
    assert np.isnan(out["pairwise_accuracy"][3:]).all()
    np.testing.assert_array_equal(out["risk"][:4], [0.5] * 4)
    np.testing.assert_array_equal(out["bayes_accuracy"][:4], [0.7] * 4)
    assert np.isnan(out["risk"][4]) and all(v.dtype == np.float64 for v in out.values())
    one = pairs.pairwise_from_counts(np.zeros((2, 4), dtype=np.int64), np.zeros((2, 4)), 1)      # m = 1: no pairs
    assert all(np.isnan(v).all() for v in one.values())
    assert set(pairs.pairwise_from_counts(counts, None, m)) == {"kendall_tau", "pairwise_accuracy"}


def _rows(m, levels, rng):
    return rng.integers(0, levels, m).astype(np.float64) / 7.0 - 1.0


@pytest.mark.parametrize("m", [2, 3, 17, 65, 300])
def test_model_tau_is_scipys(m):
    from scipy.stats import kendalltau
    rng = np.random.default_rng(100 + m)
    cases = [(_rows(m, la, rng), _rows(m, lx, rng)) for la in (3, 8, 1000) for lx in (3, 8, 1000)]
    cases.append((np.full(m, 0.25), _rows(m, 1000, rng)))                    # constant row: tau undefined
    cases.append((_rows(m, 1000, rng), np.full(m, -1.0)))
    withnan = _rows(m, 1000, rng)
    withnan[m // 2] = np.nan
    cases.append((withnan, _rows(m, 1000, rng)))
    for a, x in cases:
        counts = M.pair_counts(a, x)
        got, want = M.tau_b(counts, m), kendalltau(a, x).statistic
        if np.isnan(want):
            assert np.isnan(got), (m, counts)
        else:
            assert abs(got - want) <= 1e-12, (m, counts, got, want)
            C, D, Ta, Tx = counts
            assert C >= 0 and C + D <= m * (m - 1) // 2 and Ta >= 0 and Tx >= 0
    assert np.isnan(M.tau_b(M.pair_counts([1.0], [2.0]), 1))                    # m = 1


@pytest.mark.parametrize("scale", [1.0, 0.25, 4.0])
def test_model_risk_is_the_direct_bce_and_not_below_its_floor(scale):
    rng = np.random.default_rng(7)
    for m in (2, 17, 300):
        a, x = rng.uniform(-3, 3, m), rng.uniform(-3, 3, m)
        s = M.pair_sums(a, x, scale)
        n0 = m * (m - 1) // 2
        assert abs(s[0] - M.direct_risk(a, x, scale)) <= 1e-12 * n0
        assert s[0] >= s[1] and s[3] >= s[2] and s[3] >= 0.5 * n0
        ideal = M.pair_sums(scale * x, x, scale)                                 # the scores the label law is made of
        assert abs(ideal[0] - ideal[1]) <= 1e-12 * n0 and abs(ideal[2] - ideal[3]) <= 1e-12 * n0
    assert np.isnan(M.pair_sums([1.0, np.inf], [0.0, 1.0], scale)).all()
