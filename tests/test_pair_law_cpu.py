"""CPU-only checks of the pair-law entries (include/mfcd.h: mfcd_pair_law_stats_rows, mfcd_pair_law_grad_rows;
mfcd/pairs.py: PairLaw, strategy_law): the entries are declared and bound under the unchanged ABI version, every
MFCD_EINVAL rule holds before the device is touched, PairLaw validates at construction, the host-side parts of
strategy_law need no device, and the popularity law alpha = p / (1 - p), beta = p is the law numpy's
choice(size=2, replace=False, p) draws from."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_law_model as LM
from conftest import ROOT


def test_law_entry_points_are_declared_and_bound():
    from mfcd import _lib, pairs
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name, nargs in (("mfcd_pair_law_stats_workspace_bytes", 2), ("mfcd_pair_law_stats_rows", 13),
                        ("mfcd_pair_law_grad_rows", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\b%s\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs, name
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header)) - {"mfcd_sample"}
    assert declared == set(_lib.SIGNATURES)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    fields = re.search(r"typedef struct mfcd_pair_law \{(.*?)\} mfcd_pair_law;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.PairLawC._fields_]
    assert ctypes.sizeof(_lib.PairLawC) == 48
    L = _lib.load()
    assert L.mfcd_abi_version() == 4
    # the workspace rule: one 56-byte partial per (row, tile), 256-byte aligned, row blocks beyond 2^20 workgroups
    size = L.mfcd_pair_law_stats_workspace_bytes
    assert size(0, 10) > 0 and size(4096, 4096) >= 4096 * 4 * 56
    for rows, m in ((4, 0), (4, 1048577), (-1, 10)):
        assert size(rows, m) == 0, (rows, m)
    assert size(16, 1) == size(16, pairs.TILE) == 1024 and size(16, pairs.TILE + 1) == 2 * 1024 - 256
    assert size(1 << 30, 1 << 20) <= 56 << 20


def test_law_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()
    P = 4096                                    # a non-null address that is never dereferenced: every call is refused

    def law(alpha=None, beta=None, labels=None, stride=0, use_margin=0, margin=0.0):
        c = _lib.PairLawC()
        c.alpha, c.beta, c.labels, c.label_stride, c.use_margin, c.margin = alpha, beta, labels, stride, use_margin, margin
        return c

    def stats(c, rows=2, m=8, scale=1.0, support=P, sums=P, A=P, X=P, lda=8, ldx=8, ws=P, ws_bytes=1 << 20):
        return L.mfcd_pair_law_stats_rows(A, lda, X, ldx, rows, m, scale, None if c is None else ctypes.byref(c), support,
                                          sums, ws, ws_bytes, None)

    def grad(c, rows=2, m=8, scale=1.0, A=P, X=P, G=2 * P, lda=8, ldx=8, ldg=8):
        return L.mfcd_pair_law_grad_rows(A, lda, X, ldx, rows, m, scale, None if c is None else ctypes.byref(c), G, ldg,
                                         None)

    ok = law()
    for call in (stats, grad):
        # the unweighted entries' rules
        assert call(ok, m=0) == -1 and call(ok, m=1048577, lda=1 << 21, ldx=1 << 21) == -1
        assert call(ok, rows=-1) == -1 and call(ok, A=None) == -1 and call(ok, X=None) == -1
        assert call(ok, lda=7) == -1 and call(ok, ldx=7) == -1
        assert call(ok, scale=float("inf")) == -1 and call(ok, scale=float("nan")) == -1 and call(ok, scale=1e300) == -1
        # the law's own
        assert call(None) == -1
        assert call(law(alpha=P)) == -1 and call(law(beta=P)) == -1
        assert call(law(use_margin=1, margin=-1e-30)) == -1 and call(law(use_margin=1, margin=float("nan"))) == -1
        assert call(law(labels=P, stride=7)) == -1 and call(law(labels=P, stride=-8)) == -1
        # a refused call with rows = 0 is still refused; an accepted one launches nothing
        assert call(law(alpha=P), rows=0) == -1
        assert call(ok, rows=0) == 0
        assert call(law(alpha=P, beta=P, labels=P, stride=8, use_margin=1, margin=float("inf")), rows=0) == 0
        assert call(law(labels=P, stride=0, margin=-1.0), rows=0) == 0           # the margin is not in use
    assert stats(ok, support=None) == -1 and stats(ok, sums=None) == -1 and stats(ok, ws=None) == -1
    assert stats(ok, ws_bytes=16) == -2
    assert grad(ok, G=None) == -1 and grad(ok, ldg=7) == -1 and grad(ok, G=P) == -1


def test_pair_law_validates_at_construction():
    from mfcd import _lib, pairs
    with pytest.raises(ValueError):
        pairs.PairLaw(alpha=[1.0, 2.0])
    with pytest.raises(ValueError):
        pairs.PairLaw(beta=[1.0, 2.0])
    for bad in ([1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0]):
        with pytest.raises(ValueError):
            pairs.PairLaw(alpha=bad, beta=[1.0, 1.0])
        with pytest.raises(ValueError):
            pairs.PairLaw(alpha=[1.0, 1.0], beta=bad)
    with pytest.raises(ValueError):
        pairs.PairLaw(alpha=[1.0, 1.0], beta=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        pairs.PairLaw(alpha=[1.0, 1.0], beta=[1.0, 1.0], labels=[0, 1, 2])
    with pytest.raises(ValueError):
        pairs.PairLaw(labels=[[0, 1, 2]], columns=[[0, 1, 2], [2, 1, 0]])
    with pytest.raises(ValueError):
        pairs.PairLaw(labels=[0.5, 1.5])
    with pytest.raises(ValueError):
        pairs.PairLaw(columns=[0, -1])
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pairs.PairLaw(margin=bad)
    # scaled to a maximum of 1; positive entries below 1e-6 of it are set to 0
    law = pairs.PairLaw(alpha=[4.0, 2.0, 0.0, 3e-6, 5e-6], beta=[0.5, 0.25, 0.5, 0.0, 1e-9])
    assert law.alpha.dtype == torch.float32 and law.alpha.tolist() == [1.0, 0.5, 0.0, 0.0, np.float32(1.25e-6)]
    assert law.beta.tolist() == [1.0, 0.5, 1.0, 0.0, 0.0]
    assert not law.trivial and pairs.PairLaw().trivial and not pairs.PairLaw(margin=0.0).trivial
    assert pairs.PairLaw(alpha=[0.0, 0.0], beta=[0.0, 0.0]).alpha.tolist() == [0.0, 0.0]
    assert pairs.PairLaw(labels=[3, 1, 3]).labels.dtype == torch.int32
    # there is no CPU form of the kernels
    A = torch.zeros(2, 5)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_law_stats_rows(A, A, law)
    with pytest.raises(_lib.MfcdError):
        pairs.pair_law_grad_rows(A, A, law)


def test_strategy_law_host_side_parts():
    import structure as S
    from mfcd import pairs
    X = torch.randn(6, 9, generator=torch.Generator().manual_seed(1))
    cpu = torch.device("cpu")                   # these strategies' set-up touches no device
    assert pairs.strategy_law(X, 20, "random", cpu).trivial
    law = pairs.strategy_law(X, 20, "margin", cpu)
    head = X.numpy()
    assert law.margin == float(np.mean(head.max(1) - head.min(1)) * 20 / 54) and law.alpha is None and law.labels is None
    law = pairs.strategy_law(X, 20, "popularity", cpu, popularity_method="zipf", alpha=1.5)
    p = 1.0 / np.arange(1, 10) ** 1.5
    p /= p.sum()
    a = p / (1 - p)
    np.testing.assert_allclose(law.alpha.numpy(), a / a.max(), rtol=1e-6)
    np.testing.assert_allclose(law.beta.numpy(), p / p.max(), rtol=1e-6)
    law = pairs.strategy_law(X, 20, "variance", cpu)
    v = X.double().var(0).numpy()
    np.testing.assert_allclose(law.beta.numpy(), v / v.max(), rtol=1e-6)
    for name in ("user_similarity", "no_such_strategy"):
        with pytest.raises(ValueError):
            pairs.strategy_law(X, 20, name, cpu)
    with pytest.raises(RuntimeError):           # the public entry has no CPU form
        S.sampling_law(X, 20, "margin", device="cpu")
    for fn, first in ((S.law_risk, ["model", "X", "law", "s", "users", "row_block"]),
                      (S.compute_law_metrics, ["model", "X", "law", "s", "users", "row_block"]),
                      (S.train_model_law, ["model", "X", "s", "optimizer", "device", "law", "num_steps", "log_every",
                                           "row_block"])):
        assert list(inspect.signature(fn).parameters) == first
        assert fn.__doc__.startswith("Extension (not in the reference)")
    assert S.sampling_law.__doc__.startswith("Extension (not in the reference)")


def test_model_margin_decides_as_the_f64_compare_of_the_fp32_difference():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(200).astype(np.float32)
    d = np.abs(x[:, None] - x[None, :])
    for margin in (0.1, float(d[3, 7]), float(d[3, 7]) * (1 + 1e-12), float(d[3, 7]) * (1 - 1e-12), 0.0, 1e-50):
        assert ((d.astype(np.float64) <= margin) == (d <= LM.floor32(margin))).all(), margin
        assert float(LM.floor32(margin)) <= margin < float(np.nextafter(LM.floor32(margin), np.float32(np.inf)))


def test_popularity_law_is_the_law_of_choice_without_replacement():
    """100 000 draws of np.random.choice(5, size=2, replace=False, p) against P(i, j) = p_i p_j / (1 - p_i), over the 20
    ordered pairs: chi-square on 19 degrees of freedom, bound at its 1e-4 upper quantile (50.80).  The law's symmetric
    weight alpha_i beta_j + alpha_j beta_i with alpha = p / (1 - p), beta = p is P(i, j) + P(j, i)."""
    p = np.array([0.4, 0.25, 0.2, 0.1, 0.05])
    P = LM.attempt_law("popularity", np.zeros((1, 5), dtype=np.float32), 0, probs=p)
    np.testing.assert_allclose(P.sum(), 1.0, rtol=1e-12)
    w = LM.weights(np.zeros(5), alpha=p / (1 - p), beta=p)
    np.testing.assert_allclose(w, P + P.T, rtol=1e-6)               # fp32 inputs
    rng = np.random.RandomState(12345)
    N = 100_000
    seen = np.zeros((5, 5))
    for _ in range(N):
        i, j = rng.choice(5, size=2, replace=False, p=p)
        seen[i, j] += 1
    off = ~np.eye(5, dtype=bool)
    chi2 = float((((seen - N * P) ** 2)[off] / (N * P)[off]).sum())
    print(f"chi-square {chi2:.2f} on 19 degrees of freedom")
    assert chi2 <= 50.80
