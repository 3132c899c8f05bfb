"""CPU-only checks of the per-row top-k interface (mfcd/topk.py, structure.recommend_items / compute_topk_overlap): the
names and signatures exist, the three C entry points are declared and bound, and there is no CPU fallback."""
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def test_topk_entry_points_are_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name in ("mfcd_topk_max_k", "mfcd_topk_rows_workspace_bytes", "mfcd_topk_rows"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
    assert len(_lib.SIGNATURES["mfcd_topk_rows"][1]) == 20
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    L = _lib.load()
    assert L.mfcd_topk_max_k() >= 8192
    # sizes: a slab of whole score rows, never n x m; 0 = out of range
    c4 = L.mfcd_topk_rows_workspace_bytes(65536, 65536, 64, 6553, 1)
    assert 0 < c4 <= 256 << 20
    assert L.mfcd_topk_rows_workspace_bytes(100000, 20000, 256, 2000, 3) <= 256 << 20
    assert L.mfcd_topk_rows_workspace_bytes(10, 131072, 0, 8192, 3) > 0          # dense mode
    for rows, m, d, k, ends in ((0, 10, 2, 1, 1), (4, 10, 2, 11, 1), (4, 10, 2, 0, 1), (4, 10, 2, 1, 0), (4, 10, 2, 1, 4),
                                (4, 100000, 2, L.mfcd_topk_max_k() + 1, 1), (4, 10, 1025, 1, 1)):
        assert L.mfcd_topk_rows_workspace_bytes(rows, m, d, k, ends) == 0, (rows, m, d, k, ends)
    # bad arguments are refused before anything is launched (no GPU is touched)
    assert L.mfcd_topk_rows(None, 0, None, None, 2, None, 4, 4, 10, 1, 1, None, None, None, None, None, None, None, 0, None) == -1


def test_topk_public_signatures():
    import structure as S
    from mfcd import topk
    p = inspect.signature(topk.topk_rows).parameters
    assert list(p)[:6] == ["X", "k", "rows", "ends", "exclude", "values"]
    assert p["rows"].default is None and p["ends"].default == "best" and p["exclude"].default is None
    assert p["values"].default is False
    p = inspect.signature(S.recommend_items).parameters
    assert list(p) == ["model", "users", "k", "exclude"] and p["k"].default == 10
    p = inspect.signature(S.compute_topk_overlap).parameters
    assert list(p) == ["model", "X", "k"] and p["k"].default == 10
    for fn in (S.recommend_items, S.compute_topk_overlap):
        assert "Extension (not in the reference)" in fn.__doc__


def test_topk_has_no_cpu_fallback():
    import generation_data as gd
    import structure as S
    from mfcd import _lib, topk
    X = torch.randn(5, 9)
    with pytest.raises(_lib.MfcdError):
        topk.topk_rows(X, 3)
    with pytest.raises(_lib.MfcdError):
        topk.topk_rows((torch.randn(5, 2), torch.randn(9, 2)), 3)
    with pytest.raises(_lib.MfcdError):
        topk.topk_rows(gd.FactoredMatrix(torch.randn(5, 2), torch.randn(9, 2)), 3, device="cpu")
    with pytest.raises(ValueError):
        topk.topk_rows(X, 3, ends="middle")
    model = S.MatrixFactorization(5, 9, 2)
    with pytest.raises(RuntimeError):
        S.recommend_items(model, k=3)
    with pytest.raises(RuntimeError):
        S.compute_topk_overlap(model, X, k=3)


def test_exclude_csr_layout():
    from mfcd import topk
    off, items = topk.exclude_csr({(0, 1), (0, 3), (2, 5), (2, 1), (7, 0), (1, 99)}, torch.tensor([2, 0, 2, 1]), 3, 6, "cpu")
    assert off.tolist() == [0, 2, 4, 6, 6] and items.tolist() == [1, 5, 1, 3, 1, 5]
    off, items = topk.exclude_csr([(0, 1, 3), (2, 5, 1), (0, 3, 3)], torch.tensor([2, 0]), 3, 6, "cpu")   # triplets bar both items
    assert off.tolist() == [0, 2, 4] and items.tolist() == [1, 5, 1, 3]
    off, items = topk.exclude_csr([], torch.tensor([1]), 3, 6, "cpu")
    assert off.tolist() == [0, 0] and items.numel() == 1
