"""CPU-only checks of the full-catalogue ranking metrics (include/mfcd.h: mfcd_rank_entries; mfcd/ranking.py;
structure.compute_ranking_metrics): the entry is declared and bound, its workspace is the bounded slab, bad arguments are
refused before the device is touched, there is no CPU fallback, the numpy model the GPU tests compare with
(tests/rank_entries_model.py) agrees with the definition on a hand case, and the metric formulas reproduce a hand-worked
example."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import rank_entries_model as RM
from conftest import ROOT

NAME = "mfcd_rank_entries"
MAX_D = 1024


def test_the_entry_is_declared_and_bound():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 23
    decl = re.search(r"\b%s\(([^)]*)\);" % NAME, header).group(1)
    assert len(decl.split(",")) == 23
    assert len(_lib.SIGNATURES[NAME + "_workspace_bytes"][1]) == 4
    assert len(re.search(r"\b%s_workspace_bytes\(([^)]*)\);" % NAME, header).group(1).split(",")) == 4
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    assert re.search(r"#define MFCD_MAX_D %d\b" % MAX_D, header)
    L = _lib.load()
    assert L.mfcd_abi_version() == 4 and hasattr(L, NAME)


def test_the_workspace_is_the_bounded_slab():
    from mfcd import _lib
    L = _lib.load()
    ws = L.mfcd_rank_entries_workspace_bytes
    slab = 128 << 20
    assert ws(10, 1000, 64, 100) == 128 * 1024 * 4                    # one block of 128 rows of ld = 1024 floats
    assert ws(0, 1000, 64, 0) == 256
    # bounded by the slab, whatever n (not an argument), the rows and the entries are
    assert ws(1 << 30, 1000, 64, 1 << 40) == ws(1 << 20, 1000, 64, 0) <= slab
    assert ws(1 << 30, 1000, 64, 1 << 40) == (slab // (1024 * 4)) // 128 * 128 * 1024 * 4
    assert ws(500, 70001, 2, 1500) == 384 * 70016 * 4 <= slab        # whole blocks of 128 rows: 384 of the 479 that fit
    assert ws(10, 4194304, 1, 0) == 128 * 4194304 * 4                 # at least 128 rows, even beyond 128 MiB
    # the same slab as mfcd_topk_rows'
    for rows, m, d in ((10, 1000, 64), (500, 70001, 2), (100000, 1682, 16)):
        assert ws(rows, m, d, 0) == L.mfcd_topk_rows_workspace_bytes(rows, m, d, 1, 1)
    assert ws(1, 10, 0, 1) == 0 and ws(1, 10, MAX_D + 1, 1) == 0 and ws(1, 10, -1, 1) == 0    # d: the factor mode's
    assert ws(1, 0, 4, 1) == 0 and ws(1, 4194305, 4, 1) == 0
    assert ws(-1, 10, 4, 1) == 0 and ws(1, 10, 4, -1) == 0 and ws(1, -5, 4, 1) == 0


# non-null, never dereferenced; 1 MiB apart: no array of the calls below reaches its neighbour
XD, A, B, IDS, TO, TI, EO, EI, RANK, TIES, SCORE, ADM, ST, WS = (k << 20 for k in range(1, 15))
SLAB = 128 * 64 * 4                                                    # 4 rows of m = 50: one block of ld = 64


def test_bad_arguments_are_refused_before_the_device():
    from mfcd import _lib
    L = _lib.load()

    def call(X=None, ldx=0, A=A, B=B, d=8, row_ids=IDS, rows=4, n=30, m=50, tgt_off=TO, tgt_items=TI, entries=100,
             excl_off=EO, excl_items=EI, excl_entries=60, rank=RANK, ties=TIES, score=SCORE, admissible=ADM, status=ST,
             workspace=WS, workspace_bytes=SLAB):
        return L.mfcd_rank_entries(X, ldx, A, B, d, row_ids, rows, n, m, tgt_off, tgt_items, entries, excl_off,
                                   excl_items, excl_entries, rank, ties, score, admissible, status, workspace,
                                   workspace_bytes, None)

    def dense(**kw):
        return call(X=XD, ldx=kw.pop("ldx", 50), A=None, B=None, d=0, workspace=None, workspace_bytes=0, **kw)

    assert L.mfcd_rank_entries_workspace_bytes(4, 50, 8, 100) == SLAB
    # sizes
    assert call(d=0) == -1 and call(d=MAX_D + 1) == -1 and call(d=-1) == -1
    assert call(m=0) == -1 and call(m=4194305) == -1 and call(n=0) == -1
    assert call(rows=-1) == -1 and call(entries=-1) == -1 and call(excl_entries=-1) == -1
    assert dense(ldx=49) == -1
    # null where a count is positive
    assert call(A=None) == -1 and call(B=None) == -1
    assert call(tgt_off=None) == -1 and call(admissible=None) == -1 and call(status=None) == -1
    assert call(tgt_items=None) == -1 and call(rank=None) == -1 and call(ties=None) == -1
    assert call(excl_off=None) == -1 and call(excl_items=None) == -1             # both or neither
    # an output on an input, or on another output
    for inp in (A, B, IDS, TO, TI, EO, EI, WS):
        for out in ("rank", "ties", "score", "admissible", "status"):
            assert call(**{out: inp}) == -1
    assert dense(rank=XD) == -1 and dense(status=XD + 8) == -1
    outs = dict(rank=RANK, ties=TIES, score=SCORE, admissible=ADM, status=ST)
    for a in outs:
        for b, p in outs.items():
            if a != b:
                assert call(**{a: p}) == -1
    assert call(ties=RANK + 4 * 99) == -1 and call(status=ADM + 12) == -1 and call(rank=TI + 396) == -1   # partial overlaps
    # the workspace
    assert call(workspace_bytes=SLAB - 1) == -2 and call(workspace_bytes=0) == -2 and call(workspace=None) == -2
    assert call(workspace=WS + 4) == -3
    # a bad call stays bad with no rows, a good one succeeds with nothing launched
    assert call(rows=0, d=0) == -1 and call(rows=0, m=0) == -1 and call(rows=0, rank=TI) == -1
    assert call(rows=0, entries=0, workspace_bytes=255) == -2
    assert call(rows=0, entries=0, workspace_bytes=256) == 0
    assert call(rows=0, entries=0, row_ids=None, tgt_off=None, tgt_items=None, excl_off=None, excl_items=None,
                excl_entries=0, rank=None, ties=None, score=None, admissible=None, status=None,
                workspace_bytes=256) == 0
    assert dense(rows=0, entries=0) == 0


def test_there_is_no_cpu_fallback():
    import structure as St
    from mfcd import _lib, ranking
    from mfcd.ratings import RatingsData
    data = RatingsData([0, 0, 1, 3], [1, 2, 0, 4], [1.0, 2.0, 3.0, 4.0], 4, 5)
    U, V = torch.randn(4, 2), torch.randn(5, 2)
    off, items = data.row_off, data.item
    for call in (lambda: ranking.rank_entries(U @ V.t(), data),
                 lambda: ranking.rank_entries((U, V), data),
                 lambda: ranking.rank_entries((U, V), (off, items), exclude=data),
                 lambda: ranking.ranking_metrics(U @ V.t(), data),
                 lambda: ranking.ranking_metrics((U, V), data, data, ks=(1, 3), min_value=2.0)):
        with pytest.raises(_lib.MfcdError):
            call()
    model = St.MatrixFactorization(4, 5, 2)
    for call in (lambda: St.compute_ranking_metrics(model, data), lambda: St.compute_ranking_metrics(U @ V.t(), data, data)):
        with pytest.raises(RuntimeError):
            call()
    src = inspect.getsource(ranking.rank_entries)
    assert "mfcd_rank_entries(" in src and "sort(" not in src and "topk(" not in src   # the kernel, not a torch form


def test_public_signatures_and_docstrings():
    import structure as St
    from mfcd import ranking

    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(ranking.rank_entries) == [("X", E), ("targets", E), ("exclude", None), ("rows", None), ("scores", False)]
    assert sig(ranking.ranking_metrics)[:5] == [("X", E), ("test", E), ("train", None), ("ks", (10,)), ("min_value", None)]
    assert sig(St.compute_ranking_metrics) == [("model", E), ("test", E), ("train", None), ("ks", (10,)),
                                               ("min_value", None), ("users", None)]
    doc = " ".join(St.compute_ranking_metrics.__doc__.split())
    assert doc.startswith("Extension (not in the reference)") and "mfcd_rank_entries" in doc
    assert doc.endswith("Not part of the result dict / .pkl layout.")
    assert "half credit" in " ".join(ranking.ranking_metrics.__doc__.split())
    assert not any("rank" in k or "recall" in k for k in St._RESULT_KEYS)


def _hand_case():
    """6 x 15: row 0 holds a tie run, row 1 a signed zero pair, row 2 a NaN (and +inf), row 3 a barred target, row 4 has
    no targets, row 5 has everything at once and a repeated target."""
    nan, inf = float("nan"), float("inf")
    S = np.arange(6 * 15, dtype=np.float32).reshape(6, 15) % 7 - 3.0           # small integers: ties in every row
    S[0, [2, 5, 9, 11]] = 1.5
    S[1, [3, 8]] = [0.0, -0.0]
    S[1, 12] = 0.0
    S[2, 4], S[2, 10], S[2, 6] = nan, nan, inf
    S[5, [0, 7]] = [-0.0, 0.0]
    S[5, 3], S[5, 13], S[5, 14] = nan, -inf, inf
    targets = [[9, 2, 0], [8, 3, 14], [4, 6, 10, 1], [5, 7], [], [7, 0, 3, 13, 14, 7]]
    barred = [[5], [], [0, 1, 2], [4, 5, 6], [0, 14], [2, 8]]
    return S, RM.csr(targets), RM.csr(barred)


def test_the_model_agrees_with_the_definition_on_a_hand_case():
    S, (t_off, t_items), (e_off, e_items) = _hand_case()
    for excl in ((e_off, e_items), (None, None)):
        got = RM.rank_entries(S, t_off, t_items, *excl)
        want = RM.by_definition(S, t_off, t_items, *excl)
        for g, w in zip(got, want):
            assert g.tolist() == w.tolist()
    rank, ties, adm = RM.rank_entries(S, t_off, t_items, e_off, e_items)
    assert adm.tolist() == [14, 15, 12, 12, 13, 13]
    # row 0: columns 2, 5, 9, 11 hold 1.5, 5 is barred; 3.0 at columns 6 and 13 and 2.0 at 5 (barred) and 12 lie above
    assert rank[:2].tolist() == [4, 3] and ties[:2].tolist() == [2, 2]
    # row 1: +0.0 at 3 and 12 and -0.0 at 8 are one key, ordered by column
    r1 = dict(zip(t_items[3:6].tolist(), zip(rank[3:6].tolist(), ties[3:6].tolist())))
    assert r1[3][1] == r1[8][1] and r1[8][0] == r1[3][0] + 1
    # row 2: the NaNs lead in column order, +inf follows
    assert rank[6:9].tolist() == [0, 2, 1] and ties[6:9].tolist() == [1, 0, 1]
    # row 3: target 5 is barred
    assert rank[10] == -1 and ties[10] == -1 and rank[11] >= 0
    # row 5: NaN first, +inf second, -inf last; the repeated target 7 gets equal results; -0.0 at 0 before +0.0 at 7
    r5 = list(zip(t_items[12:].tolist(), rank[12:].tolist(), ties[12:].tolist()))
    assert r5[2][1:] == (0, 0) and r5[4][1:] == (1, 0) and r5[3][1:] == (12, 0)
    assert r5[0] == r5[5] and r5[1][1] < r5[0][1] and r5[1][2] == r5[0][2] >= 1


def test_the_keys_order_floats_as_topk_does():
    inf, nan = float("inf"), float("nan")
    x = np.array([nan, inf, 3.0, 1e-45, 0.0, -0.0, -1e-45, -2.5, -inf], dtype=np.float32)
    k = RM.best_keys(x).astype(np.int64)
    assert k[0] == 0 and (np.diff(k)[[0, 1, 2, 3, 5, 6, 7]] > 0).all() and k[4] == k[5]
    assert RM.best_keys(np.array([-nan], dtype=np.float32))[0] == 0
    assert (k != 0xFFFFFFFF).all()                                             # the kernel's "absent" key is no score's


def test_the_metric_formulas_on_a_hand_worked_example():
    """Four users.  u0: ranks 0, 3, 7 of 10 admissible; u1: rank 4, the only admissible item; u2: no target; u3: a barred
    target and rank 9 of 12.  Values below are worked by hand from the formulas (log2 3 = 1.584962500721156,
    log2 5 = 2.321928094887362, log2 6 = 2.584962500721156)."""
    from mfcd import ranking
    off = np.array([0, 3, 4, 4, 6])
    rank = np.array([3, 0, 7, 4, -1, 9])
    admissible = np.array([10, 1, 9, 12])
    status = np.zeros(4, dtype=np.int64)
    nan = float("nan")
    dcg0 = 1.0 + 1.0 / 2.321928094887362                   # ranks 0 and 3: 1 / log2(2) + 1 / log2(5)
    idcg0 = 1.0 + 1.0 / 1.584962500721156 + 0.5           # three ideal places
    want = {
        "recall@5": [2 / 3, 1.0, nan, 0.0], "precision@5": [0.4, 0.2, nan, 0.0], "hit@5": [1.0, 1.0, nan, 0.0],
        "ndcg@5": [dcg0 / idcg0, 1.0 / 2.584962500721156, nan, 0.0],
        "recall@1": [1 / 3, 0.0, nan, 0.0], "precision@1": [1.0, 0.0, nan, 0.0], "hit@1": [1.0, 0.0, nan, 0.0],
        "ndcg@1": [1.0, 0.0, nan, 0.0],
        "mrr": [1.0, 0.2, nan, 0.1], "mean_rank": [10 / 3, 4.0, nan, 9.0],
        # u0: other items ahead of the targets 0 + (3 - 1) + (7 - 2) = 7 of 3 x 7 pairs; u1: no other item; u3: 9 of 11
        "auc": [1 - 7 / 21, nan, nan, 1 - 9 / 11],
    }
    assert abs(dcg0 / idcg0 - 0.671386072523) < 1e-11     # 1.430676558073 / 2.130929753571
    for fn in (ranking.metrics_from_ranks, RM.metrics):
        got = fn(off, rank, admissible, status, ks=(5, 1))
        assert got["users"] == 3 and got["targets"] == 5 and got["dropped_barred"] == 1 and got["dropped_invalid"] == 0
        for name, w in want.items():
            w = np.array(w)
            v = got[name + "_per_user"]
            assert v.dtype == np.float64 and (np.isnan(v) == np.isnan(w)).all(), name
            assert np.nanmax(np.abs(v - w)) <= 1e-12, name
            assert abs(got[name] - np.nanmean(w)) <= 1e-12, name
    # a row with status 2 leaves, and is counted
    status[0] = 2
    for fn in (ranking.metrics_from_ranks, RM.metrics):
        got = fn(off, rank, admissible, status, ks=(5,))
        assert got["users"] == 2 and got["dropped_invalid"] == 3 and math.isnan(got["mrr_per_user"][0])
        assert abs(got["mrr"] - 0.15) <= 1e-12 and abs(got["auc"] - (1 - 9 / 11)) <= 1e-12
    # nobody has a target: the means are 0.0, as the other metric dicts of the package
    got = ranking.metrics_from_ranks(np.zeros(3, dtype=np.int64), np.zeros(0), np.array([5, 5]), np.zeros(2))
    assert got["users"] == 0 and got["recall@10"] == 0.0 and np.isnan(got["auc_per_user"]).all()
